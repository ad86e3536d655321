// pbd_kmeans.cpp — pbd_cluster_parts (include/pbd_c.h "part mixtures"): clusterparts.m on the device.  No handle: the call allocates,
// uploads def once, launches k_kmeans.hip's three kernels on a stream of its own, brings the winners and the per-trial scalars back and
// frees everything; the calling thread's device is restored on every path.
#include <vector>
#include "pbd_internal.hpp"
#include "kmeans_core.hpp"

#define KMHIP(x) do { if ((x) != hipSuccess) return PBD_ERR_HIP; } while (0)

#pragma GCC visibility push(default)
extern "C" int pbd_cluster_parts(int device, const double* def, int n, int P, const int32_t* parent, const int32_t* K, int R, uint64_t seed,
                                 int max_iter, int32_t* idx, double* centres, double* sumdist, int32_t* best_trial, double* trial_sumdist,
                                 int32_t* trial_iters, int32_t* capped) {
  const int rc = km_cluster_check(def, n, P, parent, K, R, max_iter, idx);
  if (rc != PBD_OK) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { (void)hipGetLastError(); return PBD_ERR_HIP; }
  std::vector<int> pcap((size_t)P);   // (declared before `run`: it outlives the stream that copies into it)
  DeviceRun run;
  KMHIP(hipSetDevice(device));
  CLEAR_STICKY();
  KMHIP(run.open());

  std::vector<int> pa((size_t)P), pb((size_t)P);
  for (int p = 0; p < P; ++p) km_pair(parent, P, p, &pa[p], &pb[p]);
  const size_t ndef = (size_t)P * n * 2, trials = (size_t)P * R, nc = (size_t)PBD_CLUSTER_MAX_K * 2;
  KmeansArgs a{};
  double* d_def; int *d_pa, *d_pb, *d_K;
  KMHIP(run.alloc(&d_def, ndef));
  KMHIP(run.alloc(&a.X, ndef));
  KMHIP(run.alloc(&d_pa, (size_t)P));
  KMHIP(run.alloc(&d_pb, (size_t)P));
  KMHIP(run.alloc(&d_K, (size_t)P));
  KMHIP(run.alloc(&a.lab, trials * n));
  KMHIP(run.alloc(&a.tc, trials * nc));
  KMHIP(run.alloc(&a.tsum, trials));
  KMHIP(run.alloc(&a.titers, trials));
  KMHIP(run.alloc(&a.tcap, trials));
  KMHIP(run.alloc(&a.idx, (size_t)P * n));
  KMHIP(run.alloc(&a.centres, (size_t)P * nc));
  KMHIP(run.alloc(&a.sumdist, (size_t)P));
  KMHIP(run.alloc(&a.best, (size_t)P));
  KMHIP(run.alloc(&a.pcap, (size_t)P));
  a.def = d_def; a.pa = d_pa; a.pb = d_pb; a.K = d_K;
  a.n = n; a.P = P; a.R = R; a.max_iter = max_iter; a.seed = seed;
  KMHIP(hipMemcpyAsync(d_def, def, ndef * sizeof(double), hipMemcpyHostToDevice, run.stream));
  KMHIP(hipMemcpyAsync(d_pa, pa.data(), (size_t)P * sizeof(int), hipMemcpyHostToDevice, run.stream));
  KMHIP(hipMemcpyAsync(d_pb, pb.data(), (size_t)P * sizeof(int), hipMemcpyHostToDevice, run.stream));
  KMHIP(hipMemcpyAsync(d_K, K, (size_t)P * sizeof(int), hipMemcpyHostToDevice, run.stream));
  launch_kmeans(a, run.stream);
  KMHIP(hipGetLastError());

  KMHIP(hipMemcpyAsync(idx, a.idx, (size_t)P * n * sizeof(int32_t), hipMemcpyDeviceToHost, run.stream));
  KMHIP(hipMemcpyAsync(pcap.data(), a.pcap, (size_t)P * sizeof(int), hipMemcpyDeviceToHost, run.stream));
  if (centres) KMHIP(hipMemcpyAsync(centres, a.centres, (size_t)P * nc * sizeof(double), hipMemcpyDeviceToHost, run.stream));
  if (sumdist) KMHIP(hipMemcpyAsync(sumdist, a.sumdist, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, run.stream));
  if (best_trial) KMHIP(hipMemcpyAsync(best_trial, a.best, (size_t)P * sizeof(int32_t), hipMemcpyDeviceToHost, run.stream));
  if (trial_sumdist) KMHIP(hipMemcpyAsync(trial_sumdist, a.tsum, trials * sizeof(double), hipMemcpyDeviceToHost, run.stream));
  if (trial_iters) KMHIP(hipMemcpyAsync(trial_iters, a.titers, trials * sizeof(int32_t), hipMemcpyDeviceToHost, run.stream));
  KMHIP(hipStreamSynchronize(run.stream));
  if (capped) {
    int c = 0;
    for (int p = 0; p < P; ++p) c += pcap[p];
    *capped = c;
  }
  return PBD_OK;
}
#pragma GCC visibility pop
