// k_kmeans.hip — part mixtures (include/pbd_c.h "part mixtures"): matlab/learning/clusterparts.m's P * R independent k-means on the
// device.  gfx950 only; the trial is kmeans_core.hpp's text, shared with the host functions.
//   k_kmeans_x       X[p] = def[pa[p]] - def[pb[p]], one rounded (exact IEEE) subtraction per element.
//   k_kmeans_trials  one wavefront per (part, trial), KM_WAVES of them in a workgroup that never synchronises: the waves run trials of
//                    different lengths.  Lane j walks the points j, j + 64, ...: its running sums ARE partial j of the block sum, folded
//                    by qp_fold.  The labels live in the trial's row of the label plane, which only their own lane reads back; the
//                    centroids in the wave's 512 bytes of LDS, written by lane 0 between two wave-level fences.
//   k_kmeans_pick    one workgroup per part: the first trial at the minimal sumdist, its labels widened into idx, its centroids copied.
// Every loop is bounded by max_iter, n or K; no workgroup waits on another.  Plain C++ and vector stores only.
#include "pbd_internal.hpp"
#include "kmeans_core.hpp"
#include "qp_fold.hpp"

#define KM_NT 256
#define KM_WAVES (KM_NT / KM_LANES)

namespace {
// kmeans_core.hpp's wave on the device: the lane itself
struct DevWave {
  static __device__ __forceinline__ int lane_begin() { return (int)(threadIdx.x & (KM_LANES - 1)); }
  static __device__ __forceinline__ int lane_end() { return (int)(threadIdx.x & (KM_LANES - 1)) + 1; }
  struct VecD { double v; __device__ __forceinline__ double& operator[](int) { return v; } };
  struct VecI { int v; __device__ __forceinline__ int& operator[](int) { return v; } };
  __device__ __forceinline__ double sum(VecD& s) { return __shfl(qp_fold(s.v), 0, KM_LANES); }
  __device__ __forceinline__ int isum(VecI& s) {
    int v = s.v;
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v += __shfl_xor(v, h, KM_LANES);
    return v;
  }
  __device__ __forceinline__ void put(double* p, double v) { if ((threadIdx.x & (KM_LANES - 1)) == 0) *p = v; }
  __device__ __forceinline__ void sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
};
}  // namespace

__global__ void __launch_bounds__(KM_NT) k_kmeans_x(KmeansArgs a) {
  const size_t per = (size_t)a.n * 2, total = per * a.P;
  for (size_t e = (size_t)blockIdx.x * KM_NT + threadIdx.x; e < total; e += (size_t)gridDim.x * KM_NT) {
    const size_t p = e / per, i = e - p * per;
    a.X[e] = a.def[(size_t)a.pa[p] * per + i] - a.def[(size_t)a.pb[p] * per + i];
  }
}

__global__ void __launch_bounds__(KM_NT) k_kmeans_trials(KmeansArgs a) {
  __shared__ double s_c[KM_WAVES][PBD_CLUSTER_MAX_K * 2];
  const int wave = threadIdx.x / KM_LANES, lane = threadIdx.x & (KM_LANES - 1);
  const long long g = (long long)blockIdx.x * KM_WAVES + wave;
  if (g >= (long long)a.P * a.R) return;   // the whole wavefront: nothing below waits for another wave
  const int p = (int)(g / a.R), r = (int)(g - (long long)p * a.R);
  const int k = min(max(a.K[p], 1), PBD_CLUSTER_MAX_K);   // (the host refused anything else)
  const double* X = a.X + (size_t)p * a.n * 2;
  double* c = s_c[wave];
  DevWave w;
  km_start(w, X, a.n, 2, k, km_stream(a.seed, p, a.R, r), c);
  double sd;
  int it, cap;
  km_trial(w, X, a.n, 2, k, c, a.lab + (size_t)g * a.n, a.max_iter, &sd, &it, &cap);
  if (lane == 0) { a.tsum[g] = sd; a.titers[g] = it; a.tcap[g] = cap; }
  a.tc[(size_t)g * (PBD_CLUSTER_MAX_K * 2) + lane] = lane < k * 2 ? c[lane] : 0.0;   // (64 lanes, 32 x 2 values)
}

__global__ void __launch_bounds__(KM_NT) k_kmeans_pick(KmeansArgs a) {
  __shared__ int s_best;
  const int p = blockIdx.x;
  if (threadIdx.x == 0) {
    const int best = km_first_min(a.tsum + (size_t)p * a.R, a.R);
    int cap = 0;
    for (int r = 0; r < a.R; ++r) cap += a.tcap[(size_t)p * a.R + r];
    s_best = best;
    a.best[p] = best; a.sumdist[p] = a.tsum[(size_t)p * a.R + best]; a.pcap[p] = cap;
  }
  __syncthreads();
  const size_t g = (size_t)p * a.R + s_best;
  for (int i = threadIdx.x; i < a.n; i += KM_NT) a.idx[(size_t)p * a.n + i] = a.lab[g * a.n + i];
  if (threadIdx.x < PBD_CLUSTER_MAX_K * 2)
    a.centres[(size_t)p * (PBD_CLUSTER_MAX_K * 2) + threadIdx.x] = a.tc[g * (PBD_CLUSTER_MAX_K * 2) + threadIdx.x];
}

void launch_kmeans(const KmeansArgs& a, hipStream_t s) {
  const size_t total = (size_t)a.n * 2 * a.P;
  const size_t xb = (total + KM_NT - 1) / KM_NT;
  hipLaunchKernelGGL(k_kmeans_x, dim3((unsigned)(xb < 4096 ? xb : 4096)), dim3(KM_NT), 0, s, a);
  const long long trials = (long long)a.P * a.R;
  hipLaunchKernelGGL(k_kmeans_trials, dim3((unsigned)((trials + KM_WAVES - 1) / KM_WAVES)), dim3(KM_NT), 0, s, a);
  hipLaunchKernelGGL(k_kmeans_pick, dim3(a.P), dim3(KM_NT), 0, s, a);
}
