// pbd_kmeans_host.cpp — the definitions of include/pbd_c.h "part mixtures" as host code (no HIP: callable without a GPU, built with g++
// like pbd_plan.cpp): k_means.m and clusterparts.m from kmeans_core.hpp's text, which k_kmeans.hip shares.
#include <cmath>
#include <vector>
#include "kmeans_core.hpp"
#include "../../include/pbd_c.h"

namespace {
// kmeans_core.hpp's wave on the host: the 64 lanes one after the other, their partials in an array
struct HostWave {
  static int lane_begin() { return 0; }
  static int lane_end() { return KM_LANES; }
  struct VecD { double v[KM_LANES]; double& operator[](int j) { return v[j]; } };
  struct VecI { int v[KM_LANES]; int& operator[](int j) { return v[j]; } };
  double sum(VecD& s) {   // the header's block sum
    for (int h = 32; h >= 1; h >>= 1)
      for (int t = 0; t < h; ++t) s[t] = s[t] + s[t + h];
    return s[0];
  }
  int isum(VecI& s) {
    int a = 0;
    for (int t = 0; t < KM_LANES; ++t) a += s[t];
    return a;
  }
  void put(double* p, double v) { *p = v; }
  void sync() {}
};
bool finite_all(const double* v, size_t n) {
  for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
  return true;
}
}  // namespace

int km_cluster_check(const double* def, int n, int P, const int32_t* parent, const int32_t* K, int R, int max_iter, const int32_t* idx) {
  if (!def || !parent || !K || !idx || n < 1 || P < 1 || R < 1 || max_iter < 1 || max_iter > PBD_CLUSTER_MAX_ITER) return PBD_ERR_ARG;
  if (parent[0] != -1) return PBD_ERR_ARG;
  bool child = false;
  for (int p = 1; p < P; ++p) {
    if (parent[p] < 0 || parent[p] >= p) return PBD_ERR_ARG;
    child |= parent[p] == 0;
  }
  if (!child) return PBD_ERR_ARG;   // clusterparts.m:11-13 would run off the end of pa
  for (int p = 0; p < P; ++p) if (K[p] < 1) return PBD_ERR_ARG;
  if (!finite_all(def, (size_t)P * n * 2)) return PBD_ERR_ARG;
  for (int p = 0; p < P; ++p) {     // X itself must be finite: a difference of finite values can overflow
    int a, b;
    km_pair(parent, P, p, &a, &b);
    for (size_t i = 0; i < (size_t)n * 2; ++i)
      if (!std::isfinite(def[(size_t)a * n * 2 + i] - def[(size_t)b * n * 2 + i])) return PBD_ERR_ARG;
  }
  for (int p = 0; p < P; ++p) if (K[p] > PBD_CLUSTER_MAX_K) return PBD_ERR_UNSUPPORTED;
  if ((long long)P * R > PBD_CLUSTER_MAX_TRIALS) return PBD_ERR_UNSUPPORTED;   // (the device keeps 512 bytes of centroids per trial)
  if ((long long)P * R > PBD_CLUSTER_MAX_LABELS / n) return PBD_ERR_UNSUPPORTED;
  return PBD_OK;
}

#pragma GCC visibility push(default)
extern "C" {

int pbd_kmeans_host(const double* X, int n, int m, int k, const double* c0, uint64_t state0, int max_iter, int32_t* idx, double* c,
                    double* sumdist, int* iters) {
  if (!X || !idx || n < 1 || m < 1 || k < 1 || max_iter < 1 || max_iter > PBD_CLUSTER_MAX_ITER) return PBD_ERR_ARG;
  if (!finite_all(X, (size_t)n * m) || (c0 && !finite_all(c0, (size_t)k * m))) return PBD_ERR_ARG;
  if (k > PBD_CLUSTER_MAX_K) return PBD_ERR_UNSUPPORTED;
  HostWave w;
  std::vector<double> cc((size_t)k * m);
  std::vector<unsigned char> lab((size_t)n);
  if (c0) cc.assign(c0, c0 + (size_t)k * m);
  else km_start(w, X, n, m, k, state0, cc.data());
  double sd;
  int it, capped;
  km_trial(w, X, n, m, k, cc.data(), lab.data(), max_iter, &sd, &it, &capped);
  for (int i = 0; i < n; ++i) idx[i] = lab[i];
  if (c) for (size_t i = 0; i < cc.size(); ++i) c[i] = cc[i];
  if (sumdist) *sumdist = sd;
  if (iters) *iters = it;
  return PBD_OK;
}

int pbd_cluster_parts_host(const double* def, int n, int P, const int32_t* parent, const int32_t* K, int R, uint64_t seed, int max_iter,
                           int32_t* idx, double* centres, double* sumdist, int32_t* best_trial, double* trial_sumdist,
                           int32_t* trial_iters, int32_t* capped) {
  const int rc = km_cluster_check(def, n, P, parent, K, R, max_iter, idx);
  if (rc != PBD_OK) return rc;
  HostWave w;
  std::vector<double> X((size_t)n * 2), cc(PBD_CLUSTER_MAX_K * 2), bestc(PBD_CLUSTER_MAX_K * 2), sd((size_t)R);
  std::vector<unsigned char> lab((size_t)n), bestlab((size_t)n);
  int ncapped = 0;
  for (int p = 0; p < P; ++p) {
    int a, b;
    km_pair(parent, P, p, &a, &b);
    for (size_t i = 0; i < (size_t)n * 2; ++i) X[i] = def[(size_t)a * n * 2 + i] - def[(size_t)b * n * 2 + i];
    int best = 0;
    for (int r = 0; r < R; ++r) {
      int it, cap;
      km_start(w, X.data(), n, 2, K[p], km_stream(seed, p, R, r), cc.data());
      km_trial(w, X.data(), n, 2, K[p], cc.data(), lab.data(), max_iter, &sd[r], &it, &cap);
      ncapped += cap;
      if (trial_sumdist) trial_sumdist[(size_t)p * R + r] = sd[r];
      if (trial_iters) trial_iters[(size_t)p * R + r] = it;
      if (km_first_min(sd.data(), r + 1) == r) { best = r; bestlab = lab; bestc = cc; }   // the first trial at the minimum so far
    }
    for (int i = 0; i < n; ++i) idx[(size_t)p * n + i] = bestlab[i];
    if (centres)
      for (int t = 0; t < PBD_CLUSTER_MAX_K * 2; ++t) centres[(size_t)p * PBD_CLUSTER_MAX_K * 2 + t] = t < K[p] * 2 ? bestc[t] : 0.0;
    if (sumdist) sumdist[p] = sd[best];
    if (best_trial) best_trial[p] = best;
  }
  if (capped) *capped = ncapped;
  return PBD_OK;
}

}  // extern "C"
#pragma GCC visibility pop
