// kmeans_core.hpp — matlab/learning/k_means.m:71-114 (include/pbd_c.h "part mixtures"), one text for the host functions
// (pbd_kmeans_host.cpp) and for k_kmeans.hip.  Float64 throughout, the operations in the order the file writes them; the units that
// include this are built with -ffp-contract=off, so nothing fuses.
//
// One trial is written once, for a "wave" W of 64 lanes: lane j owns the points i = j, j + 64, ... and with them partial j of the
// library's block sum.  On the device W is a wavefront and a lane loop runs its body once, on the lane itself; on the host W walks the
// 64 lanes one after the other and keeps the 64 partials in an array.  W provides
//   W::lane_begin/_end   the lanes this thread of execution stands for: KM_EACH_LANE(W, j) is the loop over them
//   W::VecD / W::VecI    one double / int per lane, indexed by the lane
//   w.sum(VecD&)         the block sum: partials folded s[t] += s[t + h], h = 32 .. 1; the same value on every lane
//   w.isum(VecI&)        the integer sum over the lanes (any order: exact)
//   w.put(p, v)          store the wave-uniform v to wave-shared memory; w.sync() makes such stores visible to every lane
#pragma once
#include <math.h>
#include <stdint.h>
#ifdef __HIPCC__
#define PBD_KM_HD __host__ __device__ __forceinline__
#else
#define PBD_KM_HD inline
#endif

#define KM_LANES 64
#define KM_EACH_LANE(W, j) for (int j = W::lane_begin(), j##_end = W::lane_end(); j < j##_end; ++j)
#define KM_NONE 255   // g0 = ones against gIdx = zeros (k_means.m:82-83): a label no assignment gives, so the first pass always changes

// the header's splitmix64 ("QP solver")
PBD_KM_HD uint64_t km_next(uint64_t* state) {
  *state += 0x9E3779B97F4A7C15ull;
  uint64_t z = *state;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// where the stream of part p, trial r (of R) starts
PBD_KM_HD uint64_t km_stream(uint64_t seed, int p, int R, int r) {
  return seed ^ (0xD1B54A32D192ED03ull * (uint64_t)((long long)p * R + r + 1));
}

// k_means.m:92-96: d = 0; d = d + (X(:,s) - c(t,s))^2, s ascending
PBD_KM_HD double km_dist(const double* x, const double* c, int m) {
  double d = 0.0;
  for (int s = 0; s < m; ++s) {
    const double e = x[s] - c[s];
    const double q = e * e;
    d = d + q;
  }
  return d;
}
// MATLAB's [z, i] = min(v): NaN is ignored, the first of equal minima wins; all NaN: (NaN, the first).  One step of it:
PBD_KM_HD void km_min_step(double d, int t, double* z, int* best) {
  if (d < *z || (*z != *z && d == d)) { *z = d; *best = t; }
}
// k_means.m:100 for one point: the nearest of c[k][m]
PBD_KM_HD int km_nearest(const double* x, const double* c, int k, int m, double* z) {
  int best = 0;
  *z = km_dist(x, c, m);
  for (int t = 1; t < k; ++t) km_min_step(km_dist(x, c + (size_t)t * m, m), t, z, &best);
  return best;
}
// clusterparts.m:25-26: [dummy ind] = min(sumdist); ind(1)
PBD_KM_HD int km_first_min(const double* v, int n) {
  int best = 0;
  double z = v[0];
  for (int t = 1; t < n; ++t) km_min_step(v[t], t, &z, &best);
  return best;
}
// k_means.m:103-108: the mean of a partition, NaN for an empty one.  Per coordinate for any count — the header's stated deviation: the
// file's mean() of a single 1 x m row runs along the row
PBD_KM_HD double km_mean(double sum, int count) {
  return count > 0 ? sum / (double)count : (double)NAN;
}

// k_means.m:78 with the header's generator: k draws row = next() mod n, c(t,:) = X(row,:); rows may repeat
template <class W>
PBD_KM_HD void km_start(W& w, const double* X, int n, int m, int k, uint64_t state, double* c) {
  for (int t = 0; t < k; ++t) {
    const size_t row = (size_t)(km_next(&state) % (uint64_t)n);
    for (int s = 0; s < m; ++s) w.put(c + (size_t)t * m + s, X[row * m + s]);
  }
  w.sync();
}

// k_means.m:81-114.  c[k][m]: the start on entry, the file's c on return; lab[n]: the labels (0-based); *sumdist = sum(z) of the last
// assignment; *iters = passes of the while loop; *capped = 1 when the partition still changed in pass max_iter.
template <class W>
PBD_KM_HD void km_trial(W& w, const double* X, int n, int m, int k, double* c, unsigned char* lab, int max_iter, double* sumdist,
                        int* iters, int* capped) {
  KM_EACH_LANE(W, j) for (int i = j; i < n; i += KM_LANES) lab[i] = KM_NONE;
  int it = 0, moved;
  double sd;
  do {
    typename W::VecD zs;
    typename W::VecI ch;
    KM_EACH_LANE(W, j) {
      double z = 0.0;
      int changed = 0;
      for (int i = j; i < n; i += KM_LANES) {
        double zi;
        const int t = km_nearest(X + (size_t)i * m, c, k, m, &zi);   // :91-100
        changed |= t != (int)lab[i];
        lab[i] = (unsigned char)t;
        z = z + zi;
      }
      zs[j] = z;
      ch[j] = changed;
    }
    sd = w.sum(zs);
    moved = w.isum(ch) != 0;
    w.sync();   // (every lane is done reading c)
    for (int t = 0; t < k; ++t) {   // :102-109
      typename W::VecI cn;
      KM_EACH_LANE(W, j) {
        int q = 0;
        for (int i = j; i < n; i += KM_LANES) q += (int)lab[i] == t;
        cn[j] = q;
      }
      const int count = w.isum(cn);
      for (int s = 0; s < m; ++s) {
        typename W::VecD xs;
        KM_EACH_LANE(W, j) {
          double a = 0.0;
          for (int i = j; i < n; i += KM_LANES)
            if ((int)lab[i] == t) a = a + X[(size_t)i * m + s];
          xs[j] = a;
        }
        w.put(c + (size_t)t * m + s, km_mean(w.sum(xs), count));
      }
    }
    w.sync();
    ++it;
  } while (moved && it < max_iter);   // :87
  *sumdist = sd;   // :114
  *iters = it;
  *capped = moved;
}

// ---- host only
// the refusals of pbd_cluster_parts_host and pbd_cluster_parts (pbd_kmeans_host.cpp), before anything is computed or uploaded
int km_cluster_check(const double* def, int n, int P, const int32_t* parent, const int32_t* K, int R, int max_iter, const int32_t* idx);
// the part whose def is the minuend of X for part p, and the one that is subtracted (clusterparts.m:9-17)
inline void km_pair(const int32_t* parent, int P, int p, int* a, int* b) {
  if (parent[p] >= 0) { *a = p; *b = parent[p]; return; }
  int i = 0;
  while (i < P && parent[i] != p) ++i;   // (km_cluster_check: the root has a child)
  *a = i; *b = p;
}
