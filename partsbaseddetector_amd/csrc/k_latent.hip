// k_latent.hip — latent detection (matlab/detection/detect.m:18-23, 60-101, 342-376; include/pbd_c.h "latent detection"): the best
// pose whose every part overlaps a given box.  Two steps around the unchanged DP:
//   k_latent_mask  between pdf and min: every cell of every response plane whose window — the box k_backtrack would report there —
//                  does not overlap its part's box by more than `overlap` becomes -1e10; a flag per (level, component, part) tells
//                  whether any cell stayed;
//   k_latent_best  in front of the back-tracking: the largest root score over the (level, component) pairs all of whose parts have
//                  a flag, as the ONE CandRec (per frame) that k_backtrack then walks.
// Plain C++ and vector stores only; the planes are never read.
#include "pbd_internal.hpp"

#define LATENT_NEG ((T)-1e10)   // detect.m's INF = 1e10: exact in float (2^10 * 5^10, 5^10 < 2^24)

// detect.m:360-376 (testoverlap) for one window, in float64, in the order written (every operand is an integer below 2^53: nothing
// rounds before the division).  The window covers x1 .. x1 + sz - 1, the truth tx .. tx + tw (a cv::Rect(xy1, xy2) as detect returns it).
__device__ __forceinline__ bool latent_admissible(int x1i, int y1i, int szi, int tx, int ty, int tw, int th, double overlap) {
  const double sz = (double)szi;
  const double x1 = (double)x1i, y1 = (double)y1i, x2 = x1 + sz - 1.0, y2 = y1 + sz - 1.0;
  const double bx1 = (double)tx, by1 = (double)ty, bx2 = bx1 + (double)tw, by2 = by1 + (double)th;
  const double w = fmax(0.0, fmin(x2, bx2) - fmax(x1, bx1) + 1.0);
  const double h = fmax(0.0, fmin(y2, by2) - fmax(y1, by1) + 1.0);
  const double inter = h * w;
  const double area = sz * sz;
  const double box = ((double)tw + 1.0) * ((double)th + 1.0);
  return inter / (area + box - inter) > overlap;
}

// One 256-thread block = 256 consecutive cells of ONE plane (host-built table, as k_root's): the job is wave-uniform.
template <typename T>
__global__ __launch_bounds__(256) void k_latent_mask(const LatentMaskArgs a) {
  const ReduceBlock rb = a.blocks[blockIdx.x];
  const LatJob& J = a.jobs[rb.job];
  if (a.component >= 0 && J.comp != a.component) return;     // a component that is not searched keeps its planes
  const unsigned cell = rb.cell0 + threadIdx.x;
  const bool live = cell < (unsigned)J.H * (unsigned)J.W;
  const int frame = J.level / a.nlevels;
  const int* t = a.truth + ((size_t)frame * a.mp + J.part) * 4;
  const int forced = a.mix ? a.mix[(size_t)frame * a.mp + J.part] : -1;
  T* plane = (T*)J.plane;
  if (forced >= 0 && forced != J.mix) {                       // bbox.m (detect.m:90-93): another mixture than the given one
    if (live) plane[cell] = LATENT_NEG;
    return;
  }
  bool adm = false;
  if (live) {
    const int y = (int)(cell / (unsigned)J.W), x = (int)(cell - (unsigned)y * (unsigned)J.W);
    // the box of k_backtrack (k_dp.hip): Point * T rounds with cvRound, the size is rows x rows scaled
    const T scale = J.scale;
    const int sz = t_round((T)J.rows * scale);
    const int x1 = t_round((T)(x - a.org) * scale), y1 = t_round((T)(y - a.org) * scale);
    adm = latent_admissible(x1, y1, sz, t[0], t[1], t[2], t[3], a.overlap);
    if (!adm) plane[cell] = LATENT_NEG;
  }
  // one vector atomic per wavefront that holds an admissible cell
  const unsigned long long any = __ballot(adm);
  if (any != 0ull && (threadIdx.x & 63) == 0) atomicOr(a.flags + J.flag, 1);
}

void launch_latent_mask(const LatentMaskArgs& a, int nblocks, int ts, hipStream_t s) {
  if (nblocks <= 0) return;
  if (ts == 8) hipLaunchKernelGGL(k_latent_mask<double>, dim3(nblocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_latent_mask<float>, dim3(nblocks), dim3(256), 0, s, a);
}

// ---- the best root ---------------------------------------------------------------------------------------------------------------
// Order: the larger score; among equal scores (-0.0 == 0.0) the smaller key = the smallest (level, component, y, x).  Scores travel as
// double (a float widens exactly and keeps its order) beside the key: two words, nothing packed.
__device__ __forceinline__ bool lat_better(double va, unsigned long long ka, double vb, unsigned long long kb) {
  if (ka == ~0ull) return false;
  if (kb == ~0ull) return true;
  return va > vb || (va == vb && ka < kb);
}
// the block's best of (v, k) -> thread 0's return values
__device__ __forceinline__ void lat_block_best(double& v, unsigned long long& k, double* sv, unsigned long long* sk) {
  const int t = threadIdx.x;
  sv[t] = v; sk[t] = k;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s && lat_better(sv[t + s], sk[t + s], sv[t], sk[t])) { sv[t] = sv[t + s]; sk[t] = sk[t + s]; }
    __syncthreads();
  }
  v = sv[0]; k = sk[0];
  __syncthreads();
}

// Stage 1: one block per 256 cells of a root job (k_root's block table): its best root, if the job's pair is admissible.
template <typename T>
__global__ __launch_bounds__(256) void k_latent_best(const LatentBestArgs a) {
  __shared__ double sv[256];
  __shared__ unsigned long long sk[256];
  const ReduceBlock rb = a.blocks[blockIdx.x];
  const RootJob& J = a.jobs[rb.job];
  const int* f = a.flags + ((size_t)J.level * a.ncomp + J.comp) * a.mp;
  const int np = a.nparts[J.comp];
  bool pair = true;                                            // detect.m:60-74: some part without an admissible cell: the pair yields nothing
  for (int p = 0; p < np; ++p) pair = pair && f[p] != 0;
  const unsigned cell = rb.cell0 + threadIdx.x;
  double v = 0.0;
  unsigned long long k = ~0ull;
  if (pair && cell < (unsigned)J.H * (unsigned)J.W) {
    v = (double)((const T*)J.rootv)[cell];
    k = ((unsigned long long)((unsigned)J.level * (unsigned)a.ncomp + (unsigned)J.comp) << 32) | cell;
  }
  lat_block_best(v, k, sv, sk);
  if (threadIdx.x == 0) { a.partial[blockIdx.x].v = v; a.partial[blockIdx.x].key = k; }
}
// Stage 2, the last block (a launch of its own: the partials are then visible whichever chiplet wrote them): per frame the best of the
// partials, written as the frame's one candidate; the count is the number of frames that have a pose.
__global__ __launch_bounds__(256) void k_latent_last(const LatentBestArgs a) {
  __shared__ double sv[256];
  __shared__ unsigned long long sk[256];
  int n = 0;
  for (int fr = 0; fr < a.nframes; ++fr) {
    double v = 0.0;
    unsigned long long k = ~0ull;
    for (int i = threadIdx.x; i < a.nblocks; i += 256) {
      const LatPartial p = a.partial[i];
      if (p.key == ~0ull || (int)((unsigned)(p.key >> 32) / (unsigned)a.ncomp) / a.nlevels != fr) continue;
      if (lat_better(p.v, p.key, v, k)) { v = p.v; k = p.key; }
    }
    lat_block_best(v, k, sv, sk);
    if (k == ~0ull) continue;
    if (threadIdx.x == 0) {
      const unsigned pairi = (unsigned)(k >> 32), cell = (unsigned)k;
      const int level = (int)(pairi / (unsigned)a.ncomp), comp = (int)(pairi - (unsigned)level * (unsigned)a.ncomp);
      int W = 1;
      for (int j = 0; j < a.nblocks; ++j) {                    // (a few hundred blocks, once per frame: the job of the pair gives W)
        const RootJob& J = a.jobs[a.blocks[j].job];
        if (J.level == level && J.comp == comp) { W = J.W; break; }
      }
      CandRec r;
      r.level = level; r.comp = comp; r.y = (int)(cell / (unsigned)W); r.x = (int)(cell - (unsigned)r.y * (unsigned)W);
      a.rec[n] = r;
    }
    ++n;
  }
  if (threadIdx.x == 0) *a.count = n;
}

void launch_latent_best(const LatentBestArgs& a, int ts, hipStream_t s) {
  if (a.nblocks > 0) {
    if (ts == 8) hipLaunchKernelGGL(k_latent_best<double>, dim3(a.nblocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_latent_best<float>, dim3(a.nblocks), dim3(256), 0, s, a);
  }
  hipLaunchKernelGGL(k_latent_last, dim3(1), dim3(256), 0, s, a);
}
