// k_partscore.hip — the per-part scores of the frame's final records (pbd_part_score, include/pbd_c.h): what each part of a
// detection contributes to its score, split into appearance, deformation and bias.  gfx950 only; compiled with
// -ffp-contract=off like k_dp.hip: the deformation is the reference's Quadratic::operator() (include/DistanceTransform.hpp:102-104)
// in double, products and sums in the order written.
//
// One wavefront per record, lanes over its parts (a loop for components of more than 64 parts).  The record's part locations are
// read ONCE into LDS — in-frame records sit in the pinned host buffers the back-tracking writes — and every lane looks its parent
// up there.  Per part: one response gather, one table row, eight double operations, three stores.  A few KB per frame: the
// launch is what it costs.
#include "pbd_internal.hpp"

#define PS_NT 64
#define PS_BLOCKS 1024

template <typename T>
__global__ void __launch_bounds__(PS_NT) k_partscore(PartScoreArgs a) {
  extern __shared__ int s_loc[];   // [mp][3]: x, y, mixture of every part of the record
  const int total = *a.in.count;
  if (total > a.in.capacity) return;   // overflowed frame: it fails with PBD_ERR_CAPACITY
  const int lane = threadIdx.x, mp = a.in.mp;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int i = blockIdx.x; i < total; i += gridDim.x) {   // (every branch on i alone is uniform over the block)
    if (record_frame(a.in, i) < 0) continue;
    const char* rec = a.in.p + a.in.stride * (size_t)i;
    const pbd_candidate_head* hd = (const pbd_candidate_head*)rec;
    const int c = hd->component, lvl = hd->level, np = hd->nparts;
    double* o = a.out + (size_t)i * mp * 3;
    // records come from k_backtrack or through the entry point's range checks; one that fits neither the model nor the plan is
    // answered with NaN and nothing of it is dereferenced
    const bool rec_ok = c >= 0 && c < a.ncomp && lvl >= 0 && lvl < a.nvl && np >= 1 && np <= mp && np == a.nparts[c < 0 || c >= a.ncomp ? 0 : c];
    if (!rec_ok) {
      for (int k = lane; k < mp * 3; k += PS_NT) o[k] = nan;
      continue;
    }
    const int* lc = (const int*)(hd + 1) + (size_t)mp * 4;   // behind the head and the mp boxes
    for (int k = lane; k < np * 3; k += PS_NT) s_loc[k] = lc[k];
    __syncthreads();
    const LevelDev L = a.levels[lvl];
    const size_t HW = (size_t)L.cw * L.ch;
    const T* planes = (const T*)a.resp + (size_t)L.cell_off * a.nfilters;
    for (int p = lane; p < mp; p += PS_NT) {
      double app = 0.0, def = 0.0, bias = 0.0;
      if (p < np) {
        const int x = s_loc[p * 3], y = s_loc[p * 3 + 1], m = s_loc[p * 3 + 2];
        const int fp = a.flat[c * mp + p], m0 = a.mix0[fp], K = a.mix0[fp + 1] - m0;
        bool ok = x >= 0 && x < L.cw && y >= 0 && y < L.ch && m >= 0 && m < K;
        int xq = 0, yq = 0, mq = 0;
        if (ok && p > 0) {
          const int q = a.parent[c * mp + p];
          ok = q >= 0 && q < p;
          if (ok) {
            xq = s_loc[q * 3]; yq = s_loc[q * 3 + 1]; mq = s_loc[q * 3 + 2];
            const int fq = a.flat[c * mp + q];
            ok = mq >= 0 && mq < a.mix0[fq + 1] - a.mix0[fq];
          }
        }
        if (ok) {
          const PsMix M = a.mix[m0 + m];
          ok = M.filter >= 0 && M.filter < a.nfilters && M.bias >= 0 && M.bias + mq < a.nbias;
          if (ok) {
            app = (double)planes[(size_t)M.filter * HW + (size_t)y * L.cw + x];
            bias = (double)a.biasw[M.bias + mq];   // the child's mixture picks the base, the parent's the offset (root: mq = 0)
            if (p > 0) {
              const int dx = xq + M.ax - x, dy = yq + M.ay - y;
              const double ax = (double)M.w[0], bx = (double)M.w[1], ay = (double)M.w[2], by = (double)M.w[3];
              def = (ax * (double)(dx * dx) + bx * (double)dx) + (ay * (double)(dy * dy) + by * (double)dy);
            }
          }
        }
        if (!ok) app = def = bias = nan;
      }
      o[p * 3] = app; o[p * 3 + 1] = def; o[p * 3 + 2] = bias;
    }
    __syncthreads();   // s_loc is rewritten by the block's next record
  }
}

void launch_partscore(const PartScoreArgs& a, int ts, hipStream_t s) {
  const int nb = a.in.capacity < PS_BLOCKS ? (a.in.capacity > 0 ? a.in.capacity : 1) : PS_BLOCKS;
  const size_t lds = sizeof(int) * 3 * (size_t)a.in.mp;   // <= 3 KB (256 parts)
  if (ts == 8) hipLaunchKernelGGL(k_partscore<double>, dim3(nb), dim3(PS_NT), lds, s, a);
  else hipLaunchKernelGGL(k_partscore<float>, dim3(nb), dim3(PS_NT), lds, s, a);
}
