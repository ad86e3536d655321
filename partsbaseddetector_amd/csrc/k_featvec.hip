// k_featvec.hip — the feature vector of a detection (pbd_feature_block, include/pbd_c.h): per part a bias id, a deformation block
// and the window of the HOG level under the part's filter, what matlab/detection/detect.m:272-308 collects while it back-tracks a
// pose.  gfx950 only.  A pure gather: no value is computed, the windows are the handle's own feature values, copied.
//
// One wavefront per (record, part), four of them to a workgroup; the record's part locations are read ONCE per workgroup into LDS,
// as k_partscore does, for the parent look-up.  The source is cell-major [ch][cw][flen]: a cell is flen * sizeof(T) contiguous
// bytes, moved as 16-byte units — eight lanes move one float cell, one wavefront instruction eight cells —, the destination one
// contiguous run per part.  The border test is per cell.  The part's wavefront also writes its block header, the zero tail of its
// window slot and, for part slots beyond the record's nparts, ids -1 and zeros: nothing is memset in front of the launch.
// Memory-bound: its floor is its own output bytes written once, the reads overlap heavily and hit L2.
#include "pbd_internal.hpp"

#define FV_NT 256
#define FV_WAVES (FV_NT / 64)
#define FV_BLOCKS (1 << 20)
#define FV_BATCH 4   // 16-byte units a lane has in flight before it stores them

template <typename T>
__global__ void __launch_bounds__(FV_NT) k_featvec(FeatVecArgs a) {
  extern __shared__ int s_loc[];   // [mp][3]: x, y, mixture of every part of the record
  constexpr int U = PBD_FLEN * (int)sizeof(T) / 16;   // 16-byte units of a cell
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, mp = a.in.mp;
  const int groups = (mp + FV_WAVES - 1) / FV_WAVES;
  const int SU = a.wmax / PBD_FLEN * U;               // units of a window slot
  const long long items = (long long)a.n * groups;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {   // (every branch on `it` alone is uniform over the block)
    const int r = (int)(it / groups), p = (int)(it % groups) * FV_WAVES + wave;
    const char* rec = a.in.p + a.in.stride * (size_t)(a.rec0 + r);
    const pbd_candidate_head* hd = (const pbd_candidate_head*)rec;
    const int c = hd->component, lvl = hd->level, np = hd->nparts;
    // records come through the entry point's range checks; one that fits neither the model nor the plan gets ids -1 and zeros, and
    // nothing of it is dereferenced
    const bool rec_ok = c >= 0 && c < a.ncomp && lvl >= 0 && lvl < a.nvl && np >= 1 && np <= mp && np == a.nparts[c < 0 || c >= a.ncomp ? 0 : c];
    if (rec_ok) {
      const int* lc = (const int*)(hd + 1) + (size_t)mp * 4;   // behind the head and the mp boxes
      for (int k = threadIdx.x; k < np * 3; k += FV_NT) s_loc[k] = lc[k];
    }
    __syncthreads();
    if (p < mp) {   // (uniform over the wavefront, like everything below but the unit a lane moves)
      int x = 0, y = 0, kh = 0, kw = 0, bias_id = -1, def_id = -1, filter_id = -1, cw = 0, ch = 0;
      long long d0 = 0, d1 = 0, d2 = 0, d3 = 0;
      const uint4* src = nullptr;
      bool ok = rec_ok && p < np;
      if (ok) {
        const LevelDev L = a.levels[lvl];
        cw = L.cw; ch = L.ch;
        src = (const uint4*)a.feat + (size_t)L.cell_off * U;
        x = s_loc[p * 3]; y = s_loc[p * 3 + 1];
        const int m = s_loc[p * 3 + 2];
        const int fp = a.flat[c * mp + p], m0 = a.mix0[fp], K = a.mix0[fp + 1] - m0;
        ok = x >= 0 && x < cw && y >= 0 && y < ch && m >= 0 && m < K;
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
          const FvMix F = a.fmix[m0 + m];
          const int b = p > 0 ? M.bias + mq : a.mix[m0].bias;   // the root's scalar: biasid[0][0]
          ok = F.filter >= 0 && F.filter < a.nfilters && b >= 0 && b < a.nbias && F.kh >= 1 && F.kw >= 1 &&
               F.kh * F.kw * PBD_FLEN <= a.wmax;
          if (ok) {
            bias_id = b; filter_id = F.filter; kh = F.kh; kw = F.kw;
            if (p > 0) {
              const long long dx = xq + M.ax - x, dy = yq + M.ay - y;
              def_id = F.def;
              d0 = -(dx * dx); d1 = -dx; d2 = -(dy * dy); d3 = -dy;   // negated as integers: a zero stays +0.0
            }
          }
        }
      }
      const size_t slot = (size_t)r * mp + p;
      if (lane < 14) {   // the 56-byte block header, a 4-byte word per lane
        int w;
        if (lane < 6) w = lane == 0 ? bias_id : lane == 1 ? def_id : lane == 2 ? filter_id : lane == 3 ? kh : lane == 4 ? kw : 0;
        else {
          const int j = (lane - 6) >> 1;
          const double v = (double)(j == 0 ? d0 : j == 1 ? d1 : j == 2 ? d2 : d3);
          w = (lane & 1) ? __double2hiint(v) : __double2loint(v);
        }
        ((int*)(a.blocks + slot))[lane] = w;
      }
      uint4* __restrict__ dst = (uint4*)a.windows + slot * (size_t)SU;
      const int ncell = ok ? kh * kw : 0, y0 = y - kh / 2, x0 = x - kw / 2;
      for (int u0 = 0; u0 < SU; u0 += 64 * FV_BATCH) {
        uint4 v[FV_BATCH];
#pragma unroll
        for (int t = 0; t < FV_BATCH; ++t) {
          const int u = u0 + t * 64 + lane;
          uint4 z = make_uint4(0u, 0u, 0u, 0u);   // the slot's tail, an unused slot
          const int cell = u / U, sub = u % U;
          if (u < SU && cell < ncell) {
            const int i = cell / kw, j = cell - i * kw;
            const int yy = y0 + i, xx = x0 + j;
            if (yy >= 0 && yy < ch && xx >= 0 && xx < cw) z = src[((size_t)yy * cw + xx) * U + sub];
            else if (sub == U - 1) {   // the bank's border: 1 in channel flen - 1
              if (sizeof(T) == 4) z.w = 0x3f800000u; else z.w = 0x3ff00000u;
            }
          }
          v[t] = z;
        }
#pragma unroll
        for (int t = 0; t < FV_BATCH; ++t) {
          const int u = u0 + t * 64 + lane;
          if (u < SU) dst[u] = v[t];
        }
      }
    }
    __syncthreads();   // s_loc is rewritten by the block's next item
  }
}

void launch_featvec(const FeatVecArgs& a, int ts, hipStream_t s) {
  const long long items = (long long)a.n * ((a.in.mp + FV_WAVES - 1) / FV_WAVES);
  const int nb = (int)(items < FV_BLOCKS ? (items > 0 ? items : 1) : FV_BLOCKS);
  const size_t lds = sizeof(int) * 3 * (size_t)a.in.mp;   // <= 3 KB (256 parts)
  if (ts == 8) hipLaunchKernelGGL(k_featvec<double>, dim3(nb), dim3(FV_NT), lds, s, a);
  else hipLaunchKernelGGL(k_featvec<float>, dim3(nb), dim3(FV_NT), lds, s, a);
}
