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
#include "featvec_gather.hpp"

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
    // records come through the entry point's range checks; one that fits neither the model nor the plan gets ids -1 and zeros
    const bool rec_ok = fv_rec_ok(a, hd);
    if (rec_ok) {
      const int* lc = (const int*)(hd + 1) + (size_t)mp * 4;   // behind the head and the mp boxes
      for (int k = threadIdx.x; k < np * 3; k += FV_NT) s_loc[k] = lc[k];
    }
    __syncthreads();
    if (p < mp) {   // (uniform over the wavefront, like everything below but the unit a lane moves)
      const FvPart P = fv_part(a, rec_ok, c, lvl, np, s_loc, p);   // featvec_gather.hpp
      const bool ok = P.ok;
      const int kh = P.kh, kw = P.kw, bias_id = P.bias_id, def_id = P.def_id, filter_id = P.filter_id;
      const long long d0 = P.d0, d1 = P.d1, d2 = P.d2, d3 = P.d3;
      const uint4* src = (const uint4*)a.feat;
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
      const int ncell = ok ? kh * kw : 0;
      for (int u0 = 0; u0 < SU; u0 += 64 * FV_BATCH) {
        uint4 v[FV_BATCH];
#pragma unroll
        for (int t = 0; t < FV_BATCH; ++t) {
          const int u = u0 + t * 64 + lane;
          uint4 z = make_uint4(0u, 0u, 0u, 0u);   // the slot's tail, an unused slot
          const int cell = u / U, sub = u % U;
          if (u < SU && cell < ncell) {
            size_t pc;
            if (fv_cell(P, cell, &pc)) z = src[pc * U + sub];
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
