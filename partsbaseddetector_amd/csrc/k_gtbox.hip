// k_gtbox.hip — the best pose per ground-truth box (matlab/detection/bestoverlap.m, what testmodel_gtbox.m:21 runs behind a detect;
// include/pbd_c.h "best pose per ground-truth box"): of the records k_backtrack left in a device list, or of a caller's records, per
// (frame, gt box) the highest-scoring one whose box of part centres covers more than `overlap` of the gt box.  Two launches:
//   k_gtbox_centres  one thread per record (a fixed grid, PBD_GT_SPAN records per pass): the centre box, once per record whatever the
//                    number of gt boxes, with the record's frame, score key and rank, into planes the second launch reads coalesced;
//   k_gtbox_pick     one block per (frame, gt box): every thread walks the planes, keeps its best matching record, the block reduces
//                    and copies the winner's whole record — and found, o — to where the host reads them (pinned memory).
// The order is total — match; the score as an ordered integer (-0.0 = +0.0); the smaller 64-bit rank — so the result does not depend
// on the order the records were written in, and equals the host function's bit for bit: the arithmetic is gt_overlap.hpp's, shared
// with it.  No atomics; a launch boundary carries the planes from the first kernel to the second.  Plain C++ and vector stores only.
#include "pbd_internal.hpp"
#include "gt_overlap.hpp"

__device__ __forceinline__ int gt_count(const RecordSet& r) {
  const int n = *r.count;
  return n < 0 ? 0 : n > r.capacity ? r.capacity : n;   // (an overflowed list: the entry reports PBD_ERR_CAPACITY; stay inside it)
}

__global__ __launch_bounds__(PBD_GT_BLOCK) void k_gtbox_centres(const GtBoxArgs a) {
  const int n = gt_count(a.in);
  for (int i = blockIdx.x * PBD_GT_BLOCK + threadIdx.x; i < n; i += PBD_GT_SPAN) {
    const char* r = a.in.p + a.in.stride * (size_t)i;
    const pbd_candidate_head hd = *(const pbd_candidate_head*)r;
    const int32_t* b = (const int32_t*)(r + sizeof(pbd_candidate_head));
    const int np = hd.nparts > a.in.mp ? a.in.mp : hd.nparts;
    int frame = a.in.nlevels ? hd.level / a.in.nlevels : 0;
    if (np <= 0 || frame < 0 || frame >= a.nframes) frame = -1;   // rule 2: no parts, no match
    GtCentreBox c{0.0, 0.0, 0.0, 0.0};
    if (frame >= 0) c = gt_centre_box(b, np);
    unsigned long long rank = (unsigned long long)(unsigned)i;    // caller's records: the input position
    if (a.in.nlevels) {                                           // in-frame: pbd_i_emit's order — (virtual) level, component, root y, root x
      const int32_t* lc = b + (size_t)a.in.mp * 4;
      rank = ((unsigned long long)(hd.level & 0xffff) << 48) | ((unsigned long long)(hd.component & 0xffff) << 32) |
             ((unsigned long long)(lc[1] & 0xffff) << 16) | (unsigned long long)(lc[0] & 0xffff);
    }
    a.cbox[i] = make_double4(c.x1, c.y1, c.x2, c.y2);
    a.key[i] = gt_score_key(hd.score);
    a.rank[i] = rank;
    a.frame[i] = frame;
  }
}

struct GtBest { unsigned key; int idx; unsigned long long rank; double o; };   // idx < 0: none
__device__ __forceinline__ bool gt_better(unsigned ka, unsigned long long ra, int ia, const GtBest& b) {
  if (ia < 0) return false;
  if (b.idx < 0) return true;
  return ka > b.key || (ka == b.key && ra < b.rank);
}

__global__ __launch_bounds__(PBD_GT_BLOCK) void k_gtbox_pick(const GtBoxArgs a) {
  __shared__ GtBest sb[PBD_GT_BLOCK];
  const int g = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
  if (g >= a.ngt[f]) return;                                     // (block-uniform)
  const int n = gt_count(a.in);
  const size_t slot = (size_t)f * PBD_GT_MAX + g;
  double gt[4];
  for (int k = 0; k < 4; ++k) gt[k] = a.gt[slot * 4 + k];
  GtBest best{0u, -1, 0ull, 0.0};
  for (int i = t; i < n; i += PBD_GT_BLOCK) {
    if (a.frame[i] != f) continue;
    const double4 q = a.cbox[i];
    const GtCentreBox c{q.x, q.y, q.z, q.w};
    const double o = gt_overlap(gt, c);
    if (!(o > a.overlap)) continue;                              // rule 4: strict, NaN is no match
    const unsigned key = a.key[i];
    const unsigned long long rank = a.rank[i];
    if (gt_better(key, rank, i, best)) best = GtBest{key, i, rank, o};
  }
  sb[t] = best;
  __syncthreads();
  for (int s = PBD_GT_BLOCK / 2; s > 0; s >>= 1) {
    if (t < s && gt_better(sb[t + s].key, sb[t + s].rank, sb[t + s].idx, sb[t])) sb[t] = sb[t + s];
    __syncthreads();
  }
  best = sb[0];
  if (t == 0) {
    a.found[slot] = best.idx >= 0;
    a.o[slot] = best.idx >= 0 ? best.o : 0.0;
    if (a.best) a.best[slot] = best.idx;
  }
  if (best.idx < 0 || !a.out) return;
  const int* src = (const int*)(a.in.p + a.in.stride * (size_t)best.idx);   // records are whole ints (pbd_rec_bytes)
  int* dst = (int*)(a.out + a.in.stride * slot);
  for (int k = t; k < (int)(a.in.stride / sizeof(int)); k += PBD_GT_BLOCK) dst[k] = src[k];
}

// gmax: the largest ngt of the frames (0: nothing to do)
void launch_gtbox(const GtBoxArgs& a, int gmax, hipStream_t s) {
  if (gmax <= 0 || a.nframes <= 0) return;
  hipLaunchKernelGGL(k_gtbox_centres, dim3(PBD_GT_GRID), dim3(PBD_GT_BLOCK), 0, s, a);
  hipLaunchKernelGGL(k_gtbox_pick, dim3(gmax, a.nframes), dim3(PBD_GT_BLOCK), 0, s, a);
}
