// k_qp_latent.hip — latent positives (include/pbd_c.h "latent positives"): what stands between a latent frame's pose, left on the
// device by the back-tracking or the candidate filter, and k_qp_write.  gfx950 only.
//
// k_qp_latent_scan: one wavefront per frame.  A latent call yields at most one record per frame, and k_latent_last compacts the found
//   frames' records: the list is not frame-aligned.  The wavefront of frame f walks the list (at most 64 records), attributes every
//   record to its frame (virtual level / nlevels; the filter's count block when the records went through k_cand_filter), finds its
//   own record and the number of found frames in front of it, validates the record with the checks pbd_qp_write makes on the host
//   (qp_record_check.hpp: the mining scan's text), and answers in the frame's pinned block: found, the refusal code, the record's
//   head, root cell and score.  perm[found frames in front] = the record: the frame-ordered index k_qp_write reads.
// Every result is one plain store by lane 0; the two reductions are wavefront shuffles.  No atomics, no LDS.
#include "pbd_internal.hpp"
#include "featvec_gather.hpp"
#include "qp_record_check.hpp"

#define QL_SCAN_NT 64
#define QL_NONE 0x7fffffff

__global__ void __launch_bounds__(QL_SCAN_NT) k_qp_latent_scan(LatentWriteArgs a) {
  const RecordSet& in = a.in;
  const int f = blockIdx.x, B = a.nframes, lane = threadIdx.x;
  const int raw = in.cf ? in.cf[0] : *in.count;
  int mine = QL_NONE, before = 0;   // the frame's record; found frames in front of this one
  if (in.cf) {   // the filter's final order: frame g's kept records at [cf[2 + B + g], + cf[2 + g])
    for (int g = lane; g < B; g += QL_SCAN_NT) {
      const int kept = in.cf[2 + g];
      if (g < f && kept > 0) ++before;
      if (g == f && kept > 0) mine = in.cf[2 + B + g];
    }
  } else {       // the back-tracking's list, one record per found frame in any order
    const int n = raw < in.capacity ? raw : in.capacity;
    for (int i = lane; i < n; i += QL_SCAN_NT) {
      const int lvl = ((const pbd_candidate_head*)(in.p + in.stride * (size_t)i))->level;
      const int g = in.nlevels > 0 && B > 1 ? lvl / in.nlevels : 0;
      if (g < f) ++before;
      if (g == f && i < mine) mine = i;
    }
  }
#pragma unroll
  for (int h = 32; h >= 1; h >>= 1) {
    const int m = __shfl_xor(mine, h, 64), b = __shfl_xor(before, h, 64);
    mine = m < mine ? m : mine;
    before += b;
  }
  if (lane != 0) return;
  LatentWriteOut o;
  o.found = 0; o.code = MINE_OK; o.component = 0; o.level = 0; o.x = 0; o.y = 0; o.raw = raw; o.reserved = 0; o.score = 0.0;
  if (mine != QL_NONE && mine >= 0 && mine < in.capacity) {
    const pbd_candidate_head* hd = (const pbd_candidate_head*)(in.p + in.stride * (size_t)mine);
    const int* lc = (const int*)(hd + 1) + (size_t)in.mp * 4;
    o.found = 1;
    o.code = qp_record_check(a.fv, a.k, a.noshare, hd, lc);
    o.component = hd->component;
    o.level = hd->level - (in.nlevels > 0 && B > 1 ? f * in.nlevels : 0);
    o.x = lc[0]; o.y = lc[1];
    o.score = (double)hd->score;
    if (before < B) a.perm[before] = mine;
  }
  a.out[f] = o;
}

void launch_qp_latent_scan(const LatentWriteArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_qp_latent_scan, dim3(a.nframes), dim3(QL_SCAN_NT), 0, s, a);
}
