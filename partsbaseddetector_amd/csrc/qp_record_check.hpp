// qp_record_check.hpp — what pbd_qp_write refuses a record for, on the device: one text for the scans that stand in front of k_qp_write
// when the records never reach the host (k_qp_mine.hip: a mining frame's records; k_qp_latent.hip: a latent frame's pose).
// The checks are the host's, in its order: pbd_i_fv_check's ranges through featvec_gather.hpp, the column length, and
// qp_write.m:34-35's repeated dense start.
#pragma once
#include "pbd_internal.hpp"
#include "featvec_gather.hpp"

// MINE_OK, or the first reason in the order of the checks.  k: the cache's column length; noshare: [ncomp] 1 when no two parts of the
// component can share a filter, def or bias id whatever mixtures a pose picks (then the pairwise test is skipped)
__device__ inline int qp_record_check(const FeatVecArgs& fv, int k, const int* noshare, const pbd_candidate_head* hd, const int* lc) {
  if (!fv_rec_ok(fv, hd)) return MINE_BAD_RECORD;
  const int c = hd->component, lvl = hd->level, np = hd->nparts;
  int off = 1;
  for (int p = 0; p < np; ++p) {
    const FvPart P = fv_part(fv, true, c, lvl, np, lc, p);
    if (!P.ok) return MINE_BAD_RECORD;
    off += (p == 0 ? 3 : 9) + 2 + P.kh * P.kw * PBD_FLEN;
    if (off > k) return MINE_BAD_COLUMN;
  }
  if (noshare[c]) return MINE_OK;
  // qp_write.m:34-35, exactly: the ids of the mixtures the pose picked, pairwise (rare: a component whose parts can share an id at all)
  for (int p = 1; p < np; ++p) {
    const FvPart P = fv_part(fv, true, c, lvl, np, lc, p);
    for (int q = 0; q < p; ++q) {
      const FvPart Q = fv_part(fv, true, c, lvl, np, lc, q);
      if (P.filter_id == Q.filter_id || P.bias_id == Q.bias_id || (q > 0 && P.def_id == Q.def_id)) return MINE_BAD_REPEAT;
    }
  }
  return MINE_OK;
}
