// featvec_gather.hpp — what a part of a detection contributes to its feature vector (pbd_feature_block, include/pbd_c.h): the ids, the
// deformation values and where its window sits in the level's feature plane.  Device code shared by k_featvec.hip (which copies the
// blocks out) and k_qp.hip (which standardises them into a cache column): one text, so the two cannot drift apart.
#pragma once
#include "pbd_internal.hpp"

#ifdef __HIPCC__
struct FvPart {
  bool ok;                                 // the part has a block (else: ids -1, zeros)
  int x, y, kh, kw, cw, ch;                // location, filter size, the level's plane
  int bias_id, def_id, filter_id;
  long long d0, d1, d2, d3;                // the deformation block, integers (negated as integers: a zero stays +0.0)
  size_t cell_off;                         // first cell of the level's plane in a.feat
};

// the record's head against the model and the plan: one that fits neither gets ids -1 and zeros, and nothing of it is dereferenced
__device__ __forceinline__ bool fv_rec_ok(const FeatVecArgs& a, const pbd_candidate_head* hd) {
  const int c = hd->component, lvl = hd->level, np = hd->nparts, mp = a.in.mp;
  return c >= 0 && c < a.ncomp && lvl >= 0 && lvl < a.nvl && np >= 1 && np <= mp && np == a.nparts[c < 0 || c >= a.ncomp ? 0 : c];
}

// part p of a record of component c at level lvl; loc: [np][3] (x, y, mixture) of every part of the record
__device__ __forceinline__ FvPart fv_part(const FeatVecArgs& a, bool rec_ok, int c, int lvl, int np, const int* loc, int p) {
  FvPart P{};
  P.bias_id = P.def_id = P.filter_id = -1;
  const int mp = a.in.mp;
  bool ok = rec_ok && p < np;
  if (ok) {
    const LevelDev L = a.levels[lvl];
    P.cw = L.cw; P.ch = L.ch;
    P.cell_off = (size_t)L.cell_off;
    const int x = P.x = loc[p * 3], y = P.y = loc[p * 3 + 1];
    const int m = loc[p * 3 + 2];
    const int fp = a.flat[c * mp + p], m0 = a.mix0[fp], K = a.mix0[fp + 1] - m0;
    ok = x >= 0 && x < P.cw && y >= 0 && y < P.ch && m >= 0 && m < K;
    int xq = 0, yq = 0, mq = 0;
    if (ok && p > 0) {
      const int q = a.parent[c * mp + p];
      ok = q >= 0 && q < p;
      if (ok) {
        xq = loc[q * 3]; yq = loc[q * 3 + 1]; mq = loc[q * 3 + 2];
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
        P.bias_id = b; P.filter_id = F.filter; P.kh = F.kh; P.kw = F.kw;
        if (p > 0) {
          const long long dx = xq + M.ax - x, dy = yq + M.ay - y;
          P.def_id = F.def;
          P.d0 = -(dx * dx); P.d1 = -dx; P.d2 = -(dy * dy); P.d3 = -dy;   // negated as integers: a zero stays +0.0
        }
      }
    }
  }
  P.ok = ok;
  if (!ok) P.kh = P.kw = 0;
  return P;
}

// window cell `cell` (row-major over kh x kw) of the part: its plane cell, or false for one outside the plane — the bank's border
// value then: 0 in channels 0 .. flen - 2, 1 in channel flen - 1
__device__ __forceinline__ bool fv_cell(const FvPart& P, int cell, size_t* plane_cell) {
  const int i = cell / P.kw, j = cell - i * P.kw;
  const int yy = P.y - P.kh / 2 + i, xx = P.x - P.kw / 2 + j;
  if (yy < 0 || yy >= P.ch || xx < 0 || xx >= P.cw) return false;
  *plane_cell = P.cell_off + (size_t)yy * P.cw + xx;
  return true;
}
#endif
