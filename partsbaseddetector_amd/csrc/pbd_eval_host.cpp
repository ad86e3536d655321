// pbd_eval_host.cpp — the definitions of include/pbd_c.h "evaluation ledger" as host code (no HIP: callable without a GPU, built with
// g++ like pbd_plan.cpp): eval_pck.m, eval_apk.m and VOCap.m from eval_core.hpp's text, which k_eval.hip shares.
#include <algorithm>
#include <cmath>
#include <vector>
#include "eval_core.hpp"
#include "../../include/pbd_c.h"

namespace {
bool finite_all(const double* v, size_t n) {
  for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
  return true;
}
bool scales_ok(const double* s, int n) {
  for (int i = 0; i < n; ++i) if (!std::isfinite(s[i]) || !(s[i] > 0.0)) return false;
  return true;
}
// the header's block sum: term k goes to partial k % 64 (k ascending, partials start at +0.0), folded s[t] += s[t + h], h = 32 .. 1
struct BlockSum {
  double s[64];
  BlockSum() { for (double& v : s) v = 0.0; }
  void add(long long k, double t) { s[k & 63] = s[k & 63] + t; }
  double fold() {
    for (int h = 32; h >= 1; h >>= 1)
      for (int t = 0; t < h; ++t) s[t] = s[t] + s[t + h];
    return s[0];
  }
};
}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int pbd_eval_keypoint_dist(const int32_t* boxes, int nparts, const double* points, double* d) {
  if (nparts < 0 || (nparts > 0 && (!boxes || !points || !d))) return PBD_ERR_ARG;
  if (!finite_all(points, (size_t)nparts * 2)) return PBD_ERR_ARG;
  for (int p = 0; p < nparts; ++p) {
    double cx, cy;
    eval_keypoint(boxes + (size_t)p * 4, &cx, &cy);
    d[p] = eval_dist(cx, cy, points[p * 2], points[p * 2 + 1]);
  }
  return PBD_OK;
}

int pbd_eval_pck_host(const double* dist, const double* scale, int n, int nparts, double thresh, int rule, double* pck) {
  if (n < 0 || nparts < 0 || (nparts > 0 && !pck) || (n > 0 && nparts > 0 && !dist) || (n > 0 && !scale)) return PBD_ERR_ARG;
  if (rule != PBD_EVAL_SCALE_LAST && rule != PBD_EVAL_SCALE_OWN) return PBD_ERR_ARG;
  if (!std::isfinite(thresh) || !scales_ok(scale, n)) return PBD_ERR_ARG;
  for (size_t i = 0; i < (size_t)n * nparts; ++i) if (std::isnan(dist[i])) return PBD_ERR_ARG;   // (+Inf: an instance without a pose)
  for (int p = 0; p < nparts; ++p) {
    long long hits = 0;
    for (int i = 0; i < n; ++i)
      hits += eval_pck_hit(dist[(size_t)i * nparts + p], thresh, scale[rule == PBD_EVAL_SCALE_LAST ? n - 1 : i]);
    pck[p] = (double)hits / (double)n;   // n == 0: 0 / 0 = NaN, the mean of nothing
  }
  return PBD_OK;
}

int pbd_eval_apk_match_host(const pbd_candidate_head* heads, const int32_t* boxes, int count, int max_parts, int nparts,
                            const double* points, const double* scale, int ngt, double thresh, uint8_t* tp) {
  if (count < 0 || nparts < 1 || max_parts < nparts || ngt < 0 || ngt > PBD_GT_MAX || !std::isfinite(thresh)) return PBD_ERR_ARG;
  if ((count > 0 && (!heads || !boxes || !tp)) || (ngt > 0 && (!points || !scale))) return PBD_ERR_ARG;
  if (!finite_all(points, (size_t)ngt * nparts * 2) || !scales_ok(scale, ngt)) return PBD_ERR_ARG;
  for (int i = 0; i < count; ++i)
    if (!std::isfinite(heads[i].score) || heads[i].nparts != nparts) return PBD_ERR_ARG;
  std::vector<unsigned long long> key((size_t)count);
  for (int i = 0; i < count; ++i) key[i] = eval_order_key(heads[i].score, (unsigned)i);
  std::sort(key.begin(), key.end());   // (distinct keys: one order)
  double q[PBD_GT_MAX];
  for (int p = 0; p < nparts; ++p) {
    unsigned long long taken = 0;
    for (int r = 0; r < count; ++r) {
      const int i = (int)(key[r] & 0xffffffffu);
      int hit = 0;
      if (ngt > 0) {
        double cx, cy;
        eval_keypoint(boxes + ((size_t)i * max_parts + p) * 4, &cx, &cy);
        for (int g = 0; g < ngt; ++g) {
          const double* pt = points + ((size_t)g * nparts + p) * 2;
          q[g] = eval_dist(cx, cy, pt[0], pt[1]) / scale[g];
        }
        hit = eval_match_step(q, ngt, thresh, &taken);
      }
      tp[(size_t)i * nparts + p] = (uint8_t)hit;
    }
  }
  return PBD_OK;
}

int pbd_eval_ap_host(const float* score, const uint8_t* tp, int m, int nparts, long long npos, double* apk, double* prec, double* rec) {
  if (m < 0 || nparts < 0 || npos < 0 || (nparts > 0 && !apk) || (m > 0 && (!score || (nparts > 0 && !tp)))) return PBD_ERR_ARG;
  for (int i = 0; i < m; ++i) if (!std::isfinite(score[i])) return PBD_ERR_ARG;
  std::vector<unsigned long long> key((size_t)m);
  for (int i = 0; i < m; ++i) key[i] = eval_order_key(score[i], (unsigned)i);
  std::sort(key.begin(), key.end());
  std::vector<int> tpc((size_t)m);
  std::vector<double> sm((size_t)m);
  for (int p = 0; p < nparts; ++p) {
    int c = 0;
    for (int i = 0; i < m; ++i) {
      c += tp[(size_t)(key[i] & 0xffffffffu) * nparts + p] != 0;
      tpc[i] = c;
      if (prec) prec[(size_t)p * m + i] = eval_prec(c, i);
      if (rec) rec[(size_t)p * m + i] = eval_rec(c, npos);
    }
    double mx = 0.0;   // mpre's closing 0
    for (int i = m - 1; i >= 0; --i) {
      const double v = eval_prec(tpc[i], i);
      mx = v > mx ? v : mx;
      sm[i] = mx;
    }
    BlockSum s;
    double prev = 0.0;
    for (int i = 0; i < m; ++i) {
      const double r = eval_rec(tpc[i], npos);
      s.add(i, eval_ap_term(prev, r, sm[i]));
      prev = r;
    }
    s.add(m, eval_ap_term(prev, 1.0, 0.0));
    apk[p] = s.fold();
  }
  return PBD_OK;
}

}  // extern "C"
#pragma GCC visibility pop
