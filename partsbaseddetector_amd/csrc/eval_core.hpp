// eval_core.hpp — the arithmetic of matlab/evaluation/eval_pck.m, eval_apk.m and VOCap.m (include/pbd_c.h "evaluation ledger"), one
// text for the host functions (pbd_eval_host.cpp) and for k_eval.hip.  Float64 throughout, the operations in the order the definition
// writes them; the units that include this are built with -ffp-contract=off, so nothing fuses.
#pragma once
#include <math.h>
#include <stdint.h>
#ifdef __HIPCC__
#define PBD_EV_HD __host__ __device__ __forceinline__
#else
#define PBD_EV_HD inline
#endif

// Keypoint: the centre of part box b = (x, y, w, h), as gt_overlap.hpp / bestoverlap.m:11-14 form it.  int32 -> double and the halves
// are exact: nothing rounds.
PBD_EV_HD void eval_keypoint(const int32_t* b, double* cx, double* cy) {
  const double x = (double)b[0], y = (double)b[1];
  const double x2 = x + (double)b[2] - 1.0, y2 = y + (double)b[3] - 1.0;
  *cx = .5 * x + .5 * x2;
  *cy = .5 * y + .5 * y2;
}

// Distance (eval_pck.m:10, eval_apk.m:21): two rounded products, one rounded sum (x term first), a correctly rounded square root
PBD_EV_HD double eval_dist(double cx, double cy, double gx, double gy) {
  const double dx = cx - gx, dy = cy - gy;
  const double xx = dx * dx, yy = dy * dy;
  const double s = xx + yy;
#ifdef __HIP_DEVICE_COMPILE__
  return __dsqrt_rn(s);   // round to nearest even, like the host's sqrt (IEEE 754 requires it correctly rounded)
#else
  return sqrt(s);
#endif
}

// A larger float is a larger key; -0.0 and +0.0 share one (gt_overlap.hpp's gt_score_key)
PBD_EV_HD unsigned eval_score_key(float s) {
  union { float f; unsigned u; } v;
  v.f = s;
  if (v.u == 0x80000000u) v.u = 0u;
  return (v.u & 0x80000000u) ? ~v.u : (v.u | 0x80000000u);
}
// ascending in this key = score descending, then sequence ascending (MATLAB's stable sort(..., 'descend')); keys of distinct seq differ
PBD_EV_HD unsigned long long eval_order_key(float score, unsigned seq) {
  return ((unsigned long long)(~eval_score_key(score)) << 32) | (unsigned long long)seq;
}

// Matching step (eval_apk.m:24-35) once the minimum qmin = q[jmin] is known, jmin the FIRST index of the minimum; *taken: bit g = gt g
// already has its detection for this keypoint.  1: true positive.
PBD_EV_HD int eval_match_decide(double qmin, int jmin, double thresh, unsigned long long* taken) {
  if (!(qmin <= thresh)) return 0;                       // :26, false positive by distance
  if ((*taken >> jmin) & 1ull) return 0;                 // :31, a second detection of the same gt
  *taken |= 1ull << jmin;
  return 1;
}
// ... and the whole step over q[0 .. ngt) (ngt >= 1) as the host runs it: the wavefront in k_eval.hip finds (qmin, jmin) across lanes
PBD_EV_HD int eval_match_step(const double* q, int ngt, double thresh, unsigned long long* taken) {
  int jmin = 0;
  for (int g = 1; g < ngt; ++g)
    if (q[g] < q[jmin]) jmin = g;                        // strict: the first index of the minimum stays (MATLAB's min)
  return eval_match_decide(q[jmin], jmin, thresh, taken);
}

// AP terms (eval_apk.m:38-41, VOCap.m).  tpc: true positives among the i + 1 best detections (i 0-based); fpc = (i + 1) - tpc.
PBD_EV_HD double eval_rec(int tpc, long long npos) { return (double)tpc / (double)npos; }
PBD_EV_HD double eval_prec(int tpc, int i) {
  const int fpc = (i + 1) - tpc;
  return (double)tpc / (double)(fpc + tpc);
}
// term k of VOCap's sum, k = 0 .. M: (mrec(k+1) - mrec(k)) * mpre(k+1) in 0-based terms of [0; rec; 1] and the suffix maximum of [0; prec; 0]
PBD_EV_HD double eval_ap_term(double rec_prev, double rec_cur, double mpre) { return (rec_cur - rec_prev) * mpre; }
// PCK hit (eval_pck.m:13): strict, the product rounded once
PBD_EV_HD int eval_pck_hit(double dist, double thresh, double scale) { return dist < thresh * scale; }
