// gt_overlap.hpp — the arithmetic of matlab/detection/bestoverlap.m (include/pbd_c.h "best pose per ground-truth box"), one text for
// the host function pbd_candidates_best_overlap (pbd_post.cpp) and for k_gtbox.hip.  Float64 throughout, the operations in the order
// the definition writes them; the units that include this are built with -ffp-contract=off, so nothing fuses.
#pragma once
#include <stdint.h>
#ifdef __HIPCC__
#define PBD_GT_HD __host__ __device__ __forceinline__
#else
#define PBD_GT_HD inline
#endif

struct GtCentreBox { double x1, y1, x2, y2; };   // bestoverlap.m:15-18: the box of a record's part centres

// rules 1-2: b = the record's boxes (x, y, w, h), np >= 1 parts.  int32 -> double and the halves are exact.
PBD_GT_HD GtCentreBox gt_centre_box(const int32_t* b, int np) {
  GtCentreBox c{0.0, 0.0, 0.0, 0.0};
  for (int p = 0; p < np; ++p) {
    const double x = (double)b[p * 4], y = (double)b[p * 4 + 1];
    const double x2 = x + (double)b[p * 4 + 2] - 1.0, y2 = y + (double)b[p * 4 + 3] - 1.0;
    const double cx = .5 * x + .5 * x2, cy = .5 * y + .5 * y2;   // :13-14
    if (p == 0) { c.x1 = c.x2 = cx; c.y1 = c.y2 = cy; continue; }
    c.x1 = cx < c.x1 ? cx : c.x1; c.x2 = cx > c.x2 ? cx : c.x2;
    c.y1 = cy < c.y1 ? cy : c.y1; c.y2 = cy > c.y2 ? cy : c.y2;
  }
  return c;
}

// rule 3: gt = (x1, y1, x2, y2), all finite.  0 / 0 is NaN (a gt box of area 0) and compares false.
PBD_GT_HD double gt_overlap(const double* gt, const GtCentreBox& c) {
  const double x1 = gt[0], y1 = gt[1], x2 = gt[2], y2 = gt[3];
  const double area = (x2 - x1 + 1.0) * (y2 - y1 + 1.0);          // :9
  const double xx1 = x1 > c.x1 ? x1 : c.x1, yy1 = y1 > c.y1 ? y1 : c.y1;   // :20-23
  const double xx2 = x2 < c.x2 ? x2 : c.x2, yy2 = y2 < c.y2 ? y2 : c.y2;
  double w = xx2 - xx1 + 1.0, h = yy2 - yy1 + 1.0;                // :25-26
  if (w < 0.0) w = 0.0;
  if (h < 0.0) h = 0.0;
  const double inter = w * h;                                     // :27
  return inter / area;                                            // :28
}

// rule 5's order on scores as an unsigned integer: a larger float is a larger key, -0.0 and +0.0 share one
PBD_GT_HD unsigned gt_score_key(float s) {
  union { float f; unsigned u; } v;
  v.f = s;
  if (v.u == 0x80000000u) v.u = 0u;
  return (v.u & 0x80000000u) ? ~v.u : (v.u | 0x80000000u);
}
