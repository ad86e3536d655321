// pbd_augment_host.cpp — the definitions of include/pbd_c.h "virtual positives" as host code (no HIP: callable without a GPU, built with
// g++ like pbd_plan.cpp): map_rotate_points.m's geometry and point maps, the mirror of a keypoint set, and the image operation from
// augment_core.hpp's text, which k_augment.hip shares.
#include <cmath>
#include <cstddef>
#include <string>
#include <vector>
#include "augment_core.hpp"
#include "../../include/pbd_c.h"

static_assert(AUG_MAX_OPS == PBD_AUGMENT_MAX_OPS && AUG_MAX_SIDE == PBD_AUGMENT_MAX_SIDE, "augment_core.hpp and pbd_c.h disagree");
static_assert(sizeof(pbd_augment_op) == 24 && offsetof(pbd_augment_op, deg) == 8 && offsetof(pbd_augment_op, rotate) == 16, "pbd_augment_op layout");
static_assert(AUG_NEAREST == PBD_ROT_NEAREST && AUG_BILINEAR == PBD_ROT_BILINEAR, "augment_core.hpp and pbd_c.h disagree");

namespace {
thread_local std::string t_err;   // the calling thread's last refusal (pbd_augment_last_error)

// the geometry of one rotation, refused where the canvas is out of range: m, and the canvas as ints
int geometry(int w, int hgt, double deg, int* rows, int* cols, double m[6]) {
  if (w < 1 || hgt < 1) return aug_fail(PBD_ERR_ARG, "virtual positives: w / hgt below 1");
  if (!std::isfinite(deg)) return aug_fail(PBD_ERR_ARG, "virtual positives: deg is not finite");
  double r, c;
  aug_geometry(w, hgt, deg, &r, &c, m);
  if (!(r <= AUG_MAX_SIDE) || !(c <= AUG_MAX_SIDE))   // (a NaN from an overflowed angle lands here too)
    return aug_fail(PBD_ERR_UNSUPPORTED, "virtual positives: a side of the rotated canvas lies beyond 16384 pixels");
  *rows = (int)r; *cols = (int)c;
  return PBD_OK;
}
}  // namespace

int aug_fail(int code, const char* msg) {
  t_err = msg;
  return code;
}

int aug_check(const void* im, int w, int hgt, int cn, int stride, const pbd_augment_op* ops, int nops, const void* const* outs,
              const int* out_strides, AugDesc* desc) {
  if (!im || !ops || !outs || !out_strides) return aug_fail(PBD_ERR_ARG, "virtual positives: im / ops / outs / out_strides is NULL");
  if (cn != 1 && cn != 3) return aug_fail(PBD_ERR_ARG, "virtual positives: cn is neither 1 nor 3");
  if (w < 1 || hgt < 1) return aug_fail(PBD_ERR_ARG, "virtual positives: w / hgt below 1");
  if ((long long)stride < (long long)w * cn) return aug_fail(PBD_ERR_ARG, "virtual positives: stride below a row of the frame");
  if (nops < 1 || nops > AUG_MAX_OPS) return aug_fail(PBD_ERR_ARG, "virtual positives: nops outside 1..64");
  for (int i = 0; i < nops; ++i)
    if (!outs[i]) return aug_fail(PBD_ERR_ARG, "virtual positives: an output pointer is NULL");
  for (int i = 0; i < nops; ++i) {
    AugDesc d{};
    d.flip = ops[i].flip != 0; d.rotate = ops[i].rotate != 0; d.method = ops[i].method;
    d.rows = hgt; d.cols = w;
    if (d.rotate) {
      if (d.method != AUG_NEAREST && d.method != AUG_BILINEAR)
        return aug_fail(PBD_ERR_ARG, ("virtual positives: op " + std::to_string(i) + " has an unknown method").c_str());
      double m[6];
      const int rc = geometry(w, hgt, ops[i].deg, &d.rows, &d.cols, m);
      if (rc) return rc;
      d.c = m[0]; d.s = m[1]; d.hiA_r = m[2]; d.hiA_c = m[3]; d.hiB_r = m[4]; d.hiB_c = m[5];
    }
    if (w > AUG_MAX_SIDE || hgt > AUG_MAX_SIDE)
      return aug_fail(PBD_ERR_UNSUPPORTED, "virtual positives: a side of the canvas lies beyond 16384 pixels");
    if ((long long)out_strides[i] < (long long)d.cols * cn)
      return aug_fail(PBD_ERR_ARG, ("virtual positives: out_strides[" + std::to_string(i) + "] below a row of the canvas").c_str());
    desc[i] = d;
  }
  return PBD_OK;
}

#pragma GCC visibility push(default)
extern "C" {

const char* pbd_augment_last_error(void) { return t_err.c_str(); }

int pbd_rotate_geometry(int w, int hgt, double deg, int* out_w, int* out_h, double* m) {
  double mm[6];
  int rows, cols;
  const int rc = geometry(w, hgt, deg, &rows, &cols, mm);
  if (rc) return rc;
  if (out_w) *out_w = cols;
  if (out_h) *out_h = rows;
  if (m) for (int i = 0; i < 6; ++i) m[i] = mm[i];
  return PBD_OK;
}

int pbd_map_rotate_points(const double* pts, int n, int w, int hgt, double deg, int dir, double* out) {
  if (n < 0 || (n > 0 && (!pts || !out))) return aug_fail(PBD_ERR_ARG, "virtual positives: pts / out / n");
  if (dir != PBD_ROT_ORI2NEW && dir != PBD_ROT_NEW2ORI) return aug_fail(PBD_ERR_ARG, "virtual positives: dir is neither ORI2NEW nor NEW2ORI");
  double m[6];
  int rows, cols;
  const int rc = geometry(w, hgt, deg, &rows, &cols, m);
  if (rc) return rc;
  for (int i = 0; i < n; ++i) {   // :38  p = [y x]
    const double x = pts[2 * (size_t)i], y = pts[2 * (size_t)i + 1];
    double orow, ocol;
    if (dir == PBD_ROT_ORI2NEW) aug_ori2new(m, y, x, &orow, &ocol);
    else aug_new2ori(m, y, x, &orow, &ocol);
    out[2 * (size_t)i] = ocol; out[2 * (size_t)i + 1] = orow;
  }
  return PBD_OK;
}

int pbd_flip_points(const double* pts, int n, int w, const int32_t* mirror, double* out) {
  if (n < 0 || (n > 0 && (!pts || !out))) return aug_fail(PBD_ERR_ARG, "virtual positives: pts / out / n");
  if (w < 1) return aug_fail(PBD_ERR_ARG, "virtual positives: w below 1");
  if (mirror) {
    std::vector<char> seen((size_t)n, 0);
    for (int p = 0; p < n; ++p) {
      if (mirror[p] < 0 || mirror[p] >= n || seen[mirror[p]]) return aug_fail(PBD_ERR_ARG, "virtual positives: mirror is not a permutation of 0..n-1");
      seen[mirror[p]] = 1;
    }
  }
  const std::vector<double> in(pts, pts + 2 * (size_t)n);   // (out may be pts)
  for (int p = 0; p < n; ++p) {
    const size_t s = (size_t)(mirror ? mirror[p] : p);
    out[2 * (size_t)p] = (double)(w - 1) - in[2 * s];
    out[2 * (size_t)p + 1] = in[2 * s + 1];
  }
  return PBD_OK;
}

int pbd_augment_host_u8(const uint8_t* im, int w, int hgt, int cn, int stride, const pbd_augment_op* ops, int nops, uint8_t* const* outs,
                        const int* out_strides) {
  AugDesc desc[AUG_MAX_OPS];
  const int rc = aug_check(im, w, hgt, cn, stride, ops, nops, (const void* const*)outs, out_strides, desc);
  if (rc) return rc;
  for (int i = 0; i < nops; ++i) {
    const AugDesc& d = desc[i];
    for (int r = 0; r < d.rows; ++r) {
      uint8_t* row = outs[i] + (size_t)r * (size_t)out_strides[i];
      for (int q = 0; q < d.cols; ++q) aug_pixel(im, w, hgt, cn, (size_t)stride, d, r, q, row + (size_t)q * cn);
    }
  }
  return PBD_OK;
}

}  // extern "C"
#pragma GCC visibility pop
