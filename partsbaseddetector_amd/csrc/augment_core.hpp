// augment_core.hpp — virtual positives (include/pbd_c.h "virtual positives"): matlab/learning/map_rotate_points.m:21-46 and the image
// operation that belongs to it, one text for the host functions (pbd_augment_host.cpp) and for k_augment.hip.  Float64 throughout, every
// operation one IEEE operation in the order written; the units that include this are built with -ffp-contract=off, so nothing fuses.
// The device never evaluates a trigonometric function: aug_geometry runs once, on the host, and the device multiplies by its numbers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#ifdef __HIPCC__
#define PBD_AUG_HD __host__ __device__ __forceinline__
#else
#define PBD_AUG_HD inline
#endif

#define AUG_MAX_OPS 64        // PBD_AUGMENT_MAX_OPS
#define AUG_MAX_SIDE 16384    // PBD_AUGMENT_MAX_SIDE
#define AUG_NEAREST 0         // PBD_ROT_NEAREST
#define AUG_BILINEAR 1        // PBD_ROT_BILINEAR
#define AUG_TILE_W 64         // a workgroup of k_augment.hip: one wavefront per output row of a 64 x 4 tile
#define AUG_TILE_H 4

// one op of a frame as the kernel and the host loop read it: wave-uniform
struct AugDesc {
  double c, s, hiA_r, hiA_c, hiB_r, hiB_c;   // pbd_rotate_geometry's m[6]
  uint8_t* out;                              // canvas row r at out + r * out_stride
  unsigned long long out_stride;
  int rows, cols;                            // the canvas
  int flip, method, rotate, pad;
};

// map_rotate_points.m:21-35 as the file computes it; rows / cols as doubles (the caller bounds them before narrowing)
inline void aug_geometry(int w, int hgt, double deg, double* rows, double* cols, double m[6]) {
  const double phi = (deg * 3.141592653589793) / 180.0;   // :21  ang*pi/180, left to right
  const double c = cos(phi), s = sin(phi);
  const double hiA_r = (double)(hgt - 1) / 2.0, hiA_c = (double)(w - 1) / 2.0;   // :31
  const double loA_r = -hiA_r;
  // :34  tformfwd([loA(1) hiA(2); hiA(1) hiA(2)], rotate): (u, v) -> (u*c - v*s, u*s + v*c)
  const double r0 = fabs(loA_r * c - hiA_c * s), r1 = fabs(hiA_r * c - hiA_c * s);
  const double c0 = fabs(loA_r * s + hiA_c * c), c1 = fabs(hiA_r * s + hiA_c * c);
  const double hiB_r = ceil((r0 > r1 ? r0 : r1) / 2.0) * 2.0, hiB_c = ceil((c0 > c1 ? c0 : c1) / 2.0) * 2.0;
  m[0] = c; m[1] = s; m[2] = hiA_r; m[3] = hiA_c; m[4] = hiB_r; m[5] = hiB_c;
  *rows = 2.0 * hiB_r + 1.0;
  *cols = 2.0 * hiB_c + 1.0;
}

// :40  tformfwd(p + loA, rotate) - loB on a (row, col) pair
PBD_AUG_HD void aug_ori2new(const double m[6], double row, double col, double* orow, double* ocol) {
  const double u = row - m[2], v = col - m[3];
  *orow = (u * m[0] - v * m[1]) + m[4];
  *ocol = (u * m[1] + v * m[0]) + m[5];
}
// :42  tforminv(p + loB, rotate) - loA, the inverse taken as the transpose
PBD_AUG_HD void aug_new2ori(const double m[6], double row, double col, double* orow, double* ocol) {
  const double u = row - m[4], v = col - m[5];
  *orow = (u * m[0] + v * m[1]) + m[2];
  *ocol = (v * m[0] - u * m[1]) + m[3];
}

// pixel (y, x) of the mirrored (or plain) source, channel ch; outside: 0
PBD_AUG_HD int aug_tap(const uint8_t* im, int w, int hgt, int cn, size_t stride, int flip, long long y, long long x, int ch) {
  if (y < 0 || y >= hgt || x < 0 || x >= w) return 0;
  const size_t sx = (size_t)(flip ? w - 1 - x : x);
  return im[(size_t)y * stride + sx * (size_t)cn + (size_t)ch];
}

// output pixel (r, q) of op d, all its CN channels, into px[CN] (CN a constant: the channel loops unroll, px stays in registers)
template <int cn> PBD_AUG_HD void aug_pixel_n(const uint8_t* im, int w, int hgt, size_t stride, const AugDesc& d, int r, int q, uint8_t* px) {
  if (!d.rotate) {
    for (int ch = 0; ch < cn; ++ch) px[ch] = (uint8_t)aug_tap(im, w, hgt, cn, stride, d.flip, r, q, ch);
    return;
  }
  const double m[6] = {d.c, d.s, d.hiA_r, d.hiA_c, d.hiB_r, d.hiB_c};
  double sr, sc;
  aug_new2ori(m, (double)r, (double)q, &sr, &sc);
  if (d.method == AUG_NEAREST) {
    const long long y = (long long)floor(sr + 0.5), x = (long long)floor(sc + 0.5);
    for (int ch = 0; ch < cn; ++ch) px[ch] = (uint8_t)aug_tap(im, w, hgt, cn, stride, d.flip, y, x, ch);
    return;
  }
  const double fy0 = floor(sr), fx0 = floor(sc);
  const double fy = sr - fy0, fx = sc - fx0;
  const long long y0 = (long long)fy0, x0 = (long long)fx0;
  for (int ch = 0; ch < cn; ++ch) {
    const double a00 = (double)aug_tap(im, w, hgt, cn, stride, d.flip, y0, x0, ch);
    const double a01 = (double)aug_tap(im, w, hgt, cn, stride, d.flip, y0, x0 + 1, ch);
    const double a10 = (double)aug_tap(im, w, hgt, cn, stride, d.flip, y0 + 1, x0, ch);
    const double a11 = (double)aug_tap(im, w, hgt, cn, stride, d.flip, y0 + 1, x0 + 1, ch);
    const double v = (1.0 - fy) * ((1.0 - fx) * a00 + fx * a01) + fy * ((1.0 - fx) * a10 + fx * a11);
    const double b = floor(v + 0.5);
    px[ch] = (uint8_t)(b < 255.0 ? b : 255.0);
  }
}
PBD_AUG_HD void aug_pixel(const uint8_t* im, int w, int hgt, int cn, size_t stride, const AugDesc& d, int r, int q, uint8_t* px) {
  if (cn == 3) aug_pixel_n<3>(im, w, hgt, stride, d, r, q, px);
  else aug_pixel_n<1>(im, w, hgt, stride, d, r, q, px);
}

// pbd_augment_host.cpp: every refusal of the three image entries, before anything is read, written or uploaded; on PBD_OK desc[nops]
// holds the ops' canvases and numbers (out and out_stride are the caller's to fill).  The message of a refusal: aug_fail.
struct pbd_augment_op;
int aug_check(const void* im, int w, int hgt, int cn, int stride, const pbd_augment_op* ops, int nops, const void* const* outs,
              const int* out_strides, AugDesc* desc);
int aug_fail(int code, const char* msg);
