// k_pyramid_mat.hip — the image pyramid of matlab/detection/featpyramid.m:24-34 (PBD_PYRAMID_MATLAB): level images in double, the
// first octave by the area resize of matlab/mex/resize.cc, every further octave by the 5-tap reduce of matlab/mex/reduce.cc.
// Bit-exact against the compiled reference files (tests/golden/ref_matpyr_v1.npz): every product and every sum below is an IEEE
// double operation of its own, in the reference's order.  Device code contracts a * b + c into one fused operation by default and
// one contraction changes a last bit.  The Makefile builds every file with -ffp-contract=off; the pragma below keeps this file's
// own expressions uncontracted also under the compiler's default mode (fast-honor-pragmas), and the arithmetic is written with
// plain operators, which the pragma governs.  (HIP's __dmul_rn / __dadd_rn are inline header functions around the same operators,
// compiled under the command line's mode: without -ffp-contract=off, __dadd_rn(t, __dmul_rn(a, b)) came out as one v_fmac_f64.
// An explicit -ffp-contract=fast ignores pragmas and breaks this file: 28 fused operations instead of none.)
//
// Both reference files run two 1-D passes, rows axis first, through a temporary image (resize.cc:100-102, reduce.cc:64-66).  The
// kernels fuse them: a thread produces one destination element and recomputes the few first-pass values it needs — a recomputed sum
// has the same bits.  The level images are interleaved and row-major like the 8-bit pyramid's (the reference's are planar and
// column-major: the arithmetic is per channel, the layout changes no value); consecutive lanes produce consecutive elements of a
// destination row.
#include <algorithm>
#include "pbd_internal.hpp"

#pragma clang fp contract(off)

// ---- area resize ------------------------------------------------------------------------------------------------------------
// out(dy, dx) = sum over the x taps of alpha_x * tmp(dy, sx), tmp(dy, sx) = sum over the y taps of alpha_y * src(sy, sx): alphacopy's
// `dst[di] += alpha * src[si]` (resize.cc:18-24) on zeroed memory (:69), the taps of a destination index in the order resize1dtran
// appended them (ascending source index).  The tap lists come from the planner (pbd_plan.cpp: resize_taps).
// One launch for all first-octave levels of all frames of a batch: blockIdx.y = job.  ST: the source's pixel type (8-bit frames;
// double images of the stand-alone entry); sstride: elements between source rows.
template <typename ST>
__global__ __launch_bounds__(256) void k_resize_area(const MatJob* __restrict__ jobs, const MatRun* __restrict__ runs,
                                                     const MatTap* __restrict__ taps, int cn, int sstride,
                                                     const uint8_t* __restrict__ src0, uint8_t* __restrict__ pyr) {
  const MatJob a = jobs[blockIdx.y];
  const ST* src = (const ST*)(src0 + a.soff);
  double* dst = (double*)(pyr + a.doff);
  const int rowe = a.dw * cn, n = rowe * a.dh;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int dy = i / rowe, xc = i - dy * rowe;
    const int dx = xc / cn, c = xc - dx * cn;
    const MatRun ry = runs[a.yrun0 + dy], rx = runs[a.xrun0 + dx];
    double acc = 0.0;
    for (int kx = 0; kx < rx.count; ++kx) {
      const MatTap tx = taps[rx.first + kx];
      const ST* col = src + tx.si * cn + c;
      double t = 0.0;
      for (int ky = 0; ky < ry.count; ++ky) {
        const MatTap ty = taps[ry.first + ky];
        t = t + ty.alpha * (double)col[(size_t)ty.si * sstride];
      }
      acc = acc + tx.alpha * t;
    }
    dst[i] = acc;
  }
}

// ---- reduce -----------------------------------------------------------------------------------------------------------------
// reduce1dtran (reduce.cc:11-45) for destination index d of an axis of slen source and dlen destination elements: the source
// indices and weights of its taps, in the order the reference's expression adds them.  dlen = round(slen / 2) >= 3 (slen >= 5), so
// the four forms address distinct rows and every index lies inside the source:
//   first row            s[0] .6875 + s[1] .25 + s[2] .0625                                               (:24)
//   rows 1 .. dlen - 3   s[c-2] .0625 + s[c-1] .25 + s[c] .375 + s[c+1] .25 + s[c+2] .0625, c = 2 d       (:29)
//   row dlen - 2         the same when dlen * 2 <= slen (:35-36), else s[c+1] .3125 + s[c] .375 + s[c-1] .25 + s[c-2] .0625  (:38)
//   last row             s[c] .6875 + s[c-1] .25 + s[c-2] .0625                                           (:42)
struct RedTaps { int n; int si[5]; double w[5]; };
__device__ __forceinline__ RedTaps reduce_taps(int d, int dlen, int slen) {
  RedTaps t;
  const int c = 2 * d;
  if (d == 0) {
    t.n = 3; t.si[0] = 0; t.si[1] = 1; t.si[2] = 2; t.w[0] = .6875; t.w[1] = .25; t.w[2] = .0625;
    t.si[3] = t.si[4] = 0; t.w[3] = t.w[4] = 0.0;
  } else if (d == dlen - 1) {
    t.n = 3; t.si[0] = c; t.si[1] = c - 1; t.si[2] = c - 2; t.w[0] = .6875; t.w[1] = .25; t.w[2] = .0625;
    t.si[3] = t.si[4] = 0; t.w[3] = t.w[4] = 0.0;
  } else if (d == dlen - 2 && dlen * 2 > slen) {
    t.n = 4; t.si[0] = c + 1; t.si[1] = c; t.si[2] = c - 1; t.si[3] = c - 2; t.w[0] = .3125; t.w[1] = .375; t.w[2] = .25; t.w[3] = .0625;
    t.si[4] = 0; t.w[4] = 0.0;
  } else {
    t.n = 5;
    t.si[0] = c - 2; t.si[1] = c - 1; t.si[2] = c; t.si[3] = c + 1; t.si[4] = c + 2;
    t.w[0] = .0625; t.w[1] = .25; t.w[2] = .375; t.w[3] = .25; t.w[4] = .0625;
  }
  return t;
}

// One launch per octave step: blockIdx.y = job (frame, level j <- level j - interval).  `*d = s[..] w + s[..] w + ...` (no zero in
// front: the first product starts the sum), rows pass then columns pass.
__global__ __launch_bounds__(256) void k_reduce_f64(const MatJob* __restrict__ jobs, int cn, uint8_t* __restrict__ pyr) {
  const MatJob a = jobs[blockIdx.y];
  const double* src = (const double*)(pyr + a.soff);
  double* dst = (double*)(pyr + a.doff);
  const int rowe = a.dw * cn, n = rowe * a.dh, srow = a.sw * cn;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int dy = i / rowe, xc = i - dy * rowe;
    const int dx = xc / cn, c = xc - dx * cn;
    const RedTaps ty = reduce_taps(dy, a.dh, a.sh), tx = reduce_taps(dx, a.dw, a.sw);
    double acc = 0.0;
#pragma unroll
    for (int kx = 0; kx < 5; ++kx) {
      if (kx < tx.n) {
        const double* col = src + tx.si[kx] * cn + c;
        double t = col[(size_t)ty.si[0] * srow] * ty.w[0];
#pragma unroll
        for (int ky = 1; ky < 5; ++ky)
          if (ky < ty.n) t = t + col[(size_t)ty.si[ky] * srow] * ty.w[ky];
        const double p = t * tx.w[kx];
        acc = kx == 0 ? p : acc + p;
      }
    }
    dst[i] = acc;
  }
}

static unsigned mat_blocks(long long elems) { return (unsigned)std::max<long long>(1, std::min<long long>((elems + 255) / 256, 65535)); }

// src_f64: the source pixels are doubles (the stand-alone entry), else 8-bit; sstride: source elements between rows
void launch_resize_area(const MatJob* jobs, int njobs, int maxpix, const MatRun* runs, const MatTap* taps, int cn, int sstride,
                        bool src_f64, const uint8_t* src, uint8_t* pyr, hipStream_t s) {
  if (njobs <= 0) return;
  dim3 grid(mat_blocks((long long)maxpix * cn), njobs);
  if (src_f64) hipLaunchKernelGGL(k_resize_area<double>, grid, dim3(256), 0, s, jobs, runs, taps, cn, sstride, src, pyr);
  else hipLaunchKernelGGL(k_resize_area<uint8_t>, grid, dim3(256), 0, s, jobs, runs, taps, cn, sstride, src, pyr);
}

void launch_reduce_f64(const MatJob* jobs, int njobs, int maxpix, int cn, uint8_t* pyr, hipStream_t s) {
  if (njobs <= 0) return;
  dim3 grid(mat_blocks((long long)maxpix * cn), njobs);
  hipLaunchKernelGGL(k_reduce_f64, grid, dim3(256), 0, s, jobs, cn, pyr);
}
