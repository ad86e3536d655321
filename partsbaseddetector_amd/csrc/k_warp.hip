// k_warp.hip — the warped positives' windows (include/pbd_c.h "warped positives"): warppos.m's crop with replicated border and
// imresize(window, cropsize, 'bilinear') as two resampling passes over (box, output tile).  gfx950 only.
//
// k_warp_first resamples the first axis of a job straight from the 8-bit frame — the crop is an index clamp inside its reads, never
// a buffer — into the job's intermediate in HBM (double): a crop may be thousands of pixels a side, far beyond LDS.  k_warp_second
// resamples the other axis into the window.  One thread per output element, threads along the contiguous axis ([x][channel]), so
// the frame reads, the intermediate's reads and stores and the window's stores coalesce; the tap tables are tap-major and go through
// L2 (a row's taps are uniform over the wavefront when the pass runs along y).  An element is the sum over ALL P taps in ascending
// order, each product rounded (__dmul_rn), added to +0.0 (__dadd_rn): the weights were computed once on the host (pbd_warp.cpp), so
// the result is the numpy restatement's bit for bit and does not depend on the grid or on the box's position in the call.
#include "pbd_internal.hpp"

#define WARP_NT 256

__global__ void __launch_bounds__(WARP_NT) k_warp_first(WarpArgs a) {
  const WarpJob j = a.jobs[blockIdx.y];
  const unsigned rowlen = (unsigned)(j.rows_first ? j.cw : a.ow) * 3u, nrows = (unsigned)(j.rows_first ? a.oh : j.ch);
  const unsigned t = blockIdx.x * WARP_NT + threadIdx.x;
  if (t >= rowlen * nrows) return;   // (rowlen * nrows <= 3 * PBD_WARP_MAX_SIDE * ow < 2^32: checked by the host)
  const unsigned r = t / rowlen, e = t - r * rowlen, q = e / 3u;
  const int c = a.cn == 3 ? (int)(e - q * 3u) : 0;   // a grey frame is replicated to three planes (warppos.m:18-20)
  double acc = 0.0;
  if (j.rows_first) {
    const int sx = min(max(j.X0 + (int)q, 0), a.w - 1);
    const uint8_t* col = a.im + (size_t)sx * a.cn + c;
    const MatTap* tp = a.taps + j.ytap + r;
    for (int p = 0; p < j.Py; ++p) {
      const MatTap tap = tp[(size_t)p * a.oh];
      const int sy = min(max(j.Y0 + tap.si, 0), a.h - 1);
      acc = __dadd_rn(acc, __dmul_rn(tap.alpha, (double)col[(size_t)sy * a.stride]));
    }
  } else {
    const int sy = min(max(j.Y0 + (int)r, 0), a.h - 1);
    const uint8_t* row = a.im + (size_t)sy * a.stride + c;
    const MatTap* tp = a.taps + j.xtap + q;
    for (int p = 0; p < j.Px; ++p) {
      const MatTap tap = tp[(size_t)p * a.ow];
      const int sx = min(max(j.X0 + tap.si, 0), a.w - 1);
      acc = __dadd_rn(acc, __dmul_rn(tap.alpha, (double)row[(size_t)sx * a.cn]));
    }
  }
  a.scratch[j.scr_off + t] = acc;
}

__global__ void __launch_bounds__(WARP_NT) k_warp_second(WarpArgs a) {
  const WarpJob j = a.jobs[blockIdx.y];
  const unsigned rowlen = (unsigned)a.ow * 3u;
  const unsigned t = blockIdx.x * WARP_NT + threadIdx.x;
  if (t >= rowlen * (unsigned)a.oh) return;
  const unsigned oy = t / rowlen, e = t - oy * rowlen, ox = e / 3u, c = e - ox * 3u;
  const double* s = a.scratch + j.scr_off;
  double acc = 0.0;
  if (j.rows_first) {                                  // the intermediate is [oh][cw][3]: the x axis
    const double* row = s + (size_t)oy * j.cw * 3 + c;
    const MatTap* tp = a.taps + j.xtap + ox;
    for (int p = 0; p < j.Px; ++p) {
      const MatTap tap = tp[(size_t)p * a.ow];
      acc = __dadd_rn(acc, __dmul_rn(tap.alpha, row[(size_t)tap.si * 3]));
    }
  } else {                                             // [ch][ow][3]: the y axis
    const double* col = s + e;
    const MatTap* tp = a.taps + j.ytap + oy;
    for (int p = 0; p < j.Py; ++p) {
      const MatTap tap = tp[(size_t)p * a.oh];
      acc = __dadd_rn(acc, __dmul_rn(tap.alpha, col[(size_t)tap.si * rowlen]));
    }
  }
  a.win[j.win_off + t] = acc;
}

void launch_warp(const WarpArgs& a, int njobs, unsigned max_first, hipStream_t s) {
  if (njobs <= 0) return;
  const unsigned nwin = (unsigned)a.ow * a.oh * 3u;
  hipLaunchKernelGGL(k_warp_first, dim3((max_first + WARP_NT - 1) / WARP_NT, njobs), dim3(WARP_NT), 0, s, a);
  hipLaunchKernelGGL(k_warp_second, dim3((nwin + WARP_NT - 1) / WARP_NT, njobs), dim3(WARP_NT), 0, s, a);
}
