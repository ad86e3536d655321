// pbd_warp.hpp — the host-only planner of the warped positives (include/pbd_c.h "warped positives"): the crop rectangle of a box
// (warppos.m:21-27), the order of the two resamples and the per-axis tap tables of the stated contributions algorithm.  No HIP:
// compiles with plain g++; pbd_qp_warp.cpp uploads what it builds, and the weights the device multiplies by are these doubles.
#pragma once
#include <stdint.h>
#include <vector>

#define PBD_WARP_MAX_SIDE 16384   // pixels of a crop side (a larger one is PBD_ERR_UNSUPPORTED)

struct WarpGeom {
  int X1, Y1, X2, Y2;      // the crop rectangle, 1-based inclusive, before any clamp (may leave the image on every side)
  int cw, ch;              // its size
  int ow, oh;              // the window's: (kw + 2) * sbin, (kh + 2) * sbin
  int rows_first;          // 1: the y axis is resampled first (sy <= sx), 0: the x axis
  int Py, Px;              // taps per output row / column
};
// PBD_OK; PBD_ERR_ARG: non-finite or inverted box, kh / kw / sbin < 1; PBD_ERR_UNSUPPORTED: a crop side beyond PBD_WARP_MAX_SIDE or
// coordinates beyond +-2^30
int warp_geometry(const double box[4], int kh, int kw, int sbin, WarpGeom* g);
int warp_ntaps(int n_in, int n_out);   // P of an axis
// the taps of one axis, [n_out][P]: 0-based source index inside the crop (mirror resolved) and normalised weight
void warp_taps(int n_in, int n_out, std::vector<int32_t>& idx, std::vector<double>& wgt);
