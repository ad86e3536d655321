// pbd_warp.cpp — the warped positives' planner (pbd_warp.hpp) and its two exported entries, and pbd_croppos (croppos.m).  Host-only, double arithmetic in the
// order include/pbd_c.h states; built with -ffp-contract=off.
#include <cmath>
#include "pbd_warp.hpp"
#include "../../include/pbd_c.h"

int warp_geometry(const double box[4], int kh, int kw, int sbin, WarpGeom* g) {
  if (!box || !g || kh < 1 || kw < 1 || sbin < 1) return PBD_ERR_ARG;
  const double x1 = box[0], y1 = box[1], x2 = box[2], y2 = box[3];
  if (!std::isfinite(x1) || !std::isfinite(y1) || !std::isfinite(x2) || !std::isfinite(y2) || x2 < x1 || y2 < y1) return PBD_ERR_ARG;
  const double lim = 1073741824.0;
  if (std::fabs(x1) > lim || std::fabs(y1) > lim || std::fabs(x2) > lim || std::fabs(y2) > lim) return PBD_ERR_UNSUPPORTED;
  const double padx = (double)sbin * (x2 - x1 + 1) / (double)(kw * sbin), pady = (double)sbin * (y2 - y1 + 1) / (double)(kh * sbin);
  const double X1 = std::round(x1 - padx), X2 = std::round(x2 + padx), Y1 = std::round(y1 - pady), Y2 = std::round(y2 + pady);
  if (X2 - X1 + 1 > PBD_WARP_MAX_SIDE || Y2 - Y1 + 1 > PBD_WARP_MAX_SIDE) return PBD_ERR_UNSUPPORTED;
  g->X1 = (int)X1; g->X2 = (int)X2; g->Y1 = (int)Y1; g->Y2 = (int)Y2;
  g->cw = g->X2 - g->X1 + 1; g->ch = g->Y2 - g->Y1 + 1;
  g->ow = (kw + 2) * sbin; g->oh = (kh + 2) * sbin;
  const double sy = (double)g->oh / (double)g->ch, sx = (double)g->ow / (double)g->cw;
  g->rows_first = sy <= sx ? 1 : 0;
  g->Py = warp_ntaps(g->ch, g->oh); g->Px = warp_ntaps(g->cw, g->ow);
  return PBD_OK;
}

int warp_ntaps(int n_in, int n_out) {
  const double s = (double)n_out / (double)n_in, width = s < 1 ? 2 / s : 2;
  return (int)std::ceil(width) + 2;
}

void warp_taps(int n_in, int n_out, std::vector<int32_t>& idx, std::vector<double>& wgt) {
  const double s = (double)n_out / (double)n_in, width = s < 1 ? 2 / s : 2;
  const int P = (int)std::ceil(width) + 2;
  idx.assign((size_t)n_out * P, 0); wgt.assign((size_t)n_out * P, 0.0);
  const long long period = 2LL * n_in;
  for (int x = 1; x <= n_out; ++x) {
    const double u = (double)x / s + 0.5 * (1 - 1 / s);
    const double left = std::floor(u - width / 2);
    double* w = &wgt[(size_t)(x - 1) * P];
    int32_t* ix = &idx[(size_t)(x - 1) * P];
    double sum = 0.0;
    for (int p = 0; p < P; ++p) {
      const double ind = left + (double)p;
      const double t = s < 1 ? s * (u - ind) : u - ind;
      const double tri = std::fmax(0.0, 1 - std::fabs(t));
      w[p] = s < 1 ? s * tri : tri;
      sum = sum + w[p];
      long long m = ((long long)ind - 1) % period;   // aux = [1 .. n_in, n_in .. 1], MATLAB's mirror
      if (m < 0) m += period;
      ix[p] = (int32_t)(m < n_in ? m : period - 1 - m);
    }
    for (int p = 0; p < P; ++p) w[p] = w[p] / sum;
  }
}

#pragma GCC visibility push(default)
extern "C" {

int pbd_warp_geometry(const double* box, int kh, int kw, int sbin, int32_t* rect, int32_t* rows_first, int32_t* py, int32_t* px) {
  WarpGeom g;
  const int rc = warp_geometry(box, kh, kw, sbin, &g);
  if (rc) return rc;
  if (rect) { rect[0] = g.X1; rect[1] = g.Y1; rect[2] = g.X2; rect[3] = g.Y2; }
  if (rows_first) *rows_first = g.rows_first;
  if (py) *py = g.Py;
  if (px) *px = g.Px;
  return PBD_OK;
}

int pbd_warp_taps(int n_in, int n_out, int32_t* index, double* weight, int capacity, int32_t* ntaps) {
  if (n_in < 1 || n_out < 1 || n_in > PBD_WARP_MAX_SIDE || n_out > PBD_WARP_MAX_SIDE || !ntaps || capacity < 0) return PBD_ERR_ARG;
  const int P = warp_ntaps(n_in, n_out);
  *ntaps = P;
  if (!index && !weight) return PBD_OK;
  if ((long long)capacity < (long long)n_out * P) return PBD_ERR_CAPACITY;
  std::vector<int32_t> idx; std::vector<double> w;
  warp_taps(n_in, n_out, idx, w);
  for (size_t i = 0; i < idx.size(); ++i) {
    if (index) index[i] = idx[i];
    if (weight) weight[i] = w[i];
  }
  return PBD_OK;
}

// croppos.m: the crop around a positive's part boxes, in MATLAB's 1-based terms, in double, with MATLAB's round (std::round: halves
// away from zero — pad is a multiple of 0.5, so halves occur, and round(a + 1) != round(a) + 1 for negative halves)
int pbd_croppos(const int32_t* truth, int nparts, int w, int hgt, int32_t roi[4], int32_t* truth_out) {
  if (!truth || !roi || nparts < 1 || w < 1 || hgt < 1) return PBD_ERR_ARG;
  double X1 = 0, Y1 = 0, X2 = 0, Y2 = 0;
  for (int p = 0; p < nparts; ++p) {
    const int32_t* t = truth + (size_t)p * 4;
    if (t[2] < 0 || t[3] < 0) return PBD_ERR_ARG;
    const double x1 = (double)t[0] + 1, y1 = (double)t[1] + 1, x2 = (double)t[0] + (double)t[2] + 1, y2 = (double)t[1] + (double)t[3] + 1;
    if (p == 0 || x1 < X1) X1 = x1;
    if (p == 0 || y1 < Y1) Y1 = y1;
    if (p == 0 || x2 > X2) X2 = x2;
    if (p == 0 || y2 > Y2) Y2 = y2;
  }
  const double pad = 0.5 * ((X2 - X1 + 1) + (Y2 - Y1 + 1));
  const double x1 = std::fmax(1.0, std::round(X1 - pad)), y1 = std::fmax(1.0, std::round(Y1 - pad));
  const double x2 = std::fmin((double)w, std::round(X2 + pad)), y2 = std::fmin((double)hgt, std::round(Y2 + pad));
  if (x2 < x1 || y2 < y1) return PBD_ERR_ARG;   // the truth lies wholly outside the frame: im(y1:y2, x1:x2, :) is empty
  roi[0] = (int32_t)x1 - 1; roi[1] = (int32_t)y1 - 1; roi[2] = (int32_t)(x2 - x1) + 1; roi[3] = (int32_t)(y2 - y1) + 1;
  if (truth_out)
    for (int p = 0; p < nparts; ++p) {
      const int32_t* t = truth + (size_t)p * 4;
      int32_t* o = truth_out + (size_t)p * 4;
      const int32_t tx = (int32_t)((int64_t)t[0] - roi[0]), ty = (int32_t)((int64_t)t[1] - roi[1]), tw = t[2], th = t[3];   // (truth_out may be truth itself)
      o[0] = tx; o[1] = ty; o[2] = tw; o[3] = th;
    }
  return PBD_OK;
}

}  // extern "C"
#pragma GCC visibility pop
