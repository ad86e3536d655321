// pbd_qp_warp.cpp — the warped positives' host side (include/pbd_c.h "warped positives"; planner: pbd_warp.cpp, kernels: k_warp.hip,
// k_hog.hip, k_qp.hip): the frame's upload (or the copy of its rows from device memory), the job and tap tables of the boxes, the three
// launches, and the entry points pbd_warp_windows_u8[_f64], pbd_qp_write_warped_u8 and pbd_qp_write_warped_dev_u8.
#include <algorithm>
#include <cmath>
#include "pbd_qp.hpp"
#include "pbd_warp.hpp"

namespace {
using namespace pbd_qp_detail;

#define WARP_CHUNK_DOUBLES ((size_t)1 << 25)   // intermediates of one pair of launches (256 MB)
#define WARP_CHUNK_TAPS ((size_t)1 << 23)      // taps of one pair of launches (128 MB)
#define WARP_CHUNK_JOBS 32768

// one launch group between two events, while pbd_set_profiling is on (pbd_debug_warp_ms)
struct EvTimer {
  hipEvent_t a = nullptr, b = nullptr;
  bool on;
  EvTimer(bool on_, hipStream_t s) : on(on_) { if (on) { on = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess; if (on) hipEventRecord(a, s); } }
  void stop(hipStream_t s) { if (on) hipEventRecord(b, s); }
  float ms() { float v = 0.f; if (on && hipEventElapsedTime(&v, a, b) != hipSuccess) v = 0.f; return v; }   // (after the stream is idle)
  ~EvTimer() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
};

// k_hog's tile side for windows of double pixels, the frame planner's rule (pbd_plan.cpp); 0: the cell size does not fit LDS
int hog_tile_side(int sbin, int ts) {
  int tc = 16;
  while (tc > 2 && hog_lds_bytes(sbin, tc, ts, 24) > 150 * 1024) tc /= 2;
  return hog_lds_bytes(sbin, tc, ts, 24) > 150 * 1024 ? 0 : tc;
}

const char* const kWhat = "warped positives: ";

struct WarpCall {
  int kh = 0, kw = 0, ow = 0, oh = 0;
  std::vector<WarpGeom> g;          // [n] every box of the call
  hipMemcpyKind kind = hipMemcpyHostToDevice;   // where the frame's rows are copied from (pbd_qp_write_warped_dev_u8: the device)
  CallScratch mem;                  // the call's frame, windows and features
  char *img = nullptr, *win = nullptr, *feat = nullptr;
  explicit WarpCall(pbd_handle* h) : mem(h) {}
};

// every refusal of the two entries' shared arguments, and the boxes' geometry: nothing touches the device
int warp_check(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, const double* boxes, int n, int filter, WarpCall* c) {
  if (!im || w < 1 || hgt < 1 || (cn != 1 && cn != 3) || stride < w * cn) return fail(h, PBD_ERR_ARG, "warped positives: im / w / hgt / cn / stride");
  if (n < 0 || (n > 0 && !boxes)) return fail(h, PBD_ERR_ARG, "warped positives: boxes / n");
  if ((long long)stride * hgt >= (1ll << 31)) return fail(h, PBD_ERR_UNSUPPORTED, "warped positives: the frame has 2^31 bytes or more");
  if (h->in_group) return fail(h, PBD_ERR_UNSUPPORTED, "warped positives: pbd_group members are not supported");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  if (filter < 0 || filter >= h->md.nfilters) return fail(h, PBD_ERR_ARG, "warped positives: filter outside [0, nfilters)");
  int32_t kh, kw;
  pbd_get_filter_size(h, filter, &kh, &kw);
  const int sbin = h->md.sbin;
  c->kh = kh; c->kw = kw; c->ow = (kw + 2) * sbin; c->oh = (kh + 2) * sbin;
  if ((long long)c->ow * 3 * PBD_WARP_MAX_SIDE >= (1ll << 31) || (long long)c->oh * 3 * PBD_WARP_MAX_SIDE >= (1ll << 31))
    return fail(h, PBD_ERR_UNSUPPORTED, "warped positives: the window is too large");
  if (!hog_tile_side(sbin, h->ts)) return fail(h, PBD_ERR_UNSUPPORTED, "sbin too large");
  c->g.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    const int rc = warp_geometry(boxes + 4 * (size_t)i, kh, kw, sbin, &c->g[i]);
    if (rc == PBD_ERR_ARG) return fail(h, rc, "warped positives: box " + std::to_string(i) + " is not finite or is inverted (x2 < x1 or y2 < y1)");
    if (rc) return fail(h, rc, "warped positives: the crop of box " + std::to_string(i) + " has a side beyond " + std::to_string(PBD_WARP_MAX_SIDE) +
                                " pixels (or coordinates beyond 2^30)");
  }
  return PBD_OK;
}

// the windows (T-independent doubles, [m][oh][ow][3]) and their features (T [m][kh][kw][flen]) of the boxes sel[0 .. m - 1], left in
// c->win / c->feat; the stream is idle when this returns
int warp_run(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, const std::vector<int>& sel, WarpCall* c) {
  const int m = (int)sel.size(), ow = c->ow, oh = c->oh, kh = c->kh, kw = c->kw, sbin = h->md.sbin;
  h->warp_ms[0] = h->warp_ms[1] = h->warp_ms[2] = 0.f;
  if (m == 0) return PBD_OK;
  const size_t rowb = (size_t)w * cn, nwin = (size_t)ow * oh * 3, wlen = (size_t)kh * kw * PBD_FLEN;
  int rc;
  if ((rc = c->mem.get(&c->img, rowb * hgt, kWhat)) || (rc = c->mem.get(&c->win, sizeof(double) * nwin * m, kWhat)) ||
      (rc = c->mem.get(&c->feat, (size_t)h->ts * wlen * m, kWhat)))
    return rc;
  if ((rc = copy_rows(h, c->img, im, (size_t)stride, rowb, (size_t)hgt, c->kind))) return rc;
  WarpArgs a{};
  a.im = (const uint8_t*)c->img; a.w = w; a.h = hgt; a.cn = cn; a.stride = rowb;
  a.win = (double*)c->win; a.ow = ow; a.oh = oh;
  std::vector<WarpJob> jobs;
  std::vector<MatTap> taps;
  std::vector<int32_t> ix; std::vector<double> wv;
  auto table = [&](int n_in, int n_out) {   // the planner's [n_out][P] taps appended tap-major
    warp_taps(n_in, n_out, ix, wv);
    const int P = (int)(ix.size() / (size_t)n_out);
    const size_t t0 = taps.size();
    taps.resize(t0 + ix.size());
    for (int x = 0; x < n_out; ++x)
      for (int p = 0; p < P; ++p) taps[t0 + (size_t)p * n_out + x] = MatTap{wv[(size_t)x * P + p], ix[(size_t)x * P + p], 0};
    return (unsigned long long)t0;
  };
  for (int i0 = 0; i0 < m;) {   // a chunk: as many boxes as the scratch, tap and job limits take, at least one
    jobs.clear(); taps.clear();
    size_t scr = 0; unsigned max_first = 0;
    int i = i0;
    for (; i < m; ++i) {
      const WarpGeom& g = c->g[sel[i]];
      const size_t first = g.rows_first ? (size_t)oh * g.cw * 3 : (size_t)g.ch * ow * 3;
      const size_t nt = (size_t)oh * g.Py + (size_t)ow * g.Px;
      if (i > i0 && (scr + first > WARP_CHUNK_DOUBLES || taps.size() + nt > WARP_CHUNK_TAPS || i - i0 >= WARP_CHUNK_JOBS)) break;
      WarpJob j{};
      j.scr_off = scr; j.win_off = (unsigned long long)i * nwin;
      j.ytap = table(g.ch, oh); j.xtap = table(g.cw, ow);
      j.X0 = g.X1 - 1; j.Y0 = g.Y1 - 1; j.cw = g.cw; j.ch = g.ch;
      j.Py = g.Py; j.Px = g.Px; j.rows_first = g.rows_first;
      jobs.push_back(j);
      scr += first; max_first = std::max(max_first, (unsigned)first);
    }
    CallScratch chunk(h);
    double* d_scr; char* d_tab;
    const size_t jb = sizeof(WarpJob) * jobs.size();
    if ((rc = chunk.get(&d_scr, scr, kWhat)) || (rc = chunk.get(&d_tab, jb + sizeof(MatTap) * taps.size(), kWhat))) return rc;
    HIPCHK(h, hipMemcpyAsync(d_tab, jobs.data(), jb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_tab + jb, taps.data(), sizeof(MatTap) * taps.size(), hipMemcpyHostToDevice, h->stream));
    a.jobs = (const WarpJob*)d_tab; a.taps = (const MatTap*)(d_tab + jb); a.scratch = d_scr;
    EvTimer tm(h->profiling, h->stream);
    launch_warp(a, (int)jobs.size(), max_first, h->stream);
    tm.stop(h->stream);
    LAUNCHCHK(h, "warped positives");
    if ((rc = finish(h, "warped positives: "))) return rc;   // (the tables are pageable and the chunk's buffers go: the launches are done)
    h->warp_ms[0] += tm.ms();
    i0 = i;
  }
  // features(window, sbin): k_hog over the windows as level images of PBD_DEPTH_64F, one level per window
  const int tc = hog_tile_side(sbin, h->ts);
  std::vector<LevelDev> lv((size_t)m);
  std::vector<HogTile> tiles;
  for (int i = 0; i < m; ++i) {
    lv[i] = LevelDev{ow, oh, kw + 2, kh + 2, kw, kh, (unsigned long long)i * nwin * sizeof(double), (unsigned long long)i * kh * kw};
    for (int y = 0; y < kh; y += tc) for (int x = 0; x < kw; x += tc) tiles.push_back(HogTile{i, y, x, 0});
  }
  CallScratch t_hog(h);
  char* d_hog;
  const size_t lb = sizeof(LevelDev) * lv.size();
  if ((rc = t_hog.get(&d_hog, lb + sizeof(HogTile) * tiles.size(), kWhat))) return rc;
  HIPCHK(h, hipMemcpyAsync(d_hog, lv.data(), lb, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_hog + lb, tiles.data(), sizeof(HogTile) * tiles.size(), hipMemcpyHostToDevice, h->stream));
  EvTimer tm(h->profiling, h->stream);
  launch_hog((const HogTile*)(d_hog + lb), (int)tiles.size(), (const LevelDev*)d_hog, (const uint8_t*)c->win, c->feat, h->ts, 3, sbin,
             tc, h->d_hog_lut, nullptr, 0, PBD_DEPTH_64F, h->stream);
  tm.stop(h->stream);
  LAUNCHCHK(h, "warped positives: features");
  if ((rc = finish(h, "warped positives: "))) return rc;
  h->warp_ms[1] = tm.ms();
  return PBD_OK;
}

int warp_windows_(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, const double* boxes, int n, int filter,
                  double* windows, void* features, int ts) {
  if (!h) return PBD_ERR_ARG;
  if (h->ts != ts) return fail(h, PBD_ERR_STATE, ts == 4 ? "handle is PartsBasedDetector<double>: use the _f64 entry point"
                                                         : "handle is PartsBasedDetector<float>: use the float entry point");
  WarpCall c(h);
  int rc = warp_check(h, im, w, hgt, cn, stride, boxes, n, filter, &c);
  if (rc || n == 0) return rc;
  ON_DEVICE(h);
  std::vector<int> sel((size_t)n);
  for (int i = 0; i < n; ++i) sel[i] = i;
  if ((rc = warp_run(h, im, w, hgt, cn, stride, sel, &c))) return rc;
  if (windows) HIPCHK(h, hipMemcpyAsync(windows, c.win, sizeof(double) * c.ow * c.oh * 3 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  if (features) HIPCHK(h, hipMemcpyAsync(features, c.feat, (size_t)ts * c.kh * c.kw * PBD_FLEN * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  return finish(h, "warped positives: ");
}

int write_warped_(pbd_qp* q, const uint8_t* im, int w, int hgt, int cn, int stride, const double* boxes, const int32_t* ids, int n,
                  int filter, int bias, double min_area, int32_t* status, int* written, hipMemcpyKind kind) {
  if (!q) return PBD_ERR_ARG;
  pbd_handle* h = q->h;
  if (!written) return fail(h, PBD_ERR_ARG, "example cache: written is NULL");
  WarpCall c(h);
  c.kind = kind;
  int rc = warp_check(h, im, w, hgt, cn, stride, boxes, n, filter, &c);
  if (rc) return rc;
  if (bias < 0 || bias >= (int)h->biasw.size()) return fail(h, PBD_ERR_ARG, "warped positives: bias outside [0, nbias)");
  if (std::isnan(min_area)) return fail(h, PBD_ERR_ARG, "warped positives: min_area is not a number");
  const int wlen = c.kh * c.kw * PBD_FLEN;
  if (6 + wlen > q->dev.k) return fail(h, PBD_ERR_UNSUPPORTED, "warped positives: the filter's window does not fit the cache's column length");
  // (the two blocks cannot repeat a dense start, qp_write.m:34-35: the bias block starts below nbias, every filter at or above it)
  *written = 0;
  // train.m:139-143: small boxes are skipped; then the first min(count, capacity - n) are written (qp_write.m:21-23)
  const int room = q->dev.capacity - q->n;
  std::vector<int> sel;
  for (int i = 0; i < n; ++i) {
    const double* b = boxes + 4 * (size_t)i;
    int st = PBD_WARP_WRITTEN;
    if ((b[2] - b[0] + 1) * (b[3] - b[1] + 1) < min_area) st = PBD_WARP_SKIPPED;
    else if ((int)sel.size() >= room) st = PBD_WARP_FULL;
    else sel.push_back(i);
    if (status) status[i] = st;
  }
  const int m = (int)sel.size();
  if (m == 0) return PBD_OK;   // (nothing to write: nothing is uploaded)
  ON_DEVICE(h);
  if ((rc = warp_run(h, im, w, hgt, cn, stride, sel, &c))) return rc;
  std::vector<int> idv((size_t)m);
  for (int i = 0; i < m; ++i) idv[i] = ids ? ids[sel[i]] : sel[i];
  int* d_ids;
  if ((rc = c.mem.get(&d_ids, (size_t)m, kWhat))) return rc;
  HIPCHK(h, hipMemcpyAsync(d_ids, idv.data(), sizeof(int) * (size_t)m, hipMemcpyHostToDevice, h->stream));
  QpPosArgs a{};
  a.q = q->dev; a.n0 = q->n; a.n = m;
  a.feat = c.feat; a.ids = d_ids;
  a.wreg = q->d_wreg; a.w0 = q->d_w0;
  a.bias_start = bias; a.filt_start = q->foff[filter]; a.wlen = wlen;
  a.C = q->cpos;
  EvTimer tm(h->profiling, h->stream);
  launch_qp_poswrite(a, h->ts, h->stream);
  tm.stop(h->stream);
  LAUNCHCHK(h, "warped positives: write");
  if ((rc = finish(h, "warped positives: "))) return rc;
  h->warp_ms[2] = tm.ms();
  for (int i = 0; i < m; ++i) q->overlap[q->slot[q->n + i]] = 0;
  q->meta_dirty = true;
  if ((rc = pbd_i_qp_appended(q, q->n, m))) return rc;
  q->n += m;
  *written = m;
  return PBD_OK;
}
}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int pbd_warp_windows_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, const double* boxes, int n, int filter,
                        double* windows, float* features) {
  return warp_windows_(h, im, w, hgt, cn, stride, boxes, n, filter, windows, features, 4);
}
int pbd_warp_windows_u8_f64(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, const double* boxes, int n, int filter,
                            double* windows, double* features) {
  return warp_windows_(h, im, w, hgt, cn, stride, boxes, n, filter, windows, features, 8);
}

int pbd_debug_warp_ms(const pbd_handle* h, float ms[3]) {
  if (!h || !ms) return PBD_ERR_ARG;
  for (int i = 0; i < 3; ++i) ms[i] = h->warp_ms[i];
  return PBD_OK;
}

int pbd_qp_write_warped_u8(pbd_qp* q, const uint8_t* im, int w, int hgt, int cn, int stride, const double* boxes, const int32_t* ids, int n,
                           int filter, int bias, double min_area, int32_t* status, int* written) {
  return write_warped_(q, im, w, hgt, cn, stride, boxes, ids, n, filter, bias, min_area, status, written, hipMemcpyHostToDevice);
}
// the frame already in device memory: the upload is a device-to-device copy of the same rows, everything else is the call above
int pbd_qp_write_warped_dev_u8(pbd_qp* q, const void* d_im, int w, int hgt, int cn, int stride, const double* boxes, const int32_t* ids, int n,
                               int filter, int bias, double min_area, int32_t* status, int* written) {
  return write_warped_(q, (const uint8_t*)d_im, w, hgt, cn, stride, boxes, ids, n, filter, bias, min_area, status, written,
                       hipMemcpyDeviceToDevice);
}

}  // extern "C"
#pragma GCC visibility pop
