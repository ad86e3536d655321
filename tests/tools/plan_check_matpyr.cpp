// plan_check_matpyr.cpp — the host planner under PBD_PYRAMID_MATLAB (pbd_set_pyramid_kind: HostModel::pyr_kind), no GPU: hands out
// the geometry and the area resize's tap lists as the planner computes them (tests/test_matlab_pyramid_cpu.py compares them with the
// numpy restatement), and plans a whole frame to check what the kernels of k_pyramid_mat.hip will address: every job's source and
// destination inside their buffers, every run and tap index inside its table, every tap's source index inside the source image.
// Built by the test with pbd_plan.cpp.
#include <cstdio>
#include <string>
#include <vector>
#include "pbd_plan.hpp"

extern "C" int matpyr_geometry(int w, int h, int sbin, int interval, int* nlevels, int32_t* iw, int32_t* ih, int32_t* cw, int32_t* ch,
                               float* scales) {
  std::vector<Level> lv((size_t)PBD_MAX_LEVELS, Level{});
  int n = 0;
  if (compute_geometry_matlab(w, h, sbin, interval, &n, lv.data())) return -1;
  *nlevels = n;
  for (int l = 0; l < n; ++l) { iw[l] = lv[l].iw; ih[l] = lv[l].ih; cw[l] = lv[l].cw; ch[l] = lv[l].ch; scales[l] = lv[l].scale; }
  return 0;
}

// one axis: first / count [dlen], si / alpha [cap]; returns the number of taps, or -1 (capacity, or a tap outside the source)
extern "C" int matpyr_taps(int slen, int dlen, int32_t* first, int32_t* count, int32_t* si, double* alpha, int cap) {
  std::vector<MatRun> runs; std::vector<MatTap> taps;
  if (!resize_taps(slen, dlen, runs, taps) || (int)taps.size() > cap || (int)runs.size() != dlen) return -1;
  for (int d = 0; d < dlen; ++d) { first[d] = runs[d].first; count[d] = runs[d].count; }
  for (size_t t = 0; t < taps.size(); ++t) { si[t] = taps[t].si; alpha[t] = taps[t].alpha; }
  return (int)taps.size();
}

// plans one frame geometry with HostModel::pyr_kind = kind; out[0..5] = level-image bytes, frame-buffer bytes, level element size,
// source element size, pyramid jobs, pyramid launches.  PBD_OK, the planner's error code, or 100 with the failed checks in `report`
extern "C" int matpyr_plan(const pbd_model_desc* md, const pbd_options* opt, int w, int h, int cn, int batch, int depth, int kind, int pad,
                           unsigned long long* out, char* report, int report_len) {
  std::string msg;
  auto say = [&](const std::string& s) { if (report && report_len > 0) snprintf(report, report_len, "%s", s.c_str()); };
  HostModel hm;
  std::string err;
  int rc = plan_model(hm, md, nullptr, false, opt, &err);
  if (rc) { say("plan_model: " + err); return rc; }
  hm.pyr_kind = kind; hm.pad = pad;
  FrameSpec f;
  f.w = w; f.h = h; f.cn = cn; f.batch = batch; f.depth = depth;
  FrameLayout lay;
  if ((rc = plan_layout(hm, f, lay, &err))) { say("plan_layout: " + err); return rc; }
  std::vector<char*> regions;
  for (size_t i = 0; i < lay.regions.size(); ++i) regions.push_back((char*)(uintptr_t)((1ull << 44) + (i << 40)));
  const FrameBases b = frame_bases(lay, regions.data());
  FrameTables t;
  const PlanKnobs kn;
  if ((rc = plan_tables(hm, f, lay, b, 256, 0, kn, t, &err))) { say("plan_tables: " + err); return rc; }
  const size_t img_bytes = lay.buf[FB_IMG].bytes, pyr_bytes = lay.buf[FB_PYR].bytes;
  out[0] = lay.pyr_bytes; out[1] = img_bytes; out[2] = lay.esz; out[3] = lay.src_esz;
  out[4] = kind == PBD_PYRAMID_MATLAB ? t.matjobs.size() : t.pyrjobs.size(); out[5] = t.pyr_launches.size();
  int nerr = 0;
  auto bad = [&](const char* m) { if (nerr++ < 20) { msg += m; msg += '\n'; } };
  if (kind != PBD_PYRAMID_MATLAB) {
    if (!t.matjobs.empty() || !t.matruns.empty() || !t.mattaps.empty()) bad("default kind: MATLAB tables are not empty");
    if (lay.esz != lay.src_esz) bad("default kind: level and source element sizes differ");
  } else {
    if (!t.pyrjobs.empty()) bad("MATLAB kind: pyrjobs are not empty");
    if (lay.esz != 8 || lay.src_esz != 1) bad("MATLAB kind: double levels from an 8-bit frame");
    if (pyr_bytes < lay.pyr_bytes) bad("FB_PYR smaller than the level images");
    const int interval = hm.md.interval, n1 = lay.nlevels;
    if ((int)t.matjobs.size() != lay.nvl) bad("one job per virtual level");
    std::vector<int> written((size_t)lay.nvl, 0);
    for (size_t li = 0; li < t.pyr_launches.size(); ++li) {
      const PyrLaunch& P = t.pyr_launches[li];
      if (P.job0 < 0 || P.njobs < 0 || (size_t)P.job0 + P.njobs > t.matjobs.size()) { bad("launch: jobs out of range"); continue; }
      for (int j = P.job0; j < P.job0 + P.njobs; ++j) {
        const MatJob& J = t.matjobs[j];
        if ((long long)J.dw * J.dh > P.maxpix) bad("launch: maxpix below a job's destination");
        if (J.dw <= 0 || J.dh <= 0 || J.doff % 8 || J.doff + (size_t)J.dw * J.dh * cn * 8 > lay.pyr_bytes) bad("job: destination outside the level images");
        int lvl = -1;
        for (int v = 0; v < lay.nvl; ++v) if (lay.lv[v].img_off == J.doff && lay.lv[v].iw == J.dw && lay.lv[v].ih == J.dh) lvl = v;
        if (lvl < 0) { bad("job: destination is no level"); continue; }
        written[lvl]++;
        if (li == 0) {   // area resize from the frame
          if (lvl % n1 >= interval) bad("resize job: not a first-octave level");
          if (J.sw != w || J.sh != h || J.soff != (unsigned long long)(lvl / n1) * w * h * cn || J.soff + (size_t)w * h * cn > img_bytes) bad("resize job: source is not its frame");
          if (J.yrun0 < 0 || J.xrun0 < 0 || (size_t)J.yrun0 + J.dh > t.matruns.size() || (size_t)J.xrun0 + J.dw > t.matruns.size()) { bad("resize job: runs out of range"); continue; }
          for (int a = 0; a < 2; ++a) {
            const int r0 = a ? J.xrun0 : J.yrun0, dl = a ? J.dw : J.dh, sl = a ? J.sw : J.sh;
            for (int d = 0; d < dl; ++d) {
              const MatRun& R = t.matruns[r0 + d];
              if (R.first < 0 || R.count <= 0 || (size_t)R.first + R.count > t.mattaps.size()) { bad("run: taps out of range"); break; }
              for (int k = 0; k < R.count; ++k) {
                const MatTap& T = t.mattaps[R.first + k];
                if (T.si < 0 || T.si >= sl) bad("tap: source index outside the frame");
                if (k > 0 && T.si != t.mattaps[R.first + k - 1].si + 1) bad("tap: a run is not ascending and contiguous");
              }
            }
          }
        } else {         // reduce from level - interval
          if ((lvl % n1) / interval != (int)li) bad("reduce job: wrong octave");
          const Level& S = lay.lv[lvl - interval];
          if (J.soff != S.img_off || J.sw != S.iw || J.sh != S.ih) bad("reduce job: source is not level - interval");
          if (J.sw < 5 || J.sh < 5 || (J.sw != 2 * J.dw && J.sw != 2 * J.dw - 1) || (J.sh != 2 * J.dh && J.sh != 2 * J.dh - 1))
            bad("reduce job: sizes outside what the kernel's tap forms address");
          if (written[lvl - interval] != 1) bad("reduce job: its source is not written by an earlier launch");
        }
      }
    }
    for (int v = 0; v < lay.nvl; ++v) if (written[v] != 1) bad("a level is not written exactly once");
  }
  say(msg);
  return nerr ? 100 : PBD_OK;
}
