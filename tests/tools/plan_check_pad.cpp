// plan_check_pad.cpp — plan_check.cpp's checks for a handle with boundary padding (pbd_set_boundary_pad: HostModel::pad), plus the
// padding's own tables: the levels grow by 2 pad cells a side, the HOG tiles stay inside the interior, k_hog's level view points at the
// interior's first cell, and the border ring's jobs / blocks (k_featpad.hip) cover every ring cell of every active level exactly once
// and no interior cell.  Built by tests/test_boundary_pad_cpu.py with the planner; includes plan_check.cpp for the shared checks.
#include "plan_check.cpp"

namespace {

void check_pad(Checker& C, const FrameTables& t, const std::vector<Level>& base) {
  const FrameLayout& lay = C.lay;
  const int pad = C.hm.pad;
  if (pad == 0) {
    if (!t.hog_levels.empty() || !t.padjobs.empty() || !t.padblk.empty()) C.bad("pad 0: padding tables are not empty");
    return;
  }
  if ((int)t.hog_levels.size() != lay.nvl) C.bad("hog_levels: one per virtual level");
  size_t njobs = 0;
  for (int l = 0; l < lay.nvl; ++l) {
    const Level& L = lay.lv[l];
    const Level& B = base[l % lay.nlevels];
    const bool cells = B.cw > 0 && B.ch > 0;
    if (L.cw != (cells ? B.cw + 2 * pad : B.cw) || L.ch != (cells ? B.ch + 2 * pad : B.ch)) C.bad("level size is not the interior + 2 pad");
    if (L.bw != B.bw || L.bh != B.bh || L.iw != B.iw || L.ih != B.ih || L.scale != B.scale) C.bad("padding changed blocks / image / scale");
    if ((int)t.hog_levels.size() == lay.nvl) {
      const LevelDev& H = t.hog_levels[l];
      if (H.cw != L.cw || H.bw != L.bw || H.bh != L.bh || H.cell_off != L.cell_off + (size_t)pad * L.cw + pad) C.bad("hog_levels: pitch / interior origin");
    }
    if (L.active && cells) ++njobs;
  }
  if (t.padjobs.size() != njobs) C.bad("padjobs: one per active level with cells");
  for (const HogTile& T : t.hog_tiles) {
    const Level& L = lay.lv[T.level];
    if (T.cy0 < 0 || T.cx0 < 0 || T.cy0 >= L.ch - 2 * pad || T.cx0 >= L.cw - 2 * pad) C.bad("HOG tile outside the interior");
  }
  // ring coverage: every block's cells through the kernel's own mapping (k_featpad.hip: featpad_ring_cell), marked in a cell map
  std::vector<unsigned char> hit(lay.cells, 0);
  std::vector<int> seen(t.padjobs.size(), 0);
  for (const ReduceBlock& b : t.padblk) {
    if (b.job < 0 || b.job >= (int)t.padjobs.size()) { C.bad("padblk: job out of range"); continue; }
    const PadJob& J = t.padjobs[b.job];
    if (b.cell0 != (unsigned)seen[b.job] || (int)b.cell0 >= J.nring) C.bad("padblk: blocks of a job are not consecutive runs of PBD_FEATPAD_CPB");
    const unsigned n = std::min<unsigned>(PBD_FEATPAD_CPB, (unsigned)J.nring - b.cell0);
    seen[b.job] += (int)n;
    for (unsigned r = b.cell0; r < b.cell0 + n; ++r) {
      const unsigned cw = J.cw, p = J.pad, ih = J.ch - 2 * p, side = 2 * p;
      unsigned q = r, cell;
      if (q < p * cw) cell = q;
      else if ((q -= p * cw) < ih * side) { const unsigned y = q / side, k = q - y * side; cell = (p + y) * cw + (k < p ? k : cw - side + k); }
      else cell = (p + ih) * cw + (q - ih * side);
      if (cell >= (unsigned)J.cw * J.ch || J.cell_off + cell >= lay.cells) { C.bad("ring cell outside its level"); continue; }
      hit[J.cell_off + cell]++;
    }
  }
  for (size_t j = 0; j < t.padjobs.size(); ++j)
    if (seen[j] != t.padjobs[j].nring) C.bad("padblk: a job's ring is not covered");
  for (int l = 0; l < lay.nvl; ++l) {
    const Level& L = lay.lv[l];
    if (!(L.active && L.cw > 0 && L.ch > 0)) continue;
    for (int y = 0; y < L.ch; ++y)
      for (int x = 0; x < L.cw; ++x) {
        const bool ring = y < pad || y >= L.ch - pad || x < pad || x >= L.cw - pad;
        if (hit[L.cell_off + (size_t)y * L.cw + x] != (ring ? 1 : 0)) { C.bad("ring cell not written exactly once / interior cell written"); y = L.ch; break; }
      }
  }
}

}  // namespace

// plan_check with HostModel::pad = pad; *cells = the plan's total cell count, *base_sum = the sum over its levels of
// (cw0 + 2 pad) (ch0 + 2 pad) from the unpadded geometry (levels without cells: 0)
extern "C" int plan_check_pad(const pbd_model_desc* md, const int32_t* fsize, int sized, const pbd_options* opt, int w, int h, int cn,
                              int batch, int depth, const int32_t* levels, int nlevels, int ncu, int pad, unsigned long long* frame_bytes,
                              unsigned long long* cells, unsigned long long* base_sum, char* report, int report_len) {
  auto say = [&](const std::string& s) { if (report && report_len > 0) snprintf(report, report_len, "%s", s.c_str()); };
  HostModel hm;
  std::string err;
  int rc = plan_model(hm, md, fsize, sized != 0, opt, &err);
  if (rc) { say("plan_model: " + err); return rc; }
  hm.pad = pad;
  FrameSpec f;
  f.w = w; f.h = h; f.cn = cn; f.batch = batch; f.depth = depth;
  for (int i = 0; i < nlevels; ++i) {
    if ((int)f.level_set.size() <= levels[i]) f.level_set.resize(levels[i] + 1, 0);
    f.level_set[levels[i]] = 1;
  }
  FrameLayout lay;
  if ((rc = plan_layout(hm, f, lay, &err))) { say("plan_layout: " + err); return rc; }
  std::vector<Level> base((size_t)PBD_MAX_LEVELS, Level{});
  int n1 = 0;
  if (compute_geometry(w, h, hm.md.sbin, hm.md.interval, &n1, base.data()) || n1 != lay.nlevels) { say("geometry"); return 101; }
  unsigned long long sum = 0;
  for (int l = 0; l < n1; ++l)
    if (base[l].cw > 0 && base[l].ch > 0) sum += (unsigned long long)(base[l].cw + 2 * pad) * (base[l].ch + 2 * pad);
  if (base_sum) *base_sum = sum * batch;
  if (cells) *cells = lay.cells;
  std::vector<char*> regions;
  for (size_t i = 0; i < lay.regions.size(); ++i) regions.push_back((char*)(uintptr_t)((1ull << 44) + (i << 40)));
  const FrameBases b = frame_bases(lay, regions.data());
  FrameTables t, t2;
  const PlanKnobs kn;
  if ((rc = plan_tables(hm, f, lay, b, ncu, 0, kn, t, &err))) { say("plan_tables: " + err); return rc; }
  unsigned long long total = 0;
  for (size_t r : lay.regions) total += r;
  total += table_bytes(t.pyrjobs) + table_bytes(t.levels) + table_bytes(t.hog_tiles) + table_bytes(t.conv_tiles) +
           (hm.mixed ? table_bytes(t.conv_tiles_mix) : 0) + table_bytes(t.maps) + table_bytes(t.tasks) + table_bytes(t.folds) +
           table_bytes(t.foldx) + table_bytes(t.red) + table_bytes(t.redblk) + table_bytes(t.rootjobs) + table_bytes(t.rootblk) +
           table_bytes(t.back) + table_bytes(t.scr_base);
  if (pad > 0) total += table_bytes(t.hog_levels) + table_bytes(t.padjobs) + table_bytes(t.padblk);   // (uploaded only with padding on)
  if (frame_bytes) *frame_bytes = total;
  Checker C{hm, lay, b, "", 0};
  check_layout(C);
  check_tables(C, t);
  check_pad(C, t, base);
  if (plan_tables(hm, f, lay, b, ncu, 0, kn, t2, &err) || canonical(t) != canonical(t2) || t.padjobs.size() != t2.padjobs.size() ||
      t.padblk.size() != t2.padblk.size())
    C.bad("planning twice gives different tables");
  char head[200];
  snprintf(head, sizeof(head), "%s plan, pad %d, %d virtual levels, %zu regions, %zu tasks, %zu folds, %zu reduce jobs, %zu root jobs, %zu ring blocks\n",
           lay.compact ? "compact" : "default", pad, lay.nvl, lay.regions.size(), t.tasks.size(), t.folds.size(), t.red.size(), t.rootjobs.size(),
           t.padblk.size());
  say(std::string(head) + C.msg);
  return C.nerr ? 100 : PBD_OK;
}
