// pbd_plan.cpp — the frame planner of libpbd_hip.so (pbd_plan.hpp): model topology, the frame's memory plan and every kernel work
// table, from the model, the frame size and the buffers' base addresses.  Pure host arithmetic: no HIP runtime, no environment.
#include "pbd_plan.hpp"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include "dt_core.hpp"   // dt_segments: the planner and the kernels share one definition
#include "pbd_lds.hpp"

static int fail(std::string* err, int code, const std::string& msg) {
  if (err) *err = msg;
  return code;
}

// ---------------------------------------------------------------------------
// pyramid geometry — HOGFeatures<T>::pyramid, src/HOGFeatures.cpp:98-127,174-175
// ---------------------------------------------------------------------------
static inline int cv_round_f(float v) { return (int)std::lrint((double)v); }

int compute_geometry(int w, int h, int sbin, int interval, int* nlevels, Level* lv) {
  const float sf = (float)std::pow(2.0, (double)(1.0f / (float)interval));  // HOGFeatures.hpp:78
  const float fw = (float)w, fh = (float)h;
  const float mn = fh < fw ? fh : fw;
  const float r = std::log(mn / (5.0f * (float)sbin)) / std::log(sf);          // :99 (float math)
  const int n = (int)(1.0f + std::floor(r));
  if (n < interval || n > PBD_MAX_LEVELS) return -1;
  for (int i = 0; i < interval; ++i) {
    const float f = (float)(1.0f / std::pow((double)sf, (double)i));            // :116
    lv[i].iw = cv_round_f(fw * f);
    lv[i].ih = cv_round_f(fh * f);
    lv[i].scale = (float)(std::pow((double)sf, (double)i) * (double)sbin);      // :118
    for (int j = i + interval; j < n; j += interval) {
      lv[j].iw = (lv[j - interval].iw + 1) / 2;                                 // :122 pyrDown
      lv[j].ih = (lv[j - interval].ih + 1) / 2;
      lv[j].scale = 2 * lv[j - interval].scale;                                 // :124
    }
  }
  for (int l = 0; l < n; ++l) {
    lv[l].bw = (int)std::round((float)lv[l].iw / (float)sbin);                  // :174
    lv[l].bh = (int)std::round((float)lv[l].ih / (float)sbin);
    lv[l].cw = std::max(lv[l].bw - 2, 0);                                       // :175
    lv[l].ch = std::max(lv[l].bh - 2, 0);
  }
  *nlevels = n;
  return 0;
}

// matlab/detection/featpyramid.m:13-34,47 — all in double; the image sizes are what resize.cc:94-95 and reduce.cc:58-59 derive (C round(),
// halves away from zero); cells as above (features.cc and k_hog agree on them)
int compute_geometry_matlab(int w, int h, int sbin, int interval, int* nlevels, Level* lv) {
  const double sc = std::pow(2.0, 1.0 / interval);                                        // featpyramid.m:13
  const int n = 1 + (int)std::floor(std::log(std::min(w, h) / (5.0 * sbin)) / std::log(sc));   // :15
  if (n < interval || n > PBD_MAX_LEVELS) return -1;
  std::vector<double> scale((size_t)n);
  for (int i = 0; i < interval; ++i) {
    const double s = 1.0 / std::pow(sc, i);                                               // :25
    lv[i].ih = (int)std::round(h * s);                                                    // resize.cc:94-95
    lv[i].iw = (int)std::round(w * s);
    scale[i] = sbin / s;                                                                  // featpyramid.m:27,47
    for (int j = i + interval; j < n; j += interval) {
      if (lv[j - interval].iw < 5 || lv[j - interval].ih < 5) return -1;                  // (reduce.cc:24,42 read three, :29 five source rows)
      lv[j].ih = (int)std::round(lv[j - interval].ih * .5);                               // reduce.cc:58-59
      lv[j].iw = (int)std::round(lv[j - interval].iw * .5);
      scale[j] = 2.0 * scale[j - interval];                                               // featpyramid.m:32,47
    }
  }
  for (int l = 0; l < n; ++l) {
    lv[l].scale = (float)scale[l];                                                        // the handle's scale type, as the last step
    lv[l].bw = (int)std::round((float)lv[l].iw / (float)sbin);
    lv[l].bh = (int)std::round((float)lv[l].ih / (float)sbin);
    lv[l].cw = std::max(lv[l].bw - 2, 0);
    lv[l].ch = std::max(lv[l].bh - 2, 0);
  }
  *nlevels = n;
  return 0;
}

// matlab/mex/resize.cc:30-66, statement by statement; one run per destination index instead of the `di` field
bool resize_taps(int slen, int dlen, std::vector<MatRun>& runs, std::vector<MatTap>& taps) {
  const size_t t0 = taps.size();
  const double scale = (double)dlen / (double)slen;
  const double invscale = (double)slen / (double)dlen;
  for (int dy = 0; dy < dlen; ++dy) {
    const double fsy1 = dy * invscale;
    const double fsy2 = fsy1 + invscale;
    const int sy1 = (int)std::ceil(fsy1);
    const int sy2 = (int)std::floor(fsy2);
    MatRun r{(int)taps.size(), 0};
    if (sy1 - fsy1 > 1e-3) taps.push_back(MatTap{(sy1 - fsy1) * scale, sy1 - 1, 0});
    for (int sy = sy1; sy < sy2; ++sy) taps.push_back(MatTap{scale, sy, 0});
    if (fsy2 - sy2 > 1e-3) taps.push_back(MatTap{(fsy2 - sy2) * scale, sy2, 0});
    r.count = (int)taps.size() - r.first;
    runs.push_back(r);
  }
  for (size_t t = t0; t < taps.size(); ++t)
    if (taps[t].si < 0 || taps[t].si >= slen) return false;   // (resize.cc:53,61 assert it)
  return true;
}

void pad_geometry(int pad, int nlevels, Level* lv) {
  for (int l = 0; l < nlevels; ++l)
    if (lv[l].cw > 0 && lv[l].ch > 0) { lv[l].cw += 2 * pad; lv[l].ch += 2 * pad; }
}

// include/pbd_c.h "pyramid store": the feature layout of ONE frame — the geometry above, the padding, and the levels' element offsets
// back to back, which are plan_layout's cell_off * PBD_FLEN for a single frame.  Host only.
extern "C" __attribute__((visibility("default")))
int pbd_pyrstore_layout(int w, int hgt, int sbin, int interval, int kind, int pad, int* nlevels, long long* level_off, long long* total) {
  if (!nlevels || !total) return PBD_ERR_ARG;
  if (sbin <= 0 || interval < 1 || interval > 16 || pad < 0 || pad > 8 || (kind != PBD_PYRAMID_OPENCV && kind != PBD_PYRAMID_MATLAB)) return PBD_ERR_ARG;
  if (w < 3 || hgt < 3) return PBD_ERR_ARG;
  std::vector<Level> lv((size_t)PBD_MAX_LEVELS, Level{});
  int n = 0;
  if (kind == PBD_PYRAMID_MATLAB ? compute_geometry_matlab(w, hgt, sbin, interval, &n, lv.data()) : compute_geometry(w, hgt, sbin, interval, &n, lv.data()))
    return PBD_ERR_ARG;
  pad_geometry(pad, n, lv.data());
  long long off = 0;
  for (int l = 0; l < n; ++l) {
    if (level_off) level_off[l] = off;
    off += (long long)lv[l].cw * lv[l].ch * PBD_FLEN;
  }
  *nlevels = n;
  *total = off;
  return PBD_OK;
}

int depth_esz(int depth) { return depth == PBD_DEPTH_8U ? 1 : depth == PBD_DEPTH_16U ? 2 : depth == PBD_DEPTH_32F ? 4 : depth == PBD_DEPTH_64F ? 8 : 0; }

// ---------------------------------------------------------------------------
// model
// ---------------------------------------------------------------------------
static int nmix_of(const HostModel* h, int fp) { return h->mix_offset[fp + 1] - h->mix_offset[fp]; }

static int ingest_model(HostModel* h, const pbd_model_desc* m, std::string* err) {
  if (!m || !m->filters || !m->defw || !m->anchors || !m->biasw || !m->part_offset || !m->parentid ||
      !m->mix_offset || !m->filterid || !m->defid || !m->biasid)
    return fail(err, PBD_ERR_ARG, "model: null pointer");
  if (m->flen != PBD_FLEN || m->norient != PBD_NORIENT)
    return fail(err, PBD_ERR_UNSUPPORTED, "model: only flen=32 / norient=18 HOG is supported");
  if (m->nfilters <= 0 || (!h->mixed && (m->kh <= 0 || m->kw <= 0 || m->kh > 9 || m->kw > 9)) || m->sbin <= 0 || m->interval <= 0 ||
      m->interval > 16 || m->ncomponents <= 0)
    return fail(err, PBD_ERR_ARG, "model: bad sizes");
  if (m->ndefs < 0 || m->nbias <= 0) return fail(err, PBD_ERR_ARG, "model: ndefs >= 0 and nbias > 0 required");
  const int nc = m->ncomponents;
  if (m->part_offset[0] != 0) return fail(err, PBD_ERR_ARG, "model: part_offset[0] must be 0");
  for (int c = 0; c < nc; ++c)
    if (m->part_offset[c + 1] <= m->part_offset[c]) return fail(err, PBD_ERR_ARG, "model: part_offset must be strictly increasing");
  h->part_offset.assign(m->part_offset, m->part_offset + nc + 1);
  const int np = h->part_offset[nc];
  if (m->mix_offset[0] != 0) return fail(err, PBD_ERR_ARG, "model: mix_offset[0] must be 0");
  for (int fp = 0; fp < np; ++fp)
    if (m->mix_offset[fp + 1] <= m->mix_offset[fp]) return fail(err, PBD_ERR_ARG, "model: mix_offset must be strictly increasing");
  h->parentid.assign(m->parentid, m->parentid + np);
  h->mix_offset.assign(m->mix_offset, m->mix_offset + np + 1);
  const int nm = h->mix_offset[np];
  h->filterid.assign(m->filterid, m->filterid + nm);
  h->defid.assign(m->defid, m->defid + nm);
  h->biasid.assign(m->biasid, m->biasid + nm);
  size_t nweights = (size_t)m->nfilters * m->kh * m->kw * m->flen;   // mixed banks (pbd_create_sized): sum of kh_i kw_i flen
  if (h->mixed) {
    nweights = 0;
    for (int n = 0; n < m->nfilters; ++n) nweights += (size_t)h->fkh[n] * h->fkw[n] * m->flen;
  }
  h->filters.assign(m->filters, m->filters + nweights);
  h->defw.assign(m->defw, m->defw + (size_t)m->ndefs * 4);
  h->anchors.assign(m->anchors, m->anchors + (size_t)m->ndefs * 2);
  h->biasw.assign(m->biasw, m->biasw + m->nbias);
  // weights: finite, all of them — a NaN / inf filter weight or bias puts non-finite scores in front of the distance transform, a
  // non-finite deformation weight is a non-finite quadratic (the DT's input domain, pbd_plan.hpp: pbd_first_nonfinite)
  if (pbd_first_nonfinite(h->filters.data(), h->filters.size()) != h->filters.size()) return fail(err, PBD_ERR_ARG, "model: non-finite filter weight");
  if (pbd_first_nonfinite(h->biasw.data(), h->biasw.size()) != h->biasw.size()) return fail(err, PBD_ERR_ARG, "model: non-finite bias");
  if (pbd_first_nonfinite(h->defw.data(), h->defw.size()) != h->defw.size()) return fail(err, PBD_ERR_ARG, "model: non-finite deformation weight");
  h->md = *m;
  h->md.filters = h->filters.data(); h->md.defw = h->defw.data(); h->md.anchors = h->anchors.data();
  h->md.biasw = h->biasw.data(); h->md.part_offset = h->part_offset.data(); h->md.parentid = h->parentid.data();
  h->md.mix_offset = h->mix_offset.data(); h->md.filterid = h->filterid.data(); h->md.defid = h->defid.data();
  h->md.biasid = h->biasid.data();

  h->parts.resize(np);
  h->comp_plane0.assign(nc + 1, 0);
  h->max_parts = 0;
  int slot_next = 0, plane_next = 0;
  bool aliasing = false;
  for (int c = 0; c < nc; ++c) {
    const int p0 = h->part_offset[c], cnp = h->part_offset[c + 1] - p0;
    if (cnp <= 0) return fail(err, PBD_ERR_ARG, "model: empty component");
    if (cnp > 256) return fail(err, PBD_ERR_UNSUPPORTED, "model: more than 256 parts in a component");   // BT_MAXP (k_backtrack)
    h->max_parts = std::max(h->max_parts, cnp);
    h->comp_plane0[c] = plane_next;
    std::map<int, int> slot_of;   // filter id -> slot (ncscores is indexed by filter id, DynamicProgram.cpp:93)
    std::map<int, int> uses;
    std::vector<int> nchild(cnp, 0);
    for (int p = 1; p < cnp; ++p) {
      const int par = h->parentid[p0 + p];
      if (par < 0 || par >= p) return fail(err, PBD_ERR_ARG, "model: parts must be ordered parent < child");
      nchild[par]++;
    }
    for (int p = 0; p < cnp; ++p) {
      PartInfo& P = h->parts[p0 + p];
      P.comp = c; P.p = p; P.parent = (p == 0) ? -1 : h->parentid[p0 + p];
      P.K = nmix_of(h, p0 + p);
      if (P.K <= 0 || P.K > PBD_MAX_MIX) return fail(err, PBD_ERR_UNSUPPORTED, "model: 1..16 mixtures per part");
      P.leaf = (nchild[p] == 0);
      const int fm0 = h->mix_offset[p0 + p];
      for (int m2 = 0; m2 < P.K; ++m2) {
        const int fid = h->filterid[fm0 + m2];
        if (fid < 0 || fid >= m->nfilters) return fail(err, PBD_ERR_ARG, "model: filterid out of range");
        P.filterid.push_back(fid);
        P.defid.push_back(h->defid[fm0 + m2]);
        P.biasid.push_back(h->biasid[fm0 + m2]);
        if (!slot_of.count(fid)) slot_of[fid] = slot_next++;
        P.slot.push_back(slot_of[fid]);
        if (++uses[fid] > 1) aliasing = true;
        if (p > 0) {
          const int did = h->defid[fm0 + m2];
          if (did < 0 || did >= m->ndefs) return fail(err, PBD_ERR_ARG, "model: defid out of range");
          if (h->defw[did * 4] == 0.f || h->defw[did * 4 + 2] == 0.f)
            return fail(err, PBD_ERR_ARG, "model: quadratic deformation weights must be non-zero "
                                        "(include/DistanceTransform.hpp:99 divides by 2a)");
        }
        const int bid = h->biasid[fm0 + m2];
        const int L = (p == 0) ? 1 : nmix_of(h, p0 + h->parentid[p0 + p]);
        if (bid < 0 || bid + L > m->nbias) return fail(err, PBD_ERR_ARG, "model: biasid out of range");
      }
      P.plane0 = -1;
      if (p > 0) {
        P.plane0 = plane_next;
        plane_next += nmix_of(h, p0 + P.parent);
      }
    }
  }
  h->comp_plane0[nc] = plane_next;
  h->nslots = slot_next;
  h->nplanes = plane_next;

  // ---- round schedule -------------------------------------------------------
  // DT of a part runs once all its children have sent their message (DynamicProgram.cpp:95 walks
  // p = P-1..1 with parent < child): round = height of the part.  Messages into one parent are
  // float adds in DESCENDING child order (:156); to keep those bits, a child's message is folded
  // no earlier than every higher-indexed sibling's (reduce round = max over them), and siblings
  // folded in the same round go through ONE reduce job that adds them in that order.
  // fold mode (messages folded by the consumer, no accumulated planes): needs every part's accumulator to be its own
  // (no filter id shared inside a component: the reference's ncscores is indexed by FILTER id, so two parts with
  // one id would share an accumulator) and its mixtures / its children's to fit the register arrays of the fold
  {
    std::vector<int> fuse(m->nfilters, 0);
    h->unique_filters = true;
    for (int fm = 0; fm < nm; ++fm) if (++fuse[h->filterid[fm]] > 1) h->unique_filters = false;   // (also across components: face-like models share a pool)
  }
  h->fold = !aliasing && h->opt.reserved[1] != 1;
  {
    std::vector<int> nchild_flat(np, 0);
    for (int fp = 0; fp < np; ++fp) {
      if (h->parts[fp].K > PBD_FOLD_MAXMIX) h->fold = false;
      h->fold_mix = std::max(h->fold_mix, h->parts[fp].K);
      if (h->parts[fp].p > 0 && ++nchild_flat[h->part_offset[h->parts[fp].comp] + h->parts[fp].parent] > PBD_MAX_CH) h->fold = false;
    }
  }
  h->rounds.clear();
  h->red_rounds.clear();
  if (aliasing) {  // shared filter ids inside a component: keep the reference's strictly sequential order
    for (int c = 0; c < nc; ++c)
      for (int p = h->part_offset[c + 1] - h->part_offset[c] - 1; p > 0; --p) {
        h->rounds.push_back(std::vector<int>(1, h->part_offset[c] + p));
        h->red_rounds.push_back({std::vector<int>(1, h->part_offset[c] + p)});
      }
  } else {
    std::vector<int> height(np, 0), rround(np, 0);
    int nrounds = 0;
    for (int c = 0; c < nc; ++c) {
      const int p0 = h->part_offset[c], cnp = h->part_offset[c + 1] - p0;
      for (int p = cnp - 1; p > 0; --p) {  // children before parents (parent < child)
        const int par = h->parts[p0 + p].parent;
        height[p0 + par] = std::max(height[p0 + par], height[p0 + p] + 1);
      }
      for (int p = cnp - 1; p > 0; --p) {  // descending index: higher siblings first
        int rr = height[p0 + p];
        for (int q = p + 1; q < cnp; ++q)
          if (h->parts[p0 + q].parent == h->parts[p0 + p].parent) rr = std::max(rr, rround[p0 + q]);
        rround[p0 + p] = rr;
        nrounds = std::max(nrounds, rr + 1);
      }
    }
    h->rounds.assign(nrounds, {});
    std::vector<std::vector<int>> red(nrounds);
    for (int fp = 0; fp < np; ++fp) {
      if (h->parts[fp].p == 0) continue;
      h->rounds[height[fp]].push_back(fp);
      red[rround[fp]].push_back(fp);
    }
    // waves: at most PBD_MAX_CH children of one parent per reduce job; overflow goes to a later wave
    h->red_rounds.assign(nrounds, {});
    for (int r = 0; r < nrounds; ++r) {
      std::vector<int> rest(red[r].rbegin(), red[r].rend());  // descending flat index
      while (!rest.empty()) {
        std::vector<int> wave, next;
        std::map<int, int> cnt;
        for (int fp : rest) {
          const int parent_fp = h->part_offset[h->parts[fp].comp] + h->parts[fp].parent;
          if (cnt[parent_fp] < PBD_MAX_CH && !std::count_if(next.begin(), next.end(), [&](int g) {
                return h->part_offset[h->parts[g].comp] + h->parts[g].parent == parent_fp; })) {
            cnt[parent_fp]++;
            wave.push_back(fp);
          } else {
            next.push_back(fp);
          }
        }
        h->red_rounds[r].push_back(wave);
        rest.swap(next);
      }
    }
  }
  return PBD_OK;
}

int plan_model(HostModel& hm, const pbd_model_desc* model, const int32_t* fsize, bool sized, const pbd_options* opt, std::string* err) {
  HostModel* h = &hm;
  pbd_options o{};
  if (opt) o = *opt;
  if (o.max_candidates <= 0) o.max_candidates = 4096;
  h->opt = o;
  if (o.scalar_type != PBD_SCALAR_F32 && o.scalar_type != PBD_SCALAR_F64) return fail(err, PBD_ERR_ARG, "scalar_type: PBD_SCALAR_F32 or PBD_SCALAR_F64");
  h->ts = (o.scalar_type == PBD_SCALAR_F64) ? 8 : 4;
  pbd_model_desc sdesc;
  std::vector<float> sorted;
  if (sized && !fsize) return fail(err, PBD_ERR_ARG, "pbd_create_sized: fsize is null");
  if (sized) {
    if (!model || !model->filters) return fail(err, PBD_ERR_ARG, "model: null pointer");
    if (model->kh != 0 || model->kw != 0) return fail(err, PBD_ERR_ARG, "pbd_create_sized: model->kh / kw must be 0 (the sizes come from fsize)");
    if (model->nfilters <= 0) return fail(err, PBD_ERR_ARG, "model: bad sizes");
    if (model->flen != PBD_FLEN || model->norient != PBD_NORIENT)
      return fail(err, PBD_ERR_UNSUPPORTED, "model: only flen=32 / norient=18 HOG is supported");
    const int nf = model->nfilters;
    for (int n = 0; n < nf; ++n)
      if (fsize[2 * n] < 1 || fsize[2 * n] > 9 || fsize[2 * n + 1] < 1 || fsize[2 * n + 1] > 9)
        return fail(err, PBD_ERR_UNSUPPORTED, "pbd_create_sized: filter " + std::to_string(n) + ": sides of 1..9 cells");
    sdesc = *model;
    bool uniform = true;
    for (int n = 1; n < nf; ++n) uniform = uniform && fsize[2 * n] == fsize[0] && fsize[2 * n + 1] == fsize[1];
    if (uniform) {
      sdesc.kh = fsize[0]; sdesc.kw = fsize[1];
    } else {
      std::vector<int> ord(nf);
      for (int n = 0; n < nf; ++n) ord[n] = n;
      std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) {
        return fsize[2 * a] != fsize[2 * b] ? fsize[2 * a] < fsize[2 * b] : fsize[2 * a + 1] < fsize[2 * b + 1]; });
      std::vector<size_t> off(nf + 1, 0);
      for (int n = 0; n < nf; ++n) off[n + 1] = off[n] + (size_t)fsize[2 * n] * fsize[2 * n + 1] * PBD_FLEN;
      h->mixed = true;
      h->fperm.assign(nf, 0);
      for (int i = 0; i < nf; ++i) {
        const int c = ord[i];
        h->fperm[c] = i;
        h->fkh.push_back(fsize[2 * c]); h->fkw.push_back(fsize[2 * c + 1]);
        sorted.insert(sorted.end(), model->filters + off[c], model->filters + off[c + 1]);
      }
      sdesc.filters = sorted.data();
    }
    model = &sdesc;
  }
  int rc = ingest_model(h, model, err);
  if (rc) return rc;
  if (h->mixed) {   // filter ids (validated by ingest_model) into the size-sorted order
    for (int& f : h->filterid) f = h->fperm[f];
    for (PartInfo& P : h->parts) for (int& f : P.filterid) f = h->fperm[f];
  }
  if (o.reserved[0] < 0 || o.reserved[0] > 1024) return fail(err, PBD_ERR_ARG, "reserved[0] (nms_sz): 0 = off, or the window of the score-map NMS");
  h->nms_sz = o.reserved[0];
  h->conv_mode = o.conv_mode;
  if (h->conv_mode == PBD_CONV_AUTO)
    // measured on MI355X for N = 26 .. 312 5x5x32 filters at 640x480 (profiles/history/archive/r03b_conv_modes.json): the fp32 MFMA
    // implicit GEMM beats the direct VALU correlation at every N (26 filters: 0.11 vs 0.38 ms; 156: 0.40 vs 1.62;
    // 312: 0.76 vs 2.89) — the contraction is K = 800 deep whatever N is, so one 16-filter n-tile already pays.
    // The VALU kernel remains the bit-exact parity path (PBD_CONV_EXACT) and what banks of fewer than 16 filters get.
    // Any filter size goes the same way (3x3 .. 9x9: the contraction is kh * kw * 32 >= 288 deep; run-time tap loop of the same kernel).
    // Round 5: float handles take the split-product bank (k_conv_split.hip: the fp32 products as six exact bfloat16 partial
    // products on the bf16 matrix units, fp32 accumulators — errors of the fp32 MFMA chain's size, 2-3x its speed, and off the
    // vector ALU's pipe); a weight outside bfloat16's finite range (|w| >= 3e38: no trained model) keeps the fp32 MFMA bank.
    {
      bool splittable = h->ts == 4 && model->flen == PBD_FLEN;
      for (size_t i = 0; splittable && i < h->filters.size(); ++i) splittable = std::fabs(h->filters[i]) < 3.0e38f;
      h->conv_mode = model->nfilters >= 16 ? (splittable ? PBD_CONV_SPLIT : PBD_CONV_MFMA) : PBD_CONV_EXACT;
    }
  if ((h->conv_mode == PBD_CONV_SPLIT || h->conv_mode == PBD_CONV_SPLIT_F16) && (h->ts != 4 || model->flen != PBD_FLEN))
    return fail(err, PBD_ERR_UNSUPPORTED, "PBD_CONV_SPLIT / PBD_CONV_SPLIT_F16: float handles (32-channel HOG features)");
  if (h->conv_mode == PBD_CONV_SPLIT || h->conv_mode == PBD_CONV_SPLIT_F16)
    for (size_t i = 0; i < h->filters.size(); ++i)
      if (!(std::fabs(h->filters[i]) < 3.0e38f)) return fail(err, PBD_ERR_UNSUPPORTED, "PBD_CONV_SPLIT: a filter weight outside bfloat16's finite range");
  if (h->conv_mode < PBD_CONV_AUTO || h->conv_mode > PBD_CONV_SPLIT_F16) return fail(err, PBD_ERR_ARG, "conv_mode: PBD_CONV_*");
  if (h->mixed)   // size groups: runs of one kh x kw in the internal (size-sorted) filter order, each uploaded as a uniform bank of its own
    for (int n = 0; n < model->nfilters;) {
      int e = n;
      while (e < model->nfilters && h->fkh[e] == h->fkh[n] && h->fkw[e] == h->fkw[n]) ++e;
      SizeGroup g;
      g.kh = h->fkh[n]; g.kw = h->fkw[n]; g.n0 = n; g.nf = e - n;
      h->groups.push_back(g);
      n = e;
    }
  h->split_parts = h->conv_mode == PBD_CONV_SPLIT ? 3 : h->conv_mode == PBD_CONV_SPLIT_F16 ? 2 : 0;
  return PBD_OK;
}

// ---------------------------------------------------------------------------
// frame layout
// ---------------------------------------------------------------------------
static bool has_cells(const Level& L) { return L.active && L.cw > 0 && L.ch > 0; }
static int plan_maxlen(const std::vector<Level>& lv) {   // the longest DT line of the plan (a row or a column of an active level)
  int maxlen = 1;
  for (const Level& L : lv) if (L.active) maxlen = std::max(maxlen, std::max(L.cw, L.ch));
  return maxlen;
}

int plan_layout(const HostModel& hm, const FrameSpec& f, FrameLayout& out, std::string* err) {
  const pbd_model_desc& m = hm.md;
  out = FrameLayout{};
  int n1 = 0;
  std::vector<Level> lv((size_t)PBD_MAX_LEVELS, Level{});
  const bool matlab = hm.pyr_kind == PBD_PYRAMID_MATLAB;
  if (matlab && f.depth != PBD_DEPTH_8U)
    return fail(err, PBD_ERR_UNSUPPORTED, "PBD_PYRAMID_MATLAB: 8-bit frames (the level images are double whatever the frame; pbd_set_pyramid_kind)");
  if (matlab) {
    if (f.w < 3 || f.h < 3 || compute_geometry_matlab(f.w, f.h, m.sbin, m.interval, &n1, lv.data()))
      return fail(err, PBD_ERR_ARG, "image too small: the pyramid needs at least `interval` levels and reduce() sources of 5 x 5 pixels "
                                    "(matlab/detection/featpyramid.m:15, matlab/mex/reduce.cc:24-42)");
  } else
  if (f.w < 3 || f.h < 3 || compute_geometry(f.w, f.h, m.sbin, m.interval, &n1, lv.data()))
    return fail(err, PBD_ERR_ARG, "image too small: the pyramid needs at least `interval` levels "
                                  "(src/HOGFeatures.cpp:99,114)");
  pad_geometry(hm.pad, n1, lv.data());
  // A batch of B same-sized frames is planned as B x nlevels "virtual levels" (frame f's level l = f * nlevels + l)
  const int n = n1 * f.batch;
  out.nlevels = n1; out.batch = f.batch; out.nvl = n;
  out.src_esz = depth_esz(f.depth);
  out.esz = matlab ? 8 : out.src_esz;
  out.lv.resize(n);
  for (int fr = 0; fr < f.batch; ++fr)
    for (int l = 0; l < n1; ++l) out.lv[fr * n1 + l] = lv[l];
  int lb = hm.opt.level_begin, le = hm.opt.level_end;
  if (le <= 0 || le > n1) le = n1;
  if (lb < 0) lb = 0;
  size_t cells = 0, pyr = 0;
  for (int vl = 0; vl < n; ++vl) {
    Level& L = out.lv[vl];
    const int l = vl % n1;
    L.active = (l >= lb && l < le) && (f.level_set.empty() || (l < (int)f.level_set.size() && f.level_set[l]));
    if (L.cw > 32767 || L.ch > 32767) return fail(err, PBD_ERR_UNSUPPORTED, "level too large for 16-bit pointers");
    // the fold loader addresses a level's planes with 32-bit offsets: cell * sizeof(T) and plane * cells + cell (<= 8 planes of a child)
    if ((size_t)L.cw * L.ch >= ((size_t)1 << 28)) return fail(err, PBD_ERR_UNSUPPORTED, "level too large (2^28 cells)");
    L.img_off = pyr; pyr += (size_t)L.iw * L.ih * f.cn * out.esz;
    L.cell_off = cells; cells += (size_t)L.cw * L.ch;
    if (L.active) out.act_cells += (size_t)L.cw * L.ch;
  }
  out.cells = cells; out.pyr_bytes = pyr;
  if (matlab && pyr > PBD_MATPYR_MAX_BYTES)
    return fail(err, PBD_ERR_UNSUPPORTED, "PBD_PYRAMID_MATLAB: the double level images of this geometry exceed the plan's budget for them (2 GiB)");
  if (cells >= (1u << 31)) return fail(err, PBD_ERR_UNSUPPORTED, "frame too large");
  for (const std::vector<int>& rnd : hm.rounds) {
    size_t k = 0;
    for (int fp : rnd) k += hm.parts[fp].K;
    out.maxK = std::max(out.maxK, k);
  }
  size_t allmaps = 0;
  for (const PartInfo& P : hm.parts) if (P.p > 0) allmaps += P.K;
  out.dt_cap_elems = std::max<size_t>(1, allmaps * out.act_cells);

  // Memory plan.  Default: every stage buffer has its own allocation and stays valid after detect() (the parity
  // tests read features / responses / tables of a finished frame).  Compact (fold structure, every filter id used by
  // one mixture only; chosen automatically for large frames — the responses alone over 400 MB, e.g. 1920x1080 —
  // or forced with dp_mode 2): buffers that are never live together share memory:
  //   * a mixture's distance-transformed scores overwrite its own raw response plane (its x pass has consumed the
  //     plane before its y pass writes it; nothing else reads the raw plane of a non-root part): no FB_DT_SDT;
  //   * the level images + HOG features (dead once the filter bank has run) share one region with the x pass's
  //     per-round output + the Ik planes (first written by the DP);
  //   * the features' split parts share the x pass's pointer planes where those are large enough (below).
  // 1920x1080, person model: 1.47 GB instead of 3.3 GB.  After min() the image / feature / response getters of a
  // compact handle answer PBD_ERR_STATE (the buffers have been reused).
  const size_t ts = (size_t)hm.ts;
  out.compact = hm.fold && hm.unique_filters && (hm.opt.reserved[1] == 2 || (hm.opt.reserved[1] == 0 && cells * m.nfilters * ts > ((size_t)400 << 20)));
  auto own = [&](FrameBuf b, size_t bytes) {   // a region of its own (at least one byte, as the allocation is)
    out.buf[b] = BufPlace{(int)out.regions.size(), 0, std::max<size_t>(bytes, 1)};
    out.regions.push_back(out.buf[b].bytes);
  };
  own(FB_IMG, (size_t)f.w * f.h * f.cn * out.src_esz * f.batch);
  own(FB_RESP, cells * m.nfilters * ts);
  const size_t pk_bytes = cells * std::max(hm.nplanes, 1), feat_bytes = cells * PBD_FLEN * ts;
  // DT planes.  The passes' own pointer planes (int16) stay for the whole frame: back-tracking composes Ix / Iy from
  // them.  Score planes — fold: the x pass's output lives only until the round's y pass (one round's worth, reused
  // by every round), the y pass's output (the message source) keeps its own plane until the parent's x pass has
  // read it; legacy: both kept per map (a message may wait several rounds for a higher-indexed sibling), plus the
  // accumulated part scores.
  const size_t tmp_elems = hm.fold ? std::max<size_t>(1, out.maxK * out.act_cells) : out.dt_cap_elems;
  if (out.compact) {
    const size_t al = 256, pyr_al = (pyr + al - 1) / al * al, pk_al = (pk_bytes + al - 1) / al * al;
    const int r = (int)out.regions.size();
    out.regions.push_back(std::max<size_t>(1, std::max(pyr_al + feat_bytes, pk_al + out.maxK * out.act_cells * ts)));
    out.buf[FB_PYR] = BufPlace{r, 0, pyr};
    out.buf[FB_FEAT] = BufPlace{r, pyr_al, feat_bytes};
    out.buf[FB_PK] = BufPlace{r, 0, pk_bytes};
    out.buf[FB_DT_TMPT] = BufPlace{r, pk_al, out.maxK * out.act_cells * ts};
  } else {
    own(FB_PYR, pyr);
    own(FB_FEAT, feat_bytes);
    own(FB_PK, pk_bytes);
    own(FB_DT_TMPT, tmp_elems * ts);
    own(FB_DT_SDT, out.dt_cap_elems * ts);
  }
  own(FB_ROOTV, cells * m.ncomponents * ts);
  own(FB_ROOTI, std::max<size_t>(cells * m.ncomponents, 1) * sizeof(int));
  if (hm.nms_sz > 0) own(FB_NMS_MASK, cells * m.ncomponents);
  // Width of their elements: bytes while every line of the plan has byte links (640x480: a third of what a DT launch writes was pointers), else
  // int16 — one width for the plan.  The buffers keep two bytes per element either way (byte planes fill their first half): what the change
  // saves is the traffic of 18 launches a frame, and the plan's footprint and the aliasing below stay what the plan check pins.
  out.ptr_bytes = dt_ptr_bytes_for(plan_maxlen(out.lv));
  own(FB_DT_IXT, out.dt_cap_elems * sizeof(int16_t));
  own(FB_DT_IY, out.dt_cap_elems * sizeof(int16_t));
  if (!hm.fold) own(FB_ACC, cells * hm.nslots * ts);
  if (hm.split_parts) {
    // the features' bfloat16 parts (192 B per cell; binary16: 128 B) live from HOG to the end of the filter bank; the x pass's pointer planes from min()
    // to argmin(): the compact plan (whose stage buffers already refuse to be read once a later stage has reused them) puts both in
    // one region where the planes are large enough (person model: 300 B per cell); the default plan keeps them apart (pdf() may be
    // called again after min() there)
    const size_t split_elems = cells * hm.split_parts * PBD_FLEN;
    if (out.compact && out.dt_cap_elems >= split_elems) out.buf[FB_FEAT_SPLIT] = BufPlace{out.buf[FB_DT_IXT].region, 0, split_elems * sizeof(uint16_t)};
    else own(FB_FEAT_SPLIT, split_elems * sizeof(uint16_t));
  }
  return PBD_OK;
}

FrameBases frame_bases(const FrameLayout& lay, char* const* regions) {
  FrameBases b{};
  for (int i = 0; i < FB_COUNT; ++i)
    b.p[i] = lay.buf[i].region < 0 ? nullptr : regions[lay.buf[i].region] + lay.buf[i].offset;
  return b;
}

// ---------------------------------------------------------------------------
// DT task lists
// ---------------------------------------------------------------------------
// DT block geometry under an LDS budget.  stride = LDS elements per line: >= len + 1 and ODD — the (y, z) pairs of
// element e of consecutive lines are then 2 * (stride mod 32) banks apart instead of in the same banks (lanes of
// different lines work on similar element indices at the same time: with an even stride of 160 every LDS access
// of the scan was an lpb-way bank conflict); lpb = lines per block: 4 .. lanes of the block (plain), or a whole
// number of rows x the K mixtures of the part (fold: unit = K).
int dt_stride_for(int len) { return (len + 1) | 1; }
static int dt_lpb_for(int stride, int len, int unit, size_t budget, int ts, int nt, int seg, bool round_lanes) {
  const int lmin = unit > 1 ? unit : 4;
  int lpb = std::min(nt, 128);   // at most one line per lane
  if (unit > 1) lpb = std::max(unit, lpb / unit * unit);
  while (lpb > lmin && dt_lds_bytes(stride, lpb, ts, nt) > budget) lpb -= (unit > 1 ? unit : 1);
  // plain: the nt / lpb lanes of a line are a whole number, so 45 lines that fit would leave 128 - 2 * 45 lanes idle and
  // every line with two segments where 42 lines get three: the largest lpb <= the fit that uses all lanes
  if (round_lanes && unit <= 1 && lpb > lmin) lpb = std::max(lmin, nt / ((nt + lpb - 1) / lpb));
  // The nt / lpb lanes that share a line scan one segment of it each (dt_core.hpp), and a block lasts as long as
  // its segments are: with a target segment length, lines are given up for lanes per line where the budget
  // would put so many lines into a block that each is left with one or two lanes.
  if (seg > 0) {
    const int P = std::max(1, std::min(nt / 4, (len + seg - 1) / seg));
    int cap = std::max(lmin, nt / P);
    if (unit > 1) cap = std::max(unit, cap / unit * unit);
    lpb = std::min(lpb, cap);
  }
  return lpb;
}
// (pbd_plan.hpp)
DtGroup dt_group(int map0, int nmaps, int nlines, int len, size_t budget, int ts, int nt, int seg, bool natural, int fold, bool round_lanes) {
  DtGroup g{};
  g.map0 = map0; g.nmaps = nmaps; g.nlines = nlines; g.len = len; g.fold = fold;
  g.fused = natural ? DT_G_NATURAL : 0;   // marks the x pass (pbd_plan.hpp; DT_G_FUSED: dt_mark_fused)
  g.stride = dt_stride_for(len);
  g.lpb = dt_lpb_for(g.stride, len, fold >= 0 ? nmaps : 1, budget, ts, nt, seg, round_lanes);
  // wave-uniform quotients of the block's index arithmetic, as constants (pbd_internal.hpp)
  g.nsub = nt / g.lpb;
  g.P = dt_segments(g.nsub, len);
  g.chunk = (len + g.nsub - 1) / g.nsub;
  g.magic_lpb = dt_magic((unsigned)g.lpb);
  g.magic_nlines = dt_magic((unsigned)nlines);
  g.magic_P = dt_magic((unsigned)g.P);
  return g;
}
// maps: the descriptor table the group indexes (plain groups: a block whose lines are contiguous in memory gets their address, DtTask::src0)
void dt_add_tasks(const DtGroup& g, std::vector<DtTask>& out, const std::vector<DtMap>* maps, int ts) {
  if (g.fold >= 0) {
    const int R = g.lpb / g.nmaps;
    for (int r0 = 0; r0 < g.nlines; r0 += R) out.push_back(DtTask{r0, std::min(R, g.nlines - r0) * g.nmaps, 0, r0, g, nullptr});
  } else {
    const int total = g.nmaps * g.nlines;
    const size_t map_bytes = (size_t)g.nlines * g.len * ts;
    for (int g0 = 0; g0 < total; g0 += g.lpb) {
      DtTask t{g0, std::min(g.lpb, total - g0), g0 / g.nlines, g0 % g.nlines, g, nullptr};
      if (maps && g.len > 1) {
        const int mlast = (g0 + t.nl - 1) / g.nlines;
        bool contig = true;
        for (int m = t.m0; m < mlast && contig; ++m)
          contig = (const char*)(*maps)[(size_t)g.map0 + m + 1].src == (const char*)(*maps)[(size_t)g.map0 + m].src + map_bytes;
        if (contig) t.src0 = (const char*)(*maps)[(size_t)g.map0 + t.m0].src + (size_t)t.l0 * g.len * ts;
      }
      out.push_back(t);
    }
  }
}
// DtGroup::fused (dt_core.hpp: dt_isect's FUSED form, the read-out's fused sum): float maps whose a and b are converted floats — the model's
// weights always (dt_map), pbd_dt2d's caller may hand in any double — on lines short enough for the products to be exact in fp64
void dt_mark_fused(std::vector<DtTask>& tasks, const DtMap* maps, int ts) {
  for (DtTask& t : tasks) {
    DtGroup& g = t.g;
    bool ok = ts == 4 && g.len <= DT_FUSE_MAXLEN;
    for (int m = 0; m < g.nmaps && ok; ++m) {
      const DtMap& mp = maps[g.map0 + m];
      ok = (double)(float)mp.a == mp.a && (double)(float)mp.b == mp.b && (long long)g.len + std::abs((long long)mp.os) <= DT_FUSE_MAXLEN;
    }
    if (ok) g.fused |= DT_G_FUSED;
  }
}
int dt_ptr_bytes_for(int maxlen) { return dt_stride_for(maxlen) <= 256 ? 1 : 2; }
void dt_mark_ptr8(std::vector<DtTask>& tasks) {
  for (DtTask& t : tasks) t.g.fused |= DT_G_PTR8;
}
DtMap dt_map(const void* src, void* dst, void* ptr, float wq, float wl, int os, int natural) {
  DtMap m{};
  m.src = src; m.dst = dst; m.ptr = ptr;
  m.a = -(double)wq; m.b = -(double)wl;      // Quadratic fx(-w0, -w1), fy(-w2, -w3) (src/DynamicProgram.cpp:125-127)
  m.r2a = 1.0 / (2.0 * m.a);                 // IEEE division (dt_core.hpp: dt_isect)
  m.os = os; m.ptr_natural = natural;
  return m;
}

// ---------------------------------------------------------------------------
// frame tables
// ---------------------------------------------------------------------------
// image pyramid jobs: the first octave of every frame from the frame (tightly packed, back to back), then the chains
static void pyramid_jobs(const HostModel& hm, const FrameSpec& f, const FrameLayout& lay, FrameTables& out) {
  const int n1 = lay.nlevels, interval = hm.md.interval;
  std::vector<PyrJob>& jobs = out.pyrjobs;
  PyrLaunch R{0, 0, 1, 1, 1};
  for (int fr = 0; fr < f.batch; ++fr)
    for (int i = 0; i < interval; ++i) {
      const Level& L = lay.lv[fr * n1 + i];
      jobs.push_back(PyrJob{(unsigned long long)fr * f.w * f.h * f.cn * lay.src_esz, (unsigned long long)L.img_off, f.w, f.h, L.iw, L.ih});
      R.maxpix = std::max(R.maxpix, L.iw * L.ih);
    }
  R.njobs = (int)jobs.size();
  out.pyr_launches.push_back(R);
  for (int base = interval; base < n1; base += interval) {
    PyrLaunch D{(int)jobs.size(), 0, 1, 1, 1};
    for (int fr = 0; fr < f.batch; ++fr)
      for (int j = base; j < std::min(base + interval, n1); ++j) {
        const Level &S = lay.lv[fr * n1 + j - interval], &L = lay.lv[fr * n1 + j];
        jobs.push_back(PyrJob{(unsigned long long)S.img_off, (unsigned long long)L.img_off, S.iw, S.ih, L.iw, L.ih});
        D.maxpix = std::max(D.maxpix, L.iw * L.ih);
        D.maxw = std::max(D.maxw, L.iw); D.maxh = std::max(D.maxh, L.ih);
      }
    D.njobs = (int)jobs.size() - D.job0;
    out.pyr_launches.push_back(D);
  }
}

// PBD_PYRAMID_MATLAB: the same launches — the first octave of every frame (area resize from the 8-bit frame, its tap lists per level
// and axis shared by the frames of a batch), then one launch per further octave (reduce)
static bool pyramid_jobs_matlab(const HostModel& hm, const FrameSpec& f, const FrameLayout& lay, FrameTables& out) {
  const int n1 = lay.nlevels, interval = hm.md.interval;
  std::vector<MatJob>& jobs = out.matjobs;
  std::vector<int> yrun0((size_t)interval), xrun0((size_t)interval);
  for (int i = 0; i < interval; ++i) {
    const Level& L = lay.lv[i];
    yrun0[i] = (int)out.matruns.size();
    if (!resize_taps(f.h, L.ih, out.matruns, out.mattaps)) return false;   // resize.cc:101: the rows axis first
    xrun0[i] = (int)out.matruns.size();
    if (!resize_taps(f.w, L.iw, out.matruns, out.mattaps)) return false;   // :102
  }
  PyrLaunch R{0, 0, 1, 1, 1};
  for (int fr = 0; fr < f.batch; ++fr)
    for (int i = 0; i < interval; ++i) {
      const Level& L = lay.lv[fr * n1 + i];
      jobs.push_back(MatJob{(unsigned long long)fr * f.w * f.h * f.cn * lay.src_esz, (unsigned long long)L.img_off, f.w, f.h, L.iw, L.ih, yrun0[i], xrun0[i]});
      R.maxpix = std::max(R.maxpix, L.iw * L.ih);
    }
  R.njobs = (int)jobs.size();
  out.pyr_launches.push_back(R);
  for (int base = interval; base < n1; base += interval) {
    PyrLaunch D{(int)jobs.size(), 0, 1, 1, 1};
    for (int fr = 0; fr < f.batch; ++fr)
      for (int j = base; j < std::min(base + interval, n1); ++j) {
        const Level &S = lay.lv[fr * n1 + j - interval], &L = lay.lv[fr * n1 + j];
        jobs.push_back(MatJob{(unsigned long long)S.img_off, (unsigned long long)L.img_off, S.iw, S.ih, L.iw, L.ih, 0, 0});
        D.maxpix = std::max(D.maxpix, L.iw * L.ih);
        D.maxw = std::max(D.maxw, L.iw); D.maxh = std::max(D.maxh, L.ih);
      }
    D.njobs = (int)jobs.size() - D.job0;
    out.pyr_launches.push_back(D);
  }
  return true;
}

// HOG tiles: TC x TC cells, the tile shrunk until its LDS footprint fits; filter-bank tiles: 16 x 16 cells
static int hog_conv_tiles(const HostModel& hm, const FrameSpec& f, const FrameLayout& lay, FrameTables& out, std::string* err) {
  const int sbin = hm.md.sbin;
  const int hog_bpp = lay.esz == 1 ? 3 : f.cn * lay.esz;    // (8-bit frames: the tile side does not depend on the channel count)
  out.hog_tc = 16;
  while (out.hog_tc > 2 && hog_lds_bytes(sbin, out.hog_tc, hm.ts, hog_bpp) > 150 * 1024) out.hog_tc /= 2;
  if (hog_lds_bytes(sbin, out.hog_tc, hm.ts, hog_bpp) > 150 * 1024) return fail(err, PBD_ERR_UNSUPPORTED, "sbin too large");
  std::vector<ConvTile> ct;
  for (int l = 0; l < lay.nvl; ++l) {
    const Level& L = lay.lv[l];
    if (!has_cells(L)) continue;
    for (int y = 0; y < L.ch - 2 * hm.pad; y += out.hog_tc)   // (the interior: the border ring is k_featpad's)
      for (int x = 0; x < L.cw - 2 * hm.pad; x += out.hog_tc) out.hog_tiles.push_back(HogTile{l, y, x, 0});
    for (int y = 0; y < L.ch; y += 16)
      for (int x = 0; x < L.cw; x += 16) ct.push_back(ConvTile{l, y, x, 0});
  }
  // The filter bank runs tile position 8 g + x of this list on XCD x (k_conv.hip: groups of 8 tiles, all n-tiles of a
  // tile on one XCD).  Horizontally adjacent tiles write the two halves of the same 128-byte lines of every response
  // plane (a tile row is 64 bytes); in list order they sat on DIFFERENT XCDs, whose L2s cannot merge the halves
  // (WRITE_SIZE 124 MB for 88 MB of responses).  Pairs of neighbours (2k, 2k + 1) go to the same XCD, one group apart.
  out.conv_tiles = ct;
  const size_t full = ct.size() / 16 * 16;
  for (size_t b = 0; b < full; b += 16)
    for (size_t x = 0; x < 8; ++x) { out.conv_tiles[b + x] = ct[b + 2 * x]; out.conv_tiles[b + 8 + x] = ct[b + 2 * x + 1]; }
  if (hm.mixed)   // one copy of the list per size group, the group's planes in the tiles' pad (ConvTile)
    for (const SizeGroup& g : hm.groups)
      for (ConvTile t : out.conv_tiles) { t.pad = g.n0 | (g.nf << 16); out.conv_tiles_mix.push_back(t); }
  return PBD_OK;
}

// DT block size and LDS budget of the frame
static int dt_geometry(const HostModel& hm, const FrameLayout& lay, int dt_geom, const PlanKnobs& kn, FrameTables& out, std::string* err) {
  // DT LDS budget per block unless the longest line needs more at the minimum number of lines per block
  const int maxlen = plan_maxlen(lay.lv);
  // block geometry, measured on MI355X (profiles/sweep_dt.sh).  float, lines with 16-bit links: two wavefronts and
  // 25 KB per block = 6 blocks = 3 wavefronts per SIMD (20 .. 40 KB swept); double (17 B per line element, an IEEE division
  // per intersection): one wavefront and 20 KB = 8 blocks per CU (0.93 ms against 1.28 with the float geometry)
  // Round 4 (profiles/experiments/README.md, seven frame sizes): while every line of the frame is short enough for byte links
  // (stride <= 256: 9 B per line element), float blocks of FOUR wavefronts and 40 KB — 4 blocks = 4 wavefronts per SIMD — beat
  // the two-wavefront / 25 KB blocks by 2-8 % of dp_min in batches (640x480: 0.328 -> 0.314 ms per frame, 0.600 -> 0.581 alone);
  // with 16-bit links (10 B per element: 1280x720, 1920x1080) they lose 9-12 %, and there the geometry above stays.
  const bool byte_links = lay.ptr_bytes == 1;   // (= dt_stride_for(maxlen) <= 256: plan_layout)
  // double (17 B per line element): two wavefronts and 40 KB per block — round 4, session 34: 0.473 / 0.721 ms per frame (batches / alone)
  // against 0.485 / 0.770 with one wavefront and 20 KB; round 5, session 3: 0.477 against 0.497 in batches, 893 against 879 frames/s
  // pbd_tune_plan: the other geometry measured on this handle's own frames (results are bit-identical under any geometry)
  const bool big_blocks = hm.ts == 4 && dt_geom ? dt_geom == 1 : byte_links;
  out.dt_nt = hm.ts == 8 ? 128 : (big_blocks ? 256 : PBD_DT_NT_DEFAULT);
  if (kn.dt_nt) out.dt_nt = kn.dt_nt;
  size_t dt_base = (hm.ts == 8 ? 40 : (big_blocks ? 40 : 25)) * 1024;
  if (kn.dt_budget_kb >= 0) dt_base = (size_t)kn.dt_budget_kb * 1024;
  if (kn.dt_budget_b >= 0) dt_base = (size_t)kn.dt_budget_b;
  int max_mix = 4;
  if (hm.fold) for (const PartInfo& P : hm.parts) max_mix = std::max(max_mix, P.K);
  const size_t dt_need = dt_lds_bytes(dt_stride_for(maxlen), max_mix, hm.ts, out.dt_nt);   // the longest line at the fewest lines a block can hold
  if (dt_need > 160 * 1024) return fail(err, PBD_ERR_UNSUPPORTED, "pyramid level too large for the LDS-resident distance transform");
  out.dt_lds = std::max(dt_base, dt_need);
  return PBD_OK;
}

// Where the planes of one frame live, from the buffers' bases
struct PlaneAddr {
  const HostModel& hm;
  const FrameLayout& lay;
  const FrameBases& b;
  std::vector<size_t> part_scr, lvl_scr;   // plane offset of (part, level, mixture) in the per-map DT planes: parts in flat order, levels inside
  PlaneAddr(const HostModel& hm_, const FrameLayout& lay_, const FrameBases& b_) : hm(hm_), lay(lay_), b(b_), part_scr(hm_.parts.size(), 0), lvl_scr(lay_.nvl, 0) {
    size_t o = 0;
    for (size_t fp = 0; fp < hm.parts.size(); ++fp) if (hm.parts[fp].p > 0) { part_scr[fp] = o; o += (size_t)hm.parts[fp].K * lay.act_cells; }
    o = 0;
    for (int l = 0; l < lay.nvl; ++l) { lvl_scr[l] = o; if (lay.lv[l].active) o += (size_t)lay.lv[l].cw * lay.lv[l].ch; }   // prefix of active cells
  }
  size_t hw(int l) const { return (size_t)lay.lv[l].cw * lay.lv[l].ch; }
  size_t scr_of(int fp, int l, int mm) const { return part_scr[fp] + (size_t)hm.parts[fp].K * lvl_scr[l] + (size_t)mm * hw(l); }
  char* resp(int l, int fid) const { return b.p[FB_RESP] + (lay.lv[l].cell_off * hm.md.nfilters + (size_t)fid * hw(l)) * hm.ts; }
  char* acc(int l, int slot) const { return b.p[FB_ACC] + (lay.lv[l].cell_off * hm.nslots + (size_t)slot * hw(l)) * hm.ts; }
  // compact: the transformed scores of (part, mixture) live in the mixture's own response plane
  char* sdt(int fp, int l, int mm) const { return lay.compact ? resp(l, hm.parts[fp].filterid[mm]) : b.p[FB_DT_SDT] + scr_of(fp, l, mm) * hm.ts; }
  uint8_t* ik(int l, int plane0) const { return (uint8_t*)b.p[FB_PK] + lay.lv[l].cell_off * hm.nplanes + (size_t)plane0 * hw(l); }
};

// FoldJob of part fp at level l (its children's messages, children in descending flat index); -1 without children
static int make_fold(const HostModel& hm, const PlaneAddr& pa, const std::vector<int>& children, int fp, int l, FrameTables& out) {
  if (children.empty()) return -1;
  std::vector<FoldJob>& folds = out.folds;
  FoldJob J{};
  for (int c : children) {
    const PartInfo& C = hm.parts[c];
    out.pick[(size_t)l * hm.parts.size() + c] = folds.size() * sizeof(FoldJob) + offsetof(FoldJob, ch) + (size_t)J.nch * sizeof(FoldChild);
    FoldChild& F = J.ch[J.nch++];
    F.K = C.K; F.L = hm.parts[fp].K;
    for (int k = 0; k < PBD_FOLD_MAXMIX; ++k) F.sdt[k] = pa.sdt(c, l, std::min(k, C.K - 1));
    const int Lp = hm.parts[fp].K;
    for (int k = 0; k < PBD_FOLD_MAXMIX; ++k)
      for (int mm = 0; mm < PBD_FOLD_MAXMIX; ++mm)
        F.bias[k][mm] = hm.biasw[C.biasid[std::min(k, C.K - 1)] + std::min(mm, Lp - 1)];
    F.ok = pa.ik(l, C.plane0);
  }
  folds.push_back(J);
  return (int)folds.size() - 1;
}

// Launch geometry of a plain (not fold) DT launch: the base budget with full-lane lines per block if all blocks of the launch are then
// resident at once; else the same without the rounding; else the smallest larger budget that makes them resident (fewer, larger
// blocks; up to 1.6 x); else the base.  (Measured: budgets BELOW the base — more, shorter blocks, 8 per CU — are slower: dp_min
// 0.79 / 0.82 ms fold / three-kernel against 0.72 / 0.76, more contention per CU.)  A launch whose blocks do not all fit on the chip
// at once lasts two block times instead of one.
// Fold launches keep the base budget: their blocks hold whole rows of all mixtures and quantise badly (1772 blocks for 1536 slots
// in the 4-part rounds), but the budgets that make them resident at once (36-40 KB, 4 per CU) cost more with four frames in flight
// than the second wave of blocks does (measured: 1 170 frames/s and dp_min 0.70 ms at 40 KB, 1 181 / 0.73 at 28 KB, 1 235 / 0.725
// at the base 25 KB).
struct Geo { size_t budget; bool round; };
static Geo launch_geometry(const HostModel& hm, const FrameLayout& lay, const std::vector<int>& rnd, size_t base, bool fold_x, bool ypass,
                           int nt, int seg, int ncu) {
  if (fold_x) return Geo{base, true};
  int nm = 0;
  for (int fp : rnd) nm += hm.parts[fp].K;
  const int waves_blk = std::max(1, nt / 64);
  auto resident = [&](size_t budget, bool round_lanes) {
    size_t nb = 0, lds = 0;
    for (const Level& L : lay.lv) {
      if (!has_cells(L)) continue;
      const int len = ypass ? L.ch : L.cw, nlines = ypass ? L.cw : L.ch;
      const DtGroup g = dt_group(0, nm, nlines, len, budget, hm.ts, nt, seg, !ypass, -1, round_lanes);
      nb += ((size_t)nm * nlines + g.lpb - 1) / g.lpb;
      lds = std::max(lds, dt_lds_bytes(g.stride, g.lpb, hm.ts, nt));
    }
    const size_t per_cu = std::min<size_t>(160 * 1024 / std::max<size_t>(lds, 1), 24 / waves_blk);
    return nb <= per_cu * ncu;
  };
  if (resident(base, true)) return Geo{base, true};
  if (resident(base, false)) return Geo{base, false};
  for (size_t b = base + 1024; b <= base * 8 / 5 && b <= 150 * 1024; b += 1024) {
    if (resident(b, true)) return Geo{b, true};
    if (resident(b, false)) return Geo{b, false};
  }
  return Geo{base, true};
}

// Workgroup b runs on XCD b % 8, each with its own L2.  A block writes its lines transposed, i.e. runs of a few
// elements — a fraction of a 128-byte line; the neighbouring runs belong to the next tasks of the same map.
// Order a launch's table so that `c` consecutive tasks share an XCD and the partial lines merge in one
// L2 instead of going out to HBM from several.
static void xcd_order(std::vector<DtTask>& v, int c) {
  if (c <= 0) return;
  const size_t win = (size_t)8 * c, full = v.size() / win * win;
  std::vector<DtTask> o(v);
  for (size_t b = 0; b < full; ++b) {
    const size_t xcd = b & 7, idx = b >> 3;
    o[b] = v[((idx / c) * 8 + xcd) * c + idx % c];
  }
  v.swap(o);
}
static size_t launch_lds(const std::vector<DtTask>& v, int ts, int nt) {
  size_t lds = 0;
  for (const DtTask& t : v) lds = std::max(lds, dt_lds_bytes(t.g.stride, t.g.lpb, ts, nt));
  return lds;
}

// One round's DT launches: the maps of every active level, the x and y tasks, and (fold) the x tasks' loader records
static void dt_round(const HostModel& hm, const FrameLayout& lay, const PlaneAddr& pa, const std::vector<std::vector<int>>& children,
                     size_t r, int ncu, const PlanKnobs& kn, const std::vector<char>& slot_init, FrameTables& out, RoundLaunch& R) {
  const std::vector<int>& rnd = hm.rounds[r];
  const bool fold = hm.fold, fold_x = fold && r > 0;   // round 0 = the leaves: their lines are their raw responses
  const int ts = hm.ts, nt = out.dt_nt, seg = kn.dt_seg;
  const Geo geox = launch_geometry(hm, lay, rnd, out.dt_lds, fold_x, false, nt, seg, ncu);
  const Geo geoy = launch_geometry(hm, lay, rnd, out.dt_lds, false, true, nt, seg, ncu);
  size_t roundK = 0;   // maps transformed in this round (per level)
  for (int fp : rnd) roundK += hm.parts[fp].K;
  std::vector<DtMap>& maps = out.maps;
  std::vector<DtTask> xt, yt;
  for (int l = 0; l < lay.nvl; ++l) {
    const Level& L = lay.lv[l];
    if (!has_cells(L)) continue;
    const size_t HW = (size_t)L.cw * L.ch;
    const int gx_map0 = (int)maps.size();
    int gx_nmaps = 0;
    std::vector<DtMap> ymaps;
    size_t tmp_round = 0;   // fold: maps of this level in front of the part's, in the round's x-pass output (level-major: all maps of a
                            // level back to back, so that every block of the y pass reads ONE contiguous run — DtTask::src0)
    for (int fp : rnd) {
      const PartInfo& P = hm.parts[fp];
      const int part_map0 = (int)maps.size();
      for (int mm = 0; mm < P.K; ++mm) {
        const int fid = P.filterid[mm], did = P.defid[mm];
        const size_t so = pa.scr_of(fp, l, mm);
        const size_t to = fold ? roundK * pa.lvl_scr[l] + (tmp_round + (size_t)mm) * HW : so;
        const char* src = (!fold && slot_init[P.slot[mm]]) ? pa.acc(l, P.slot[mm]) : pa.resp(l, fid);
        const float* wv = &hm.defw[(size_t)did * 4];
        char* tmp = pa.b.p[FB_DT_TMPT] + to * ts;
        maps.push_back(dt_map(src, tmp, pa.b.p[FB_DT_IXT] + so * (size_t)lay.ptr_bytes, wv[0], wv[1], hm.anchors[did * 2], 1));
        ymaps.push_back(dt_map(tmp, pa.sdt(fp, l, mm), pa.b.p[FB_DT_IY] + so * (size_t)lay.ptr_bytes, wv[2], wv[3], hm.anchors[did * 2 + 1], 0));
        gx_nmaps++;
      }
      tmp_round += (size_t)P.K;
      if (fold_x) dt_add_tasks(dt_group(part_map0, P.K, L.ch, L.cw, geox.budget, ts, nt, seg, true, make_fold(hm, pa, children[fp], fp, l, out)), xt);
    }
    if (!fold_x) dt_add_tasks(dt_group(gx_map0, gx_nmaps, L.ch, L.cw, geox.budget, ts, nt, seg, true, -1, geox.round), xt, &maps, ts);
    const DtGroup gy = dt_group((int)maps.size(), gx_nmaps, L.cw, L.ch, geoy.budget, ts, nt, seg, false, -1, geoy.round);
    for (auto& my : ymaps) maps.push_back(my);
    dt_add_tasks(gy, yt, &maps, ts);
  }
  dt_mark_fused(xt, maps.data(), ts);
  dt_mark_fused(yt, maps.data(), ts);
  if (lay.ptr_bytes == 1) { dt_mark_ptr8(xt); dt_mark_ptr8(yt); }
  xcd_order(xt, kn.xcd_chunk);
  xcd_order(yt, kn.xcd_chunk);
  R.lds_x = launch_lds(xt, ts, nt); R.lds_y = launch_lds(yt, ts, nt); R.fold_x = fold_x ? 1 : 0;
  if (fold_x) {   // the loader's first addresses of every fold x task, in task order
    R.foldx0 = out.foldx.size();
    for (const DtTask& t : xt) {
      const DtGroup& g = t.g;
      for (int mm = 0; mm < 8; ++mm) out.foldx.push_back((unsigned long long)(uintptr_t)maps[(size_t)g.map0 + std::min(mm, g.nmaps - 1)].src);
      const unsigned long long* cq = (const unsigned long long*)&out.folds[(size_t)g.fold].ch[0];   // sdt[8], ok (k_dp.hip: fold_child_qw)
      for (int i = 0; i < 9; ++i) out.foldx.push_back(cq[i]);
      out.foldx.push_back((unsigned long long)out.folds[(size_t)g.fold].nch);
    }
  }
  R.xtask0 = (int)out.tasks.size(); R.nxtasks = (int)xt.size();
  out.tasks.insert(out.tasks.end(), xt.begin(), xt.end());
  R.ytask0 = (int)out.tasks.size(); R.nytasks = (int)yt.size();
  out.tasks.insert(out.tasks.end(), yt.begin(), yt.end());
}

// legacy (three-kernel) structure: the reduce waves of round r (slot state is advanced once per wave)
static void reduce_waves(const HostModel& hm, const FrameLayout& lay, const PlaneAddr& pa, size_t r, std::vector<char>& slot_init,
                         FrameTables& out, RoundLaunch& R) {
  for (const std::vector<int>& wave : hm.red_rounds[r]) {
    ReduceWave Wv{(int)out.redblk.size(), 0};
    std::vector<int> parents;  // distinct parents, in first-appearance order
    for (int fp : wave) {
      const int pf = hm.part_offset[hm.parts[fp].comp] + hm.parts[fp].parent;
      if (std::find(parents.begin(), parents.end(), pf) == parents.end()) parents.push_back(pf);
    }
    for (int l = 0; l < lay.nvl; ++l) {
      const Level& L = lay.lv[l];
      if (!has_cells(L)) continue;
      const size_t HW = (size_t)L.cw * L.ch;
      for (int pf : parents) {
        const PartInfo& Par = hm.parts[pf];
        ReduceJob J{};
        J.H = L.ch; J.W = L.cw; J.L = Par.K;
        for (int pm = 0; pm < Par.K; ++pm) {
          char* accp = pa.acc(l, Par.slot[pm]);
          J.par_in[pm] = slot_init[Par.slot[pm]] ? accp : pa.resp(l, Par.filterid[pm]);
          J.par_out[pm] = accp;
        }
        for (int fp : wave) {  // `wave` is in descending child order
          const PartInfo& P = hm.parts[fp];
          if (hm.part_offset[P.comp] + P.parent != pf) continue;
          ReduceChild& C = J.ch[J.nch++];
          C.sdt = pa.sdt(fp, l, 0);
          C.ok = pa.ik(l, P.plane0);
          C.K = P.K;
          for (int mm = 0; mm < P.K; ++mm) C.bias_off[mm] = P.biasid[mm];
        }
        for (unsigned c0 = 0; c0 < (unsigned)HW; c0 += 256) out.redblk.push_back(ReduceBlock{(int)out.red.size(), c0});
        out.red.push_back(J);
      }
    }
    for (int pf : parents)
      for (int pm = 0; pm < hm.parts[pf].K; ++pm) slot_init[hm.parts[pf].slot[pm]] = 1;
    Wv.nblks = (int)out.redblk.size() - Wv.blk0;
    R.waves.push_back(Wv);
  }
}

// root jobs + back-tracking info
static void root_tables(const HostModel& hm, const FrameLayout& lay, const PlaneAddr& pa, const std::vector<std::vector<int>>& children,
                        const std::vector<char>& slot_init, FrameTables& out) {
  const int nc = hm.md.ncomponents;
  const size_t ts = (size_t)hm.ts;
  out.back.assign((size_t)lay.nvl * nc, BackLevel{});
  for (int l = 0; l < lay.nvl; ++l) {
    const Level& L = lay.lv[l];
    const size_t HW = (size_t)L.cw * L.ch;
    for (int c = 0; c < nc; ++c) {
      BackLevel& B = out.back[(size_t)l * nc + c];
      B.pk = pa.ik(l, hm.comp_plane0[c]);
      B.rootv = pa.b.p[FB_ROOTV] + (L.cell_off * nc + (size_t)c * HW) * ts;
      B.rooti = (int*)pa.b.p[FB_ROOTI] + L.cell_off * nc + (size_t)c * HW;
      B.H = L.ch; B.W = L.cw; B.scale = L.scale;
      if (!L.active || HW == 0) continue;
      const PartInfo& R0 = hm.parts[hm.part_offset[c]];
      RootJob J{};
      for (int kk = 0; kk < PBD_MAX_MIX; ++kk) {   // entries beyond K repeat mixture K - 1 (the fold's register arrays are never predicated)
        const int k = std::min(kk, R0.K - 1);
        J.score[kk] = (!hm.fold && slot_init[R0.slot[k]]) ? pa.acc(l, R0.slot[k]) : pa.resp(l, R0.filterid[k]);
      }
      J.rootv = (void*)B.rootv; J.rooti = (int*)B.rooti;
      J.H = L.ch; J.W = L.cw; J.K = R0.K; J.level = l; J.comp = c;
      J.bias = hm.biasw[R0.biasid[0]];  // root.bias(0)[0], DynamicProgram.cpp:165
      J.cell0 = out.root_cells;
      J.fold = hm.fold ? make_fold(hm, pa, children[hm.part_offset[c]], hm.part_offset[c], l, out) : -1;   // fold: the root's messages are folded by k_root
      out.root_cells += (unsigned)HW;
      out.root_maxcells = std::max(out.root_maxcells, (unsigned)HW);
      for (unsigned c0 = 0; c0 < (unsigned)HW; c0 += 256) out.rootblk.push_back(ReduceBlock{(int)out.rootjobs.size(), c0});
      out.rootjobs.push_back(J);
    }
  }
}

int plan_tables(const HostModel& hm, const FrameSpec& f, const FrameLayout& lay, const FrameBases& b, int ncu, int dt_geom,
                const PlanKnobs& kn, FrameTables& out, std::string* err) {
  out = FrameTables{};
  if (hm.pyr_kind == PBD_PYRAMID_MATLAB) {
    if (!pyramid_jobs_matlab(hm, f, lay, out)) return fail(err, PBD_ERR_ARG, "PBD_PYRAMID_MATLAB: a resize tap outside the frame (matlab/mex/resize.cc:53,61)");
  } else pyramid_jobs(hm, f, lay, out);
  for (const Level& L : lay.lv)
    out.levels.push_back(LevelDev{L.iw, L.ih, L.bw, L.bh, L.cw, L.ch, (unsigned long long)L.img_off, (unsigned long long)L.cell_off});
  if (hm.pad > 0)
    for (int l = 0; l < lay.nvl; ++l) {
      const Level& L = lay.lv[l];
      const int pad = hm.pad;
      out.hog_levels.push_back(LevelDev{L.iw, L.ih, L.bw, L.bh, L.cw, L.ch, (unsigned long long)L.img_off,
                                        (unsigned long long)(L.cell_off + (size_t)pad * L.cw + pad)});
      if (!has_cells(L)) continue;
      const int nring = L.cw * L.ch - (L.cw - 2 * pad) * (L.ch - 2 * pad);
      for (int r0 = 0; r0 < nring; r0 += PBD_FEATPAD_CPB) out.padblk.push_back(ReduceBlock{(int)out.padjobs.size(), (unsigned)r0});
      out.padjobs.push_back(PadJob{(unsigned long long)L.cell_off, L.cw, L.ch, pad, nring});
    }
  int rc = hog_conv_tiles(hm, f, lay, out, err);
  if (!rc) rc = dt_geometry(hm, lay, dt_geom, kn, out, err);
  if (rc) return rc;
  const PlaneAddr pa(hm, lay, b);
  // children of every part, descending flat index (the order their messages are added in, src/DynamicProgram.cpp:95)
  std::vector<std::vector<int>> children(hm.parts.size());
  for (int fp = (int)hm.parts.size() - 1; fp >= 0; --fp)
    if (hm.parts[fp].p > 0) children[hm.part_offset[hm.parts[fp].comp] + hm.parts[fp].parent].push_back(fp);
  if (hm.fold) out.pick.assign((size_t)lay.nvl * hm.parts.size(), PBD_NO_PICK);   // filled by make_fold
  std::vector<char> slot_init((size_t)hm.nslots, 0);  // legacy: ncscores[fid].empty() emulation (same for every level)
  for (size_t r = 0; r < hm.rounds.size(); ++r) {
    RoundLaunch R{};
    if (!hm.rounds[r].empty()) {
      dt_round(hm, lay, pa, children, r, ncu, kn, slot_init, out, R);
      if (!hm.fold) reduce_waves(hm, lay, pa, r, slot_init, out, R);
    }
    out.rl.push_back(R);
  }
  root_tables(hm, lay, pa, children, slot_init, out);
  // where the DT pointer planes of (level, part) live: back-tracking composes Ix / Iy from them on the fly
  out.scr_base.assign((size_t)lay.nvl * hm.parts.size(), 0);
  for (int l = 0; l < lay.nvl; ++l)
    for (size_t fp = 0; fp < hm.parts.size(); ++fp)
      if (hm.parts[fp].p > 0 && lay.lv[l].active) out.scr_base[(size_t)l * hm.parts.size() + fp] = pa.scr_of((int)fp, l, 0);
  return PBD_OK;
}
