// pbd_post.cpp — the stages behind back-tracking: candidate sort + NMS (k_cand.hip), depth-consistency pruning
// (k_zfilter.hip), 3-D boxes (k_box3d.hip), object clusters (k_cluster3d.hip), per-part scores (k_partscore.hip), the stand-alone
// feature vectors (k_featvec.hip) and the best pose per ground-truth box (k_gtbox.hip).  Their handle buffers, their launches behind k_backtrack, the collect's gathering of their results
// and their C entry points (pbd_set_*, pbd_get_box3d, pbd_get_cluster3d, pbd_get_part_scores, pbd_candidates_*).  pbd_api.cpp calls in
// through the pbd_i_* functions of pbd_internal.hpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include "pbd_internal.hpp"
#include "gt_overlap.hpp"

// the depth image of a stand-alone call: NULL only with an empty size
static int depth_image_args(pbd_handle* h, const void* depth, int dw, int dh, bool* empty) {
  if (dw < 0 || dh < 0 || (!depth && dw > 0 && dh > 0)) return fail(h, PBD_ERR_ARG, "depth image: NULL only with an empty size");
  *empty = !depth || dw == 0 || dh == 0;
  return PBD_OK;
}

// ---- candidate sort + NMS (k_cand.hip) -----------------------------------------------------------------------------------
static CandFilterArgs cand_args(pbd_handle* h, int mode, float overlap, int im_w, int im_h) {
  CandFilterArgs a{};
  a.in.capacity = h->opt.max_candidates; a.in.stride = h->cand_stride; a.in.mp = h->max_parts;
  a.ts = h->ts; a.ncomp = h->md.ncomponents;
  a.nms = mode == PBD_CAND_SORT_NMS; a.overlap = (double)overlap; a.im_w = im_w; a.im_h = im_h;
  a.keys = h->d_cf_keys; a.idx = h->d_cf_idx; a.box = h->d_cf_box; a.st = h->d_cf_st;
  return a;
}
// the filter's scratch: model-sized once (first use), the per-frame masks with the frame plan.  Called outside any capture;
// a (re)allocation drops a captured graph (its launches point at the old buffers).
static int cand_filter_buffers(pbd_handle* h, bool masks) {
  const size_t cap = (size_t)h->opt.max_candidates;
  if (!h->d_cf_keys) {
    int rc;
    if ((rc = model_alloc(h, &h->d_cf_keys, 2 * cap)) || (rc = model_alloc(h, &h->d_cf_idx, 2 * cap)) ||
        (rc = model_alloc(h, &h->d_cf_box, 4 * cap)) || (rc = model_alloc(h, &h->d_cf_st, cap)) ||
        (rc = model_alloc(h, &h->d_cand_raw, h->cand_stride * cap)) ||
        (rc = model_alloc(h, &h->d_cf_cnt, 2 + 2 * PBD_MAX_BATCH, false, false)) ||   // (the counts were never part of the footprint)
        (rc = model_alloc(h, &h->h_cf_cnt, 2 + 2 * PBD_MAX_BATCH, true, false)))
      return rc;
    drop_graph(h);
  }
  if (masks && h->fw > 0) {
    const size_t need = cand_filter_mask_bytes(h->fw, h->fh) * h->batch;
    if (need > h->cf_mask_bytes) {
      int rc = dev_alloc(h, &h->d_cf_mask, need / sizeof(unsigned long long));
      if (rc) return rc;
      h->cf_mask_bytes = need;
      drop_graph(h);
    }
  }
  return PBD_OK;
}

// ---- part-wise overlap NMS (k_cand_parts.hip) ----------------------------------------------------------------------------
static bool parts_nms(const pbd_handle* h, int cm) { return cm == PBD_CAND_SORT_NMS && h->cand_nms == PBD_NMS_PARTS; }
// the kept record's rectangles and areas travel through dynamic LDS: 40 bytes per rectangle
static int cand_parts_lds_ok(pbd_handle* h) {
  return (size_t)(h->max_parts + 1) * 40 <= 32768 ? PBD_OK : fail(h, PBD_ERR_UNSUPPORTED, "parts NMS: more than 818 parts per component");
}
static CandPartsArgs cand_parts_args(const pbd_handle* h, float overlap, int top, int capacity) {
  CandPartsArgs p{};
  p.stride = h->cand_stride; p.mp = h->max_parts; p.capacity = capacity;
  p.overlap = (double)overlap; p.top = top;
  return p;
}
// the sort's staging buffer and the rectangle planes: model-sized, on the first frame that needs them.  Called outside any capture.
static int cand_parts_buffers(pbd_handle* h) {
  if (h->d_cp_stage) return PBD_OK;
  const size_t cap = (size_t)h->opt.max_candidates;
  int rc;
  if ((rc = cand_parts_lds_ok(h)) || (rc = model_alloc(h, &h->d_cp_stage, h->cand_stride * cap)) ||
      (rc = model_alloc(h, &h->d_cp_cnt, 2 + 2 * PBD_MAX_BATCH)) || (rc = model_alloc(h, &h->d_cp_rect, (size_t)(h->max_parts + 2) * cap)) ||
      (rc = model_alloc(h, &h->d_cp_np, cap)) || (rc = model_alloc(h, &h->d_cp_kept, cap)) ||
      (rc = model_alloc(h, &h->d_cp_bits, cand_parts_bits_words((int)cap, PBD_MAX_BATCH))))
    return rc;
  drop_graph(h);
  return PBD_OK;
}

// ---- depth-consistency pruning (k_zfilter.hip) ----------------------------------------------------------------------
// per (component, part): parentid and norm(anchor(0)) * zfactor, the reference's double expression (src/SearchSpacePruning.cpp:82-88):
// anchor(0) = anchors[defid[first mixture of the part]] (include/Parts.hpp:183), whatever mixture the candidate chose
static void zf_table(const pbd_handle* h, float zfactor, std::vector<int>& npart, std::vector<int>& par, std::vector<double>& thr) {
  const int nc = h->md.ncomponents, mp = h->max_parts;
  npart.assign((size_t)nc, 0); par.assign((size_t)nc * mp, 0); thr.assign((size_t)nc * mp, 0.0);
  for (int c = 0; c < nc; ++c) {
    const int f0 = h->part_offset[c], np = h->part_offset[c + 1] - f0;
    npart[c] = np;
    for (int p = 1; p < np; ++p) {
      const int did = h->defid[h->mix_offset[f0 + p]];
      const double ax = h->anchors[did * 2], ay = h->anchors[did * 2 + 1];
      par[(size_t)c * mp + p] = h->parentid[f0 + p];
      thr[(size_t)c * mp + p] = std::sqrt(ax * ax + ay * ay) * (double)zfactor;
    }
  }
}
// the pruning's device state: allocated on the first depth-carrying frame with the setting on; the table follows zfactor.
// Called outside any capture (depth-carrying frames run their launches eagerly).
static int zf_buffers(pbd_handle* h) {
  int rc = cand_filter_buffers(h, pbd_i_cand_mode(h) == PBD_CAND_SORT_NMS && !parts_nms(h, pbd_i_cand_mode(h)));   // (d_cand_raw: the back-tracking's device output)
  if (rc) return rc;
  const size_t cap = (size_t)h->opt.max_candidates, nc = (size_t)h->md.ncomponents, mp = (size_t)h->max_parts;
  if (!h->d_zf_med) {
    if ((rc = model_alloc(h, &h->d_zf_npart, nc)) || (rc = model_alloc(h, &h->d_zf_par, nc * mp)) ||
        (rc = model_alloc(h, &h->d_zf_thr, nc * mp)) || (rc = model_alloc(h, &h->d_zf_med, cap * mp)) ||
        (rc = model_alloc(h, &h->d_zf_large, cap * mp)) || (rc = model_alloc(h, &h->d_zf_cnt, 2)) ||
        (rc = model_alloc(h, &h->d_zf_out, h->cand_stride * cap)))
      return rc;
    h->zf_thr_factor = std::nanf("");
  }
  if (!(h->zf_thr_factor == h->zf_factor)) {
    std::vector<int> npart, par; std::vector<double> thr;
    zf_table(h, h->zf_factor, npart, par, thr);
    HIPCHK(h, hipMemcpy(h->d_zf_npart, npart.data(), sizeof(int) * nc, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->d_zf_par, par.data(), sizeof(int) * nc * mp, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->d_zf_thr, thr.data(), sizeof(double) * nc * mp, hipMemcpyHostToDevice));
    h->zf_thr_factor = h->zf_factor;
  }
  return PBD_OK;
}
static int zf_type(const pbd_handle* h) { return h->ts == 8 ? PBD_DEPTH_64F : PBD_DEPTH_32F; }
// the depth arguments of a depth-carrying frame: element type T, rows of >= w elements, stride a multiple of the element size
int pbd_i_depth_check(pbd_handle* h, int depth_type, long long dstride, int w) {
  if (depth_type != zf_type(h))
    return fail(h, PBD_ERR_UNSUPPORTED, h->ts == 8 ? "depth image: PBD_DEPTH_64F for a double handle (Math::median<T> reads it as T)"
                                                   : "depth image: PBD_DEPTH_32F for a float handle (Math::median<T> reads it as T)");
  if (dstride < (long long)w * h->ts || dstride % h->ts) return fail(h, PBD_ERR_ARG, "depth stride: bytes, >= w * element size and a multiple of it");
  return PBD_OK;
}

// ---- 3-D boxes (k_box3d.hip) ------------------------------------------------------------------------------------------
// dog = filter2D(getGaussianKernel(35, 4, CV_32F), (-1, 0, 1) as a column), OpenCV 2.4's arithmetic; its nonzero taps in raster order
static void b3_taps(Box3dArgs& a) {
  const int n = 35;
  float g[35], dog[35];
  double sum = 0;
  for (int i = 0; i < n; ++i) {
    const double x = i - (n - 1) * 0.5;
    g[i] = (float)std::exp(-0.5 / (4.0 * 4.0) * x * x);
    sum += g[i];
  }
  sum = 1. / sum;
  for (int i = 0; i < n; ++i) g[i] = (float)(g[i] * sum);
  for (int i = 0; i < n; ++i) {   // taps -1 and +1 (0 skipped: a zero coefficient), BORDER_REFLECT_101
    const int im = i - 1 < 0 ? 1 - i : i - 1, ip = i + 1 >= n ? 2 * (n - 1) - (i + 1) : i + 1;
    float s = 0.0f;
    s = s + -1.0f * g[im];
    s = s + 1.0f * g[ip];
    dog[i] = s;
  }
  a.ntaps = 0;
  for (int i = 0; i < n; ++i)
    if (dog[i] != 0.0f) { a.tap_off[a.ntaps] = i - (n - 1) / 2; a.tap[a.ntaps] = dog[i]; a.ntaps++; }
}
static bool b3_cam_ok(const pbd_camera* c) {
  return c && std::isfinite(c->fx) && std::isfinite(c->fy) && std::isfinite(c->cx) && std::isfinite(c->cy) && std::isfinite(c->tx) &&
         std::isfinite(c->ty) && c->fx != 0.0 && c->fy != 0.0;
}
static int b3_buffers(pbd_handle* h) {
  if (h->h_b3) return PBD_OK;
  const size_t cap = (size_t)h->opt.max_candidates, mp = (size_t)h->max_parts;
  int rc;
  if ((rc = model_alloc(h, &h->h_b3, cap, true)) || (rc = model_alloc(h, &h->h_b3c, cap * mp * 3, true))) return rc;
  return PBD_OK;
}

// ---- object clusters (k_cluster3d.hip) --------------------------------------------------------------------------------
// Scratch: one slot of a whole cloud's points per concurrent record, as many slots as fit this budget (at least one, at most one
// per record and PBD_CL3_MAX_SLOTS), so that no record can fail for lack of scratch.
#define PBD_CL3_SCRATCH_BUDGET ((size_t)256 << 20)
#define PBD_CL3_MAX_SLOTS 256
static int cl3_slots(int pcap, long long records) {
  const size_t s = PBD_CL3_SCRATCH_BUDGET / cluster3d_slot_bytes(pcap);
  return (int)std::max<long long>(1, std::min<long long>({(long long)s, records, (long long)PBD_CL3_MAX_SLOTS}));
}
static int cl3_buffers(pbd_handle* h) {
  const size_t cap = (size_t)h->opt.max_candidates;
  int rc;
  if (!h->h_cl3 && ((rc = model_alloc(h, &h->h_cl3, cap, true)) || (rc = model_alloc(h, &h->d_cl3_used, 1)))) return rc;
  const int pcap = h->fw * h->fh;
  if (pcap > h->cl3_pcap) {
    const int slots = cl3_slots(pcap, (long long)cap);
    if ((rc = model_grow(h, &h->d_cl3_scratch, h->cl3_pcap, pcap, cluster3d_slot_bytes(pcap) * slots))) return rc;
    h->cl3_slots = slots;
  }
  // grows when a frame's kept clusters need more (cl3_resolve)
  return model_grow(h, &h->d_cl3_pool, h->cl3_pool_cap, 4ull * (unsigned long long)pcap);
}
// After the launch `a` (synchronised): the records `lst` = (record, frame) pairs in output order -> res[] and their kept clusters'
// indices one after the other in idx[].  Records whose indices did not fit the pool run again, alone, into a pool grown to what
// they need (and at least what the launch claimed in all, so that the next launch fits): the handle's own pool, or (s_pool) one of
// the caller's scratch.
static int cl3_resolve(pbd_handle* h, Cluster3dArgs a, int src, int slots, CallScratch* s_pool, const std::vector<int>& lst,
                       std::vector<pbd_cluster3d>& res, std::vector<int32_t>& idx) {
  CallScratch s(h);
  unsigned long long used = 0;
  s.down(&used, a.pool_used, sizeof(used));
  int rc = s.finish("cluster3d: ");
  if (rc) return rc;
  std::vector<int32_t> first((size_t)std::min(used, a.pool_cap));
  s.down(first.data(), a.pool, sizeof(int32_t) * first.size());
  if ((rc = s.finish("cluster3d: "))) return rc;   // (before a growth frees the pool)
  const size_t n = lst.size() / 2;
  std::vector<int> spill;
  std::vector<char> again(n, 0);
  unsigned long long need = 0;
  for (size_t k = 0; k < n; ++k) {
    const Cl3Res& r = a.out[lst[2 * k]];
    if (r.off < 0 && r.r.size > 0) { spill.push_back(lst[2 * k]); spill.push_back(lst[2 * k + 1]); need += r.r.size; again[k] = 1; }
  }
  std::vector<int32_t> second((size_t)need);
  if (!spill.empty()) {
    const unsigned long long ncap = std::max(need, used);
    if (ncap > a.pool_cap) {
      if (s_pool) { a.pool = s_pool->dev<int>(ncap); s.chk(s_pool->e); a.pool_cap = ncap; }
      else {
        if ((rc = model_grow(h, &h->d_cl3_pool, h->cl3_pool_cap, ncap))) return rc;
        a.pool = h->d_cl3_pool; a.pool_cap = h->cl3_pool_cap;
      }
    }
    int* d_list = s.dev<int>(spill.size());
    s.up(d_list, spill.data(), sizeof(int) * spill.size());
    s.zero(a.pool_used, sizeof(unsigned long long));
    if (s.ok()) {
      a.list = d_list; a.nlist = (int)(spill.size() / 2);
      launch_cluster3d(a, src, std::min(slots, a.nlist), h->stream);
      s.launched();
    }
    s.down(second.data(), a.pool, sizeof(int32_t) * need);
  }
  if ((rc = s.finish("cluster3d: "))) return rc;
  res.resize(n);
  idx.clear();
  for (size_t k = 0; k < n; ++k) {
    const Cl3Res& r = a.out[lst[2 * k]];
    res[k] = r.r;
    if (r.r.size <= 0) continue;
    const std::vector<int32_t>& from = again[k] ? second : first;
    if (r.off < 0 || (unsigned long long)r.off + r.r.size > from.size()) return fail(h, PBD_ERR_HIP, "cluster3d: a record's indices are missing");
    idx.insert(idx.end(), from.begin() + r.off, from.begin() + r.off + r.r.size);
  }
  return PBD_OK;
}

// ---- per-part scores (k_partscore.hip) --------------------------------------------------------------------------------
// the model tables (per flat mixture: response plane, bias base, anchor, negated deformation weights) and the pinned results
static std::vector<PsMix> ps_mix_table(const pbd_handle* h) {
  const size_t nm = h->filterid.size(), nfp = h->parts.size();
  std::vector<PsMix> mix(nm);
  for (size_t fp = 0; fp < nfp; ++fp)
    for (int fm = h->mix_offset[fp]; fm < h->mix_offset[fp + 1]; ++fm) {
      PsMix& M = mix[fm];
      M = PsMix{h->filterid[fm], h->biasid[fm], 0, 0, {0.f, 0.f, 0.f, 0.f}};
      if (h->parts[fp].p == 0) continue;   // (a root has no deformation: its defid is ignored)
      const int did = h->defid[fm];
      M.ax = h->anchors[did * 2]; M.ay = h->anchors[did * 2 + 1];
      for (int k = 0; k < 4; ++k) M.w[k] = -h->defw[(size_t)did * 4 + k];
    }
  return mix;
}
static int ps_tables(pbd_handle* h) {
  if (h->d_ps_mix) return PBD_OK;
  const size_t nfp = h->parts.size();
  const std::vector<PsMix> mix = ps_mix_table(h);
  int rc;
  if ((rc = model_alloc(h, &h->d_ps_mix0, nfp + 1)) || (rc = model_alloc(h, &h->d_ps_mix, mix.size()))) return rc;
  HIPCHK(h, hipMemcpy(h->d_ps_mix0, h->mix_offset.data(), sizeof(int) * (nfp + 1), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_ps_mix, mix.data(), sizeof(PsMix) * mix.size(), hipMemcpyHostToDevice));
  return PBD_OK;
}
// the handle's deformation weights have changed (pbd_weights.cpp): the mixture table, if it has been built, written again in place
int pbd_i_ps_reweigh(pbd_handle* h) {
  if (!h->d_ps_mix) return PBD_OK;
  const std::vector<PsMix> mix = ps_mix_table(h);
  HIPCHK(h, hipMemcpy(h->d_ps_mix, mix.data(), sizeof(PsMix) * mix.size(), hipMemcpyHostToDevice));
  return PBD_OK;
}
static int ps_buffers(pbd_handle* h) {
  int rc = ps_tables(h);
  if (rc || h->h_ps) return rc;
  return model_alloc(h, &h->h_ps, (size_t)h->opt.max_candidates * h->max_parts * 3, true);
}
// everything of the launch but the records and the output
static PartScoreArgs ps_args(const pbd_handle* h) {
  PartScoreArgs a{};
  a.levels = h->d_levels; a.nvl = h->nvl;
  a.resp = h->d_resp; a.nfilters = h->md.nfilters;
  a.ncomp = h->md.ncomponents; a.nbias = (int)h->biasw.size();
  a.nparts = h->d_nparts; a.parent = h->d_parent; a.flat = h->d_flat;
  a.mix0 = h->d_ps_mix0; a.mix = h->d_ps_mix; a.biasw = h->d_biasw;
  return a;
}
static const char* const kPsCompact =
    "part scores: this frame runs the compact memory plan (dp_mode 2, or automatic for large frames), whose min() overwrites the "
    "raw response planes the scores are read from";
// the range checks of a stand-alone call's records (part scores, feature vectors): nothing of a record that fails is read on the device
static int check_records(pbd_handle* h, const pbd_candidate_head* heads, const int32_t* locs, int count) {
  const int mp = h->max_parts;
  for (int i = 0; i < count; ++i) {
    const int c = heads[i].component, l = heads[i].level;
    if (c < 0 || c >= h->md.ncomponents) return fail(h, PBD_ERR_ARG, "component out of range");
    const int f0 = h->part_offset[c], np = h->part_offset[c + 1] - f0;
    if (heads[i].nparts != np) return fail(h, PBD_ERR_ARG, "nparts differs from the model's component");
    if (l < 0 || l >= h->nvl || !h->lv[l].active) return fail(h, PBD_ERR_ARG, "level outside the levels this handle processes");
    const int32_t* lc = locs + (size_t)i * mp * 3;
    for (int p = 0; p < np; ++p)
      if (lc[p * 3] < 0 || lc[p * 3] >= h->lv[l].cw || lc[p * 3 + 1] < 0 || lc[p * 3 + 1] >= h->lv[l].ch || lc[p * 3 + 2] < 0 ||
          lc[p * 3 + 2] >= h->parts[f0 + p].K)
        return fail(h, PBD_ERR_ARG, "part location (x, y, mixture) outside its level's cells / the part's mixtures");
  }
  return PBD_OK;
}

// ---- feature vectors (k_featvec.hip) ------------------------------------------------------------------------------------
// the largest window of the bank in elements, and the table beside k_partscore's: per flat mixture its defid and its filter — the
// caller's index and the size pbd_get_filter_size answers with (mixed banks keep filterid in their internal order)
static int fv_wmax(const pbd_handle* h) {
  int m = h->md.kh * h->md.kw;
  if (h->mixed) for (size_t n = 0; n < h->fkh.size(); ++n) m = std::max(m, h->fkh[n] * h->fkw[n]);
  return m * PBD_FLEN;
}
static int fv_tables(pbd_handle* h) {
  int rc = ps_tables(h);
  if (rc || h->d_fv_mix) return rc;
  const size_t nm = h->filterid.size();
  std::vector<int> caller((size_t)h->md.nfilters);
  for (int n = 0; n < h->md.nfilters; ++n) caller[h->mixed ? h->fperm[n] : n] = n;
  std::vector<FvMix> mix(nm);
  for (size_t fm = 0; fm < nm; ++fm) {
    const int f = h->filterid[fm];
    mix[fm] = FvMix{h->defid[fm], caller[f], h->mixed ? h->fkh[f] : h->md.kh, h->mixed ? h->fkw[f] : h->md.kw};
  }
  if ((rc = model_alloc(h, &h->d_fv_mix, nm))) return rc;
  HIPCHK(h, hipMemcpy(h->d_fv_mix, mix.data(), sizeof(FvMix) * nm, hipMemcpyHostToDevice));
  return PBD_OK;
}
static const char* const kFvCompact =
    "feature vectors: this frame runs the compact memory plan (dp_mode 2, or automatic for large frames), whose min() reuses the "
    "memory of the feature planes the windows are read from";
static int fv_upload(pbd_handle* h, const pbd_candidate_head* heads, const int32_t* locs, int count, FeatVecArgs* a);
// every refusal of the three entry points, in the order of the part scores'; then the tables and the records on the device
static int fv_begin(pbd_handle* h, const pbd_candidate_head* heads, const int32_t* locs, int count, const void* blocks, const void* windows,
                    int ts, FeatVecArgs* a) {
  if (count < 0 || (count > 0 && (!heads || !locs || !blocks || !windows))) return fail(h, PBD_ERR_ARG, "heads / locs / blocks / windows / count");
  if (h->in_group) return fail(h, PBD_ERR_UNSUPPORTED, "feature vectors: pbd_group members are not supported");
  if (ts && ts != h->ts) return fail(h, PBD_ERR_STATE, ts == 4 ? "handle is PartsBasedDetector<double>: use the _f64 entry point"
                                                               : "handle is PartsBasedDetector<float>: use the float entry point");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  if (h->fw == 0) return fail(h, PBD_ERR_STATE, "feature vectors: no frame planned");
  if (!h->have_feat) return fail(h, PBD_ERR_STATE, h->compact ? kFvCompact : "feature vectors: features not computed");
  int rc = check_records(h, heads, locs, count);
  if (rc || count == 0) return rc;
  return a ? fv_upload(h, heads, locs, count, a) : PBD_OK;   // (a null: the refusals alone, nothing touches the device)
}
// the tables and the first `count` records on the device; everything of the launch but its outputs
static int fv_upload(pbd_handle* h, const pbd_candidate_head* heads, const int32_t* locs, int count, FeatVecArgs* a) {
  int rc;
  ON_DEVICE(h);
  if ((rc = fv_tables(h))) return rc;
  const int mp = h->max_parts;
  const size_t st = h->cand_stride, n = (size_t)count;
  if ((rc = model_grow(h, &h->d_fv_rec, h->fv_rec_cap, st * n))) return rc;
  std::vector<char> rec(st * n, 0);
  for (size_t i = 0; i < n; ++i) pbd_rec_put(rec.data() + st * i, mp, heads, nullptr, locs, i);
  HIPCHK(h, hipMemcpyAsync(h->d_fv_rec, rec.data(), st * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // (`rec` goes out of scope; earlier work on the stream — the frame — is done too)
  pbd_i_fv_args(h, a);
  a->in.p = h->d_fv_rec; a->in.stride = st; a->in.mp = mp; a->in.capacity = count;
  return PBD_OK;
}
int pbd_i_fv_tables(pbd_handle* h) { return fv_tables(h); }
void pbd_i_fv_args(const pbd_handle* h, FeatVecArgs* a) {
  FeatVecArgs& A = *a;
  A = FeatVecArgs{};
  A.levels = h->d_levels; A.nvl = h->nvl; A.feat = h->d_feat;
  A.ncomp = h->md.ncomponents; A.nbias = (int)h->biasw.size(); A.nfilters = h->md.nfilters;
  A.nparts = h->d_nparts; A.parent = h->d_parent; A.flat = h->d_flat;
  A.mix0 = h->d_ps_mix0; A.mix = h->d_ps_mix; A.fmix = h->d_fv_mix;
  A.wmax = fv_wmax(h);
}
int pbd_i_fv_check(pbd_handle* h, const pbd_candidate_head* heads, const int32_t* locs, int count) {
  return fv_begin(h, heads, locs, count, heads, heads, 0, nullptr);   // (no caller buffers to check: the cache owns the outputs)
}
int pbd_i_fv_upload(pbd_handle* h, const pbd_candidate_head* heads, const int32_t* locs, int count, FeatVecArgs* a) {
  return fv_upload(h, heads, locs, count, a);
}
// the host variants: chunks of records through the staging buffer — a chunk's blocks, then (128-byte aligned) its windows
static int fv_host(pbd_handle* h, const pbd_candidate_head* heads, const int32_t* locs, int count, pbd_feature_block* blocks, void* windows, int ts) {
  FeatVecArgs a;
  int rc = fv_begin(h, heads, locs, count, blocks, windows, ts, &a);
  if (rc || count == 0) return rc;
  const size_t mp = (size_t)h->max_parts, bbytes = mp * sizeof(pbd_feature_block), wbytes = mp * a.wmax * h->ts;
  const size_t chunk = std::max<size_t>(1, (PBD_FEATVEC_STAGING_BYTES - 128) / (bbytes + wbytes));
  if (!h->d_fv_stage && (rc = model_alloc(h, &h->d_fv_stage, std::max<size_t>(PBD_FEATVEC_STAGING_BYTES, bbytes + wbytes + 128)))) return rc;
  char* d_win = h->d_fv_stage + (chunk * bbytes + 127) / 128 * 128;
  for (size_t r0 = 0; r0 < (size_t)count; r0 += chunk) {
    const size_t n = std::min(chunk, (size_t)count - r0);
    a.rec0 = (int)r0; a.n = (int)n;
    a.blocks = (pbd_feature_block*)h->d_fv_stage; a.windows = d_win;
    CallScratch s(h);
    launch_featvec(a, h->ts, h->stream);
    s.launched();
    s.down((char*)blocks + r0 * bbytes, h->d_fv_stage, n * bbytes);
    s.down((char*)windows + r0 * wbytes, d_win, n * wbytes);
    if ((rc = s.finish("feature vectors: "))) return rc;   // (the next chunk overwrites the staging buffer)
  }
  return PBD_OK;
}

// ---- best pose per ground-truth box (k_gtbox.hip) -------------------------------------------------------------------------
// every refusal that depends on the arguments alone (and, for the whole-path entries, on the handle's settings)
int pbd_i_gt_check(pbd_handle* h, const double* gt, const int* ngt, int nframes, double overlap, bool whole) {
  if (whole) {
    if (h->in_group) return fail(h, PBD_ERR_UNSUPPORTED, "gt boxes: pbd_group members are not supported (detect through a handle of its own)");
    if (pbd_i_cand_mode(h) != PBD_CAND_RAW)
      return fail(h, PBD_ERR_UNSUPPORTED, "gt boxes: the selection searches the RAW records: set the candidate filter to PBD_CAND_RAW (pbd_candidates_* work on the returned records)");
    if (h->zf_on) return fail(h, PBD_ERR_UNSUPPORTED, "gt boxes: not with depth pruning on (pbd_candidates_depth_filter works on the returned records)");
    if (h->b3_on) return fail(h, PBD_ERR_UNSUPPORTED, "gt boxes: not with 3-D boxes on (pbd_candidates_box3d works on the returned records)");
    if (h->cl3_on) return fail(h, PBD_ERR_UNSUPPORTED, "gt boxes: not with object clusters on (pbd_candidates_cluster3d works on the returned boxes)");
    if (h->ps_on) return fail(h, PBD_ERR_UNSUPPORTED, "gt boxes: not with per-part scores on (pbd_candidates_part_scores works on the returned records)");
  }
  if (nframes < 1 || nframes > PBD_MAX_BATCH) return fail(h, PBD_ERR_ARG, "batch: 1..64 frames");
  if (!std::isfinite(overlap)) return fail(h, PBD_ERR_ARG, "gt boxes: overlap must be finite");
  if (!ngt) return fail(h, PBD_ERR_ARG, "gt boxes: null ngt");
  for (int f = 0; f < nframes; ++f) {
    if (ngt[f] < 0 || ngt[f] > PBD_GT_MAX) return fail(h, PBD_ERR_ARG, "gt boxes: ngt outside 0..PBD_GT_MAX");
    if (ngt[f] > 0 && !gt) return fail(h, PBD_ERR_ARG, "gt boxes: null boxes");
    for (int k = 0; k < ngt[f] * 4; ++k)
      if (!std::isfinite(gt[(size_t)f * PBD_GT_MAX * 4 + k])) return fail(h, PBD_ERR_ARG, "gt boxes: a non-finite coordinate");
  }
  return PBD_OK;
}
// the planes of `cap` records and the tables of PBD_MAX_BATCH frames: model-sized, on first use
static int gt_buffers(pbd_handle* h) {
  if (h->d_gt_cbox) return PBD_OK;
  const size_t cap = (size_t)h->opt.max_candidates, slots = (size_t)PBD_MAX_BATCH * PBD_GT_MAX;
  int rc;
  if ((rc = model_alloc(h, &h->d_gt_key, cap)) || (rc = model_alloc(h, &h->d_gt_rank, cap)) || (rc = model_alloc(h, &h->d_gt_frame, cap)) ||
      (rc = model_alloc(h, &h->d_gt, slots * 4 + PBD_MAX_BATCH)) || (rc = model_alloc(h, &h->h_gt, slots * 4 + PBD_MAX_BATCH, true, false)) ||
      (rc = model_alloc(h, &h->h_gt_out, h->cand_stride * slots, true, false)) || (rc = model_alloc(h, &h->h_gt_found, slots, true, false)) ||
      (rc = model_alloc(h, &h->h_gt_o, slots, true, false)) || (rc = model_alloc(h, &h->d_gt_cbox, cap)))
    return rc;
  return PBD_OK;
}
static GtBoxArgs gt_args(const pbd_handle* h, int nframes, double overlap) {
  GtBoxArgs a{};
  a.in.stride = h->cand_stride; a.in.mp = h->max_parts;
  a.nframes = nframes; a.overlap = overlap;
  return a;
}
// On a planned frame: the in-frame rank packs (virtual level, component, root y, root x) into 16 bits each; then the boxes of every
// frame, uploaded in the handle's stream from a pinned staging copy (the caller's arrays may go away once the entry returns)
int pbd_i_gt_begin(pbd_handle* h, const GtSource& s, int nframes) {
  if (h->nvl > 65536 || h->md.ncomponents > 65536) return fail(h, PBD_ERR_UNSUPPORTED, "gt boxes: more than 65536 (virtual) levels or components");
  for (const Level& L : h->lv)
    if (L.cw > 65536 || L.ch > 65536) return fail(h, PBD_ERR_UNSUPPORTED, "gt boxes: a level of more than 65536 cells a side");
  int rc = gt_buffers(h);
  if (rc) return rc;
  const size_t nd = (size_t)nframes * PBD_GT_MAX * 4;
  int* hn = (int*)(h->h_gt + (size_t)PBD_MAX_BATCH * PBD_GT_MAX * 4);
  h->gt_max = 0;
  for (int f = 0; f < nframes; ++f) {
    if (s.ngt[f]) memcpy(h->h_gt + (size_t)f * PBD_GT_MAX * 4, s.gt + (size_t)f * PBD_GT_MAX * 4, sizeof(double) * 4 * s.ngt[f]);
    hn[f] = s.ngt[f];
    h->gt_max = std::max(h->gt_max, s.ngt[f]);
  }
  HIPCHK(h, hipMemcpyAsync(h->d_gt, h->h_gt, sizeof(double) * nd, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d_gt + (size_t)PBD_MAX_BATCH * PBD_GT_MAX * 4, hn, sizeof(int) * nframes, hipMemcpyHostToDevice, h->stream));
  h->gt_overlap = s.overlap;
  return PBD_OK;
}
// behind launch_backtrack (into a device list): the selection, its results straight into pinned memory; the records' count follows
// by a copy (the collect refuses an overflowed list: the selection would be incomplete)
int pbd_i_gt_enqueue(pbd_handle* h, const FrameRoute& r) {
  GtBoxArgs a = gt_args(h, h->batch, h->gt_overlap);
  a.in = pbd_i_route_records(h, r.bt.out, r.bt.out_count);
  a.gt = h->d_gt; a.ngt = (const int*)(h->d_gt + (size_t)PBD_MAX_BATCH * PBD_GT_MAX * 4);
  a.cbox = h->d_gt_cbox; a.key = h->d_gt_key; a.rank = h->d_gt_rank; a.frame = h->d_gt_frame;
  a.out = h->h_gt_out; a.found = h->h_gt_found; a.o = h->h_gt_o;
  launch_gtbox(a, h->gt_max, h->stream);
  return PBD_OK;
}
// the collect (stream synchronised, the list did not overflow): the winners of every frame -> the caller's arrays
void pbd_i_gt_gather(pbd_handle* h, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int* found, double* o) {
  const int mp = h->max_parts;
  const int* hn = (const int*)(h->h_gt + (size_t)PBD_MAX_BATCH * PBD_GT_MAX * 4);
  for (int f = 0; f < h->batch; ++f)
    for (int g = 0; g < hn[f]; ++g) {
      const size_t slot = (size_t)f * PBD_GT_MAX + g;
      const bool hit = h->gt_max > 0 && h->h_gt_found[slot] != 0;
      if (found) found[slot] = hit;
      if (o) o[slot] = hit ? h->h_gt_o[slot] : 0.0;
      if (!hit) continue;
      pbd_rec_get(h->h_gt_out + h->cand_stride * slot, mp, heads, boxes, locs, slot);
      if (heads) heads[slot].level -= f * h->nlevels;   // virtual level -> the frame's own pyramid level
    }
}

// ---- behind the back-tracking ---------------------------------------------------------------------------------------------
// the handle's buffers behind the route's names (pbd_route.hpp)
char* pbd_i_route_buf(const pbd_handle* h, RouteBuf b) {
  switch (b) {
    case HOST_OUT: return h->h_cand_out;
    case DEV_OUT: return h->d_cand_out;
    case DEV_RAW: return h->d_cand_raw;
    case DEV_ZF: return h->d_zf_out;
    case DEV_CP_STAGE: return h->d_cp_stage;
    case BUF_NONE: break;
  }
  return nullptr;
}
int* pbd_i_route_count(const pbd_handle* h, RouteCount c) {
  switch (c) {
    case CNT_DEV: return h->d_cand_count;
    case CNT_DEV_ZF: return h->d_zf_cnt;
    case CNT_HOST_CF: return h->h_cf_cnt;
    case CNT_DEV_CF: return h->d_cf_cnt;
    case CNT_DEV_CP: return h->d_cp_cnt;
    case CNT_NONE: break;
  }
  return nullptr;
}
RecordSet pbd_i_route_records(const pbd_handle* h, RouteBuf b, RouteCount c) {
  RecordSet in{};
  in.p = pbd_i_route_buf(h, b); in.stride = h->cand_stride; in.mp = h->max_parts;
  in.count = pbd_i_route_count(h, c); in.capacity = h->opt.max_candidates;
  in.nlevels = h->nlevels;
  if (route_cf_block(c)) { in.cf = in.count; in.nframes = h->batch; }
  return in;
}

int pbd_i_post_buffers(pbd_handle* h, const FrameRoute& r) {
  int rc = PBD_OK;
  if (r.filter.on) {
    rc = cand_filter_buffers(h, r.filter_mode == PBD_CAND_SORT_NMS);
    if (!rc && r.parts.on) rc = cand_parts_buffers(h);
  }
  if (!rc && r.pending.ps) rc = ps_buffers(h);
  if (!rc && r.zf.on) rc = zf_buffers(h);
  if (!rc && r.pending.b3) rc = b3_buffers(h);
  if (!rc && r.pending.cl3) rc = cl3_buffers(h);
  return rc;
}

int pbd_i_post_enqueue(pbd_handle* h, const FrameJob& job, const FrameRoute& r) {
  if (r.zf.on) {
    // depth pruning: k_zfilter writes the kept records straight into the pinned host buffers (the count follows by a copy), or into
    // the buffer k_cand_filter then sorts (and suppresses) as usual
    HIPCHK(h, hipMemsetAsync(h->d_zf_cnt, 0, sizeof(int) * 2, h->stream));
    ZFilterArgs z{};
    z.in = pbd_i_route_records(h, r.zf.in, r.zf.in_count);
    z.z = job.z;
    z.npart = h->d_zf_npart; z.par = h->d_zf_par; z.thr = h->d_zf_thr;
    z.med = h->d_zf_med; z.large = h->d_zf_large; z.nlarge = (unsigned*)(h->d_zf_cnt + 1);
    z.out = pbd_i_route_buf(h, r.zf.out); z.cnt = pbd_i_route_count(h, r.zf.out_count);
    launch_zfilter(z, h->ts, h->stream);
  }
  if (r.filter.on) {
    // Candidate::sort (+ nonMaximaSuppression): k_cand_filter writes the kept records in final order + the per-frame counts — straight
    // into the pinned host buffers, or, for a member of an RCCL-gathering group, into the device buffer the all-gather block is packed from
    // With the part-wise NMS the kernel only sorts, into the staging buffer, and k_cand_parts writes what it would have written
    CandFilterArgs a = cand_args(h, r.filter_mode, h->cand_overlap, h->fw, h->fh);
    a.in = pbd_i_route_records(h, r.filter.in, r.filter.in_count);
    a.back = h->d_back; a.rootv_base = h->d_rootv; a.gmask = h->d_cf_mask;
    a.out = pbd_i_route_buf(h, r.filter.out); a.cnt_out = pbd_i_route_count(h, r.filter.out_count);
    launch_cand_filter(a, h->batch, h->stream);
    if (r.parts.on) {
      CandPartsArgs p = cand_parts_args(h, h->cand_overlap, h->cand_top, h->opt.max_candidates);
      p.in = pbd_i_route_buf(h, r.parts.in); p.cnt_in = pbd_i_route_count(h, r.parts.in_count);
      p.rect = h->d_cp_rect; p.np = h->d_cp_np; p.kept = h->d_cp_kept; p.gbits = h->d_cp_bits;
      p.out = pbd_i_route_buf(h, r.parts.out); p.cnt_out = pbd_i_route_count(h, r.parts.out_count);
      launch_cand_parts(p, h->batch, h->stream);
    }
  }
  return PBD_OK;
}

// the frame's final records (behind the depth pruning and the candidate filter) -> one box per record slot, pinned
int pbd_i_run_box3d(pbd_handle* h, const FrameJob& job, const FrameRoute& r) {
  Box3dArgs a{};
  a.in = pbd_i_route_records(h, r.final_buf, r.final_count);
  a.z = job.z;
  a.im_w = h->fw; a.im_h = h->fh; a.cam = h->b3_cam;
  b3_taps(a);
  a.out = h->h_b3; a.centres = h->h_b3c;
  launch_box3d(a, h->ts, h->stream);
  LAUNCHCHK(h, "box3d");
  if (r.pending.cl3) {   // the object clusters of the same records, right behind
    Cluster3dArgs c{};
    c.in = a.in; c.z = a.z; c.pstride = h->ts;
    c.boxes = h->h_b3;
    c.cam = h->b3_cam; c.tol = h->cl3_tol;
    c.scratch = h->d_cl3_scratch; c.slot_bytes = cluster3d_slot_bytes(h->cl3_pcap); c.pcap = h->cl3_pcap;
    c.out = h->h_cl3; c.pool = h->d_cl3_pool; c.pool_cap = h->cl3_pool_cap; c.pool_used = h->d_cl3_used;
    HIPCHK(h, hipMemsetAsync(h->d_cl3_used, 0, sizeof(unsigned long long), h->stream));
    launch_cluster3d(c, h->ts, std::min(h->cl3_slots, a.in.capacity), h->stream);
    LAUNCHCHK(h, "cluster3d");
    h->cl3_args = c;
  }
  return PBD_OK;
}

// the frame's final records -> three doubles per part and record slot, pinned
int pbd_i_run_part_scores(pbd_handle* h, const FrameRoute& r) {
  PartScoreArgs a = ps_args(h);
  a.in = pbd_i_route_records(h, r.final_buf, r.final_count);
  a.out = h->h_ps;
  launch_partscore(a, h->ts, h->stream);
  LAUNCHCHK(h, "part scores");
  return PBD_OK;
}
void pbd_i_ps_begin(pbd_handle* h, int nframes) {
  h->ps_res.assign((size_t)nframes, {}); h->ps_res_on.assign((size_t)nframes, 0);
  h->ps_ready = true;
}
void pbd_i_ps_gather(pbd_handle* h, int f, const std::vector<const char*>& recs, const std::vector<int>& order) {
  const size_t n = recs.size(), m3 = (size_t)h->max_parts * 3;
  std::vector<double>& o = h->ps_res[f];
  o.resize(n * m3);
  for (size_t i = 0; i < n; ++i) {
    const size_t slot = (size_t)(recs[order[i]] - h->h_cand_out) / h->cand_stride;
    memcpy(o.data() + i * m3, h->h_ps + slot * m3, sizeof(double) * m3);
  }
  h->ps_res_on[f] = 1;
}

// ---- 3-D boxes of a collected frame: the pinned per-slot results, in the order the records are returned ---------------------
void pbd_i_b3_begin(pbd_handle* h, int nframes) {
  h->b3_res.assign((size_t)nframes, {}); h->b3_cen.assign((size_t)nframes, {}); h->b3_res_on.assign((size_t)nframes, 0);
  h->b3_ready = true;
  h->cl3_ready = false;
  h->cl3_slot.assign((size_t)nframes, {}); h->cl3_res.assign((size_t)nframes, {}); h->cl3_idx.assign((size_t)nframes, {});
  h->cl3_res_on.assign((size_t)nframes, 0);
}
void pbd_i_b3_gather(pbd_handle* h, int f, const std::vector<const char*>& recs, const std::vector<int>& order) {
  if (!((h->pf.b3_has >> f) & 1ull)) return;
  const size_t n = recs.size(), m3 = (size_t)h->max_parts * 3;
  std::vector<pbd_box3d>& o = h->b3_res[f];
  std::vector<double>& c = h->b3_cen[f];
  o.resize(n); c.resize(n * m3);
  for (size_t i = 0; i < n; ++i) {
    const size_t slot = (size_t)(recs[order[i]] - h->h_cand_out) / h->cand_stride;
    o[i] = h->h_b3[slot];
    memcpy(c.data() + i * m3, h->h_b3c + slot * m3, sizeof(double) * m3);
    if (h->pf.cl3) h->cl3_slot[f].push_back((int)slot);
  }
  h->b3_res_on[f] = 1;
}
// the object clusters of the frames pbd_i_b3_gather listed (the collect synchronised the stream)
int pbd_i_b3_end(pbd_handle* h) {
  if (!h->pf.cl3) return PBD_OK;
  std::vector<int> lst;
  const int nf = (int)h->cl3_slot.size();
  for (int f = 0; f < nf; ++f)
    if (h->b3_res_on[f]) for (int s : h->cl3_slot[f]) { lst.push_back(s); lst.push_back(f); }
  std::vector<pbd_cluster3d> res;
  std::vector<int32_t> idx;
  int rc = cl3_resolve(h, h->cl3_args, h->ts, h->cl3_slots, nullptr, lst, res, idx);
  if (rc) return rc;
  size_t r0 = 0, i0 = 0;
  for (int f = 0; f < nf; ++f) {
    if (!h->b3_res_on[f]) continue;
    const size_t m = h->cl3_slot[f].size();
    size_t ni = 0;
    for (size_t k = 0; k < m; ++k) ni += (size_t)std::max(res[r0 + k].size, 0);
    h->cl3_res[f].assign(res.begin() + r0, res.begin() + r0 + m);
    h->cl3_idx[f].assign(idx.begin() + i0, idx.begin() + i0 + ni);
    h->cl3_res_on[f] = 1;
    r0 += m; i0 += ni;
  }
  h->cl3_ready = true;
  return PBD_OK;
}

// ---- the stand-alone device round trip of the candidate filter --------------------------------------------------------------
int pbd_i_filter_host(pbd_handle* h, int mode, float overlap, int im_w, int im_h, char* recs, int count, int* kept, int kind, int top) {
  if (mode == PBD_CAND_RAW || count == 0) { *kept = count; return PBD_OK; }
  const bool parts = mode == PBD_CAND_SORT_NMS && kind == PBD_NMS_PARTS;
  if (parts) {
    int rc = cand_parts_lds_ok(h);
    if (rc) return rc;
    mode = PBD_CAND_SORT;
  }
  ON_DEVICE(h);
  const size_t st = h->cand_stride, n = (size_t)count, mask = cand_filter_mask_bytes(im_w, im_h);
  CallScratch s(h);
  char* d_in = s.dev<char>(st * n);
  char* d_out = s.dev<char>(st * n);
  int* d_cnt = s.dev<int>(5);
  CandFilterArgs a = cand_args(h, mode, overlap, im_w, im_h);
  a.in.p = d_in; a.in.count = d_cnt; a.in.capacity = count; a.in.nlevels = 0; a.back = nullptr;
  a.keys = s.dev<unsigned long long>(2 * n); a.idx = s.dev<unsigned>(2 * n); a.box = s.dev<int>(4 * n); a.st = s.dev<uint8_t>(n);
  a.gmask = mode == PBD_CAND_SORT_NMS ? s.dev<unsigned long long>(mask / 8) : nullptr;
  a.out = d_out; a.cnt_out = d_cnt + 1;
  CandPartsArgs p = cand_parts_args(h, overlap, top, count);
  if (parts) {   // the sorted records go back into d_in's place: a second buffer, and a count block of its own
    p.in = s.dev<char>(st * n); p.cnt_in = s.dev<int>(4);
    p.rect = s.dev<int4>((size_t)(h->max_parts + 2) * n); p.np = s.dev<int>(n); p.kept = s.dev<unsigned>(n);
    p.gbits = s.dev<unsigned long long>(cand_parts_bits_words(count, 1));
    p.out = d_out; p.cnt_out = d_cnt + 1;
    a.out = (char*)p.in; a.cnt_out = (int*)p.cnt_in;
  }
  s.up(d_in, recs, st * n);
  s.up(d_cnt, &count, sizeof(int));
  if (s.ok()) {
    launch_cand_filter(a, 1, h->stream);
    if (parts) launch_cand_parts(p, 1, h->stream);
    s.launched();
  }
  int cnt[4] = {0, 0, 0, 0};
  s.down(cnt, d_cnt + 1, sizeof(cnt));
  s.down(recs, d_out, st * n);
  int rc = s.finish("candidate filter: ");
  if (rc) return rc;
  *kept = cnt[1];
  return PBD_OK;
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------
#pragma GCC visibility push(default)
extern "C" {

// ---- host-side post-processing (include/Candidate.hpp:91-99, 277-304) --------
int pbd_candidates_sort(pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int count, int mp) {
  if (!heads || count < 0 || mp <= 0) return PBD_ERR_ARG;
  std::vector<int> order(count);
  for (int i = 0; i < count; ++i) order[i] = i;
  // Candidate::descending; stable, so equal scores keep detect() order (std::sort leaves it unspecified)
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return heads[a].score > heads[b].score; });
  const size_t st = pbd_rec_bytes(mp);
  std::vector<char> rec(st * count);
  for (int i = 0; i < count; ++i) pbd_rec_put(rec.data() + st * i, mp, heads, boxes, locs, i);
  for (int i = 0; i < count; ++i) pbd_rec_get(rec.data() + st * order[i], mp, heads, boxes, locs, i);
  return PBD_OK;
}

int pbd_candidates_nms(pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int count, int mp, int im_w, int im_h,
                       float overlap, int* kept) {
  if (!heads || !boxes || !kept || count < 0 || mp <= 0 || im_w <= 0 || im_h <= 0) return PBD_ERR_ARG;
  std::vector<uint8_t> scratch((size_t)im_w * im_h, 0), keep((size_t)count, 0);
  for (int n = 0; n < count; ++n) {
    const int32_t* b = boxes + (size_t)n * mp * 4;
    int x = b[0], y = b[1], bw = b[2], bh = b[3];  // Candidate::boundingBox(): union of the part rects
    for (int p = 0; p < heads[n].nparts; ++p) {
      const int32_t* q = b + p * 4;
      const int x1 = std::min(x, q[0]), y1 = std::min(y, q[1]);
      bw = std::max(x + bw, q[0] + q[2]) - x1;
      bh = std::max(y + bh, q[1] + q[3]) - y1;
      x = x1; y = y1;
    }
    int ix1 = std::max(x, 0), iy1 = std::max(y, 0);  // & bounds
    int iw = std::min(x + bw, im_w) - ix1, ih = std::min(y + bh, im_h) - iy1;
    if (iw <= 0 || ih <= 0) ix1 = iy1 = iw = ih = 0;
    double sum = 0;
    for (int yy = iy1; yy < iy1 + ih; ++yy)
      for (int xx = ix1; xx < ix1 + iw; ++xx) sum += scratch[(size_t)yy * im_w + xx];
    if (sum / (double)(iw * ih) > (double)overlap) continue;  // :296
    for (int yy = iy1; yy < iy1 + ih; ++yy) memset(&scratch[(size_t)yy * im_w + ix1], 1, iw);
    keep[n] = 1;
  }
  *kept = pbd_rec_compact(heads, boxes, locs, count, mp, keep.data());
  return PBD_OK;
}

// nms.m's rule (include/pbd_c.h); k_cand_parts.hip computes the same
namespace {
struct PRect { long long x0, y0, x1, y1; };   // empty: all zero
inline PRect p_part(const int32_t* b) {
  if (b[2] <= 0 || b[3] <= 0) return PRect{0, 0, 0, 0};
  return PRect{b[0], b[1], (long long)b[0] + b[2], (long long)b[1] + b[3]};
}
inline double p_area(const PRect& r) { return (double)(r.x1 - r.x0) * (double)(r.y1 - r.y0); }
inline double p_inter(const PRect& a, const PRect& b) {
  const long long w = std::min(a.x1, b.x1) - std::max(a.x0, b.x0), h = std::min(a.y1, b.y1) - std::max(a.y0, b.y0);
  return (w > 0 && h > 0) ? (double)w * (double)h : 0.0;
}
}  // namespace
int pbd_candidates_nms_parts(pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int count, int mp, float overlap, int top,
                             int* kept) {
  if (!heads || !boxes || !kept || count < 0 || mp <= 0 || top < 0 || !std::isfinite(overlap)) return PBD_ERR_ARG;
  for (int i = 0; i < count; ++i)
    if (heads[i].nparts < 0 || heads[i].nparts > mp) return PBD_ERR_ARG;
  const int n = top > 0 && count > top ? top : count;   // nms.m:18-22
  const size_t R = (size_t)mp + 1;
  std::vector<PRect> rect(R * n);   // [record][part .. , covering box at mp]
  for (int i = 0; i < n; ++i) {
    PRect c{0, 0, 0, 0};
    bool any = false;
    for (int p = 0; p < heads[i].nparts; ++p) {
      const PRect r = p_part(boxes + ((size_t)i * mp + p) * 4);
      rect[R * i + p] = r;
      if (r.x1 == r.x0) continue;
      c = any ? PRect{std::min(c.x0, r.x0), std::min(c.y0, r.y0), std::max(c.x1, r.x1), std::max(c.y1, r.y1)} : r;
      any = true;
    }
    rect[R * i + mp] = c;
  }
  const double ov = (double)overlap;
  std::vector<uint8_t> keep((size_t)count, 0), gone((size_t)n, 0);
  for (int i = 0; i < n; ++i) {
    if (gone[i]) continue;
    keep[i] = 1;
    const PRect* ri = &rect[R * i];
    for (int j = i + 1; j < n; ++j) {
      if (gone[j]) continue;
      const PRect* rj = &rect[R * j];
      bool rej = p_inter(ri[mp], rj[mp]) / p_area(ri[mp]) > ov;
      const int P = std::min(heads[i].nparts, heads[j].nparts);
      for (int p = 0; p < P && !rej; ++p) rej = p_inter(ri[p], rj[p]) / p_area(ri[p]) > ov;
      gone[j] = rej;
    }
  }
  *kept = pbd_rec_compact(heads, boxes, locs, count, mp, keep.data());
  return PBD_OK;
}

// ---- the post-step on the device (k_cand.hip) -------------------------------------
static bool cand_mode_ok(int mode, float overlap) {
  return (mode == PBD_CAND_RAW || mode == PBD_CAND_SORT || mode == PBD_CAND_SORT_NMS) && std::isfinite(overlap);
}
int pbd_set_candidate_filter(pbd_handle* h, int mode, float overlap) {
  if (!h) return PBD_ERR_ARG;
  if (!cand_mode_ok(mode, overlap)) return fail(h, PBD_ERR_ARG, "candidate filter: mode PBD_CAND_RAW / _SORT / _SORT_NMS, finite overlap");
  if (h->in_group) return fail(h, PBD_ERR_STATE, "handle belongs to a pbd_group: set the filter on the group");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  if ((mode != h->cand_mode || overlap != h->cand_overlap) && h->gexec) {   // the filter's launch (or its absence) is part of a captured graph
    ON_DEVICE(h);
    drop_graph(h);
  }
  h->cand_mode = mode;
  h->cand_overlap = overlap;
  return PBD_OK;
}

int pbd_set_candidate_nms(pbd_handle* h, int kind, int top) {
  if (!h) return PBD_ERR_ARG;
  if ((kind != PBD_NMS_PAINTED && kind != PBD_NMS_PARTS) || top < 0) return fail(h, PBD_ERR_ARG, "candidate NMS: kind PBD_NMS_PAINTED / _PARTS, top >= 0");
  if (h->in_group) return fail(h, PBD_ERR_STATE, "handle belongs to a pbd_group: set the NMS on the group");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  if ((kind != h->cand_nms || top != h->cand_top) && h->gexec) {   // which kernels run behind the sort is part of a captured graph
    ON_DEVICE(h);
    drop_graph(h);
  }
  h->cand_nms = kind;
  h->cand_top = top;
  return PBD_OK;
}

int pbd_candidates_filter_parts(pbd_handle* h, float overlap, int top, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs,
                                int count, int* kept) {
  if (!h) return PBD_ERR_ARG;
  if (!std::isfinite(overlap) || top < 0) return fail(h, PBD_ERR_ARG, "parts NMS: finite overlap, top >= 0");
  if (!kept || count < 0 || (count > 0 && (!heads || !boxes))) return fail(h, PBD_ERR_ARG, "heads / boxes / kept / count");
  for (int i = 0; i < count; ++i) {
    if (!std::isfinite(heads[i].score)) return fail(h, PBD_ERR_ARG, "non-finite score: its order is undefined");
    if (heads[i].nparts < 0 || heads[i].nparts > h->max_parts) return fail(h, PBD_ERR_ARG, "nparts outside 0..max_parts");
  }
  if (count == 0) { *kept = 0; return PBD_OK; }
  const int mp = h->max_parts;
  const size_t st = h->cand_stride;
  std::vector<char> rec(st * count, 0);
  for (int i = 0; i < count; ++i) pbd_rec_put(rec.data() + st * i, mp, heads, boxes, locs, i);
  int k = 0, rc = pbd_i_filter_host(h, PBD_CAND_SORT_NMS, overlap, 1, 1, rec.data(), count, &k, PBD_NMS_PARTS, top);
  if (rc) return rc;
  for (int i = 0; i < k; ++i) pbd_rec_get(rec.data() + st * i, mp, heads, boxes, locs, i);
  *kept = k;
  return PBD_OK;
}

int pbd_candidates_filter(pbd_handle* h, int mode, float overlap, int im_w, int im_h, pbd_candidate_head* heads, int32_t* boxes,
                          int32_t* locs, int count, int* kept) {
  if (!h) return PBD_ERR_ARG;
  if (!cand_mode_ok(mode, overlap)) return fail(h, PBD_ERR_ARG, "candidate filter: mode PBD_CAND_RAW / _SORT / _SORT_NMS, finite overlap");
  if (!kept || count < 0 || (count > 0 && !heads)) return fail(h, PBD_ERR_ARG, "heads / kept / count");
  if (mode == PBD_CAND_SORT_NMS && (!boxes || im_w <= 0 || im_h <= 0)) return fail(h, PBD_ERR_ARG, "NMS needs boxes and the image size");
  for (int i = 0; i < count; ++i) {
    if (!std::isfinite(heads[i].score)) return fail(h, PBD_ERR_ARG, "non-finite score: its order is undefined");
    if (mode == PBD_CAND_SORT_NMS && (heads[i].nparts < 0 || heads[i].nparts > h->max_parts)) return fail(h, PBD_ERR_ARG, "nparts outside 0..max_parts");
  }
  if (mode == PBD_CAND_RAW || count == 0) { *kept = count; return PBD_OK; }
  const int mp = h->max_parts;
  const size_t st = h->cand_stride;
  std::vector<char> rec(st * count, 0);
  for (int i = 0; i < count; ++i) pbd_rec_put(rec.data() + st * i, mp, heads, boxes, locs, i);
  int k = 0, rc = pbd_i_filter_host(h, mode, overlap, im_w, im_h, rec.data(), count, &k);
  if (rc) return rc;
  for (int i = 0; i < k; ++i) pbd_rec_get(rec.data() + st * i, mp, heads, boxes, locs, i);
  *kept = k;
  return PBD_OK;
}

// ---- depth-consistency pruning (k_zfilter.hip) --------------------------------------------------------------------
int pbd_set_depth_filter(pbd_handle* h, int on, float zfactor) {
  if (!h) return PBD_ERR_ARG;
  if (!std::isfinite(zfactor)) return fail(h, PBD_ERR_ARG, "depth filter: zfactor must be finite");
  if (h->in_group) return fail(h, PBD_ERR_UNSUPPORTED, "depth filter: pbd_group members are not supported (detect through a handle of its own)");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  h->zf_on = on != 0;      // (depth-carrying frames never replay a captured graph: nothing captured depends on the setting)
  h->zf_factor = zfactor;
  return PBD_OK;
}

int pbd_candidates_depth_filter(pbd_handle* h, float zfactor, const void* depth, int depth_type, int dw, int dh, int dstride,
                                pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int count, int* kept) {
  if (!h) return PBD_ERR_ARG;
  if (!std::isfinite(zfactor)) return fail(h, PBD_ERR_ARG, "depth filter: zfactor must be finite");
  if (!kept || count < 0 || (count > 0 && (!heads || !boxes))) return fail(h, PBD_ERR_ARG, "heads / boxes / kept / count");
  bool empty;
  int rc = depth_image_args(h, depth, dw, dh, &empty);
  if (rc) return rc;
  if (depth_type != zf_type(h) || !empty) { if ((rc = pbd_i_depth_check(h, depth_type, dstride, dw))) return rc; }   // (the handle's type only)
  for (int i = 0; i < count; ++i) {
    const int c = heads[i].component;
    if (c < 0 || c >= h->md.ncomponents) return fail(h, PBD_ERR_ARG, "component out of range");
    if (heads[i].nparts != h->part_offset[c + 1] - h->part_offset[c]) return fail(h, PBD_ERR_ARG, "nparts differs from the model's component");
  }
  if (count == 0) { *kept = 0; return PBD_OK; }
  ON_DEVICE(h);
  const int mp = h->max_parts, nc = h->md.ncomponents;
  const size_t st = h->cand_stride, n = (size_t)count, row = (size_t)dw * h->ts;
  std::vector<char> rec(st * n, 0);
  for (size_t i = 0; i < n; ++i) pbd_rec_put(rec.data() + st * i, mp, heads, boxes, nullptr, i);
  std::vector<int> npart, par; std::vector<double> thr;
  zf_table(h, zfactor, npart, par, thr);
  const int cnt3[3] = {count, 0, 0};
  CallScratch s(h);
  ZFilterArgs z{};
  z.in.p = s.dev<char>(st * n); z.in.capacity = count; z.in.stride = st; z.in.mp = mp; z.in.nlevels = 0;
  z.z.img = empty ? nullptr : s.dev<char>(row * dh); z.z.pitch = row; z.z.fbytes = 0; z.z.w = empty ? 0 : dw; z.z.h = empty ? 0 : dh; z.z.has = 1;
  int* d_cnt = s.dev<int>(3); int* d_np = s.dev<int>(nc); int* d_par = s.dev<int>((size_t)nc * mp); double* d_thr = s.dev<double>((size_t)nc * mp);
  z.in.count = d_cnt; z.cnt = d_cnt + 1; z.nlarge = (unsigned*)(d_cnt + 2);
  z.npart = d_np; z.par = d_par; z.thr = d_thr;
  z.med = s.dev<unsigned long long>(n * mp); z.large = s.dev<unsigned>(n * mp); z.flags = s.dev<uint8_t>(n);
  s.up((void*)z.in.p, rec.data(), st * n);
  s.up(d_cnt, cnt3, sizeof(cnt3));
  s.up(d_np, npart.data(), sizeof(int) * nc);
  s.up(d_par, par.data(), sizeof(int) * nc * mp);
  s.up(d_thr, thr.data(), sizeof(double) * nc * mp);
  if (!empty) s.up2d((void*)z.z.img, row, depth, dstride, row, dh);
  if (s.ok()) {
    launch_zfilter(z, h->ts, h->stream);
    s.launched();
  }
  std::vector<uint8_t> flags(n, 0);
  s.down(flags.data(), z.flags, n);
  if ((rc = s.finish("depth filter: "))) return rc;
  *kept = pbd_rec_compact(heads, boxes, locs, count, mp, flags.data());
  return PBD_OK;
}

// ---- 3-D boxes (k_box3d.hip) --------------------------------------------------------------------------------------------

int pbd_set_box3d(pbd_handle* h, int on, const pbd_camera* cam) {
  if (!h) return PBD_ERR_ARG;
  if (on && !b3_cam_ok(cam)) return fail(h, PBD_ERR_ARG, "box3d: a camera with finite intrinsics and nonzero fx, fy");
  if (h->in_group) return fail(h, PBD_ERR_UNSUPPORTED, "box3d: pbd_group members are not supported (detect through a handle of its own)");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  h->b3_on = on != 0;
  if (on) h->b3_cam = *cam;
  return PBD_OK;
}

int pbd_get_box3d(pbd_handle* h, int frame, pbd_box3d* out, double* centres, int capacity, int* count) {
  if (!h || !count || capacity < 0 || (capacity > 0 && !out)) return PBD_ERR_ARG;
  if (h->in_group) return fail(h, PBD_ERR_UNSUPPORTED, "box3d: pbd_group members are not supported");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  if (!h->b3_ready || frame < 0 || frame >= (int)h->b3_res_on.size() || !h->b3_res_on[frame])
    return fail(h, PBD_ERR_STATE, "box3d: the last frame did not compute 3-D boxes for this frame (plain entry point, setting off, or no depth)");
  const std::vector<pbd_box3d>& r = h->b3_res[frame];
  const int n = (int)r.size();
  *count = n;
  if (n > capacity) return fail(h, PBD_ERR_CAPACITY, "output capacity too small");
  std::copy(r.begin(), r.end(), out);
  if (centres) std::copy(h->b3_cen[frame].begin(), h->b3_cen[frame].end(), centres);
  return PBD_OK;
}

int pbd_candidates_box3d(pbd_handle* h, const pbd_camera* cam, const void* depth, int depth_type, int dw, int dh, int dstride,
                         int im_w, int im_h, const pbd_candidate_head* heads, const int32_t* boxes, int count, pbd_box3d* out,
                         double* centres) {
  if (!h) return PBD_ERR_ARG;
  if (!b3_cam_ok(cam)) return fail(h, PBD_ERR_ARG, "box3d: a camera with finite intrinsics and nonzero fx, fy");
  if (im_w <= 0 || im_h <= 0) return fail(h, PBD_ERR_ARG, "box3d: im_w, im_h > 0");
  if (count < 0 || (count > 0 && (!heads || !boxes || !out))) return fail(h, PBD_ERR_ARG, "heads / boxes / out / count");
  bool empty;
  int rc = depth_image_args(h, depth, dw, dh, &empty);
  if (rc) return rc;
  if (depth_type != PBD_DEPTH_32F && depth_type != PBD_DEPTH_64F)   // (either type, whatever the handle's)
    return fail(h, PBD_ERR_UNSUPPORTED, "box3d: depth PBD_DEPTH_32F or PBD_DEPTH_64F (Mat_<float> reads it)");
  const int esz = depth_type == PBD_DEPTH_64F ? 8 : 4;
  if (!empty && (dstride < (long long)dw * esz || dstride % esz)) return fail(h, PBD_ERR_ARG, "depth stride: bytes, >= dw * element size and a multiple of it");
  const int mp = h->max_parts;
  for (int i = 0; i < count; ++i)
    if (heads[i].nparts < 1 || heads[i].nparts > mp) return fail(h, PBD_ERR_ARG, "nparts outside 1 .. max_parts");
  if (count == 0) return PBD_OK;
  ON_DEVICE(h);
  const size_t st = h->cand_stride, n = (size_t)count, row = (size_t)dw * esz;
  std::vector<char> rec(st * n, 0);
  for (size_t i = 0; i < n; ++i) pbd_rec_put(rec.data() + st * i, mp, heads, boxes, nullptr, i);
  CallScratch s(h);
  Box3dArgs a{};
  a.in.p = s.dev<char>(st * n); a.in.stride = st; a.in.mp = mp; a.in.count = s.dev<int>(1); a.in.capacity = count; a.in.nlevels = 0;
  a.z.img = empty ? nullptr : s.dev<char>(row * dh); a.z.pitch = row; a.z.fbytes = 0; a.z.w = empty ? 0 : dw; a.z.h = empty ? 0 : dh; a.z.has = 1;
  a.im_w = im_w; a.im_h = im_h; a.cam = *cam;
  b3_taps(a);
  a.out = s.dev<pbd_box3d>(n); a.centres = centres ? s.dev<double>(n * mp * 3) : nullptr;
  s.up((void*)a.in.p, rec.data(), st * n);
  s.up((void*)a.in.count, &count, sizeof(int));
  if (!empty) s.up2d((void*)a.z.img, row, depth, dstride, row, dh);
  if (s.ok()) {
    launch_box3d(a, esz, h->stream);
    s.launched();
  }
  s.down(out, a.out, sizeof(pbd_box3d) * n);
  if (centres) s.down(centres, a.centres, sizeof(double) * n * mp * 3);
  return s.finish("box3d: ");
}

// ---- object clusters (k_cluster3d.hip) ----------------------------------------------------------------------------------
static bool cl3_tol_ok(float t) { return std::isfinite(t) && t > 0.f; }

int pbd_set_cluster3d(pbd_handle* h, int on, float tolerance) {
  if (!h) return PBD_ERR_ARG;
  if (on && !cl3_tol_ok(tolerance)) return fail(h, PBD_ERR_ARG, "cluster3d: a finite tolerance > 0");
  if (h->in_group) return fail(h, PBD_ERR_UNSUPPORTED, "cluster3d: pbd_group members are not supported (detect through a handle of its own)");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  h->cl3_on = on != 0;
  if (on) h->cl3_tol = tolerance;
  return PBD_OK;
}

// results + their indices (the exclusive prefix sum of size) -> the caller's arrays
static int cl3_copy_out(pbd_handle* h, const std::vector<int32_t>& idx, int32_t* indices, int idx_capacity, int* idx_total) {
  if (idx_total) *idx_total = (int)idx.size();
  if (!indices) return PBD_OK;
  if ((long long)idx.size() > (long long)idx_capacity) return fail(h, PBD_ERR_CAPACITY, "cluster3d: index capacity too small");
  std::copy(idx.begin(), idx.end(), indices);
  return PBD_OK;
}

int pbd_get_cluster3d(pbd_handle* h, int frame, pbd_cluster3d* out, int capacity, int* count, int32_t* indices, int idx_capacity,
                      int* idx_total) {
  if (!h || !count || capacity < 0 || (capacity > 0 && !out) || (indices && (idx_capacity < 0 || !idx_total))) return PBD_ERR_ARG;
  if (h->in_group) return fail(h, PBD_ERR_UNSUPPORTED, "cluster3d: pbd_group members are not supported");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  if (!h->cl3_ready || frame < 0 || frame >= (int)h->cl3_res_on.size() || !h->cl3_res_on[frame])
    return fail(h, PBD_ERR_STATE, "cluster3d: the last frame did not compute object clusters for this frame (plain entry point, "
                                  "3-D boxes or clusters off, or no depth)");
  const std::vector<pbd_cluster3d>& r = h->cl3_res[frame];
  const int n = (int)r.size();
  *count = n;
  if (idx_total) *idx_total = (int)h->cl3_idx[frame].size();
  if (n > capacity) return fail(h, PBD_ERR_CAPACITY, "output capacity too small");
  std::copy(r.begin(), r.end(), out);
  return cl3_copy_out(h, h->cl3_idx[frame], indices, idx_capacity, idx_total);
}

int pbd_candidates_cluster3d(pbd_handle* h, const void* cloud, int cw, int ch, int point_stride, int row_stride,
                             const pbd_box3d* boxes, int count, float tolerance, pbd_cluster3d* out, int32_t* indices,
                             int idx_capacity, int* idx_total) {
  if (!h) return PBD_ERR_ARG;
  if (!cl3_tol_ok(tolerance)) return fail(h, PBD_ERR_ARG, "cluster3d: a finite tolerance > 0");
  if (cw < 0 || ch < 0 || (long long)cw * ch > (1ll << 30)) return fail(h, PBD_ERR_ARG, "cluster3d: cloud size");
  const long long npts = (long long)cw * ch;
  if (point_stride < 12 || point_stride % 4) return fail(h, PBD_ERR_ARG, "cluster3d: point stride: bytes, >= 12 and a multiple of 4");
  if (npts > 0 && (!cloud || row_stride % 4 || (long long)row_stride < (long long)(cw - 1) * point_stride + 12))
    return fail(h, PBD_ERR_ARG, "cluster3d: a cloud (NULL only when empty), row stride: bytes, >= (cw - 1) * point stride + 12, a multiple of 4");
  if (count < 0 || (count > 0 && (!boxes || !out))) return fail(h, PBD_ERR_ARG, "boxes / out / count");
  if (indices && (idx_capacity < 0 || !idx_total)) return fail(h, PBD_ERR_ARG, "indices: idx_capacity >= 0 and idx_total");
  if (count == 0) return cl3_copy_out(h, {}, indices, idx_capacity, idx_total);
  ON_DEVICE(h);
  const int pcap = (int)std::max<long long>(npts, 1);
  const int slots = cl3_slots(pcap, count);
  const size_t bytes = npts ? (size_t)(ch - 1) * row_stride + (size_t)(cw - 1) * point_stride + 12 : 0, n = (size_t)count;
  unsigned long long pool_cap = std::min<unsigned long long>((unsigned long long)count * (unsigned long long)npts, 4ull * (unsigned long long)pcap);
  pool_cap = std::max<unsigned long long>(pool_cap, 1);
  CallScratch s(h);
  Cluster3dArgs a{};
  a.in.count = s.dev<int>(1); a.in.capacity = count;
  a.z.img = s.dev<char>(bytes); a.z.pitch = (size_t)row_stride; a.z.w = cw; a.z.h = ch; a.z.has = 1; a.pstride = (size_t)point_stride;
  pbd_box3d* d_box = s.dev<pbd_box3d>(n);
  a.boxes = d_box; a.tol = tolerance;
  a.scratch = s.dev<char>(cluster3d_slot_bytes(pcap) * slots); a.slot_bytes = cluster3d_slot_bytes(pcap); a.pcap = pcap;
  a.out = s.alloc<Cl3Res>(n, true); a.pool = s.dev<int>(pool_cap); a.pool_cap = pool_cap; a.pool_used = s.dev<unsigned long long>(1);
  s.up((void*)a.z.img, cloud, bytes);
  s.up((void*)a.in.count, &count, sizeof(int));
  s.up(d_box, boxes, sizeof(pbd_box3d) * n);
  s.zero(a.pool_used, sizeof(unsigned long long));
  if (s.ok()) {
    launch_cluster3d(a, 0, slots, h->stream);
    s.launched();
  }
  int rc = s.finish("cluster3d: ");
  if (rc) return rc;
  std::vector<int> lst(2 * n);
  for (size_t i = 0; i < n; ++i) { lst[2 * i] = (int)i; lst[2 * i + 1] = 0; }
  std::vector<pbd_cluster3d> res;
  std::vector<int32_t> idx;
  if ((rc = cl3_resolve(h, a, 0, slots, &s, lst, res, idx))) return rc;
  std::copy(res.begin(), res.end(), out);
  return cl3_copy_out(h, idx, indices, idx_capacity, idx_total);
}

// ---- per-part scores (k_partscore.hip) ------------------------------------------------------------------------------------
int pbd_set_part_scores(pbd_handle* h, int on) {
  if (!h) return PBD_ERR_ARG;
  if (h->in_group) return fail(h, PBD_ERR_UNSUPPORTED, "part scores: pbd_group members are not supported (detect through a handle of its own)");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  if ((on != 0) != h->ps_on && h->gexec) {   // the step's launch (or its absence) is part of a captured graph
    ON_DEVICE(h);
    drop_graph(h);
  }
  h->ps_on = on != 0;
  if (!h->ps_on) h->ps_ready = h->pf.ps_compact = false;   // (no frame is pending: the getter's answer follows the setting)
  return PBD_OK;
}

int pbd_get_part_scores(pbd_handle* h, int frame, pbd_part_score* out, int capacity, int* count) {
  if (!h || !count || capacity < 0 || (capacity > 0 && !out)) return PBD_ERR_ARG;
  if (h->in_group) return fail(h, PBD_ERR_UNSUPPORTED, "part scores: pbd_group members are not supported");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  if (h->pf.ps_compact) return fail(h, PBD_ERR_UNSUPPORTED, kPsCompact);
  if (!h->ps_ready || frame < 0 || frame >= (int)h->ps_res_on.size() || !h->ps_res_on[frame])
    return fail(h, PBD_ERR_STATE, "part scores: the last frame did not compute them for this frame (setting off, a stage entry point, or a frame out of range)");
  const std::vector<double>& r = h->ps_res[frame];
  const size_t m3 = (size_t)h->max_parts * 3;
  const int n = (int)(r.size() / m3);
  *count = n;
  if (n > capacity) return fail(h, PBD_ERR_CAPACITY, "output capacity too small");
  if (n) memcpy(out, r.data(), sizeof(double) * r.size());
  return PBD_OK;
}

int pbd_candidates_part_scores(pbd_handle* h, const pbd_candidate_head* heads, const int32_t* locs, int count, pbd_part_score* out) {
  if (!h) return PBD_ERR_ARG;
  if (count < 0 || (count > 0 && (!heads || !locs || !out))) return fail(h, PBD_ERR_ARG, "heads / locs / out / count");
  if (h->in_group) return fail(h, PBD_ERR_UNSUPPORTED, "part scores: pbd_group members are not supported");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  if (h->fw == 0) return fail(h, PBD_ERR_STATE, "part scores: no frame planned");
  if (!h->have_resp) return fail(h, PBD_ERR_STATE, h->compact ? kPsCompact : "part scores: responses not computed");
  const int mp = h->max_parts;
  int rc = check_records(h, heads, locs, count);
  if (rc || count == 0) return rc;
  ON_DEVICE(h);
  if ((rc = ps_tables(h))) return rc;
  const size_t st = h->cand_stride, n = (size_t)count, m3 = (size_t)mp * 3;
  std::vector<char> rec(st * n, 0);
  for (size_t i = 0; i < n; ++i) pbd_rec_put(rec.data() + st * i, mp, heads, nullptr, locs, i);
  CallScratch s(h);
  PartScoreArgs a = ps_args(h);
  a.in.p = s.dev<char>(st * n); a.in.stride = st; a.in.mp = mp; a.in.count = s.dev<int>(1); a.in.capacity = count; a.in.nlevels = 0;
  a.out = s.dev<double>(n * m3);
  s.up((void*)a.in.p, rec.data(), st * n);
  s.up((void*)a.in.count, &count, sizeof(int));
  if (s.ok()) {
    launch_partscore(a, h->ts, h->stream);
    s.launched();
  }
  s.down(out, a.out, sizeof(double) * n * m3);
  return s.finish("part scores: ");
}

// ---- feature vectors (k_featvec.hip) ------------------------------------------------------------------------------------
int pbd_feature_window_max(const pbd_handle* h) { return h ? fv_wmax(h) : -PBD_ERR_ARG; }

int pbd_candidates_features(pbd_handle* h, const pbd_candidate_head* heads, const int32_t* locs, int count, pbd_feature_block* blocks,
                            float* windows) {
  return h ? fv_host(h, heads, locs, count, blocks, windows, 4) : PBD_ERR_ARG;
}
int pbd_candidates_features_f64(pbd_handle* h, const pbd_candidate_head* heads, const int32_t* locs, int count, pbd_feature_block* blocks,
                                double* windows) {
  return h ? fv_host(h, heads, locs, count, blocks, windows, 8) : PBD_ERR_ARG;
}
int pbd_candidates_features_dev(pbd_handle* h, const pbd_candidate_head* heads, const int32_t* locs, int count, pbd_feature_block* d_blocks,
                                void* d_windows) {
  if (!h) return PBD_ERR_ARG;
  if (count > 0 && ((uintptr_t)d_windows % 16 || (uintptr_t)d_blocks % 8)) return fail(h, PBD_ERR_ARG, "feature vectors: d_windows 16-byte, d_blocks 8-byte aligned");
  FeatVecArgs a;
  int rc = fv_begin(h, heads, locs, count, d_blocks, d_windows, 0, &a);
  if (rc || count == 0) return rc;
  a.rec0 = 0; a.n = count; a.blocks = d_blocks; a.windows = d_windows;
  launch_featvec(a, h->ts, h->stream);
  LAUNCHCHK(h, "feature vectors");
  return PBD_OK;
}

// ---- best pose per ground-truth box (k_gtbox.hip) ---------------------------------------------------------------------------
// bestoverlap.m's rule (include/pbd_c.h); k_gtbox.hip computes the same from the same text (gt_overlap.hpp)
int pbd_candidates_best_overlap(const pbd_candidate_head* heads, const int32_t* boxes, int count, int mp, const double* gt, int ngt,
                                double overlap, int32_t* best, double* o) {
  if (count < 0 || mp <= 0 || ngt < 0 || ngt > PBD_GT_MAX || !std::isfinite(overlap)) return PBD_ERR_ARG;
  if ((count > 0 && (!heads || !boxes)) || (ngt > 0 && (!gt || !best || !o))) return PBD_ERR_ARG;
  for (int k = 0; k < ngt * 4; ++k) if (!std::isfinite(gt[k])) return PBD_ERR_ARG;
  for (int i = 0; i < count; ++i)
    if (!std::isfinite(heads[i].score) || heads[i].nparts < 0 || heads[i].nparts > mp) return PBD_ERR_ARG;
  std::vector<GtCentreBox> cb((size_t)count);
  for (int i = 0; i < count; ++i)
    if (heads[i].nparts > 0) cb[i] = gt_centre_box(boxes + (size_t)i * mp * 4, heads[i].nparts);
  for (int g = 0; g < ngt; ++g) {
    int b = -1;
    double ob = 0.0;
    for (int i = 0; i < count; ++i) {
      if (heads[i].nparts == 0) continue;
      const double ov = gt_overlap(gt + (size_t)g * 4, cb[i]);
      if (!(ov > overlap)) continue;
      if (b < 0 || heads[i].score > heads[b].score) { b = i; ob = ov; }   // (the first of equal scores stays: MATLAB's max)
    }
    best[g] = b; o[g] = ob;
  }
  return PBD_OK;
}

int pbd_candidates_select_gt(pbd_handle* h, const double* gt, int ngt, double overlap, const pbd_candidate_head* heads,
                             const int32_t* boxes, int count, int32_t* best, double* o) {
  if (!h) return PBD_ERR_ARG;
  int rc = pbd_i_gt_check(h, gt, &ngt, 1, overlap, false);
  if (rc) return rc;
  if (count < 0 || (count > 0 && (!heads || !boxes)) || (ngt > 0 && (!best || !o))) return fail(h, PBD_ERR_ARG, "heads / boxes / count / best / o");
  for (int i = 0; i < count; ++i) {
    if (!std::isfinite(heads[i].score)) return fail(h, PBD_ERR_ARG, "non-finite score: its order is undefined");
    if (heads[i].nparts < 0 || heads[i].nparts > h->max_parts) return fail(h, PBD_ERR_ARG, "nparts outside 0..max_parts");
  }
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  for (int g = 0; g < ngt; ++g) { best[g] = -1; o[g] = 0.0; }
  if (ngt == 0 || count == 0) return PBD_OK;
  ON_DEVICE(h);
  const int mp = h->max_parts;
  const size_t st = h->cand_stride, n = (size_t)count;
  std::vector<char> rec(st * n, 0);
  for (size_t i = 0; i < n; ++i) pbd_rec_put(rec.data() + st * i, mp, heads, boxes, nullptr, i);
  CallScratch s(h);
  GtBoxArgs a = gt_args(h, 1, overlap);
  char* d_rec = s.dev<char>(st * n);
  int* d_cnt = s.dev<int>(2);
  double* d_gt = s.dev<double>((size_t)ngt * 4);
  a.in.p = d_rec; a.in.count = d_cnt; a.in.capacity = count; a.in.nlevels = 0;
  a.gt = d_gt; a.ngt = d_cnt + 1;
  a.cbox = s.dev<double4>(n); a.key = s.dev<unsigned>(n); a.rank = s.dev<unsigned long long>(n); a.frame = s.dev<int>(n);
  a.found = s.dev<int>(PBD_GT_MAX); a.o = s.dev<double>(PBD_GT_MAX); a.best = s.dev<int>(PBD_GT_MAX);
  const int cnt2[2] = {count, ngt};
  s.up(d_rec, rec.data(), st * n);
  s.up(d_cnt, cnt2, sizeof(cnt2));
  s.up(d_gt, gt, sizeof(double) * 4 * ngt);
  if (s.ok()) {
    launch_gtbox(a, ngt, h->stream);
    s.launched();
  }
  s.down(best, a.best, sizeof(int) * ngt);
  s.down(o, a.o, sizeof(double) * ngt);
  return s.finish("gt boxes: ");
}

}  // extern "C"
#pragma GCC visibility pop
