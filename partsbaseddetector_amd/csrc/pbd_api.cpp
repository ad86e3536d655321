// pbd_api.cpp — host side of libpbd_hip.so: model ingestion, part-tree round
// scheduling, per-geometry frame plan (buffers + kernel work tables), stage
// orchestration and the C ABI of include/pbd_c.h.
//
// The product path never falls back to a CPU implementation: every stage is a
// HIP kernel launch; host code only plans, launches and (for the few hundred
// candidates of a frame) orders the output like a single-threaded reference run.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <new>
#include "pbd_internal.hpp"
#include "pbd_split.hpp"

// ---------------------------------------------------------------------------
// model
// ---------------------------------------------------------------------------
// The weights of one bank of nf filters of ONE size (the whole model, or one size group of a mixed bank) in every layout the filter-bank
// kernels read: g.nfpad, g.d_wT (transposed, converted to T, the 16-byte B copies and the border cell), and for a split bank g.d_wS /
// g.d_oscale.
static int upload_bank(pbd_handle* h, const float* filt, int nf, int kh, int kw, SizeGroup& g) {
  const pbd_model_desc& m = h->md;
  g.kh = kh; g.kw = kw; g.nf = nf;
  // filters transposed to [tap][c][nfpad] (n contiguous): scalar loads in the VALU kernel,
  // B-operand rows in the MFMA kernel.  nfpad is a multiple of 160 (5 x 32-wide MFMA n-tiles).
  g.nfpad = ((nf + 159) / 160) * 160;
  // + one trailing border cell (0, and 1 in the truncation channel flen - 1): the source the persistent filter-bank kernel
  // streams out-of-level cells from (src/SpatialConvolutionEngine.cpp:147-155)
  const size_t wt_n = (size_t)kh * kw * m.flen * g.nfpad;
  std::vector<float> wT(3 * wt_n + m.flen, 0.f);
  wT[wt_n + m.flen - 1] = 1.f;
  // ... and the same filters once more as [tap][16-channel half][k = 0..3][nfpad][s = 0..3] = channel 16 half + 4 k + s: the lane
  // (k, filter) of the persistent kernel's B operand reads its four k-steps of a tap with ONE 16-byte load (eight
  // global_load_dword per 32 MFMAs cost the MFMA pipe a quarter of its rate: tests/tools/mfma_rate_probe.hip)
  if (m.flen == PBD_FLEN)
    for (int n = 0; n < nf; ++n)
      for (int tap = 0; tap < kh * kw; ++tap)
        for (int c = 0; c < m.flen; ++c)
        {
          const float w = filt[((size_t)n * kh * kw + tap) * m.flen + c];
          wT[wt_n + m.flen + ((((size_t)tap * 2 + c / 16) * 4 + (c % 16) / 4) * g.nfpad + n) * 4 + c % 4] = w;     // k = (c % 16) / 4, s = c % 4
          // third copy, [tap][half][k][nfpad][u] with channel = 16 half + 4 u + k: the B operand of k_conv_mfma16<.., B4>
          wT[2 * wt_n + m.flen + ((((size_t)tap * 2 + c / 16) * 4 + c % 4) * g.nfpad + n) * 4 + (c % 16) / 4] = w;
        }
  for (int n = 0; n < nf; ++n)
    for (int i = 0; i < kh; ++i)
      for (int j = 0; j < kw; ++j)
        for (int c = 0; c < m.flen; ++c)
          wT[((size_t)(i * kw + j) * m.flen + c) * g.nfpad + n] =
              filt[(((size_t)n * kh + i) * kw + j) * m.flen + c];
  int rc;
  if ((rc = model_alloc(h, (char**)&g.d_wT, wT.size() * h->ts))) return rc;
  if (h->ts == 8) {   // filters convertTo(DataType<double>), src/PartsBasedDetector.cpp:113-117 (exact widening)
    std::vector<double> wd(wT.begin(), wT.end());
    // the double filter bank's 16-byte B layout replaces the (unused) float copy behind the border cell:
    // [tap][8-channel group][k][nfpad][u = 0, 1], channel = 8 group + 4 u + k (k_conv_mfma16<double, 4, .., B4>)
    if (m.flen == PBD_FLEN)
      for (int n = 0; n < nf; ++n)
        for (int tap = 0; tap < kh * kw; ++tap)
          for (int c = 0; c < m.flen; ++c)
            wd[wt_n + m.flen + ((((size_t)tap * 4 + c / 8) * 4 + c % 4) * g.nfpad + n) * 2 + (c % 8) / 4] =
                (double)filt[((size_t)n * kh * kw + tap) * m.flen + c];
    HIPCHK(h, hipMemcpy(g.d_wT, wd.data(), wd.size() * sizeof(double), hipMemcpyHostToDevice));
  } else {
    HIPCHK(h, hipMemcpy(g.d_wT, wT.data(), wT.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  if (h->split_parts) {   // the three exact bfloat16 parts of every weight (or two binary16 parts of the scaled weight), in the MFMA operand order of k_conv_split32
    std::vector<uint16_t> wS;
    if (h->split_parts == 3) conv_split_filters(filt, nf, kh, kw, wS);
    else {
      std::vector<float> osc;
      conv_split16_filters(filt, nf, kh, kw, wS, osc);
      if ((rc = model_alloc(h, &g.d_oscale, osc.size()))) return rc;
      HIPCHK(h, hipMemcpy(g.d_oscale, osc.data(), osc.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if ((rc = model_alloc(h, &g.d_wS, wS.size()))) return rc;
    HIPCHK(h, hipMemcpy(g.d_wS, wS.data(), wS.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  }
  return PBD_OK;
}

static int upload_model(pbd_handle* h) {
  const pbd_model_desc& m = h->md;
  int rc;
  if (!h->mixed) {
    SizeGroup g;
    rc = upload_bank(h, h->filters.data(), m.nfilters, m.kh, m.kw, g);
    h->d_wT = g.d_wT; h->d_wS = g.d_wS; h->d_split_oscale = g.d_oscale; h->nfpad = g.nfpad;
    if (rc) return rc;
  } else {
    // size groups (plan_model): each uploaded as a uniform bank of its own
    size_t off = 0;
    for (SizeGroup& g : h->groups) {
      if ((rc = upload_bank(h, h->filters.data() + off, g.nf, g.kh, g.kw, g))) return rc;
      off += (size_t)g.nf * g.kh * g.kw * m.flen;
    }
  }
  // orientation-snap table of the HOG kernel (k_hog.hip): 511 x 511 bytes, computed on the device by the reference's own
  // comparison chain in T
  if ((rc = model_alloc(h, &h->d_hog_lut, hog_binlut_bytes()))) return rc;
  launch_hog_binlut(h->d_hog_lut, h->ts, h->stream);
  LAUNCHCHK(h, "HOG orientation table");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // biasw plus one trailing 0 (used by the stand-alone pbd_dt2d)
  std::vector<float> bw(h->biasw);
  bw.push_back(0.f);
  if ((rc = model_alloc(h, &h->d_biasw, bw.size()))) return rc;
  HIPCHK(h, hipMemcpy(h->d_biasw, bw.data(), bw.size() * sizeof(float), hipMemcpyHostToDevice));
  const int nc = m.ncomponents, mp = h->max_parts;
  std::vector<int> par(nc * mp, 0), pl0(nc * mp, 0), npv(nc, 0), flt(nc * mp, 0), dep(nc * mp, 0);
  h->max_depth = 0;
  for (int c = 0; c < nc; ++c) {
    const int p0 = h->part_offset[c], cnp = h->part_offset[c + 1] - p0;
    npv[c] = cnp;
    for (int p = 0; p < cnp; ++p) {
      par[c * mp + p] = h->parts[p0 + p].parent;
      pl0[c * mp + p] = (p > 0) ? h->parts[p0 + p].plane0 - h->comp_plane0[c] : 0;
      flt[c * mp + p] = p0 + p;
      dep[c * mp + p] = (p > 0) ? dep[c * mp + h->parts[p0 + p].parent] + 1 : 0;   // parents precede children (validated)
      h->max_depth = std::max(h->max_depth, dep[c * mp + p]);
    }
  }
  if ((rc = model_alloc(h, &h->d_flat, flt.size())) || (rc = model_alloc(h, &h->d_depth, dep.size()))) return rc;
  HIPCHK(h, hipMemcpy(h->d_flat, flt.data(), flt.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_depth, dep.data(), dep.size() * sizeof(int), hipMemcpyHostToDevice));
  if ((rc = model_alloc(h, &h->d_parent, par.size())) || (rc = model_alloc(h, &h->d_plane0, pl0.size())) ||
      (rc = model_alloc(h, &h->d_nparts, npv.size())))
    return rc;
  HIPCHK(h, hipMemcpy(h->d_parent, par.data(), par.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_plane0, pl0.data(), pl0.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_nparts, npv.data(), npv.size() * sizeof(int), hipMemcpyHostToDevice));
  // rows of the filter of every (flat part, mixture): the box size of back-tracking (entries beyond a part's K repeat its last mixture)
  std::vector<int> mix_rows(h->parts.size() * PBD_MAX_MIX, 0);
  for (size_t fp = 0; fp < h->parts.size(); ++fp)
    for (int k = 0; k < PBD_MAX_MIX; ++k) {
      const int fid = h->parts[fp].filterid[std::min(k, h->parts[fp].K - 1)];
      mix_rows[fp * PBD_MAX_MIX + k] = h->mixed ? h->fkh[fid] : m.kh;
    }
  if ((rc = model_alloc(h, &h->d_mix_rows, mix_rows.size()))) return rc;
  HIPCHK(h, hipMemcpy(h->d_mix_rows, mix_rows.data(), mix_rows.size() * sizeof(int), hipMemcpyHostToDevice));
  // candidates
  const int cap = h->opt.max_candidates;
  h->cand_stride = pbd_rec_bytes(mp);
  if ((rc = model_alloc(h, &h->d_cand_count, 1)) || (rc = model_alloc(h, &h->d_cand_rec, cap)) ||
      (rc = model_alloc(h, &h->d_cand_out, h->cand_stride * cap)) ||
      (rc = model_alloc(h, &h->h_cand_out, h->cand_stride * cap, true, false)) ||   // (the pinned candidate buffers are not part of the footprint)
      (rc = model_alloc(h, &h->h_cand_count, 4, true, false)))
    return rc;
  return PBD_OK;
}

// ---------------------------------------------------------------------------
// frame plan
// ---------------------------------------------------------------------------
static const int kFirstCopy = PBD_FIRST_COPY;  // records fetched together with the count (per frame of the plan; grows, pbd_i_finish_frame)
template <typename T>
static int dev_upload(pbd_handle* h, T** p, const std::vector<T>& v) {
  int rc = dev_alloc(h, p, v.size());
  if (rc) return rc;
  if (!v.empty()) HIPCHK(h, hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return PBD_OK;
}

// ---- stage state: the ONE place the validity flags of the frame's planes change.  A run_* stage calls its transition behind its
// launches, a replayed graph (enqueue_all) the same four in stage order, and so do the setters that hand a whole stage in.
// Compact plan: validity of the stage planes the DP overwrites (pbd_internal.hpp).  all = true: a producer stage has just
// written every plane; false: min() has just reused the memory.
static void compact_mark_feat(pbd_handle* h, bool all) { if (h->compact) h->feat_ok.assign((size_t)h->nvl, all ? 1 : 0); }
static void compact_mark_resp(pbd_handle* h, bool all) { if (h->compact) h->resp_ok.assign((size_t)h->nvl * h->md.nfilters, all ? 1 : 0); }
// nothing of the plan's geometry has been computed or handed in (a new plan, pbd_begin_frame)
static void reset_stages(pbd_handle* h) {
  h->have_pyr = h->have_feat = h->have_resp = h->have_dp = false;
  h->min_ran = h->ik_lazy = false;
  h->feat_ok.clear(); h->resp_ok.clear(); h->ext_set.clear(); h->root_set.clear();   // (sized again by whoever marks a plane next)
  h->lat_masked = false;
}
static void mark_pyramid(pbd_handle* h) {
  h->have_pyr = true;
  if (h->compact) h->have_dp = h->min_ran = h->ik_lazy = false;   // the level images + features share their memory with the Ik planes / the x pass's scratch:
                                                     // the previous min()'s tables are gone (a plane handed in later is then NOT on top of a min())
}
// split_written: the split-product bank's copy of the features was written with them (k_hog's epilogue)
static void mark_features(pbd_handle* h, bool split_written) {
  h->feat_split_ok = split_written;
  h->have_feat = true;
  compact_mark_feat(h, true);
  if (h->compact) h->have_dp = h->min_ran = h->ik_lazy = false;
}
static void mark_responses(pbd_handle* h) { h->have_resp = true; compact_mark_resp(h, true); h->lat_masked = false; }
// latent detection: the resident responses now carry a mask, and d_lat_flags its flags, until responses are produced or handed in again
// (the planes stay valid responses: pbd_get_level_response returns them masked, min() runs on them)
static void mark_latent_mask(pbd_handle* h, int component) { h->lat_masked = true; h->lat_component = component; }
static void mark_min(pbd_handle* h, bool timed) {
  h->min_timed = timed;
  h->have_dp = h->min_ran = true;
  h->ik_lazy = h->fold;                 // fold plans: the Ik planes are not materialised (ensure_ik); the three-kernel structure's k_reduce has written them
  h->ext_ptr = h->root_dirty = false;   // back-tracking reads this min()'s own tables again, thresholded by it
  if (h->compact) {     // their memory now holds the DP's planes: every feature / response plane is stale until produced or handed in again
    h->have_pyr = h->have_feat = h->have_resp = false;
    h->feat_split_ok = false;   // (the split bank's copy of the features shared the x pass's pointer planes)
    compact_mark_feat(h, false);
    compact_mark_resp(h, false);
  }
}

void free_frame(pbd_handle* h) {
  drop_graph(h);   // the captured launches point into the buffers freed below
  h->frames_on_plan = 0;
  h->frame_allocs.clear();
  h->d_extx = h->d_exty = nullptr; h->d_ext_base = nullptr; h->ext_ptr = false;
  h->d_cf_mask = nullptr; h->cf_mask_bytes = 0;
  h->d_ik_blocks = nullptr; h->d_ik_cells = nullptr; h->n_ik_blocks = 0;
  h->d_lat_jobs = nullptr; h->d_lat_blocks = nullptr; h->d_lat_flags = nullptr; h->d_lat_partial = nullptr; h->n_lat_blocks = 0;
  h->fw = h->fh = h->fcn = 0; h->fdepth = 0; h->fesz = 1; h->ldepth = 0; h->lesz = 1;
  h->d_matjobs = nullptr; h->d_matruns = nullptr; h->d_mattaps = nullptr;
  reset_stages(h);
  h->feat_split_ok = false;
}

static bool all_active_set(const pbd_handle* h, const std::vector<char>& v, int per_level) {
  if (v.size() != (size_t)h->nvl * per_level) return false;
  for (int l = 0; l < h->nvl; ++l) {
    if (!h->lv[l].active || h->lv[l].cw == 0 || h->lv[l].ch == 0) continue;
    for (int k = 0; k < per_level; ++k) if (!v[(size_t)l * per_level + k]) return false;
  }
  return true;
}

// Probe and tune builds: the planner's DT knobs from the environment (product builds: the defaults)
static PlanKnobs read_plan_knobs() {
  PlanKnobs k;
  if (const char* e = PBD_PROBE_ENV("PBD_DT_NT")) k.dt_nt = std::max(64, std::min(256, atoi(e) & ~63));
  if (const char* e = PBD_PROBE_ENV("PBD_DT_SEG")) k.dt_seg = atoi(e);
  if (const char* e = PBD_PROBE_ENV("PBD_DT_BUDGET_KB")) k.dt_budget_kb = atoi(e);
  if (const char* e = PBD_PROBE_ENV("PBD_DT_BUDGET_B")) k.dt_budget_b = atoi(e);
  if (const char* e = PBD_PROBE_ENV("PBD_DT_XCD_CHUNK")) k.xcd_chunk = atoi(e);
  return k;
}

// The frame plan of one geometry (pbd_plan.cpp): buffers, then every work table, uploaded once and reused
int plan_frame(pbd_handle* h, int w, int hgt, int cn, int batch, int depth) {
  if (h->fw == w && h->fh == hgt && h->fcn == cn && h->batch == batch && h->fdepth == depth) return PBD_OK;
  if (cn != 1 && cn != 3) return fail(h, PBD_ERR_UNSUPPORTED, "image: 1 or 3 channels");
  const int esz = depth_esz(depth);
  if (!esz) return fail(h, PBD_ERR_UNSUPPORTED, "Unsupported image type (src/HOGFeatures.cpp:136-146: CV_8U, CV_16U, CV_32F, CV_64F)");
  if (esz > 1 && batch != 1) return fail(h, PBD_ERR_UNSUPPORTED, "batches of frames: 8-bit images");
  if (batch < 1 || batch > 64) return fail(h, PBD_ERR_ARG, "batch: 1..64 frames");
  hipStreamSynchronize(h->stream);
  free_frame(h);
  FrameSpec fs;
  fs.w = w; fs.h = hgt; fs.cn = cn; fs.batch = batch; fs.depth = depth; fs.level_set = h->level_set;
  FrameLayout lay;
  int rc = plan_layout(*h, fs, lay, &h->err);
  if (rc) return rc;
  std::vector<char*> regions(lay.regions.size(), nullptr);
  for (size_t i = 0; i < regions.size(); ++i)
    if ((rc = dev_alloc(h, &regions[i], lay.regions[i]))) return rc;
  const FrameBases b = frame_bases(lay, regions.data());
  int ncu = 256;
  { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, h->opt.device) == hipSuccess && pr.multiProcessorCount > 0) ncu = pr.multiProcessorCount; }
  h->ncu = ncu;
  FrameTables t;
  if ((rc = plan_tables(*h, fs, lay, b, ncu, h->dt_geom, h->knobs, t, &h->err))) return rc;
  if ((rc = dev_upload(h, &h->d_pyrjobs, t.pyrjobs)) || (rc = dev_upload(h, &h->d_levels, t.levels)) ||
      (h->pyr_kind == PBD_PYRAMID_MATLAB && ((rc = dev_upload(h, &h->d_matjobs, t.matjobs)) || (rc = dev_upload(h, &h->d_matruns, t.matruns)) ||
                                             (rc = dev_upload(h, &h->d_mattaps, t.mattaps)))) ||
      (h->pad > 0 && ((rc = dev_upload(h, &h->d_hog_levels, t.hog_levels)) || (rc = dev_upload(h, &h->d_padjobs, t.padjobs)) ||
                      (rc = dev_upload(h, &h->d_padblocks, t.padblk)))) ||
      (rc = dev_upload(h, &h->d_hog_tiles, t.hog_tiles)) || (rc = dev_upload(h, &h->d_conv_tiles, t.conv_tiles)) ||
      (h->mixed && (rc = dev_upload(h, &h->d_conv_tiles_mix, t.conv_tiles_mix))) ||
      (rc = dev_upload(h, &h->d_dtmaps, t.maps)) || (rc = dev_upload(h, &h->d_dttasks, t.tasks)) ||
      (rc = dev_upload(h, &h->d_foldjobs, t.folds)) || (rc = dev_upload(h, &h->d_foldx, t.foldx)) ||
      (rc = dev_upload(h, &h->d_redjobs, t.red)) || (rc = dev_upload(h, &h->d_redblocks, t.redblk)) ||
      (rc = dev_upload(h, &h->d_rootjobs, t.rootjobs)) || (rc = dev_upload(h, &h->d_rootblocks, t.rootblk)) ||
      (rc = dev_upload(h, &h->d_back, t.back)) || (rc = dev_upload(h, &h->d_scr_base, t.scr_base)) ||
      (rc = dev_upload(h, &h->d_pick, t.pick)))
    return rc;
  {   // k_ik_fill's work table (fold plans): one job per (level, part) that has a message, one block per 256 cells
    const size_t nflat = h->parts.size();
    std::vector<ReduceBlock> blocks;
    std::vector<unsigned> cells(t.pick.size(), 0);
    for (size_t i = 0; i < t.pick.size(); ++i) {
      if (t.pick[i] == PBD_NO_PICK) continue;
      const Level& L = lay.lv[i / nflat];
      cells[i] = (unsigned)L.cw * (unsigned)L.ch;
      for (unsigned c0 = 0; c0 < cells[i]; c0 += 256) blocks.push_back(ReduceBlock{(int)i, c0});
    }
    if ((rc = dev_upload(h, &h->d_ik_cells, cells)) || (rc = dev_upload(h, &h->d_ik_blocks, blocks))) return rc;
    h->n_ik_blocks = (int)blocks.size();
  }
  h->lv = lay.lv; h->nlevels = lay.nlevels; h->batch = batch; h->nvl = lay.nvl;
  h->first_copy = kFirstCopy * batch;
  h->cells = lay.cells; h->pyr_bytes = lay.pyr_bytes; h->compact = lay.compact; h->dt_cap_elems = lay.dt_cap_elems;
  h->d_img = (uint8_t*)b.p[FB_IMG]; h->d_pyr = (uint8_t*)b.p[FB_PYR]; h->d_feat = b.p[FB_FEAT]; h->d_resp = b.p[FB_RESP];
  h->d_pk = (uint8_t*)b.p[FB_PK]; h->d_rootv = b.p[FB_ROOTV]; h->d_rooti = (int*)b.p[FB_ROOTI]; h->d_nms_mask = (uint8_t*)b.p[FB_NMS_MASK];
  h->d_dt_tmpT = b.p[FB_DT_TMPT]; h->d_dt_sdt = b.p[FB_DT_SDT]; h->d_dt_ixT = b.p[FB_DT_IXT]; h->d_dt_iy = b.p[FB_DT_IY]; h->dt_ptr_bytes = lay.ptr_bytes;
  h->d_acc = b.p[FB_ACC]; h->d_feat_split = (uint16_t*)b.p[FB_FEAT_SPLIT];
  h->pyr_launches = std::move(t.pyr_launches);
  if (h->pad == 0) { h->d_hog_levels = h->d_levels; h->d_padjobs = nullptr; h->d_padblocks = nullptr; }
  h->n_padblocks = (int)t.padblk.size();
  h->hog_tc = t.hog_tc; h->n_hog_tiles = (int)t.hog_tiles.size(); h->n_conv_tiles = (int)t.conv_tiles.size();
  h->dt_nt = t.dt_nt; h->dt_lds = t.dt_lds;
  h->rl = std::move(t.rl);
  h->n_rootjobs = (int)t.rootjobs.size(); h->n_rootblocks = (int)t.rootblk.size();
  h->root_cells = t.root_cells; h->root_maxcells = t.root_maxcells;
  h->scr_base = std::move(t.scr_base);
  h->fw = w; h->fh = hgt; h->fcn = cn; h->fdepth = depth; h->fesz = esz;
  h->lesz = lay.esz; h->ldepth = h->pyr_kind == PBD_PYRAMID_MATLAB ? PBD_DEPTH_64F : depth;
  return PBD_OK;
}
// ---------------------------------------------------------------------------
// stages
// ---------------------------------------------------------------------------
static int run_image_pyramid(pbd_handle* h, const uint8_t* d_src, int stride) {
  // one launch for the first octave of every frame of the batch (cv::resize), one per octave step below it (cv::pyrDown)
  for (size_t i = 0; i < h->pyr_launches.size(); ++i) {
    const PyrLaunch& P = h->pyr_launches[i];
    if (h->pyr_kind == PBD_PYRAMID_MATLAB) {   // featpyramid.m:24-34: area resize of the 8-bit frame into double levels, then reduce (k_pyramid_mat.hip)
      if (i == 0) launch_resize_area(h->d_matjobs + P.job0, P.njobs, P.maxpix, h->d_matruns, h->d_mattaps, h->fcn, stride, false, d_src, h->d_pyr, h->stream);
      else launch_reduce_f64(h->d_matjobs + P.job0, P.njobs, P.maxpix, h->fcn, h->d_pyr, h->stream);
    } else
    if (h->fdepth != PBD_DEPTH_8U) {   // 16-bit / float / double frames (pbd_detect_image): the plain per-element kernels
      if (i == 0) launch_resize_any(h->d_pyrjobs + P.job0, P.njobs, P.maxpix, h->fcn, h->fdepth, stride, d_src, h->d_pyr, h->stream);
      else launch_pyrdown_any(h->d_pyrjobs + P.job0, P.njobs, P.maxpix, h->fcn, h->fdepth, h->d_pyr, h->stream);
    } else
    if (i == 0) launch_resize(h->d_pyrjobs + P.job0, P.njobs, P.maxpix, h->fcn, stride, d_src, h->d_pyr, h->stream);
    else launch_pyrdown(h->d_pyrjobs + P.job0, P.njobs, P.maxw, P.maxh, h->fcn, h->d_pyr, h->stream);
  }
  LAUNCHCHK(h, "image pyramid");
  mark_pyramid(h);
  return PBD_OK;
}

static int run_hog(pbd_handle* h) {
  uint16_t* split = h->split_parts ? h->d_feat_split : nullptr;
  launch_hog(h->d_hog_tiles, h->n_hog_tiles, h->d_hog_levels, h->d_pyr, h->d_feat, h->ts, h->fcn, h->md.sbin, h->hog_tc, h->d_hog_lut, split, h->split_parts, h->ldepth, h->stream);
  // boundary padding: the border ring of every level, on every frame — the compact plan's DP reuses the feature memory, and
  // pbd_set_level_features may have left a caller's border there (a frame's result never depends on what ran before it)
  if (h->pad > 0) launch_featpad(h->d_padjobs, h->d_padblocks, h->n_padblocks, h->d_feat, h->ts, split, h->split_parts, h->stream);
  LAUNCHCHK(h, "HOG");
  mark_features(h, split != nullptr);
  return PBD_OK;
}

// A pyramid-store frame's front end (include/pbd_c.h "pyramid store"): k_pyrstore_load writes the batch's features from the slots, and
// the split banks' parts with them.  The level images are not produced: whatever d_pyr holds belongs to an earlier frame.
static int run_stored_load(pbd_handle* h, const PyrCopyTable& t) {
  launch_pyrstore_load(t, h->batch, h->split_parts ? h->d_feat_split : nullptr, h->split_parts, h->stream);
  LAUNCHCHK(h, "pyramid store load");
  h->have_pyr = false;
  mark_features(h, true);
  return PBD_OK;
}

// The split-product banks read the features as bfloat16 / binary16 parts: written by k_hog's epilogue; features handed in by the
// caller (pbd_set_level_features) are split here, in front of the bank (a pass over 25 MB per frame)
static void ensure_feat_split(pbd_handle* h) {
  if (!h->split_parts || h->feat_split_ok) return;
  if (h->split_parts == 2) launch_feat_split16((const float*)h->d_feat, h->d_feat_split, h->cells, h->stream);
  else launch_feat_split((const float*)h->d_feat, h->d_feat_split, h->cells, h->stream);
  h->feat_split_ok = true;
}

// One bank launch by the handle's mode and scalar type: `tiles` over nf filters of kh x kw (wT / wS / oscale: that bank's uploads).  nf_stride > 0:
// a size group of a mixed bank — the run-time-size instantiation, writing the group's planes of every level block of nf_stride planes
static void launch_bank(pbd_handle* h, const ConvTile* tiles, int nf, int nfpad, int kh, int kw, const void* wT, const uint16_t* wS,
                        const float* oscale, int nf_stride) {
  // wT: [tap][channel][nfpad], a border cell, (float: the [tap][half][k][n][s] copy,) then the [tap][group][k][n][u] copy the MFMA banks load 16 bytes at a time
  const size_t wt_n = (size_t)kh * kw * h->md.flen * nfpad, cell = h->md.flen;
  if (h->conv_mode == PBD_CONV_SPLIT_F16)   // ... over two scaled binary16 parts
    launch_conv_split16(tiles, h->n_conv_tiles, h->d_levels, h->d_feat_split, wS, (float*)h->d_resp, nf, kh, kw, oscale, h->stream, nf_stride);
  else if (h->conv_mode == PBD_CONV_SPLIT)   // the bank on the bf16 matrix units, over the features' three exact bfloat16 parts
    launch_conv_split(tiles, h->n_conv_tiles, h->d_levels, h->d_feat_split, wS, (float*)h->d_resp, nf, kh, kw, h->stream, nf_stride);
  else if (h->conv_mode == PBD_CONV_MFMA && h->ts == 8)
    launch_conv_mfma_f64(tiles, h->n_conv_tiles, h->d_levels, (const double*)h->d_feat, (const double*)wT + wt_n + cell, (double*)h->d_resp, nf, nfpad, kh, kw, h->stream, nf_stride);
  else if (h->conv_mode == PBD_CONV_MFMA)
    launch_conv_mfma16_f32(tiles, h->n_conv_tiles, h->d_levels, (const float*)h->d_feat, (const float*)wT + 2 * wt_n + cell, (float*)h->d_resp, nf, nfpad, kh, kw, h->stream, nf_stride);
  else
    launch_conv_exact(tiles, h->n_conv_tiles, h->d_levels, h->d_feat, wT, h->d_resp, h->ts, nf, nfpad, kh, kw, h->stream, nf_stride);
}

// Tuning and probe libraries (k_conv_variants.hip): the uniform bank of a handle under PBD_MFMA_VARIANT, PBD_SPLIT_VARIANT, PBD_CONV_LDS_KB or, probe
// build, PBD_MFMA64_QUARTERS / PBD_CONV_PRIO — a measured-and-dropped kernel or configuration; false: no knob is set for the handle's mode, or the bank
// is mixed: nothing launched.  The product has no such unit.
#if defined(PBD_TUNE) || defined(PBD_PROBES)
bool launch_conv_variant(const pbd_handle* h);
#else
static bool launch_conv_variant(const pbd_handle*) { return false; }
#endif

// The filter bank: one launch over the plan's tiles; a mixed bank: one launch per size group, over the group's copy of the tile list
static int run_pdf(pbd_handle* h) {
  const pbd_model_desc& m = h->md;
  ensure_feat_split(h);
  const bool variant_ran = launch_conv_variant(h);
  if (h->mixed) {
    for (size_t gi = 0; gi < h->groups.size(); ++gi) {
      const SizeGroup& g = h->groups[gi];
      launch_bank(h, h->d_conv_tiles_mix + gi * h->n_conv_tiles, g.nf, g.nfpad, g.kh, g.kw, g.d_wT, g.d_wS, g.d_oscale, m.nfilters);
    }
  } else if (!variant_ran) {
    launch_bank(h, h->d_conv_tiles, m.nfilters, h->nfpad, m.kh, m.kw, h->d_wT, h->d_wS, h->d_split_oscale, 0);
  }
  LAUNCHCHK(h, "filter bank");
  mark_responses(h);
  return PBD_OK;
}

// k_root over the plan's root jobs into the hit list: the root tables written (rescan: read back) and the hits above thresh, under `mask`
// (null: every cell) listed
static void root_hits(pbd_handle* h, double thresh, int rescan, const uint8_t* mask) {
  launch_root(h->d_rootjobs, h->d_rootblocks, h->n_rootblocks, thresh, h->d_cand_count, h->d_cand_rec, h->opt.max_candidates, h->ts,
              h->d_foldjobs, h->d_biasw, rescan, h->fold_mix, mask, mask ? h->d_rootv : nullptr, h->stream);
}
// pbd_options.reserved[0] = sz > 0: nonMaximaSuppression(rootv, sz) of every (level, component) plane on the device, then the hits
static void nms_and_rescan(pbd_handle* h) {
  hipMemsetAsync(h->d_nms_mask, 0, h->cells * (size_t)h->md.ncomponents, h->stream);
  launch_nms_roots(h->d_rootjobs, h->n_rootjobs, h->root_maxcells, h->d_rootv, h->ts, h->nms_sz, h->d_nms_mask, h->stream);
  root_hits(h, (double)h->md.thresh, 1, h->d_nms_mask);
}

// latent: the frame takes no hit list from the threshold (FrameRoute::latent)
static int run_dp_min(pbd_handle* h, bool latent = false) {
  const bool dpt = h->profiling && h->dp_timer_on;
  if (dpt) hipEventRecord(h->ev_dp0, h->stream);
  // one chain of rounds on the handle's stream.  fold: x pass (from round 1 on its loader folds the children's
  // messages) + y pass per round, the root's messages folded by k_root: 2 * rounds + 1 launches; legacy (models that
  // alias a filter id inside a component, or more than 8 mixtures): + the round's reduce launches.
  for (auto& R : h->rl) {
    launch_dt_pass(h->d_dttasks + R.xtask0, R.nxtasks, h->d_dtmaps, R.fold_x ? h->d_foldjobs : nullptr, R.fold_x ? h->d_foldx + R.foldx0 : nullptr, h->d_biasw, R.lds_x, h->ts, h->dt_nt, h->fold_mix, h->stream);
    launch_dt_pass(h->d_dttasks + R.ytask0, R.nytasks, h->d_dtmaps, nullptr, nullptr, h->d_biasw, R.lds_y, h->ts, h->dt_nt, 0, h->stream);
    for (auto& Wv : R.waves)
      launch_reduce(h->d_redjobs, h->d_redblocks + Wv.blk0, Wv.nblks, h->d_biasw, h->opt.dt_correct_ptr, h->ts, h->stream);
  }
  hipMemsetAsync(h->d_cand_count, 0, sizeof(int), h->stream);
  if (h->nms_sz > 0) {
    // score-map NMS in front of the back-tracking (src/nms.cpp:84-129; the reference's call site is commented out,
    // src/PartsBasedDetector.cpp:86): the root tables are written with no hit (threshold +inf), the block NMS runs on the
    // resident rootv planes, and the hit list is then compacted from (score > thresh) AND (local maximum)
    root_hits(h, INFINITY, 0, nullptr);
    nms_and_rescan(h);
  } else
  // (a latent frame takes no hit list from the threshold — detect.m:20 —: k_latent_best writes its one candidate)
  root_hits(h, latent ? (double)INFINITY : (double)h->md.thresh, 0, nullptr);
  if (dpt) hipEventRecord(h->ev_dp1, h->stream);
  LAUNCHCHK(h, "DP min");
  mark_min(h, dpt);
  return PBD_OK;
}

// Fold plans: the Ik planes of the current min(), written from the children's kept scores when somebody needs the planes themselves —
// never by a frame entry (enter_frame -> enqueue_all, captured graphs included), whose back-tracking picks Ik for the cells it visits.
// The kept scores stay intact as long as ik_lazy is set: the one entry that overwrites them under a valid min() (a response plane
// handed in on the compact plan, whose planes hold them) calls this first.
static int ensure_ik(pbd_handle* h) {
  if (!h->ik_lazy || !h->have_dp || !h->min_ran) return PBD_OK;
  launch_ik_fill(h->d_foldjobs, h->d_pick, h->d_ik_blocks, h->n_ik_blocks, h->d_ik_cells, h->ts, h->stream);
  LAUNCHCHK(h, "Ik planes");
  h->ik_lazy = false;
  return PBD_OK;
}

// ---- latent detection (include/pbd_c.h "latent detection"; k_latent.hip) ------------------------------------------------------
// The argument checks every latent entry makes, before anything is planned, uploaded or launched
int pbd_i_latent_check(pbd_handle* h, const int32_t* truth, const int32_t* mix, int nframes, int component, double overlap) {
  if (!truth) return fail(h, PBD_ERR_ARG, "latent detection: null truth boxes");
  if (h->in_group) return fail(h, PBD_ERR_UNSUPPORTED, "latent detection: not for a pbd_group member");
  if (h->nms_sz > 0) return fail(h, PBD_ERR_UNSUPPORTED, "latent detection: not with the score-map NMS (pbd_options.reserved[0] > 0)");
  if (!(overlap >= 0.0 && overlap < 1.0)) return fail(h, PBD_ERR_ARG, "latent detection: overlap must be in [0, 1)");
  const int nc = h->md.ncomponents, mp = h->max_parts;
  if (component < -1 || component >= nc) return fail(h, PBD_ERR_ARG, "latent detection: component out of range (-1: all)");
  if (nframes < 1 || nframes > PBD_MAX_BATCH) return fail(h, PBD_ERR_ARG, "batch: 1..64 frames");
  if (nframes > h->opt.max_candidates) return fail(h, PBD_ERR_CAPACITY, "latent detection: one record per frame; raise pbd_options.max_candidates");
  std::vector<int> owner((size_t)h->md.nfilters, -1);   // the (component, part) slot whose planes a filter id's mask is written into
  for (int c = 0; c < nc; ++c) {
    if (component >= 0 && c != component) continue;
    const int p0 = h->part_offset[c], np = h->part_offset[c + 1] - p0;
    for (int p = 0; p < np; ++p) {
      const PartInfo& P = h->parts[p0 + p];
      bool forced = false;
      for (int f = 0; f < nframes; ++f) {
        const int32_t* t = truth + ((size_t)f * mp + p) * 4;
        if (t[2] < 0 || t[3] < 0) return fail(h, PBD_ERR_ARG, "latent detection: a truth box with negative width or height");
        if (mix) {
          const int m = mix[(size_t)f * mp + p];
          if (m < -1 || m >= P.K) return fail(h, PBD_ERR_ARG, "latent detection: mix outside the part's mixtures (-1: free)");
          forced = forced || m >= 0;
        }
      }
      for (int k = 0; k < P.K; ++k) {
        int& o = owner[P.filterid[k]];
        // the mask is written into the plane in place: a plane two slots share would carry both slots' masks (and a forced mixture
        // would blank the plane of the one it shares a filter with)
        if (o >= 0 && (o != p0 + p || forced))
          return fail(h, PBD_ERR_UNSUPPORTED, "latent detection: a filter id is used by two (component, part) slots of the components searched: the mask is written into the shared response plane in place");
        o = p0 + p;
      }
    }
  }
  return PBD_OK;
}

// The frame plan's share (built on the first latent use of a plan): the work table of k_latent_mask — one job per (level, component,
// part, mixture) plane, one block per 256 cells —, the flags and k_latent_best's partials
static int latent_tables(pbd_handle* h) {
  if (h->d_lat_jobs) return PBD_OK;
  const int nc = h->md.ncomponents, mp = h->max_parts;
  std::vector<LatJob> jobs;
  std::vector<ReduceBlock> blocks;
  for (int l = 0; l < h->nvl; ++l) {
    const Level& L = h->lv[l];
    const size_t HW = (size_t)L.cw * L.ch;
    if (!L.active || HW == 0) continue;
    for (int c = 0; c < nc; ++c) {
      const int p0 = h->part_offset[c], np = h->part_offset[c + 1] - p0;
      for (int p = 0; p < np; ++p)
        for (int k = 0; k < h->parts[p0 + p].K; ++k) {
          const int fid = h->parts[p0 + p].filterid[k];
          LatJob J{};
          J.plane = h->d_resp + (L.cell_off * h->md.nfilters + (size_t)fid * HW) * h->ts;
          J.H = L.ch; J.W = L.cw; J.level = l; J.comp = c; J.part = p; J.mix = k;
          J.rows = h->mixed ? h->fkh[fid] : h->md.kh;
          J.flag = (l * nc + c) * mp + p;
          J.scale = L.scale;
          for (size_t c0 = 0; c0 < HW; c0 += 256) blocks.push_back(ReduceBlock{(int)jobs.size(), (unsigned)c0});
          jobs.push_back(J);
        }
    }
  }
  int rc;
  if ((rc = dev_upload(h, &h->d_lat_jobs, jobs)) || (rc = dev_upload(h, &h->d_lat_blocks, blocks)) ||
      (rc = dev_alloc(h, &h->d_lat_flags, (size_t)h->nvl * nc * mp)) || (rc = dev_alloc(h, &h->d_lat_partial, (size_t)std::max(h->n_rootblocks, 1))))
    return rc;
  h->n_lat_blocks = (int)blocks.size();
  return PBD_OK;
}

// On a planned frame: the tables above, and the truth / mixture tables of the frame (or of every frame of the batch), small device
// arrays uploaded in the handle's stream from a pinned staging copy (the caller's arrays may go away once the entry returns)
int pbd_i_latent_begin(pbd_handle* h, const LatentSource& s, int nframes) {
  int rc = latent_tables(h);
  if (rc) return rc;
  const int mp = h->max_parts;
  const size_t cap = (size_t)PBD_MAX_BATCH * mp * 5;
  if (!h->d_lat_truth && ((rc = model_alloc(h, &h->d_lat_truth, cap)) || (rc = model_alloc(h, &h->h_lat_truth, cap, true, false)))) return rc;
  const size_t nt = (size_t)nframes * mp * 4, nm = (size_t)nframes * mp;
  memcpy(h->h_lat_truth, s.truth, nt * sizeof(int));
  if (s.mix) memcpy(h->h_lat_truth + nt, s.mix, nm * sizeof(int));
  HIPCHK(h, hipMemcpyAsync(h->d_lat_truth, h->h_lat_truth, (nt + (s.mix ? nm : 0)) * sizeof(int), hipMemcpyHostToDevice, h->stream));
  h->lat_has_mix = s.mix != nullptr;
  h->lat_component = s.component; h->lat_overlap = s.overlap;
  return PBD_OK;
}

// between pdf() and min(): the mask of the resident response planes, the flags of every (level, component, part)
static int run_latent_mask(pbd_handle* h, int nframes) {
  const int nc = h->md.ncomponents, mp = h->max_parts;
  hipMemsetAsync(h->d_lat_flags, 0, (size_t)h->nvl * nc * mp * sizeof(int), h->stream);
  LatentMaskArgs a{};
  a.jobs = h->d_lat_jobs; a.blocks = h->d_lat_blocks;
  a.truth = h->d_lat_truth; a.mix = h->lat_has_mix ? h->d_lat_truth + (size_t)nframes * mp * 4 : nullptr;
  a.flags = h->d_lat_flags;
  a.nlevels = h->nlevels; a.mp = mp; a.component = h->lat_component; a.org = 1 + h->pad;
  a.overlap = h->lat_overlap;
  launch_latent_mask(a, h->n_lat_blocks, h->ts, h->stream);
  LAUNCHCHK(h, "latent mask");
  mark_latent_mask(h, h->lat_component);
  return PBD_OK;
}
// behind min(): the best root of every frame over its admissible pairs, as the candidate list k_backtrack walks
static int run_latent_best(pbd_handle* h) {
  LatentBestArgs a{};
  a.jobs = h->d_rootjobs; a.blocks = h->d_rootblocks; a.nblocks = h->n_rootblocks;
  a.flags = h->d_lat_flags; a.nparts = h->d_nparts;
  a.ncomp = h->md.ncomponents; a.mp = h->max_parts; a.nlevels = h->nlevels; a.nframes = h->batch;
  a.partial = h->d_lat_partial;
  a.count = h->d_cand_count; a.rec = h->d_cand_rec;
  launch_latent_best(a, h->ts, h->stream);
  LAUNCHCHK(h, "latent best");
  return PBD_OK;
}

// ---- the route of a frame on this handle (pbd_route.hpp) ----------------------------------------------------------------------
static RouteSettings route_settings(const pbd_handle* h, const FrameJob& job) {
  RouteSettings s;
  s.cand_mode = pbd_i_cand_mode(h); s.cand_nms = h->cand_nms;
  s.zf_on = h->zf_on; s.b3_on = h->b3_on; s.cl3_on = h->cl3_on; s.ps_on = h->ps_on;
  s.compact = h->compact; s.member = h->d_gsend != nullptr; s.zero_copy = PBD_ARGMIN_ZERO_COPY != 0;
  s.ps_compact_was = h->pf.ps_compact;
  // a frame's own min() records the DP events while profiling (run_dp_min); a stage entry back-tracks the tables of whichever min() ran last
  s.dp_timed = job.kind == FRAME_STAGE ? h->min_timed : h->profiling && h->dp_timer_on;
  return s;
}
// The frame's route, computed once and outside any capture, and the ONE assignment of the pending frame, whole, for every way a frame is enqueued:
// eager, replayed from the captured graph, by a stage entry (a failed enqueue flips pf.active back).  The kept results of the frame before go with it.
static int begin_pending(pbd_handle* h, const FrameJob& job, FrameRoute* r) {
  if (!route_frame(route_settings(h, job), job, r))
    return fail(h, PBD_ERR_STATE, "internal: no route for this frame under the handle's settings (an entry should have refused it)");
  h->pf = r->pending;
  h->b3_ready = h->cl3_ready = h->ps_ready = false;
  return PBD_OK;
}

// Back-tracking into the route's buffer, the route's post-stages behind it, then the records' way to the host.
// Round 6: a handle that is not a member of an RCCL-gathering group lets the back-tracking kernel write the records and the count straight
// into its pinned host buffers (device-mapped, coherent): no copy nodes behind the kernel, and never a second copy for
// records beyond a first block.  Group members keep the device buffer: the all-gather reads it.  In front of a post-stage (depth
// pruning, candidate filter: pbd_post.cpp) the records go to the device buffer it reads.
static int run_argmin_enqueue(pbd_handle* h, const FrameJob& job, const FrameRoute& r) {
  if (h->root_dirty) {   // root tables injected since min(): the hits are those of the tables now on the device
    hipMemsetAsync(h->d_cand_count, 0, sizeof(int), h->stream);
    if (h->nms_sz > 0) nms_and_rescan(h);
    else root_hits(h, (double)h->md.thresh, 1, nullptr);
    h->root_dirty = false;
  }
  BacktrackArgs a{};
  a.count = h->d_cand_count; a.rec = h->d_cand_rec; a.capacity = h->opt.max_candidates;
  a.back = h->d_back; a.ncomp = h->md.ncomponents;
  a.parent = h->d_parent; a.plane0 = h->d_plane0; a.nparts = h->d_nparts; a.max_parts = h->max_parts; a.mix_rows = h->d_mix_rows;
  a.out = pbd_i_route_buf(h, r.bt.out); a.out_stride = h->cand_stride;
  a.flat = h->d_flat; a.depth = h->d_depth; a.max_depth = h->max_depth; a.nflat = (int)h->parts.size();
  a.scr_base = h->d_scr_base; a.ix = h->d_dt_ixT; a.iy = h->d_dt_iy; a.ptr_bytes = h->dt_ptr_bytes; a.correct_ptr = h->opt.dt_correct_ptr;
  a.extx = h->ext_ptr ? h->d_extx : nullptr; a.exty = h->d_exty; a.ext_base = h->d_ext_base;
  a.count_out = r.bt_host_count ? h->h_cand_count : nullptr; a.pad = h->pad;
  a.folds = h->d_foldjobs; a.pick = h->ik_lazy && !h->ext_ptr ? h->d_pick : nullptr;
  launch_backtrack(a, h->ts, h->stream);
  int rc;
  if ((r.zf.on || r.filter.on) && (rc = pbd_i_post_enqueue(h, job, r))) return rc;
  if (r.gt && (rc = pbd_i_gt_enqueue(h, r))) return rc;
  if (job.kind == FRAME_MINE && (rc = pbd_i_mine_enqueue(h, r))) return rc;
  if (job.kind == FRAME_LATENT_WRITE && (rc = pbd_i_latent_write_enqueue(h, r))) return rc;
  if (job.kind == FRAME_EVAL && (rc = pbd_i_eval_enqueue(h, r))) return rc;
  LAUNCHCHK(h, r.zf.on ? "argmin + depth filter" : r.filter.on ? "argmin + candidate filter" : r.gt ? "argmin + gt boxes" : "argmin");
  if (r.count_d2h != CNT_NONE) HIPCHK(h, hipMemcpyAsync(h->h_cand_count, pbd_i_route_count(h, r.count_d2h), sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (!r.first_d2h && r.pack_count == CNT_NONE) return PBD_OK;
  // a first block of DEV_OUT's records goes with the count; members of an RCCL-gathering group send a fixed block (pbd_group.cpp sizes
  // its buffers for PBD_FIRST_COPY records)
  if (r.pack_count != CNT_NONE || h->first_copy < kFirstCopy * h->batch) h->first_copy = kFirstCopy * h->batch;
  const int first = std::min(h->first_copy, h->opt.max_candidates);
  if (r.pack_count != CNT_NONE) {   // {count, first records} for the all-gather instead of the D2H; of a cf block, [1]: kept in frame 0
    const int* count = pbd_i_route_count(h, r.pack_count) + (route_cf_block(r.pack_count) ? 1 : 0);
    HIPCHK(h, hipMemcpyAsync(h->d_gsend, count, sizeof(int), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_gsend + 16, h->d_cand_out, h->cand_stride * first, hipMemcpyDeviceToDevice, h->stream));
  } else
    HIPCHK(h, hipMemcpyAsync(h->h_cand_out, h->d_cand_out, h->cand_stride * first, hipMemcpyDeviceToHost, h->stream));
  return PBD_OK;
}

static int enqueue_stages(pbd_handle* h, const FrameJob& job, const FrameRoute& r, const uint8_t* d_src, int stride) {
  int rc;
  const bool prof = h->profiling;
  if (prof) hipEventRecord(h->ev[0], h->stream);
  if (job.stored) {   // a pyramid-store frame: its features (and the split banks' parts) come from the slots in one launch
    if ((rc = run_stored_load(h, *job.stored))) return rc;
    if (prof) { hipEventRecord(h->ev[1], h->stream); hipEventRecord(h->ev[2], h->stream); }   // (the load's time reads as the pyramid's)
  } else {
  if ((rc = run_image_pyramid(h, d_src, stride))) return rc;
  if (prof) hipEventRecord(h->ev[1], h->stream);
  if ((rc = run_hog(h))) return rc;
  if (prof) hipEventRecord(h->ev[2], h->stream);
  }
  if ((rc = run_pdf(h))) return rc;
  if (r.latent && (rc = run_latent_mask(h, h->batch))) return rc;   // (a latent frame's stage times: the mask in pdf's, the best root in min()'s)
  if (prof) hipEventRecord(h->ev[3], h->stream);
  if ((rc = run_dp_min(h, r.latent))) return rc;
  if (r.latent && (rc = run_latent_best(h))) return rc;
  if (prof) hipEventRecord(h->ev[4], h->stream);
  if ((rc = run_argmin_enqueue(h, job, r))) return rc;
  if (r.latent) h->root_dirty = true;   // the hit list is the latent record: a later pbd_dp_argmin thresholds the root tables again
  if (prof) hipEventRecord(h->ev[5], h->stream);
  if (r.pending.ps && (rc = pbd_i_run_part_scores(h, r))) return rc;
  if (r.pending.b3 && (rc = pbd_i_run_box3d(h, job, r))) return rc;
  return PBD_OK;
}

// A frame is ~40 launches whose arguments depend only on the frame geometry (the work tables are built once per
// geometry): with pbd_options.graph the second frame of a geometry is captured into a hipGraph (the first one
// runs eagerly: it also does the one-time per-device kernel attribute set-up, which is not a stream operation)
// and every later frame is ONE hipGraphLaunch.  The graph reads the frame from the handle's own image buffer, so
// an image that lives elsewhere in HBM is copied there first (0.9 MB, on the same stream).  Profiling runs (stage
// events) and level groups on extra streams use the eager path.
static int enqueue_routed(pbd_handle* h, const FrameJob& job, const FrameRoute& r, const uint8_t* d_src, int stride) {
  const bool graphable = h->opt.graph && !h->profiling;   // (frames of any depth: the launches depend on the plan only; round 5 replayed 8-bit plans only)
  int rc = pbd_i_post_buffers(h, r);
  if (rc) return rc;
  // depth-carrying frames run eagerly: the depth pointers are per frame; a captured graph stays for plain frames
  // latent frames too: the mask stage and the best-root reduction are theirs alone, the captured graph stays the plain frames'
  // gt-box frames too: the selection behind the back-tracking is theirs alone
  // pyramid-store frames too: their front end is the load; frames_on_plan and the captured graph stay the plain frames'
  if (job.kind != FRAME_PLAIN || job.stored) return enqueue_stages(h, job, r, d_src, stride);
  if (!graphable || h->frames_on_plan == 0) {
    h->frames_on_plan++;
    return enqueue_stages(h, job, r, d_src, stride);
  }
  const size_t row = (size_t)h->fw * h->fcn * h->fesz;
  if (d_src != h->d_img && (rc = copy_rows(h, h->d_img, d_src, (size_t)stride, row, (size_t)h->fh * h->batch, hipMemcpyDeviceToDevice))) return rc;   // (strided sources: single frames only)
  if (!h->gexec) {
    hipGraph_t graph = nullptr;
    HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    rc = enqueue_stages(h, job, r, h->d_img, (int)row);
    hipError_t e = hipStreamEndCapture(h->stream, &graph);
    if (rc) { if (graph) hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return fail(h, PBD_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    e = hipGraphInstantiate(&h->gexec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (e != hipSuccess) { h->gexec = nullptr; return fail(h, PBD_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e)); }
  }
  HIPCHK(h, hipGraphLaunch(h->gexec, h->stream));
  h->frames_on_plan++;
  // what the replayed stages leave behind: their own transitions, in stage order (graphs are never captured under profiling: no DP timing)
  mark_pyramid(h);
  mark_features(h, h->split_parts != 0);
  mark_responses(h);
  mark_min(h, false);
  return PBD_OK;
}
int enqueue_all(pbd_handle* h, const FrameJob& job, const uint8_t* d_src, int stride) {
  FrameRoute r;
  int rc = begin_pending(h, job, &r);
  if (!rc && (rc = enqueue_routed(h, job, r, d_src, stride))) h->pf.active = false;
  return rc;
}
// pbd_dp_argmin, pbd_dp_argbest: the back-tracking of the resident tables as a frame of its own; it scores nothing and computes no boxes
static int enqueue_stage_argmin(pbd_handle* h) {
  const FrameJob job{FRAME_STAGE};
  FrameRoute r;
  int rc = begin_pending(h, job, &r);
  if (!rc && (rc = run_argmin_enqueue(h, job, r))) h->pf.active = false;
  return rc;
}

// pyramid(): the frame(s) of `s` planned and uploaded, then the level images and the HOG features enqueued (pbd_pyramid_image; a
// pyramid-store put, whose frames may be a batch or on the device)
int pbd_i_front_end(pbd_handle* h, const FrameSource& s) {
  int rc = enter_frame(h, s, false);
  if (rc) return rc;
  const uint8_t* d_src = s.on_device ? (const uint8_t*)s.one : h->d_img;
  if ((rc = run_image_pyramid(h, d_src, s.on_device ? s.stride : s.w * s.cn * h->fesz))) return rc;
  return run_hog(h);
}

void read_stage_times(pbd_handle* h) {
  if (!h->profiling) return;
  for (int i = 0; i < 5; ++i) hipEventElapsedTime(&h->stage_ms[i], h->ev[i], h->ev[i + 1]);
  hipEventElapsedTime(&h->stage_ms[5], h->ev[0], h->ev[5]);
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
// the layouts of include/pbd_c.h that capi.py's ctypes / numpy mirrors rely on
static_assert(sizeof(pbd_camera) == 48, "pbd_camera layout");
static_assert(sizeof(pbd_box3d) == 80 && offsetof(pbd_box3d, zmin) == 20 && offsetof(pbd_box3d, x3d) == 32, "pbd_box3d layout");
static_assert(sizeof(pbd_part_score) == 24 && offsetof(pbd_part_score, bias) == 16, "pbd_part_score layout");
static_assert(sizeof(pbd_cluster3d) == 40 && offsetof(pbd_cluster3d, first) == 12 && offsetof(pbd_cluster3d, cx) == 16,
              "pbd_cluster3d layout");
#pragma GCC visibility push(default)
extern "C" {

// pbd_create / pbd_create_sized.  fsize != null: a size per filter (fsize[n] = {kh, kw}); all equal -> exactly the uniform handle,
// else a mixed bank (pbd_handle::mixed): the filters stably sorted by (kh, kw) into size groups, filter ids remapped to that order.
static int create_impl(const pbd_model_desc* model, const int32_t* fsize, const pbd_options* opt, pbd_handle** out, bool sized) {
  if (!out) return PBD_ERR_ARG;
  *out = nullptr;
  pbd_handle* h = new (std::nothrow) pbd_handle();
  if (!h) return PBD_ERR_ARG;
  *out = h;  // returned even on failure so that pbd_last_error() can be read; destroy it either way
  int rc = plan_model(*h, model, fsize, sized, opt, &h->err);
  if (rc) return rc;
  h->knobs = read_plan_knobs();
  const pbd_options& o = h->opt;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(h, PBD_ERR_HIP, "no HIP device visible");
  if (o.device < 0 || o.device >= ndev) return fail(h, PBD_ERR_ARG, "bad device ordinal");
  HIPCHK(h, hipSetDevice(o.device));
  HIPCHK(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  h->own_stream = true;
  for (int i = 0; i < 8; ++i) HIPCHK(h, hipEventCreate(&h->ev[i]));
  HIPCHK(h, hipEventCreate(&h->ev_dp0));
  HIPCHK(h, hipEventCreate(&h->ev_dp1));
  return upload_model(h);
}

int pbd_create(const pbd_model_desc* model, const pbd_options* opt, pbd_handle** out) { return create_impl(model, nullptr, opt, out, false); }
int pbd_create_sized(const pbd_model_desc* model, const int32_t* fsize, const pbd_options* opt, pbd_handle** out) {
  return create_impl(model, fsize, opt, out, true);
}
int pbd_get_filter_size(const pbd_handle* h, int filter, int32_t* kh, int32_t* kw) {
  if (!h || !kh || !kw || filter < 0 || filter >= h->md.nfilters) return PBD_ERR_ARG;
  if (h->mixed) { *kh = h->fkh[h->fperm[filter]]; *kw = h->fkw[h->fperm[filter]]; }
  else { *kh = h->md.kh; *kw = h->md.kw; }
  return PBD_OK;
}

int pbd_destroy(pbd_handle* h) {
  if (!h) return PBD_ERR_ARG;
  if (h->stream) hipStreamSynchronize(h->stream);
  free_frame(h);
  h->model_allocs.clear();
  for (int i = 0; i < 8; ++i) if (h->ev[i]) hipEventDestroy(h->ev[i]);
  if (h->ev_dp0) hipEventDestroy(h->ev_dp0);
  if (h->ev_dp1) hipEventDestroy(h->ev_dp1);
  if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
  delete h;
  return PBD_OK;
}

const char* pbd_last_error(const pbd_handle* h) { return h ? h->err.c_str() : "null handle"; }
int pbd_set_levels(pbd_handle* h, const int32_t* levels, int n) {
  if (!h || n < 0 || (n > 0 && !levels)) return PBD_ERR_ARG;
  std::vector<char> set;
  for (int i = 0; i < n; ++i) {
    if (levels[i] < 0 || levels[i] >= PBD_MAX_LEVELS) return fail(h, PBD_ERR_ARG, "level index out of range");
    if ((int)set.size() <= levels[i]) set.resize(levels[i] + 1, 0);
    set[levels[i]] = 1;
  }
  if (n > 0 && set.empty()) return fail(h, PBD_ERR_ARG, "empty level set");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  hipStreamSynchronize(h->stream);
  h->level_set.swap(set);
  free_frame(h);   // the work tables are per geometry AND level set: re-planned on the next frame
  return PBD_OK;
}
// train.m:95-96,121 model.interval = 2 while mining (include/pbd_c.h "one training round"): the interval enters the frame plan alone —
// the pyramid's geometry and job tables — so the plan and the captured graph are dropped and the next frame plans with the new one.
// The weights, the banks, the tuned DT geometry (h->dt_geom) and every setter's state are not the interval's and stay.
int pbd_set_interval(pbd_handle* h, int interval) {
  if (!h) return PBD_ERR_ARG;
  if (interval < 1 || interval > 16) return fail(h, PBD_ERR_ARG, "interval: 1..16 levels per octave");
  if (h->in_group) return fail(h, PBD_ERR_UNSUPPORTED, "interval: pbd_group members are not supported");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  if (interval == h->md.interval) return PBD_OK;
  ON_DEVICE(h);
  hipStreamSynchronize(h->stream);
  h->md.interval = interval;
  free_frame(h);
  return PBD_OK;
}
int pbd_get_interval(const pbd_handle* h) { return h ? h->md.interval : 0; }
// Boundary padding (include/pbd_c.h): the plan — buffers, work tables, captured graph — is per padding, dropped like pbd_set_levels does
int pbd_set_boundary_pad(pbd_handle* h, int pad) {
  if (!h) return PBD_ERR_ARG;
  if (pad < 0 || pad > 8) return fail(h, PBD_ERR_ARG, "boundary pad: 0 (off) .. 8 cells");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  if (pad == h->pad) return PBD_OK;
  ON_DEVICE(h);
  hipStreamSynchronize(h->stream);
  h->pad = pad;
  free_frame(h);
  return PBD_OK;
}
int pbd_get_boundary_pad(const pbd_handle* h) { return h ? h->pad : 0; }
// Pyramid kind (include/pbd_c.h): like the padding, the plan — geometry, buffers, work tables, captured graph — is per kind
int pbd_set_pyramid_kind(pbd_handle* h, int kind) {
  if (!h) return PBD_ERR_ARG;
  if (kind != PBD_PYRAMID_OPENCV && kind != PBD_PYRAMID_MATLAB) return fail(h, PBD_ERR_ARG, "pyramid kind: PBD_PYRAMID_OPENCV or PBD_PYRAMID_MATLAB");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  if (kind == h->pyr_kind) return PBD_OK;
  ON_DEVICE(h);
  hipStreamSynchronize(h->stream);
  h->pyr_kind = kind;
  free_frame(h);
  return PBD_OK;
}
int pbd_get_pyramid_kind(const pbd_handle* h) { return h ? h->pyr_kind : PBD_PYRAMID_OPENCV; }
int pbd_max_parts(const pbd_handle* h) { return h ? h->max_parts : 0; }

int pbd_set_stream(pbd_handle* h, void* s) {
  if (!h) return PBD_ERR_ARG;
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
  h->stream = (hipStream_t)s;
  h->own_stream = false;
  return PBD_OK;
}

// ---- stage entry points -----------------------------------------------------
int pbd_pyramid_geometry(const pbd_handle* h, int w, int hgt, int* nlevels, int32_t* img_w, int32_t* img_h,
                         int32_t* cell_w, int32_t* cell_h, float* scales) {
  if (!h || !nlevels) return PBD_ERR_ARG;
  static thread_local Level lv[PBD_MAX_LEVELS];
  int n = 0;
  if (w < 3 || hgt < 3 || (h->pyr_kind == PBD_PYRAMID_MATLAB ? compute_geometry_matlab(w, hgt, h->md.sbin, h->md.interval, &n, lv)
                                                             : compute_geometry(w, hgt, h->md.sbin, h->md.interval, &n, lv))) return PBD_ERR_ARG;
  pad_geometry(h->pad, n, lv);   // (the planes of a padded handle: what the stage getters and setters address)
  *nlevels = n;
  for (int l = 0; l < n; ++l) {
    if (img_w) img_w[l] = lv[l].iw;
    if (img_h) img_h[l] = lv[l].ih;
    if (cell_w) cell_w[l] = lv[l].cw;
    if (cell_h) cell_h[l] = lv[l].ch;
    if (scales) scales[l] = lv[l].scale;
  }
  return PBD_OK;
}

int pbd_begin_frame(pbd_handle* h, int w, int hgt, int cn) {
  if (!h) return PBD_ERR_ARG;
  ON_DEVICE(h);
  int rc = plan_frame(h, w, hgt, cn);
  if (rc) return rc;
  reset_stages(h);
  return PBD_OK;
}

// pyramid() on a host image of any depth the reference accepts (src/HOGFeatures.cpp:136-146): level images + HOG features
int pbd_pyramid_image(pbd_handle* h, const void* im, int depth, int w, int hgt, int cn, int stride) {
  if (!h || !im) return PBD_ERR_ARG;
  int rc = pbd_i_front_end(h, host_frame(im, w, hgt, cn, stride, depth));
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PBD_OK;
}
int pbd_pyramid_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride) {
  return pbd_pyramid_image(h, im, PBD_DEPTH_8U, w, hgt, cn, stride);
}

#define CHECK_LEVEL(h, level)                                                     \
  if (!(h)) return PBD_ERR_ARG;                                                   \
  if ((h)->fw == 0) return fail(h, PBD_ERR_STATE, "no frame geometry");           \
  if ((h)->batch > 1) return fail(h, PBD_ERR_STATE, "the current plan is a batch of frames (pbd_detect_batch_*): the stage entry points address single-frame plans"); \
  if ((level) < 0 || (level) >= (h)->nlevels) return fail(h, PBD_ERR_ARG, "level out of range");

int pbd_get_level_image(pbd_handle* h, int level, uint8_t* out) {
  CHECK_LEVEL(h, level);
  if (!h->have_pyr) return fail(h, PBD_ERR_STATE, "pyramid not computed");
  const Level& L = h->lv[level];
  ON_DEVICE(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->ldepth != PBD_DEPTH_8U) return fail(h, PBD_ERR_STATE, "the plan's level images are not 8-bit: pbd_get_level_image_raw");
  HIPCHK(h, hipMemcpy(out, h->d_pyr + L.img_off, (size_t)L.iw * L.ih * h->fcn, hipMemcpyDeviceToHost));
  return PBD_OK;
}
int pbd_get_level_image_raw(pbd_handle* h, int level, void* out, size_t out_bytes) {
  CHECK_LEVEL(h, level);
  if (!out) return PBD_ERR_ARG;
  if (!h->have_pyr) return fail(h, PBD_ERR_STATE, "pyramid not computed");
  const Level& L = h->lv[level];
  const size_t bytes = (size_t)L.iw * L.ih * h->fcn * h->lesz;
  if (out_bytes < bytes) return fail(h, PBD_ERR_CAPACITY, "pbd_get_level_image_raw: iw * ih * cn * element size bytes");
  ON_DEVICE(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, h->d_pyr + L.img_off, bytes, hipMemcpyDeviceToHost));
  return PBD_OK;
}
// The float / _f64 entry points share one body; a handle only answers the pair that matches the
// instantiation it was created for (cv::Mat depth CV_32F vs CV_64F in the reference).
#define CHECK_SCALAR(h, want) \
  do { if ((h)->ts != (want)) return fail((h), PBD_ERR_STATE, (want) == 4 ? "handle is PartsBasedDetector<double>: use the _f64 entry point" \
                                                                         : "handle is PartsBasedDetector<float>: use the float entry point"); } while (0)
static int get_level_features_(pbd_handle* h, int level, void* out, int ts) {
  CHECK_LEVEL(h, level);
  CHECK_SCALAR(h, ts);
  if (!h->have_feat) return fail(h, PBD_ERR_STATE, "features not computed");
  const Level& L = h->lv[level];
  if (!L.active) return fail(h, PBD_ERR_STATE, "level is not processed by this handle (pbd_set_levels / level_begin..level_end)");
  ON_DEVICE(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, h->d_feat + L.cell_off * PBD_FLEN * ts, (size_t)L.cw * L.ch * PBD_FLEN * ts, hipMemcpyDeviceToHost));
  return PBD_OK;
}
static int set_level_features_(pbd_handle* h, int level, const void* in, int ts) {
  CHECK_LEVEL(h, level);
  CHECK_SCALAR(h, ts);
  const Level& L = h->lv[level];
  if (!in) return fail(h, PBD_ERR_ARG, "null feature matrix");
  // The split-product banks carry a feature as bfloat16 / binary16 parts: a value outside the parts' finite range would become inf / NaN parts
  // and poison every response the MFMA sums it into, where the EXACT / MFMA banks propagate it as ordinary fp32.  HOG features
  // are in [0, 0.4]; a caller's own features are held to the bank's domain here, on the host copy that is being uploaded anyway.
  if (ts == 4 && (h->conv_mode == PBD_CONV_SPLIT || h->conv_mode == PBD_CONV_SPLIT_F16)) {
    const float lim = h->conv_mode == PBD_CONV_SPLIT_F16 ? SPLIT16_FMAX : 3.0e38f;   // (binary16: f 2^12 rounds to inf from 65520 on)
    const float* f = (const float*)in;
    const size_t nf = (size_t)L.cw * L.ch * PBD_FLEN;
    for (size_t i = 0; i < nf; ++i)
      if (!(std::fabs(f[i]) < lim))
        return fail(h, PBD_ERR_ARG, h->conv_mode == PBD_CONV_SPLIT_F16 ? "PBD_CONV_SPLIT_F16: a feature outside the bank's domain (|f| < 15.99609375 = 65520 / 4096, finite)"
                                                                        : "PBD_CONV_SPLIT: a feature outside bfloat16's finite range (|f| < 3e38, finite): use PBD_CONV_MFMA / PBD_CONV_EXACT");
  }
  // every bank: finite features only — a NaN / inf feature becomes non-finite responses, which the distance transform does not take (DESIGN.md
  // "Input domain of the distance transform"); the scan reads the host copy that is uploaded below
  {
    const size_t nf = (size_t)L.cw * L.ch * PBD_FLEN;
    if ((ts == 4 ? pbd_first_nonfinite((const float*)in, nf) : pbd_first_nonfinite((const double*)in, nf)) != nf)
      return fail(h, PBD_ERR_ARG, "non-finite feature: responses must stay finite for the distance transform");
  }
  ON_DEVICE(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(h->d_feat + L.cell_off * PBD_FLEN * ts, in, (size_t)L.cw * L.ch * PBD_FLEN * ts, hipMemcpyHostToDevice));
  // (split_written = false: the split-product bank's copy of the features is re-derived in front of the next pdf())
  if (h->compact) {   // not mark_features: ONE plane handed in — the write went over the Ik planes / the x pass's scratch; the other levels may still be stale
    h->feat_split_ok = false;
    h->have_dp = h->min_ran = h->ik_lazy = false;
    if (h->feat_ok.size() != (size_t)h->nvl) compact_mark_feat(h, false);
    h->feat_ok[level] = 1;
    h->have_feat = all_active_set(h, h->feat_ok, 1);
  } else {
    mark_features(h, false);
  }
  return PBD_OK;
}
// Read-only view of ONE frame of the current plan, batch plans included (frame f's level l is virtual level f * nlevels + l):
// what k_pyramid / k_hog wrote for that frame.  The single-frame getters above keep refusing batch plans.
#define CHECK_FRAME_LEVEL(h, frame, level)                                        \
  if (!(h)) return PBD_ERR_ARG;                                                   \
  if ((h)->fw == 0) return fail(h, PBD_ERR_STATE, "no frame geometry");           \
  if ((frame) < 0 || (frame) >= (h)->batch) return fail(h, PBD_ERR_ARG, "frame out of range");   \
  if ((level) < 0 || (level) >= (h)->nlevels) return fail(h, PBD_ERR_ARG, "level out of range");
int pbd_get_frame_level_image_raw(pbd_handle* h, int frame, int level, void* out, size_t out_bytes) {
  CHECK_FRAME_LEVEL(h, frame, level);
  if (!out) return PBD_ERR_ARG;
  if (!h->have_pyr) return fail(h, PBD_ERR_STATE, "pyramid not computed");
  const Level& L = h->lv[(size_t)frame * h->nlevels + level];
  const size_t bytes = (size_t)L.iw * L.ih * h->fcn * h->lesz;
  if (out_bytes < bytes) return fail(h, PBD_ERR_CAPACITY, "pbd_get_frame_level_image_raw: iw * ih * cn * element size bytes");
  ON_DEVICE(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, h->d_pyr + L.img_off, bytes, hipMemcpyDeviceToHost));
  return PBD_OK;
}
static int get_frame_level_features_(pbd_handle* h, int frame, int level, void* out, int ts) {
  CHECK_FRAME_LEVEL(h, frame, level);
  CHECK_SCALAR(h, ts);
  if (!out) return PBD_ERR_ARG;
  if (!h->have_feat) return fail(h, PBD_ERR_STATE, "features not computed");
  const Level& L = h->lv[(size_t)frame * h->nlevels + level];
  if (!L.active) return fail(h, PBD_ERR_STATE, "level is not processed by this handle (pbd_set_levels / level_begin..level_end)");
  ON_DEVICE(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, h->d_feat + L.cell_off * PBD_FLEN * ts, (size_t)L.cw * L.ch * PBD_FLEN * ts, hipMemcpyDeviceToHost));
  return PBD_OK;
}
int pbd_get_frame_level_features(pbd_handle* h, int frame, int level, float* out) { return get_frame_level_features_(h, frame, level, out, 4); }
int pbd_get_frame_level_features_f64(pbd_handle* h, int frame, int level, double* out) { return get_frame_level_features_(h, frame, level, out, 8); }
int pbd_get_level_features(pbd_handle* h, int level, float* out) { return get_level_features_(h, level, out, 4); }
int pbd_get_level_features_f64(pbd_handle* h, int level, double* out) { return get_level_features_(h, level, out, 8); }
int pbd_set_level_features(pbd_handle* h, int level, const float* in) { return set_level_features_(h, level, in, 4); }
int pbd_set_level_features_f64(pbd_handle* h, int level, const double* in) { return set_level_features_(h, level, in, 8); }
int pbd_pdf(pbd_handle* h) {
  if (!h) return PBD_ERR_ARG;
  if (!h->have_feat) return fail(h, PBD_ERR_STATE, h->compact ? "pdf(): features are not resident (compact memory plan: min() reuses their memory — run pyramid() or hand in every level again)" : "pdf() before pyramid()");
  ON_DEVICE(h);
  int rc = run_pdf(h);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PBD_OK;
}
static int get_level_response_(pbd_handle* h, int level, int filter, void* out, int ts) {
  CHECK_LEVEL(h, level);
  CHECK_SCALAR(h, ts);
  if (!h->have_resp) return fail(h, PBD_ERR_STATE, "responses not computed");
  if (filter < 0 || filter >= h->md.nfilters) return fail(h, PBD_ERR_ARG, "filter out of range");
  if (!h->fperm.empty()) filter = h->fperm[filter];   // mixed bank: the caller's filter -> its plane in the size-sorted order
  const Level& L = h->lv[level];
  if (!L.active) return fail(h, PBD_ERR_STATE, "level is not processed by this handle (pbd_set_levels / level_begin..level_end)");
  const size_t HW = (size_t)L.cw * L.ch;
  ON_DEVICE(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, h->d_resp + (L.cell_off * h->md.nfilters + filter * HW) * ts, HW * ts, hipMemcpyDeviceToHost));
  return PBD_OK;
}
static int set_level_response_(pbd_handle* h, int level, int filter, const void* in, int ts) {
  CHECK_LEVEL(h, level);
  CHECK_SCALAR(h, ts);
  if (filter < 0 || filter >= h->md.nfilters) return fail(h, PBD_ERR_ARG, "filter out of range");
  if (!h->fperm.empty()) filter = h->fperm[filter];
  const Level& L = h->lv[level];
  const size_t HW = (size_t)L.cw * L.ch;
  if (!in) return fail(h, PBD_ERR_ARG, "null response map");
  // the distance transform's domain is finite scores (DESIGN.md "Input domain of the distance transform"): scanned on the host copy that is uploaded below
  if ((ts == 4 ? pbd_first_nonfinite((const float*)in, HW) : pbd_first_nonfinite((const double*)in, HW)) != HW)
    return fail(h, PBD_ERR_ARG, "non-finite response: the distance transform takes finite scores only");
  ON_DEVICE(h);
  if (h->compact) { int rc = ensure_ik(h); if (rc) return rc; }   // the plane holds a mixture's transformed scores, which this min()'s Ik is picked from: planes first
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(h->d_resp + (L.cell_off * h->md.nfilters + filter * HW) * ts, in, HW * ts, hipMemcpyHostToDevice));
  if (h->compact) {   // not mark_responses: ONE plane handed in — min() transformed the planes in place: the responses are valid again once EVERY plane has been handed in (or pdf() re-run)
    if (h->resp_ok.size() != (size_t)h->nvl * h->md.nfilters) compact_mark_resp(h, false);
    h->resp_ok[(size_t)level * h->md.nfilters + filter] = 1;
    h->have_resp = all_active_set(h, h->resp_ok, h->md.nfilters);
    h->lat_masked = false;
  } else {
    mark_responses(h);
  }
  return PBD_OK;
}
int pbd_get_level_response(pbd_handle* h, int level, int filter, float* out) { return get_level_response_(h, level, filter, out, 4); }
int pbd_get_level_response_f64(pbd_handle* h, int level, int filter, double* out) { return get_level_response_(h, level, filter, out, 8); }
int pbd_set_level_response(pbd_handle* h, int level, int filter, const float* in) { return set_level_response_(h, level, filter, in, 4); }
int pbd_set_level_response_f64(pbd_handle* h, int level, int filter, const double* in) { return set_level_response_(h, level, filter, in, 8); }
int pbd_dp_min(pbd_handle* h) {
  if (!h) return PBD_ERR_ARG;
  if (!h->have_resp) return fail(h, PBD_ERR_STATE, h->compact ? "min(): responses are not resident (compact memory plan: min() transforms them in place — run pdf() or hand in every plane again)" : "min() before pdf()");
  ON_DEVICE(h);
  int rc = run_dp_min(h);
  if (!rc) rc = ensure_ik(h);   // the stage entry leaves the tables there, Ik planes included (a frame entry does not: its back-tracking picks)
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PBD_OK;
}
// level: a level of the plan (a batch plan's frame f, level l: f * nlevels + l), checked by the callers
static int get_dp_pointers_(pbd_handle* h, int level, int component, int part, int parent_mix, int32_t* ix, int32_t* iy, int32_t* ik) {
  if (!h->have_dp) return fail(h, PBD_ERR_STATE, "min() not run");
  if (component < 0 || component >= h->md.ncomponents) return fail(h, PBD_ERR_ARG, "component out of range");
  const int p0 = h->part_offset[component], cnp = h->part_offset[component + 1] - p0;
  if (part < 1 || part >= cnp) return fail(h, PBD_ERR_ARG, "part out of range (1..nparts-1)");
  const PartInfo& P = h->parts[p0 + part];
  const int L_ = h->parts[p0 + P.parent].K;
  if (parent_mix < 0 || parent_mix >= L_) return fail(h, PBD_ERR_ARG, "parent mixture out of range");
  const Level& L = h->lv[level];
  const size_t HW = (size_t)L.cw * L.ch;
  const size_t po = L.cell_off * h->nplanes + (size_t)(P.plane0 + parent_mix) * HW;
  if (!L.active) return fail(h, PBD_ERR_STATE, "level is not processed by this handle");
  // Ik is stored; Ix / Iy (reducePickIndex of the composed DT pointers, src/DynamicProgram.cpp:144-149) are
  // composed here from the DT pointer planes of the winning mixture, exactly as k_backtrack does per candidate
  std::vector<uint8_t> c(HW);
  const size_t pb = (size_t)h->dt_ptr_bytes;   // the planes' width on the device (bytes while every line of the plan has byte links); widened here
  std::vector<uint8_t> X((size_t)P.K * HW * pb), Y((size_t)P.K * HW * pb);
  auto at = [pb](const std::vector<uint8_t>& v, size_t i) { return pb == 1 ? (int)v[i] : (int)((const int16_t*)v.data())[i]; };
  const size_t so = (size_t)h->scr_base[(size_t)level * h->parts.size() + (p0 + part)];
  ON_DEVICE(h);
  { int rc = ensure_ik(h); if (rc) return rc; }   // a frame entry's min() has not written the Ik planes
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(c.data(), h->d_pk + po, HW, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(X.data(), (const char*)h->d_dt_ixT + so * pb, X.size(), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(Y.data(), (const char*)h->d_dt_iy + so * pb, Y.size(), hipMemcpyDeviceToHost));
  const int W = L.cw, H = L.ch;   // X: the x pass's planes, stored transposed ([column][row], pitch H); Y: [row][column]
  for (size_t i = 0; i < HW; ++i) {
    const size_t mo = (size_t)c[i] * HW;
    const int m_ = (int)(i / W), n_ = (int)(i - (size_t)m_ * W);
    int x, y;
    if (!h->opt.dt_correct_ptr) { x = at(X, mo + (size_t)n_ * H + m_); y = at(Y, mo + (size_t)m_ * W + x); }
    else { y = at(Y, mo + i); x = at(X, mo + (size_t)n_ * H + y); }
    if (ix) ix[i] = x;
    if (iy) iy[i] = y;
    if (ik) ik[i] = c[i];
  }
  return PBD_OK;
}
int pbd_get_dp_pointers(pbd_handle* h, int level, int component, int part, int parent_mix, int32_t* ix, int32_t* iy, int32_t* ik) {
  CHECK_LEVEL(h, level);
  return get_dp_pointers_(h, level, component, part, parent_mix, ix, iy, ik);
}
// Read-only, batch plans included (like pbd_get_frame_level_features): the tables the batched launches wrote for frame `frame`
int pbd_get_frame_dp_pointers(pbd_handle* h, int frame, int level, int component, int part, int parent_mix, int32_t* ix, int32_t* iy, int32_t* ik) {
  CHECK_FRAME_LEVEL(h, frame, level);
  return get_dp_pointers_(h, frame * h->nlevels + level, component, part, parent_mix, ix, iy, ik);
}
static int get_root_(pbd_handle* h, int level, int component, void* rootv, int32_t* rooti, int ts) {
  CHECK_LEVEL(h, level);
  CHECK_SCALAR(h, ts);
  if (!h->have_dp) return fail(h, PBD_ERR_STATE, "min() not run");
  if (component < 0 || component >= h->md.ncomponents) return fail(h, PBD_ERR_ARG, "component out of range");
  const Level& L = h->lv[level];
  if (!L.active) return fail(h, PBD_ERR_STATE, "level is not processed by this handle (pbd_set_levels / level_begin..level_end)");
  const size_t HW = (size_t)L.cw * L.ch;
  ON_DEVICE(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (rootv) HIPCHK(h, hipMemcpy(rootv, h->d_rootv + (L.cell_off * h->md.ncomponents + component * HW) * ts, HW * ts, hipMemcpyDeviceToHost));
  if (rooti) HIPCHK(h, hipMemcpy(rooti, h->d_rooti + L.cell_off * h->md.ncomponents + component * HW, HW * 4, hipMemcpyDeviceToHost));
  return PBD_OK;
}
int pbd_get_root(pbd_handle* h, int level, int component, float* rootv, int32_t* rooti) { return get_root_(h, level, component, rootv, rooti, 4); }
int pbd_get_root_f64(pbd_handle* h, int level, int component, double* rootv, int32_t* rooti) { return get_root_(h, level, component, rootv, rooti, 8); }
// DynamicProgram<T>::argmin takes rootv / rooti / Ix / Iy / Ik as ARGUMENTS (include/DynamicProgram.hpp:75): a caller
// that hands it tables other than the ones this handle's min() left on the device injects them here.
static int set_root_(pbd_handle* h, int level, int component, const void* rootv, const int32_t* rooti, int ts) {
  CHECK_LEVEL(h, level);
  CHECK_SCALAR(h, ts);
  if (component < 0 || component >= h->md.ncomponents) return fail(h, PBD_ERR_ARG, "component out of range");
  const Level& L = h->lv[level];
  if (!L.active) return fail(h, PBD_ERR_STATE, "level is not processed by this handle (pbd_set_levels / level_begin..level_end)");
  const size_t HW = (size_t)L.cw * L.ch;
  if (rooti) {   // rooti becomes the root's mixture in back-tracking and indexes the children's Ik planes
    const int K0 = h->parts[h->part_offset[component]].K;
    for (size_t i = 0; i < HW; ++i)
      if (rooti[i] < 0 || rooti[i] >= K0) return fail(h, PBD_ERR_ARG, "rooti entry out of range (0..K_root-1)");
  }
  ON_DEVICE(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (rootv) HIPCHK(h, hipMemcpy(h->d_rootv + (L.cell_off * h->md.ncomponents + component * HW) * ts, rootv, HW * ts, hipMemcpyHostToDevice));
  if (rooti) HIPCHK(h, hipMemcpy(h->d_rooti + L.cell_off * h->md.ncomponents + component * HW, rooti, HW * 4, hipMemcpyHostToDevice));
  h->root_dirty = true;
  if (rootv && rooti) {
    if (h->root_set.size() != (size_t)h->nvl * h->md.ncomponents) h->root_set.assign((size_t)h->nvl * h->md.ncomponents, 0);
    h->root_set[(size_t)level * h->md.ncomponents + component] = 1;
  }
  return PBD_OK;
}
int pbd_set_root(pbd_handle* h, int level, int component, const float* rootv, const int32_t* rooti) { return set_root_(h, level, component, rootv, rooti, 4); }
int pbd_set_root_f64(pbd_handle* h, int level, int component, const double* rootv, const int32_t* rooti) { return set_root_(h, level, component, rootv, rooti, 8); }
int pbd_set_dp_pointers(pbd_handle* h, int level, int component, int part, int parent_mix, const int32_t* ix, const int32_t* iy, const int32_t* ik) {
  CHECK_LEVEL(h, level);
  if (!ix || !iy || !ik) return fail(h, PBD_ERR_ARG, "null table");
  if (component < 0 || component >= h->md.ncomponents) return fail(h, PBD_ERR_ARG, "component out of range");
  const int p0 = h->part_offset[component], cnp = h->part_offset[component + 1] - p0;
  if (part < 1 || part >= cnp) return fail(h, PBD_ERR_ARG, "part out of range (1..nparts-1)");
  const PartInfo& P = h->parts[p0 + part];
  if (parent_mix < 0 || parent_mix >= h->parts[p0 + P.parent].K) return fail(h, PBD_ERR_ARG, "parent mixture out of range");
  const Level& L = h->lv[level];
  if (!L.active) return fail(h, PBD_ERR_STATE, "level is not processed by this handle");
  const size_t HW = (size_t)L.cw * L.ch;
  ON_DEVICE(h);
  { int rc = ensure_ik(h); if (rc) return rc; }   // the planes NOT handed in keep this handle's Ik: back-tracking reads all of them from d_pk from here on
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (!h->d_extx) {   // first use on this frame plan: composed planes for every (level, plane), 2 x int16
    const size_t n = h->cells * (size_t)std::max(h->nplanes, 1);
    int rc;
    if ((rc = dev_alloc(h, &h->d_extx, n))) return rc;
    if ((rc = dev_alloc(h, &h->d_exty, n))) return rc;
    HIPCHK(h, hipMemset(h->d_extx, 0, n * sizeof(int16_t)));   // planes never handed in read as (0, 0): in range for every level
    HIPCHK(h, hipMemset(h->d_exty, 0, n * sizeof(int16_t)));
    std::vector<unsigned long long> base((size_t)h->nvl * h->md.ncomponents);
    for (int l = 0; l < h->nvl; ++l)
      for (int c = 0; c < h->md.ncomponents; ++c)
        base[(size_t)l * h->md.ncomponents + c] = h->lv[l].cell_off * h->nplanes + (size_t)h->comp_plane0[c] * h->lv[l].cw * h->lv[l].ch;
    if ((rc = dev_upload(h, &h->d_ext_base, base))) return rc;
  }
  if (!h->ext_ptr && h->have_dp && h->min_ran) {
    // the planes the caller does NOT hand in keep this handle's own tables: materialise all of them once, composed
    // (costly, but this is the compatibility path of a mixed-engine caller, not detect())
    std::vector<int32_t> x, y, k;
    std::vector<int16_t> xs, ys;
    for (int l = 0; l < h->nlevels; ++l) {
      const Level& LL = h->lv[l];
      const size_t hw = (size_t)LL.cw * LL.ch;
      if (!LL.active || hw == 0) continue;
      x.resize(hw); y.resize(hw); k.resize(hw); xs.resize(hw); ys.resize(hw);
      for (int c = 0; c < h->md.ncomponents; ++c) {
        const int q0 = h->part_offset[c], qn = h->part_offset[c + 1] - q0;
        for (int pp = 1; pp < qn; ++pp)
          for (int m2 = 0; m2 < h->parts[q0 + h->parts[q0 + pp].parent].K; ++m2) {
            int rc = pbd_get_dp_pointers(h, l, c, pp, m2, x.data(), y.data(), k.data());
            if (rc) return rc;
            for (size_t i = 0; i < hw; ++i) { xs[i] = (int16_t)x[i]; ys[i] = (int16_t)y[i]; }
            const size_t eo = LL.cell_off * h->nplanes + (size_t)(h->parts[q0 + pp].plane0 + m2) * hw;
            HIPCHK(h, hipMemcpy(h->d_extx + eo, xs.data(), hw * 2, hipMemcpyHostToDevice));
            HIPCHK(h, hipMemcpy(h->d_exty + eo, ys.data(), hw * 2, hipMemcpyHostToDevice));
          }
      }
    }
  }
  std::vector<int16_t> xs(HW), ys(HW);
  std::vector<uint8_t> ks(HW);
  for (size_t i = 0; i < HW; ++i) {
    if (ix[i] < 0 || ix[i] >= L.cw || iy[i] < 0 || iy[i] >= L.ch || ik[i] < 0 || ik[i] >= P.K)
      return fail(h, PBD_ERR_ARG, "pointer table entry out of range");
    xs[i] = (int16_t)ix[i]; ys[i] = (int16_t)iy[i]; ks[i] = (uint8_t)ik[i];
  }
  const size_t eo = L.cell_off * h->nplanes + (size_t)(P.plane0 + parent_mix) * HW;
  HIPCHK(h, hipMemcpy(h->d_extx + eo, xs.data(), HW * 2, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_exty + eo, ys.data(), HW * 2, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_pk + eo, ks.data(), HW, hipMemcpyHostToDevice));
  // not mark_min: tables handed in, with or without a min() of this handle behind them (min_ran, root_dirty, min_timed keep their values)
  h->ext_ptr = true;
  if (h->compact) {   // d_pk is the memory of the level images + features (and the first call's d_extx / d_exty allocation moved nothing, but the
                      // Ik write above went over them): pyramid() -> set_dp_pointers -> pdf() must not run on clobbered features
    h->have_pyr = h->have_feat = false;
    compact_mark_feat(h, false);
  }
  if (h->ext_set.size() != (size_t)h->nvl * std::max(h->nplanes, 1)) h->ext_set.assign((size_t)h->nvl * std::max(h->nplanes, 1), 0);
  h->ext_set[(size_t)level * std::max(h->nplanes, 1) + P.plane0 + parent_mix] = 1;
  // with a min() of this handle behind them the planes not handed in keep its tables; without one, back-tracking may only
  // run once EVERY plane and every root table of the active levels has been provided (pbd_dp_argmin checks)
  h->have_dp = true;
  return PBD_OK;
}
int pbd_get_footprint(const pbd_handle* h, size_t* frame_bytes, size_t* model_bytes) {
  if (!h) return PBD_ERR_ARG;
  if (frame_bytes) *frame_bytes = h->frame_allocs.bytes();
  if (model_bytes) *model_bytes = h->model_allocs.bytes();
  return PBD_OK;
}
int pbd_debug_live_allocs(long long* buffers, long long* bytes) {
  if (buffers) *buffers = pbd_live_buffers.load();
  if (bytes) *bytes = pbd_live_bytes.load();
  return PBD_OK;
}
int pbd_abi_version(void) { return PBD_ABI_VERSION; }
int pbd_get_conv_mode(const pbd_handle* h) { return h ? h->conv_mode : -PBD_ERR_ARG; }   // what PBD_CONV_AUTO resolved to (negative: error)
int pbd_get_stage_state(const pbd_handle* h, int32_t state[4]) {
  if (!h || !state) return PBD_ERR_ARG;
  state[0] = h->have_pyr; state[1] = h->have_feat; state[2] = h->have_resp; state[3] = h->have_dp;
  return PBD_OK;
}

// what back-tracking needs of the frame's tables (pbd_dp_argmin, pbd_dp_argbest)
static int argmin_ready(pbd_handle* h) {
  if (!h->have_dp) return fail(h, PBD_ERR_STATE, "argmin() before min()");
  if (h->batch > 1) return fail(h, PBD_ERR_STATE, "the current plan is a batch of frames: its candidates come from pbd_detect_batch_collect");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "previous frame not collected");
  if (!h->min_ran) {   // tables handed in by the caller only: all of them, or back-tracking would walk uninitialised planes
    if (!all_active_set(h, h->ext_set, std::max(h->nplanes, 1)) && h->nplanes > 0)
      return fail(h, PBD_ERR_STATE, "argmin(): no min() on this frame and not every pointer table has been handed in (pbd_set_dp_pointers)");
    if (!all_active_set(h, h->root_set, h->md.ncomponents))
      return fail(h, PBD_ERR_STATE, "argmin(): no min() on this frame and not every root table has been handed in (pbd_set_root)");
  }
  return PBD_OK;
}

int pbd_dp_argmin(pbd_handle* h, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int capacity, int* count) {
  if (!h) return PBD_ERR_ARG;
  int ready = argmin_ready(h);
  if (ready) return ready;
  ON_DEVICE(h);
  int rc = enqueue_stage_argmin(h);
  return rc ? rc : collect_frame(h, heads, boxes, locs, capacity, count);
}

// ---- latent detection: the two stage entry points ----------------------------------------------------------------------------
int pbd_latent_mask(pbd_handle* h, const int32_t* truth, const int32_t* mix, int component, double overlap, int32_t* admissible) {
  if (!h) return PBD_ERR_ARG;
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  int rc = pbd_i_latent_check(h, truth, mix, 1, component, overlap);
  if (rc) return rc;
  if (h->fw == 0) return fail(h, PBD_ERR_STATE, "no frame geometry");
  if (h->batch > 1) return fail(h, PBD_ERR_STATE, "the current plan is a batch of frames (pbd_detect_batch_*): the stage entry points address single-frame plans");
  if (!h->have_resp) return fail(h, PBD_ERR_STATE, h->compact ? "latent mask: responses are not resident (compact memory plan: min() transforms them in place — run pdf() or hand in every plane again)" : "latent mask before pdf()");
  ON_DEVICE(h);
  const LatentSource s{truth, mix, component, overlap};
  if ((rc = pbd_i_latent_begin(h, s, 1)) || (rc = run_latent_mask(h, 1))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (admissible) {   // a pair counts when every part of the component has an admissible cell at the level
    const int nc = h->md.ncomponents, mp = h->max_parts;
    std::vector<int> fl((size_t)h->nvl * nc * mp);
    HIPCHK(h, hipMemcpy(fl.data(), h->d_lat_flags, fl.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int l = 0; l < h->nlevels; ++l)
      for (int c = 0; c < nc; ++c) {
        int ok = 1;
        for (int p = 0; p < h->part_offset[c + 1] - h->part_offset[c]; ++p) ok = ok && fl[((size_t)l * nc + c) * mp + p] != 0;
        admissible[(size_t)l * nc + c] = ok;
      }
  }
  return PBD_OK;
}
int pbd_dp_argbest(pbd_handle* h, pbd_candidate_head* head, int32_t* boxes, int32_t* locs, int* found) {
  if (!h) return PBD_ERR_ARG;
  int rc = argmin_ready(h);
  if (rc) return rc;
  if (h->in_group) return fail(h, PBD_ERR_UNSUPPORTED, "latent detection: not for a pbd_group member");
  if (h->nms_sz > 0) return fail(h, PBD_ERR_UNSUPPORTED, "latent detection: not with the score-map NMS (pbd_options.reserved[0] > 0)");
  ON_DEVICE(h);
  if ((rc = latent_tables(h))) return rc;
  if (!h->lat_masked)   // no mask on this frame's responses: every pair counts (the unconstrained best pose)
    HIPCHK(h, hipMemsetAsync(h->d_lat_flags, 1, (size_t)h->nvl * h->md.ncomponents * h->max_parts * sizeof(int), h->stream));
  if ((rc = run_latent_best(h))) return rc;
  h->root_dirty = false;                      // the record is the best root of the tables now on the device, whoever wrote them
  rc = enqueue_stage_argmin(h);
  h->root_dirty = true;                       // ... and a later pbd_dp_argmin thresholds them again
  return rc ? rc : collect_frame(h, head, boxes, locs, 1, found);
}

// ---- stand-alone primitives -------------------------------------------------
static int dt2d_(pbd_handle* h, const void* in, int rows, int cols, double ax, double bx, double ay, double by, int osx,
                 int osy, void* out, int32_t* ix, int32_t* iy, int tsz) {
  if (!h || !in || rows <= 0 || cols <= 0 || rows > 32767 || cols > 32767) return PBD_ERR_ARG;
  CHECK_SCALAR(h, tsz);
  if (ax == 0 || ay == 0) return fail(h, PBD_ERR_ARG, "a must be non-zero");
  if (!std::isfinite(ax) || !std::isfinite(bx) || !std::isfinite(ay) || !std::isfinite(by)) return fail(h, PBD_ERR_ARG, "a and b must be finite");
  const size_t HW = (size_t)rows * cols;
  // finite scores only (DESIGN.md "Input domain of the distance transform"): nothing non-finite is ever handed to k_dt_pass; the scan reads the
  // array that is copied below
  if ((tsz == 4 ? pbd_first_nonfinite((const float*)in, HW) : pbd_first_nonfinite((const double*)in, HW)) != HW)
    return fail(h, PBD_ERR_ARG, "non-finite score: the distance transform takes finite maps only");
  ON_DEVICE(h);
  const size_t ts = (size_t)tsz;
  char *d_in, *d_tmp, *d_sdt;
  char *d_ixT, *d_iy;
  const size_t pb = (size_t)dt_ptr_bytes_for(std::max(rows, cols));   // the pointer planes' width, as a frame plan chooses it: bytes while both passes' lines have byte links
  CallScratch s(h);   // (a refusal below gives the buffers back like every other way out)
  static const char* const what = "pbd_dt2d: ";
  int rc;
  if ((rc = s.get(&d_in, HW * ts, what)) || (rc = s.get(&d_tmp, HW * ts, what)) || (rc = s.get(&d_sdt, HW * ts, what)) ||
      (rc = s.get(&d_ixT, HW * pb, what)) || (rc = s.get(&d_iy, HW * pb, what)))
    return rc;
  HIPCHK(h, hipMemcpyAsync(d_in, in, HW * ts, hipMemcpyHostToDevice, h->stream));
  DtMap maps[2] = {dt_map(d_in, d_tmp, d_ixT, 0.f, 0.f, osx, 1), dt_map(d_tmp, d_sdt, d_iy, 0.f, 0.f, osy, 0)};
  maps[0].a = ax; maps[0].b = bx; maps[0].r2a = 1.0 / (2.0 * ax);   // the caller's quadratics (not the model's -w)
  maps[1].a = ay; maps[1].b = by; maps[1].r2a = 1.0 / (2.0 * ay);
  // block size of THIS call's two launches: a local — the handle's dt_nt belongs to the frame plan, whose uploaded tasks carry
  // the geometry derived from it (nsub, P, chunk); overwriting it here made a detect() after a pbd_dt2d launch 128-lane blocks
  // over 256-lane tasks
  const int nt = h->knobs.dt_nt ? h->knobs.dt_nt : tsz == 8 ? 64 : PBD_DT_NT_DEFAULT;
  const size_t dt_base = h->knobs.dt_budget_kb >= 0 ? (size_t)h->knobs.dt_budget_kb * 1024 : 40 * 1024;
  const size_t budget = std::max<size_t>(dt_base, dt_lds_bytes(dt_stride_for(std::max(rows, cols)), 4, tsz, nt));
  if (budget > 160 * 1024) return fail(h, PBD_ERR_UNSUPPORTED, "map too large for the LDS-resident distance transform");
  DtGroup groups[2] = {dt_group(0, 1, rows, cols, budget, tsz, nt, h->knobs.dt_seg, true), dt_group(1, 1, cols, rows, budget, tsz, nt, h->knobs.dt_seg, false)};
  std::vector<DtTask> tasks;
  dt_add_tasks(groups[0], tasks);
  const int nx = (int)tasks.size();
  dt_add_tasks(groups[1], tasks);
  dt_mark_fused(tasks, maps, tsz);   // (the caller's quadratics: fused arithmetic only if they are converted floats)
  if (pb == 1) dt_mark_ptr8(tasks);
  DtMap* d_maps; DtTask* d_tasks;
  if ((rc = s.get(&d_maps, 2, what)) || (rc = s.get(&d_tasks, tasks.size(), what))) return rc;
  HIPCHK(h, hipMemcpyAsync(d_maps, maps, sizeof(maps), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_tasks, tasks.data(), sizeof(DtTask) * tasks.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // host staging buffers above are pageable
  launch_dt_pass(d_tasks, nx, d_maps, nullptr, nullptr, h->d_biasw, budget, tsz, nt, 0, h->stream);
  if (PBD_PROBE_ENV("PBD_DEBUG_SKIP_Y")) { hipMemsetAsync(d_sdt, 0, HW * ts, h->stream); hipMemsetAsync(d_iy, 0, HW * pb, h->stream); }   // probe build: leave the x pass as the last DT launch (its stamps are then readable)
  else launch_dt_pass(d_tasks + nx, (int)tasks.size() - nx, d_maps, nullptr, nullptr, h->d_biasw, budget, tsz, nt, 0, h->stream);
  std::vector<uint8_t> hx(HW * pb), hy(HW * pb);
  auto at = [pb](const std::vector<uint8_t>& v, size_t i) { return pb == 1 ? (int)v[i] : (int)((const int16_t*)v.data())[i]; };
  HIPCHK(h, hipMemcpyAsync(out, d_sdt, HW * ts, hipMemcpyDeviceToHost, h->stream));   // the y pass's scores, untouched
  HIPCHK(h, hipMemcpyAsync(hx.data(), d_ixT, HW * pb, hipMemcpyDeviceToHost, h->stream));   // the passes' own pointers
  HIPCHK(h, hipMemcpyAsync(hy.data(), d_iy, HW * pb, hipMemcpyDeviceToHost, h->stream));
  // finite arguments can still leave the domain BETWEEN the passes: the x pass's a d^2 + b d + y may overflow.  The kernel ends on any bit pattern
  // (dt_core.hpp: dt_stitch1), but only finite lines are the reference's bit for bit, so the x pass's scores come back too and both are scanned
  std::vector<char> htmp(HW * ts);
  HIPCHK(h, hipMemcpyAsync(htmp.data(), d_tmp, HW * ts, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const bool left_domain = tsz == 4 ? pbd_first_nonfinite((const float*)htmp.data(), HW) != HW || pbd_first_nonfinite((const float*)out, HW) != HW
                                    : pbd_first_nonfinite((const double*)htmp.data(), HW) != HW || pbd_first_nonfinite((const double*)out, HW) != HW;
  for (size_t i = 0; i < HW; ++i) {   // pointer composition of compute() (:233-244), or the true arg-max one
    const int m_ = (int)(i / cols), n_ = (int)(i - (size_t)m_ * cols);
    int x, y;
    if (!h->opt.dt_correct_ptr) { x = at(hx, (size_t)n_ * rows + m_); y = at(hy, (size_t)m_ * cols + x); }   // hx: [column][row] (the x pass writes transposed)
    else { y = at(hy, i); x = at(hx, (size_t)n_ * rows + y); }
    if (ix) ix[i] = x;
    if (iy) iy[i] = y;
  }
  if (left_domain)
    return fail(h, PBD_ERR_ARG, "the scores left the finite range in the x or the y pass (|y| + |a| d^2 + |b| d overflows): outside the distance transform's domain");
  return PBD_OK;
}
int pbd_dt2d(pbd_handle* h, const float* in, int rows, int cols, double ax, double bx, double ay, double by, int osx,
             int osy, float* out, int32_t* ix, int32_t* iy) {
  return dt2d_(h, in, rows, cols, ax, bx, ay, by, osx, osy, out, ix, iy, 4);
}
int pbd_dt2d_f64(pbd_handle* h, const double* in, int rows, int cols, double ax, double bx, double ay, double by, int osx,
                 int osy, double* out, int32_t* ix, int32_t* iy) {
  return dt2d_(h, in, rows, cols, ax, bx, ay, by, osx, osy, out, ix, iy, 8);
}

static int hog_u8_(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, void* out, int* cell_w, int* cell_h, int ts) {
  if (!h || !im || w < 3 || hgt < 3 || (cn != 1 && cn != 3) || stride < w * cn) return PBD_ERR_ARG;
  CHECK_SCALAR(h, ts);
  ON_DEVICE(h);
  const int sbin = h->md.sbin;
  LevelDev L{};
  L.iw = w; L.ih = hgt;
  L.bw = (int)std::round((float)w / (float)sbin); L.bh = (int)std::round((float)hgt / (float)sbin);
  L.cw = std::max(L.bw - 2, 0); L.ch = std::max(L.bh - 2, 0);
  if (cell_w) *cell_w = L.cw;
  if (cell_h) *cell_h = L.ch;
  if (L.cw == 0 || L.ch == 0) return PBD_OK;
  int tc = 16;
  while (tc > 2 && hog_lds_bytes(sbin, tc, ts) > 150 * 1024) tc /= 2;
  std::vector<HogTile> tiles;
  for (int y = 0; y < L.ch; y += tc) for (int x = 0; x < L.cw; x += tc) tiles.push_back(HogTile{0, y, x, 0});
  uint8_t* d_im; char* d_feat; LevelDev* d_lv; HogTile* d_tiles;
  CallScratch s(h);
  static const char* const what = "pbd_hog_u8: ";
  int rc;
  if ((rc = s.get(&d_im, (size_t)w * hgt * cn, what)) || (rc = s.get(&d_feat, (size_t)L.cw * L.ch * PBD_FLEN * ts, what)) ||
      (rc = s.get(&d_lv, 1, what)) || (rc = s.get(&d_tiles, tiles.size(), what)))
    return rc;
  HIPCHK(h, hipMemcpy2D(d_im, (size_t)w * cn, im, stride, (size_t)w * cn, hgt, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(d_lv, &L, sizeof(L), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(d_tiles, tiles.data(), sizeof(HogTile) * tiles.size(), hipMemcpyHostToDevice));
  launch_hog(d_tiles, (int)tiles.size(), d_lv, d_im, d_feat, ts, cn, sbin, tc, h->d_hog_lut, nullptr, 0, PBD_DEPTH_8U, h->stream);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, d_feat, (size_t)L.cw * L.ch * PBD_FLEN * ts, hipMemcpyDeviceToHost));
  return PBD_OK;
}
int pbd_hog_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, float* out, int* cell_w, int* cell_h) {
  return hog_u8_(h, im, w, hgt, cn, stride, out, cell_w, cell_h, 4);
}
int pbd_hog_u8_f64(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, double* out, int* cell_w, int* cell_h) {
  return hog_u8_(h, im, w, hgt, cn, stride, out, cell_w, cell_h, 8);
}

int pbd_resize_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, uint8_t* out, int ow, int oh) {
  if (!h || !im || !out || w <= 0 || hgt <= 0 || ow <= 0 || oh <= 0 || (cn != 1 && cn != 3) || stride < w * cn) return PBD_ERR_ARG;
  ON_DEVICE(h);
  uint8_t *d_im, *d_out;
  CallScratch s(h);
  static const char* const what = "pbd_resize_u8: ";
  int rc;
  if ((rc = s.get(&d_im, (size_t)w * hgt * cn, what)) || (rc = s.get(&d_out, (size_t)ow * oh * cn, what))) return rc;
  HIPCHK(h, hipMemcpy2D(d_im, (size_t)w * cn, im, stride, (size_t)w * cn, hgt, hipMemcpyHostToDevice));
  PyrJob job{0, 0, w, hgt, ow, oh}, *d_job;
  if ((rc = s.get(&d_job, 1, what))) return rc;
  HIPCHK(h, hipMemcpy(d_job, &job, sizeof(job), hipMemcpyHostToDevice));
  launch_resize(d_job, 1, ow * oh, cn, w * cn, d_im, d_out, h->stream);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, d_out, (size_t)ow * oh * cn, hipMemcpyDeviceToHost));
  return PBD_OK;
}

int pbd_pyrdown_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, uint8_t* out) {
  if (!h || !im || !out || w <= 0 || hgt <= 0 || (cn != 1 && cn != 3) || stride < w * cn) return PBD_ERR_ARG;
  ON_DEVICE(h);
  const size_t sb = (size_t)w * hgt * cn, db = (size_t)((w + 1) / 2) * ((hgt + 1) / 2) * cn;
  uint8_t* d_buf;
  CallScratch s(h);
  static const char* const what = "pbd_pyrdown_u8: ";
  int rc;
  if ((rc = s.get(&d_buf, sb + db, what))) return rc;
  HIPCHK(h, hipMemcpy2D(d_buf, (size_t)w * cn, im, stride, (size_t)w * cn, hgt, hipMemcpyHostToDevice));
  PyrJob job{0, (unsigned long long)sb, w, hgt, (w + 1) / 2, (hgt + 1) / 2}, *d_job;
  if ((rc = s.get(&d_job, 1, what))) return rc;
  HIPCHK(h, hipMemcpy(d_job, &job, sizeof(job), hipMemcpyHostToDevice));
  launch_pyrdown(d_job, 1, job.dw, job.dh, cn, d_buf, h->stream);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, d_buf + sb, db, hipMemcpyDeviceToHost));
  return PBD_OK;
}

// resize(im, scale) of matlab/mex/resize.cc:82-106 on an interleaved double image
int pbd_resize_area_f64(pbd_handle* h, const double* im, int w, int hgt, int cn, double scale, double* out, int* ow, int* oh) {
  if (!h || !im || !out || !ow || !oh || w <= 0 || hgt <= 0 || (cn != 1 && cn != 3) || !(scale > 0)) return PBD_ERR_ARG;
  if (scale > 1) return fail(h, PBD_ERR_ARG, "Invalid scaling factor (matlab/mex/resize.cc:90)");
  const int dh = (int)std::round(hgt * scale), dw = (int)std::round(w * scale);   // resize.cc:94-95
  if (dw <= 0 || dh <= 0 || (long long)w * hgt * cn >= (1ll << 28)) return fail(h, PBD_ERR_ARG, "pbd_resize_area_f64: empty result or image too large");
  std::vector<MatRun> runs; std::vector<MatTap> taps;
  if (!resize_taps(hgt, dh, runs, taps) || !resize_taps(w, dw, runs, taps)) return fail(h, PBD_ERR_ARG, "a resize tap outside the image (matlab/mex/resize.cc:53,61)");
  ON_DEVICE(h);
  const size_t sb = (size_t)w * hgt * cn * 8, db = (size_t)dw * dh * cn * 8;
  uint8_t *d_im, *d_out; MatRun* d_runs; MatTap* d_taps;
  MatJob job{0, 0, w, hgt, dw, dh, 0, dh}, *d_job;
  CallScratch s(h);
  static const char* const what = "pbd_resize_area_f64: ";
  int rc;
  if ((rc = s.get(&d_im, sb, what)) || (rc = s.get(&d_out, db, what)) || (rc = s.get(&d_job, 1, what)) ||
      (rc = s.get(&d_runs, runs.size(), what)) || (rc = s.get(&d_taps, taps.size(), what)))
    return rc;
  HIPCHK(h, hipMemcpy(d_im, im, sb, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(d_job, &job, sizeof(job), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(d_runs, runs.data(), runs.size() * sizeof(MatRun), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(d_taps, taps.data(), taps.size() * sizeof(MatTap), hipMemcpyHostToDevice));
  launch_resize_area(d_job, 1, dw * dh, d_runs, d_taps, cn, w * cn, true, d_im, d_out, h->stream);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, d_out, db, hipMemcpyDeviceToHost));
  *ow = dw; *oh = dh;
  return PBD_OK;
}
// reduce(im) of matlab/mex/reduce.cc:50-70 on an interleaved double image
int pbd_reduce_f64(pbd_handle* h, const double* im, int w, int hgt, int cn, double* out, int* ow, int* oh) {
  if (!h || !im || !out || !ow || !oh || (cn != 1 && cn != 3)) return PBD_ERR_ARG;
  if (w < 5 || hgt < 5) return fail(h, PBD_ERR_ARG, "pbd_reduce_f64: both dimensions >= 5 (matlab/mex/reduce.cc:24-42 reads rows 0..2 and the last three of each axis)");
  if ((long long)w * hgt * cn >= (1ll << 28)) return fail(h, PBD_ERR_ARG, "pbd_reduce_f64: image too large");
  const int dh = (int)std::round(hgt * .5), dw = (int)std::round(w * .5);   // reduce.cc:58-59
  ON_DEVICE(h);
  const size_t sb = (size_t)w * hgt * cn * 8, db = (size_t)dw * dh * cn * 8;
  uint8_t* d_buf;
  MatJob job{0, (unsigned long long)sb, w, hgt, dw, dh, 0, 0}, *d_job;
  CallScratch s(h);
  static const char* const what = "pbd_reduce_f64: ";
  int rc;
  if ((rc = s.get(&d_buf, sb + db, what)) || (rc = s.get(&d_job, 1, what))) return rc;
  HIPCHK(h, hipMemcpy(d_buf, im, sb, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(d_job, &job, sizeof(job), hipMemcpyHostToDevice));
  launch_reduce_f64(d_job, 1, dw * dh, cn, d_buf, h->stream);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, d_buf + sb, db, hipMemcpyDeviceToHost));
  *ow = dw; *oh = dh;
  return PBD_OK;
}

int pbd_nms_map(pbd_handle* h, const float* src, int rows, int cols, int sz, uint8_t* dst) {
  if (!h || !src || !dst || rows <= 0 || cols <= 0 || sz < 0) return PBD_ERR_ARG;
  ON_DEVICE(h);
  float* d_src; uint8_t* d_dst;
  const size_t n = (size_t)rows * cols;
  CallScratch s(h);
  int rc;
  if ((rc = s.get(&d_src, n, "pbd_nms_map: ")) || (rc = s.get(&d_dst, n, "pbd_nms_map: "))) return rc;
  HIPCHK(h, hipMemcpy(d_src, src, n * 4, hipMemcpyHostToDevice));
  launch_nms_map(d_src, rows, cols, sz, d_dst, h->stream);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(dst, d_dst, n, hipMemcpyDeviceToHost));
  return PBD_OK;
}

// ---- instrumentation ---------------------------------------------------------
int pbd_get_stage_ms(const pbd_handle* h, float ms[6]) {
  if (!h || !ms) return PBD_ERR_ARG;
  for (int i = 0; i < 6; ++i) ms[i] = h->stage_ms[i];
  return PBD_OK;
}
int pbd_set_profiling(pbd_handle* h, int on) {
  if (!h) return PBD_ERR_ARG;
  h->profiling = on != 0;
  return PBD_OK;
}
int pbd_get_work(const pbd_handle* h, double work[6]) {
  if (!h || !work) return PBD_ERR_ARG;
  if (h->fw == 0) return PBD_ERR_STATE;
  const pbd_model_desc& m = h->md;
  double C = 0, pix = 0;
  for (int l = 0; l < h->nlevels; ++l) {
    if (!h->lv[l].active) continue;
    C += (double)h->lv[l].cw * h->lv[l].ch;
    pix += (double)h->lv[l].iw * h->lv[l].ih * h->fcn * h->lesz;   // (bytes: pixels of the level images' depth)
  }
  // reference element types (scores of type T: 4 or 8 bytes, int32 pointers)
  const double ts = h->ts;
  double per_cell = 0, dtmaps = 0;
  for (int c = 0; c < m.ncomponents; ++c) {
    const int p0 = h->part_offset[c], cnp = h->part_offset[c + 1] - p0;
    for (int p = 1; p < cnp; ++p) {
      const double K = h->parts[p0 + p].K, L = h->parts[p0 + h->parts[p0 + p].parent].K;
      per_cell += ts * K + 12 * L + 2 * ts * L;
      dtmaps += K;
    }
    per_cell += ts * h->parts[p0].K + ts + 4;
  }
  work[0] = pix + 32.0 * ts * C;
  double taps = (double)m.nfilters * m.kh * m.kw;   // sum over the filters of kh_i kw_i (mixed banks: per filter)
  if (h->mixed) { taps = 0; for (int n = 0; n < m.nfilters; ++n) taps += (double)h->fkh[n] * h->fkw[n]; }
  work[1] = 32.0 * ts * C + ts * m.nfilters * C + ts * taps * m.flen;
  work[2] = 2.0 * C * taps * m.flen;
  work[3] = C * per_cell;
  work[4] = C;
  work[5] = C * dtmaps;
  return PBD_OK;
}
#ifdef PBD_PROBES
#define PROBE_RC PBD_OK
#else
#define PROBE_RC PBD_ERR_UNSUPPORTED   /* stamps exist only in libpbd_hip_probes.so (make probes) */
#endif
#ifdef PBD_PROBES
extern "C" int pbd_debug_dt_trace(unsigned long long* t, unsigned* hw, int* nlaunch) { return dt_debug_trace(t, hw, nlaunch); }
#endif
int pbd_debug_dt_stamps(unsigned long long* out) { if (!out) return PBD_ERR_ARG; dt_debug_read(out); return PROBE_RC; }
int pbd_debug_dt_counters(unsigned long long* out) { if (!out) return PBD_ERR_ARG; dt_debug_counters(out); return PROBE_RC; }
int pbd_debug_hog_stamps(unsigned long long* out) { if (!out) return PBD_ERR_ARG; hog_debug_read(out); return PROBE_RC; }
int pbd_debug_conv_stamps(unsigned long long* out) { if (!out) return PBD_ERR_ARG; conv_debug_read(out); return PROBE_RC; }

int pbd_dp_timer(pbd_handle* h, int reset, double* avg_ms, int* nframes) {
  if (!h) return PBD_ERR_ARG;
  if (avg_ms) *avg_ms = h->dp_frames ? h->dp_ms_sum / h->dp_frames : 0.0;
  if (nframes) *nframes = h->dp_frames;
  if (reset) { h->dp_ms_sum = 0; h->dp_frames = 0; }
  return PBD_OK;
}

}  // extern "C"
#pragma GCC visibility pop
