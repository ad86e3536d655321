// pbd_detect.cpp — frames in, candidates out: the one way a frame or a batch enters (enter_frame), the one collect (collect_frames),
// the detect entry points of include/pbd_c.h as their thin callers, pbd_tune_plan.  Plan, stages and stage state: pbd_api.cpp.
#include <algorithm>
#include "pbd_internal.hpp"

// ---- frame entry -----------------------------------------------------------------------------------------
int copy_rows(pbd_handle* h, void* dst, const void* src, size_t src_pitch, size_t row_bytes, size_t rows, hipMemcpyKind kind) {
  if (src_pitch == row_bytes) HIPCHK(h, hipMemcpyAsync(dst, src, row_bytes * rows, kind, h->stream));
  else HIPCHK(h, hipMemcpy2DAsync(dst, row_bytes, src, src_pitch, row_bytes, rows, kind, h->stream));
  return PBD_OK;
}

// The refusals, in the order every entry has always made them: the depth image's arguments, a pending frame, the stride, then
// what plan_frame refuses; a null frame of a host batch is found when its turn to be uploaded comes.  (Null handles and null
// images are the entries' own first line: PBD_ERR_ARG without a message.)
int enter_frame(pbd_handle* h, const FrameSource& s, bool detect) {
  int rc;
  if (s.z && (rc = pbd_i_depth_check(h, s.z->type, s.z->stride, s.w))) return rc;
  if (detect && h->pf.active) return fail(h, PBD_ERR_STATE, "previous frame not collected");
  const int esz = depth_esz(s.depth);
  const size_t row = (size_t)s.w * s.cn * esz;
  if (s.depth == PBD_DEPTH_8U) {
    if (s.stride < s.w * s.cn) return fail(h, PBD_ERR_ARG, "stride < w*cn");
  } else {
    if (!esz) return fail(h, PBD_ERR_UNSUPPORTED, "Unsupported image type (src/HOGFeatures.cpp:136-146: CV_8U, CV_16U, CV_32F, CV_64F)");
    if (s.stride < 0 || (size_t)s.stride < row || s.stride % esz) return fail(h, PBD_ERR_ARG, "stride: bytes, >= w * cn * element size and a multiple of the element size");
  }
  ON_DEVICE(h);
  if ((rc = plan_frame(h, s.w, s.hgt, s.cn, s.nframes, s.depth))) return rc;
  if (s.eval && h->compact)   // (an evaluation frame is routed as a mining frame and refuses what that refuses)
    return fail(h, PBD_ERR_UNSUPPORTED, "evaluation: this frame runs the compact memory plan (dp_mode 2, or automatic for large frames and batches), "
                                        "which the mining route the records take refuses: add the frames one by one or in smaller batches");
  if ((s.mine || s.lat_write) && h->compact)   // (known once the geometry is planned; nothing has been uploaded or enqueued)
    return fail(h, PBD_ERR_UNSUPPORTED, std::string(s.mine ? "mining" : "latent positives") +
                                        ": this frame runs the compact memory plan (dp_mode 2, or automatic for large frames), whose min() reuses "
                                        "the memory of the feature planes the examples are read from");
  PyrCopyTable stored_jobs;
  if (s.stored) {
    if (h->compact)
      return fail(h, PBD_ERR_UNSUPPORTED, "pyramid store: this frame runs the compact memory plan (dp_mode 2, or automatic for large frames and batches), "
                                          "which stored frames do not support");
    if ((rc = pbd_i_stored_jobs(h, *s.stored, s.nframes, &stored_jobs))) return rc;
  }
  if (!s.on_device)   // on the handle's stream, in front of the kernels
    for (int f = 0; f < s.nframes; ++f) {
      const void* im = s.each ? s.each[f] : s.one;
      if (!im) return fail(h, PBD_ERR_ARG, "null frame pointer");
      if ((rc = copy_rows(h, h->d_img + row * s.hgt * f, im, (size_t)s.stride, row, (size_t)s.hgt, hipMemcpyHostToDevice))) return rc;
    }
  if (!detect) return PBD_OK;
  const uint8_t* d_src = s.on_device ? (const uint8_t*)s.one : h->d_img;
  const int stride = s.on_device ? s.stride : (int)row;
  // what the frame is, once: the truth tables / gt boxes / depth images go in front of the kernels like the image
  FrameJob job;
  if (s.stored) job.stored = &stored_jobs;
  if (s.lat) {
    job.kind = s.lat_write ? FRAME_LATENT_WRITE : FRAME_LATENT;
    if ((rc = pbd_i_latent_begin(h, *s.lat, s.nframes))) return rc;
  } else if (s.gt) {
    job.kind = FRAME_GTBOX;
    if ((rc = pbd_i_gt_begin(h, *s.gt, s.nframes))) return rc;
  } else if (s.mine) {
    job.kind = FRAME_MINE;
  } else if (s.eval) {
    job.kind = FRAME_EVAL;
  } else if (s.z) {
    const DepthSource& z = *s.z;
    job.kind = FRAME_DEPTH;
    job.z = {(const char*)z.p, (size_t)z.stride, z.fbytes, s.w, s.hgt, z.has};
    if (!z.on_device) {
      const size_t zrow = (size_t)s.w * h->ts;
      if ((rc = model_grow(h, &h->d_zimg, h->zimg_bytes, zrow * s.hgt))) return rc;
      if ((rc = copy_rows(h, h->d_zimg, z.p, (size_t)z.stride, zrow, (size_t)s.hgt, hipMemcpyHostToDevice))) return rc;
      job.z.img = h->d_zimg; job.z.pitch = zrow;
    }
  }
  return enqueue_all(h, job, d_src, stride);
}

// ---- collect ---------------------------------------------------------------------------------------------
// frame finished on the stream: timers, and the records beyond the first block (rare) fetched into h_cand_out.
// `found` = the device-side count (h_cand_count[0], or the count a group gather delivered).
int pbd_i_finish_frame(pbd_handle* h, int found) {
  h->pf.active = false;
  if (h->pf.dp_timed && h->have_dp) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->ev_dp0, h->ev_dp1) == hipSuccess) { h->dp_ms_sum += ms; h->dp_frames++; }
  }
  const int n = std::min(found, h->opt.max_candidates);
  const int first = h->pf.on_host ? n : std::min(h->first_copy, h->opt.max_candidates);   // (zero-copy: every record is on the host already)
  if (n > first) {
    HIPCHK(h, hipMemcpyAsync(h->h_cand_out + h->cand_stride * first, h->d_cand_out + h->cand_stride * first,
                             h->cand_stride * (n - first), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!h->d_gsend) {
      // this geometry / threshold yields more records than the first copy carries: size it for what was seen (+25 %), so
      // that the following frames need no second copy and no second synchronisation.  The copy's size is baked into a
      // captured graph: drop it, the next frame captures again (host cost of one capture, once).
      h->first_copy = std::min(h->opt.max_candidates, n + n / 4 + 16);
      drop_graph(h);
    }
  }
  if (found > h->opt.max_candidates) return fail(h, PBD_ERR_CAPACITY, "device candidate capacity exceeded; raise pbd_options.max_candidates");
  return PBD_OK;
}

// Candidate records (cand_stride bytes each, possibly from several handles of one group: recs[i] points at record i)
// -> the caller's arrays, ordered like a single-threaded reference run: level, component, row-major root location.
int pbd_i_emit(pbd_handle* h, const std::vector<const char*>& recs, pbd_candidate_head* heads, int32_t* boxes,
               int32_t* locs, int capacity, bool ordered, std::vector<int>* order_out) {
  const int mp = h->max_parts, n = (int)recs.size();
  std::vector<int> order(n);
  for (int i = 0; i < n; ++i) order[i] = i;
  auto key = [&](int i, int k) -> int {
    const pbd_candidate_head* hd = (const pbd_candidate_head*)recs[i];
    const int32_t* lc = pbd_rec_locs(recs[i], mp);
    return k == 0 ? hd->level : k == 1 ? hd->component : k == 2 ? lc[1] : lc[0];
  };
  if (!ordered)
  std::sort(order.begin(), order.end(), [&](int a, int b) {
    for (int k = 0; k < 4; ++k) { int ka = key(a, k), kb = key(b, k); if (ka != kb) return ka < kb; }
    return false;
  });
  if (order_out) *order_out = order;
  if (n > capacity) return fail(h, PBD_ERR_CAPACITY, "output capacity too small");
  for (int i = 0; i < n; ++i) pbd_rec_get(recs[order[i]], mp, heads, boxes, locs, i);
  return PBD_OK;
}

int pbd_i_found(const pbd_handle* h) { return h->pf.filtered ? h->h_cf_cnt[1] : h->h_cand_count[0]; }

// The pending frames' records -> the caller's arrays, frame f's at heads[f * capacity], boxes[f * capacity * max_parts * 4],
// locs[f * capacity * max_parts * 3]; counts[f] = number found in frame f.  A single frame is a batch of one.  single (pbd_detect_collect,
// pbd_dp_argmin): the count is frame 0's own (pbd_i_found), set before anything can fail, and the first refusal is returned.  Batch: the
// device count of all frames (filtered: the records in FRONT of the filter, so the fetch covers every kept one); counts[] are written
// once the records are on the host, a frame beyond `capacity` is skipped and PBD_ERR_CAPACITY returned after the others.
// A gt-box frame or batch (gt != null, and only then): counts[0] = the records in front of the selection, and once the list is known
// not to have overflowed, the winners — frame f's at heads[f * PBD_GT_MAX] — with found and o instead of the records.
struct GtOut { int* found; double* o; };
static int collect_frames(pbd_handle* h, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int capacity, int* counts, bool single,
                          const GtOut* gt = nullptr) {
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->pf.gt) {
    const int nrec = h->h_cand_count[0];
    if (counts) *counts = nrec;
    int rc = pbd_i_finish_frame(h, nrec);
    if (rc) return rc;
    if (!gt) return fail(h, PBD_ERR_STATE, "a gt-box frame is collected by the entry that enqueued it");
    pbd_i_gt_gather(h, heads, boxes, locs, gt->found, gt->o);
    return PBD_OK;
  }
  const bool filt = h->pf.filtered;
  const int found = single ? pbd_i_found(h) : filt ? h->h_cf_cnt[0] : h->h_cand_count[0];
  if (single && counts) *counts = found;
  int rc = pbd_i_finish_frame(h, found);
  if (rc) return rc;
  const int mp = h->max_parts, n1 = h->nlevels, B = h->batch;
  std::vector<std::vector<const char*>> per(B);
  if (filt) {   // frame f's kept records, in final order, at its offset
    for (int f = 0; f < B; ++f)
      for (int j = 0; j < h->h_cf_cnt[2 + f]; ++j) per[f].push_back(h->h_cand_out + h->cand_stride * ((size_t)h->h_cf_cnt[2 + B + f] + j));
  } else
  for (int i = 0; i < found; ++i) {
    const char* r = h->h_cand_out + h->cand_stride * i;
    per[((const pbd_candidate_head*)r)->level / n1].push_back(r);
  }
  int status = PBD_OK;
  if (h->pf.b3) pbd_i_b3_begin(h, B);
  if (h->pf.ps) pbd_i_ps_begin(h, B);
  std::vector<int> order;
  for (int f = 0; f < B; ++f) {
    if (counts) counts[f] = (int)per[f].size();
    pbd_candidate_head* hf = heads ? heads + (size_t)f * capacity : nullptr;
    rc = pbd_i_emit(h, per[f], hf, boxes ? boxes + (size_t)f * capacity * mp * 4 : nullptr, locs ? locs + (size_t)f * capacity * mp * 3 : nullptr, capacity, filt,
                    h->pf.b3 || h->pf.ps ? &order : nullptr);
    if (rc == PBD_ERR_CAPACITY && !single) { status = rc; continue; }
    if (rc) return rc;
    if (h->pf.b3) pbd_i_b3_gather(h, f, per[f], order);
    if (h->pf.ps) pbd_i_ps_gather(h, f, per[f], order);
    for (size_t i = 0; f && i < per[f].size(); ++i) hf[i].level -= f * n1;   // virtual level -> the frame's own pyramid level
  }
  if (h->pf.b3 && (rc = pbd_i_b3_end(h))) return rc;
  return status;
}

int collect_frame(pbd_handle* h, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int capacity, int* count) {
  if (!h->pf.active) return fail(h, PBD_ERR_STATE, "collect without a pending detect");
  if (h->d_gsend) return fail(h, PBD_ERR_STATE, "handle belongs to an RCCL-gathering pbd_group: collect through the group");
  if (h->batch > 1) return fail(h, PBD_ERR_STATE, "a batch of frames is pending: collect it with pbd_detect_batch_collect");
  return collect_frames(h, heads, boxes, locs, capacity, count, true);
}

// ---- C ABI: detect ---------------------------------------------------------------------------------------
#pragma GCC visibility push(default)
extern "C" {

int pbd_detect_collect(pbd_handle* h, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int capacity, int* count) {
  if (!h) return PBD_ERR_ARG;
  ON_DEVICE(h);
  int rc = collect_frame(h, heads, boxes, locs, capacity, count);
  read_stage_times(h);
  return rc;
}
int pbd_detect_batch_collect(pbd_handle* h, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int capacity, int* counts) {
  if (!h || !heads || !counts || capacity < 0) return PBD_ERR_ARG;
  if (!h->pf.active) return fail(h, PBD_ERR_STATE, "collect without a pending detect");
  if (h->d_gsend) return fail(h, PBD_ERR_STATE, "handle belongs to an RCCL-gathering pbd_group: collect through the group");
  ON_DEVICE(h);
  int rc = collect_frames(h, heads, boxes, locs, capacity, counts, false);
  read_stage_times(h);
  return rc;
}

// ---- single frames: a device image read in place, a host image (pinned for true asynchrony) uploaded on the handle's stream ----
int pbd_detect_enqueue_dev_u8(pbd_handle* h, const void* d_im, int w, int hgt, int cn, int stride) {
  if (!h || !d_im) return PBD_ERR_ARG;
  return enter_frame(h, device_frames(d_im, 1, w, hgt, cn, stride));
}
int pbd_detect_dev_u8(pbd_handle* h, const void* d_im, int w, int hgt, int cn, int stride, pbd_candidate_head* heads,
                      int32_t* boxes, int32_t* locs, int capacity, int* count) {
  int rc = pbd_detect_enqueue_dev_u8(h, d_im, w, hgt, cn, stride);
  return rc ? rc : pbd_detect_collect(h, heads, boxes, locs, capacity, count);
}
int pbd_detect_enqueue_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride) {
  if (!h || !im) return PBD_ERR_ARG;
  return enter_frame(h, host_frame(im, w, hgt, cn, stride, PBD_DEPTH_8U));
}
int pbd_detect_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, pbd_candidate_head* heads,
                  int32_t* boxes, int32_t* locs, int capacity, int* count) {
  int rc = pbd_detect_enqueue_u8(h, im, w, hgt, cn, stride);
  return rc ? rc : pbd_detect_collect(h, heads, boxes, locs, capacity, count);
}
// images of the other depths the reference accepts (src/HOGFeatures.cpp:136-146): single frames, host images; 8-bit frames are pbd_detect_u8's
int pbd_detect_image(pbd_handle* h, const void* im, int depth, int w, int hgt, int cn, int stride, pbd_candidate_head* heads,
                     int32_t* boxes, int32_t* locs, int capacity, int* count) {
  if (!h || !im) return PBD_ERR_ARG;
  if (depth == PBD_DEPTH_8U) return pbd_detect_u8(h, (const uint8_t*)im, w, hgt, cn, stride, heads, boxes, locs, capacity, count);
  int rc = enter_frame(h, host_frame(im, w, hgt, cn, stride, depth));
  return rc ? rc : pbd_detect_collect(h, heads, boxes, locs, capacity, count);
}

// ---- a batch of same-sized frames through ONE handle ---------------------------------------------------------
// (SURVEY 8b lists pbd_detect_batch_u8; configs[2] hands every GPU 4 frames.)  The frames of a batch are planned as
// extra "virtual levels" (pbd_internal.hpp), so every stage is one launch — or one chain of launches — for the whole
// batch: the same kernels, B times the blocks per launch.  Results per frame are identical to pbd_detect_u8.
int pbd_detect_batch_enqueue_dev_u8(pbd_handle* h, const void* d_ims, int nframes, int w, int hgt, int cn) {
  if (!h || !d_ims || nframes < 1) return PBD_ERR_ARG;
  return enter_frame(h, device_frames(d_ims, nframes, w, hgt, cn, w * cn));
}
int pbd_detect_batch_enqueue_u8(pbd_handle* h, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride) {
  if (!h || !ims || nframes < 1) return PBD_ERR_ARG;
  return enter_frame(h, host_batch(ims, nframes, w, hgt, cn, stride));
}
int pbd_detect_batch_u8(pbd_handle* h, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride,
                        pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int capacity, int* counts) {
  int rc = pbd_detect_batch_enqueue_u8(h, ims, nframes, w, hgt, cn, stride);
  return rc ? rc : pbd_detect_batch_collect(h, heads, boxes, locs, capacity, counts);
}

// ---- frames with a depth image (the depth pruning, 3-D boxes and object clusters of pbd_post.cpp behind back-tracking) ----
// With neither the depth filter nor the 3-D boxes on, or without a depth image, these are the plain entries.
int pbd_detect_rgbd_enqueue_dev_u8(pbd_handle* h, const void* d_im, int w, int hgt, int cn, int stride, const void* d_depth,
                                   int depth_type, int dstride) {
  if (!h) return PBD_ERR_ARG;
  if ((!h->zf_on && !h->b3_on) || !d_depth) return pbd_detect_enqueue_dev_u8(h, d_im, w, hgt, cn, stride);
  if (!d_im) return PBD_ERR_ARG;
  const DepthSource z = depth_images(true, d_depth, depth_type, dstride, 0, 1);
  return enter_frame(h, device_frames(d_im, 1, w, hgt, cn, stride, &z));
}
int pbd_detect_rgbd_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, const void* depth, int depth_type,
                       int dstride, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int capacity, int* count) {
  if (!h) return PBD_ERR_ARG;
  if ((!h->zf_on && !h->b3_on) || !depth) return pbd_detect_u8(h, im, w, hgt, cn, stride, heads, boxes, locs, capacity, count);
  if (!im) return PBD_ERR_ARG;
  const DepthSource z = depth_images(false, depth, depth_type, dstride, 0, 1);
  int rc = enter_frame(h, host_frame(im, w, hgt, cn, stride, PBD_DEPTH_8U, &z));
  return rc ? rc : pbd_detect_collect(h, heads, boxes, locs, capacity, count);
}
int pbd_detect_batch_rgbd_enqueue_dev_u8(pbd_handle* h, const void* d_ims, const void* d_depths, int nframes, int w, int hgt, int cn,
                                         int depth_type) {
  if (!h) return PBD_ERR_ARG;
  if (!h->zf_on && !h->b3_on) return pbd_detect_batch_enqueue_dev_u8(h, d_ims, nframes, w, hgt, cn);
  if (!d_depths) return fail(h, PBD_ERR_ARG, "device batch: the depth images are one packed buffer (NULL: use pbd_detect_batch_enqueue_dev_u8)");
  if (!d_ims || nframes < 1) return PBD_ERR_ARG;
  const size_t zrow = (size_t)w * h->ts;
  const DepthSource z = depth_images(true, d_depths, depth_type, (long long)zrow, zrow * hgt, nframes >= 64 ? ~0ull : (1ull << nframes) - 1);
  return enter_frame(h, device_frames(d_ims, nframes, w, hgt, cn, w * cn, &z));
}
// Host batch: a depth image per frame, any of them null.  This entry packs them into the handle's depth buffer in FRONT of the
// frames' own checks (stride, plan), as it always has; enter_frame then sees one packed device buffer.
int pbd_detect_batch_rgbd_u8(pbd_handle* h, const uint8_t* const* ims, const void* const* depths, int nframes, int w, int hgt, int cn,
                             int stride, int depth_type, int dstride, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs,
                             int capacity, int* counts) {
  if (!h) return PBD_ERR_ARG;
  unsigned long long has = 0;
  for (int f = 0; depths && f < nframes && f < 64; ++f) if (depths[f]) has |= 1ull << f;
  if ((!h->zf_on && !h->b3_on) || !has) return pbd_detect_batch_u8(h, ims, nframes, w, hgt, cn, stride, heads, boxes, locs, capacity, counts);
  int rc = pbd_i_depth_check(h, depth_type, dstride, w);
  if (rc) return rc;
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "previous frame not collected");
  if (!ims || nframes < 1 || nframes > 64) return fail(h, PBD_ERR_ARG, "batch: 1..64 frames");
  ON_DEVICE(h);
  const size_t zrow = (size_t)w * h->ts, fb = zrow * hgt;
  if ((rc = model_grow(h, &h->d_zimg, h->zimg_bytes, fb * nframes))) return rc;
  for (int f = 0; f < nframes; ++f)
    if (depths[f] && (rc = copy_rows(h, h->d_zimg + fb * f, depths[f], (size_t)dstride, zrow, (size_t)hgt, hipMemcpyHostToDevice))) return rc;
  const DepthSource z = depth_images(true, h->d_zimg, depth_type, (long long)zrow, fb, has);   // (enter_frame repeats the depth and pending checks: they passed above and cannot refuse now)
  if ((rc = enter_frame(h, host_batch(ims, nframes, w, hgt, cn, stride, &z)))) return rc;
  return pbd_detect_batch_collect(h, heads, boxes, locs, capacity, counts);
}

// ---- latent detection: detect(im, model, thresh, bbox, overlap) of matlab/detection/detect.m ------------------------------------
// The plain entries with a truth set per frame: one record (or none) per frame.  Arguments are checked before anything is planned.
static int latent_enter(pbd_handle* h, FrameSource s, const int32_t* truth, const int32_t* mix, int component, double overlap) {
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "previous frame not collected");
  int rc = pbd_i_latent_check(h, truth, mix, s.nframes, component, overlap);
  if (rc) return rc;
  const LatentSource ls{truth, mix, component, overlap};
  s.lat = &ls;
  return enter_frame(h, s);
}
int pbd_detect_latent_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, const int32_t* truth, const int32_t* mix,
                         int component, double overlap, pbd_candidate_head* head, int32_t* boxes, int32_t* locs, int* found) {
  if (!h || !im) return PBD_ERR_ARG;
  int rc = latent_enter(h, host_frame(im, w, hgt, cn, stride, PBD_DEPTH_8U), truth, mix, component, overlap);
  return rc ? rc : pbd_detect_collect(h, head, boxes, locs, 1, found);
}
int pbd_detect_latent_dev_u8(pbd_handle* h, const void* d_im, int w, int hgt, int cn, int stride, const int32_t* truth, const int32_t* mix,
                             int component, double overlap, pbd_candidate_head* head, int32_t* boxes, int32_t* locs, int* found) {
  if (!h || !d_im) return PBD_ERR_ARG;
  int rc = latent_enter(h, device_frames(d_im, 1, w, hgt, cn, stride), truth, mix, component, overlap);
  return rc ? rc : pbd_detect_collect(h, head, boxes, locs, 1, found);
}
int pbd_detect_batch_latent_u8(pbd_handle* h, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride,
                               const int32_t* truth, const int32_t* mix, int component, double overlap, pbd_candidate_head* heads,
                               int32_t* boxes, int32_t* locs, int* found) {
  if (!h || !ims || !heads || !found || nframes < 1) return PBD_ERR_ARG;
  int rc = latent_enter(h, host_batch(ims, nframes, w, hgt, cn, stride), truth, mix, component, overlap);
  return rc ? rc : pbd_detect_batch_collect(h, heads, boxes, locs, 1, found);
}

// ---- best pose per ground-truth box: testmodel_gtbox.m / bestoverlap.m (include/pbd_c.h) -----------------------------------------
// The plain entries with the gt boxes of every frame: behind the back-tracking the selection of k_gtbox.hip, and only its winners
// come home.  Arguments and settings are checked before anything is planned.
static int gtbox_run(pbd_handle* h, FrameSource s, const double* gt, const int* ngt, double overlap, pbd_candidate_head* heads,
                     int32_t* boxes, int32_t* locs, int* found, double* o, int* nrecords) {
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "previous frame not collected");
  int rc = pbd_i_gt_check(h, gt, ngt, s.nframes, overlap, true);
  if (rc) return rc;
  const GtSource gs{gt, ngt, overlap};
  s.gt = &gs;
  if ((rc = enter_frame(h, s))) return rc;
  const GtOut out{found, o};
  rc = collect_frames(h, heads, boxes, locs, PBD_GT_MAX, nrecords, s.nframes == 1, &out);
  read_stage_times(h);
  return rc;
}
int pbd_detect_gtbox_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, const double* gt, int ngt, double overlap,
                        pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int* found, double* o, int* nrecords) {
  if (!h || !im || (ngt > 0 && (!heads || !found))) return PBD_ERR_ARG;
  return gtbox_run(h, host_frame(im, w, hgt, cn, stride, PBD_DEPTH_8U), gt, &ngt, overlap, heads, boxes, locs, found, o, nrecords);
}
int pbd_detect_gtbox_dev_u8(pbd_handle* h, const void* d_im, int w, int hgt, int cn, int stride, const double* gt, int ngt, double overlap,
                            pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int* found, double* o, int* nrecords) {
  if (!h || !d_im || (ngt > 0 && (!heads || !found))) return PBD_ERR_ARG;
  return gtbox_run(h, device_frames(d_im, 1, w, hgt, cn, stride), gt, &ngt, overlap, heads, boxes, locs, found, o, nrecords);
}
int pbd_detect_batch_gtbox_u8(pbd_handle* h, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride, const double* gt,
                              const int* ngt, double overlap, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int* found,
                              double* o, int* nrecords) {
  if (!h || !ims || !heads || !found || nframes < 1) return PBD_ERR_ARG;
  return gtbox_run(h, host_batch(ims, nframes, w, hgt, cn, stride), gt, ngt, overlap, heads, boxes, locs, found, o, nrecords);
}

// ---- the planner's one measured rule, re-measured on the caller's own frames ---------------------------------
// The distance transform's block geometry (lanes and LDS per block) changes the stage's time by a few per cent either way depending on
// the frame size, the model and whether frames come singly or in batches, and never its results (dt_core.hpp: the same exact
// algorithm under any segmentation).  plan_frame picks by a rule measured on seven sizes with the person model;
// pbd_tune_plan runs the caller's frame through both geometries of a float handle — `batch` copies per call, 2 warm-up + 3 timed
// calls each, the dp_min stage's GPU time from the stage events — and keeps the faster one for every later plan of this handle.
// im == NULL: back to the rule.  chosen: 1 = 256 lanes / 40 KB, 2 = 128 lanes / 25 KB, 0 = nothing to choose (double handles).
int pbd_tune_plan(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, int batch, int* chosen, double ms[2]) {
  if (!h) return PBD_ERR_ARG;
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "previous frame not collected");
  // (a member of an RCCL-gathering group collects through the group only: the measurement's own collect() would fail with the frame
  //  left pending — ADVICE r05)
  if (h->d_gsend) return fail(h, PBD_ERR_STATE, "handle belongs to an RCCL-gathering pbd_group: tune a handle of its own");
  if (h->pyr_kind == PBD_PYRAMID_MATLAB) return fail(h, PBD_ERR_UNSUPPORTED, "pbd_tune_plan: PBD_PYRAMID_OPENCV handles (tune before pbd_set_pyramid_kind)");
  if (chosen) *chosen = 0;
  if (ms) ms[0] = ms[1] = 0.0;
  ON_DEVICE(h);
  // the plan is dropped as a whole (buffers, stage flags, captured graph): a stage getter after pbd_tune_plan answers "no frame
  // geometry" AND the stage flags say so — nothing can run on the last measured geometry
  auto drop_plan = [&]() { if (h->stream) hipStreamSynchronize(h->stream); h->pf.active = false; free_frame(h); };
  if (!im) { h->dt_geom = 0; drop_plan(); return PBD_OK; }
  if (h->ts != 4) return PBD_OK;
  if (batch < 1 || batch > 64) return fail(h, PBD_ERR_ARG, "batch: 1..64 frames");
  const int cap = h->opt.max_candidates;            // per frame (pbd_detect_batch_collect: heads[batch][capacity])
  std::vector<pbd_candidate_head> heads((size_t)cap * batch);
  std::vector<int> counts((size_t)batch);
  std::vector<const uint8_t*> ims((size_t)batch, im);
  const bool prof = h->profiling;
  const int before = h->dt_geom;
  float stage_before[6];
  for (int i = 0; i < 6; ++i) stage_before[i] = h->stage_ms[i];
  double t[2] = {0, 0};
  int rc = PBD_OK;
  h->profiling = true;
  for (int g = 1; g <= 2 && !rc; ++g) {
    h->dt_geom = g; drop_plan();                    // (plan_frame re-plans under the geometry)
    double v[3] = {0, 0, 0};
    for (int i = 0; i < 5 && !rc; ++i) {
      rc = batch == 1 ? pbd_detect_u8(h, im, w, hgt, cn, stride, heads.data(), nullptr, nullptr, cap, counts.data())
                      : pbd_detect_batch_u8(h, ims.data(), batch, w, hgt, cn, stride, heads.data(), nullptr, nullptr, cap, counts.data());
      if (rc == PBD_ERR_CAPACITY) rc = PBD_OK;      // (a low threshold: the stage times are what is wanted)
      if (i >= 2) v[i - 2] = h->stage_ms[3];
    }
    std::sort(v, v + 3);
    t[g - 1] = v[1];
  }
  h->profiling = prof;
  for (int i = 0; i < 6; ++i) h->stage_ms[i] = stage_before[i];   // the caller's last stage times, not the measurement's
  const std::string err = h->err;
  h->dt_geom = rc ? before : (t[0] <= t[1] ? 1 : 2);
  drop_plan();                                      // whatever happened: nothing in flight, no plan of the measurement's call shape left behind
  if (rc) { h->err = err; return rc; }
  if (chosen) *chosen = h->dt_geom;
  if (ms) { ms[0] = t[0]; ms[1] = t[1]; }
  return PBD_OK;
}

}  // extern "C"
#pragma GCC visibility pop
