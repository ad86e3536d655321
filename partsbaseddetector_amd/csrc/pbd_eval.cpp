// pbd_eval.cpp — the evaluation ledger's host side (include/pbd_c.h "evaluation ledger"; kernels: k_eval.hip; the definitions as host
// code: pbd_eval_host.cpp): the ledger's buffers, the argument checks, the append positions (the host knows ngt; k_eval_span answers the
// frames' detection counts) and the pbd_eval_* entry points.  The ledger borrows its handle's model, stream and device; errors go
// through the handle.  PCK frames run as gt-box frames (FRAME_GTBOX) and read the winners where k_gtbox_pick left them; APK frames run
// as FRAME_EVAL jobs (pbd_route.hpp), routed like mining frames, and read the final records through pbd_i_route_records.
#include <algorithm>
#include <cmath>
#include "pbd_internal.hpp"

struct pbd_eval {
  pbd_handle* h = nullptr;
  EvalLedgerDev L{};
  int n = 0, m = 0, frames = 0;
  long long npos = 0;
  double thresh = .5;
  unsigned long long* d_key = nullptr; int n2cap = 0;
  int* d_tpc = nullptr; double* d_sm = nullptr; double* d_out = nullptr;
  DevBufs bufs;
  template <typename T> int alloc(T** p, size_t n) {
    const hipError_t e = bufs.alloc(p, n);
    return e == hipSuccess ? PBD_OK : fail(h, PBD_ERR_HIP, pbd_alloc_error("evaluation: ", e));
  }
};

namespace {
// the small tables of one call: sections of one host blob, uploaded into one device buffer of the call's scratch
struct Blob {
  std::vector<char> host;
  char* dev = nullptr;
  size_t put(const void* p, size_t bytes) {   // -> the section's offset (16-byte aligned)
    const size_t off = (host.size() + 15) & ~(size_t)15;
    host.resize(off + bytes);
    if (bytes && p) memcpy(host.data() + off, p, bytes);
    return off;
  }
  size_t room(size_t bytes) { return put(nullptr, bytes); }
  int upload(CallScratch& s) {
    dev = s.dev<char>(std::max<size_t>(host.size(), 16));
    s.up(dev, host.data(), host.size());
    return s.status("evaluation: ");
  }
  template <typename T> T* at(size_t off) const { return (T*)(dev + off); }
};
int finish(pbd_handle* h, const char* what) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  return e == hipSuccess ? PBD_OK : fail(h, PBD_ERR_HIP, std::string(what) + hipGetErrorString(e));
}

// the annotated persons of nframes frames: points[f][g][P][2], scale[f][g], frame f's at stride `slots` persons (1 frame: packed)
int check_persons(pbd_eval* ev, const double* points, const double* scale, const int* ngt, int nframes, int slots) {
  pbd_handle* h = ev->h;
  const int P = ev->L.P;
  if (nframes < 1 || nframes > PBD_MAX_BATCH) return fail(h, PBD_ERR_ARG, "batch: 1..64 frames");
  if (!ngt) return fail(h, PBD_ERR_ARG, "evaluation: null ngt");
  for (int f = 0; f < nframes; ++f) {
    if (ngt[f] < 0 || ngt[f] > PBD_GT_MAX) return fail(h, PBD_ERR_ARG, "evaluation: ngt outside 0..PBD_GT_MAX");
    if (ngt[f] > 0 && (!points || !scale)) return fail(h, PBD_ERR_ARG, "evaluation: null points / scale");
    for (int g = 0; g < ngt[f]; ++g) {
      const size_t person = (size_t)f * slots + g;
      const double s = scale[person];
      if (!std::isfinite(s) || !(s > 0.0)) return fail(h, PBD_ERR_ARG, "evaluation: every scale must be finite and > 0");
      for (int k = 0; k < P * 2; ++k)
        if (!std::isfinite(points[person * P * 2 + k])) return fail(h, PBD_ERR_ARG, "evaluation: a non-finite point coordinate");
    }
  }
  return PBD_OK;
}
// the persons of a call back to back, with the frames' table: -> the offsets of frames / points / scale in the blob
struct PersonTables { size_t frames, points, scale; int total; };
PersonTables put_persons(Blob& b, std::vector<EvalFrame>& fr, int P, const double* points, const double* scale, const int* ngt, int slots) {
  PersonTables t{};
  int goff = 0;
  for (size_t f = 0; f < fr.size(); ++f) { fr[f].ngt = ngt[f]; fr[f].goff = goff; goff += ngt[f]; }
  t.total = goff;
  std::vector<double> pts((size_t)goff * P * 2), sc((size_t)goff);
  for (size_t f = 0; f < fr.size(); ++f)
    for (int g = 0; g < ngt[f]; ++g) {
      const size_t src = f * slots + g, dst = (size_t)fr[f].goff + g;
      std::copy(points + src * P * 2, points + (src + 1) * P * 2, pts.begin() + dst * P * 2);
      sc[dst] = scale[src];
    }
  t.frames = b.put(fr.data(), sizeof(EvalFrame) * fr.size());
  t.points = b.put(pts.data(), sizeof(double) * pts.size());
  t.scale = b.put(sc.data(), sizeof(double) * sc.size());
  return t;
}
int capacity_fail(pbd_handle* h, const char* what, long long need, int cap) {
  return fail(h, PBD_ERR_CAPACITY, std::string("evaluation: the ledger would hold ") + std::to_string(need) + " " + what + ", its capacity is " +
                                   std::to_string(cap) + ": nothing was added (an evaluation that drops records is wrong)");
}

// PCK: nframes * slots record slots at rec (device-readable), found per slot, -> the instance columns n ...
int pck_append(pbd_eval* ev, const char* rec, size_t stride, int slots, const int* found, int nframes, const double* points,
               const double* scale, const int* ngt) {
  pbd_handle* h = ev->h;
  CallScratch s(h);
  Blob b;
  std::vector<EvalFrame> fr((size_t)nframes);
  const PersonTables t = put_persons(b, fr, ev->L.P, points, scale, ngt, slots);
  if (t.total > 0) {
    const size_t o_found = b.put(found, sizeof(int) * (size_t)nframes * slots);
    int rc = b.upload(s);
    if (rc) return rc;
    EvalPckAddArgs a{};
    a.L = ev->L; a.n0 = ev->n;
    a.rec = rec; a.stride = stride; a.slots = slots;
    a.found = b.at<int>(o_found); a.frames = b.at<EvalFrame>(t.frames);
    a.points = b.at<double>(t.points); a.scale = b.at<double>(t.scale);
    launch_eval_pck_add(a, nframes, h->stream);
    if ((rc = finish(h, "evaluation (PCK add): "))) return rc;
  }
  ev->n += t.total; ev->frames += nframes;
  return PBD_OK;
}

// the gt box of a person: [min x, min y, max x, max y] of its points (testmodel_gtbox.m:18-20); exact
void person_box(const double* pts, int P, double* box) {
  box[0] = box[2] = pts[0]; box[1] = box[3] = pts[1];
  for (int p = 1; p < P; ++p) {
    box[0] = std::min(box[0], pts[p * 2]); box[2] = std::max(box[2], pts[p * 2]);
    box[1] = std::min(box[1], pts[p * 2 + 1]); box[3] = std::max(box[3], pts[p * 2 + 1]);
  }
}

int pck_run(pbd_eval* ev, const uint8_t* im, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride,
            const double* points, const double* scale, const int* ngt, double overlap, int* found, int* nrecords, int* needed) {
  pbd_handle* h = ev->h;
  const int P = ev->L.P, slots = ims ? PBD_GT_MAX : std::max(ngt ? ngt[0] : 0, 1);
  int rc = check_persons(ev, points, scale, ngt, nframes, slots);
  if (rc) return rc;
  int total = 0;
  for (int f = 0; f < nframes; ++f) total += ngt[f];
  if (total > 0 && !found) return fail(h, PBD_ERR_ARG, "evaluation: found is NULL");
  if (needed) *needed = ev->n + total;
  if ((long long)ev->n + total > ev->L.ncap) return capacity_fail(h, "instances", (long long)ev->n + total, ev->L.ncap);
  std::vector<double> gt((size_t)nframes * PBD_GT_MAX * 4, 0.0);
  for (int f = 0; f < nframes; ++f)
    for (int g = 0; g < ngt[f]; ++g) person_box(points + ((size_t)f * slots + g) * P * 2, P, gt.data() + ((size_t)f * PBD_GT_MAX + g) * 4);
  std::vector<pbd_candidate_head> heads((size_t)nframes * PBD_GT_MAX);
  std::vector<int> fnd((size_t)nframes * PBD_GT_MAX, 0);
  rc = ims ? pbd_detect_batch_gtbox_u8(h, ims, nframes, w, hgt, cn, stride, gt.data(), ngt, overlap, heads.data(), nullptr, nullptr, fnd.data(), nullptr, nrecords)
           : pbd_detect_gtbox_u8(h, im, w, hgt, cn, stride, gt.data(), ngt[0], overlap, heads.data(), nullptr, nullptr, fnd.data(), nullptr, nrecords);
  if (rc) return rc;
  for (int f = 0; f < nframes; ++f)
    for (int g = 0; g < ngt[f]; ++g) found[(size_t)f * slots + g] = fnd[(size_t)f * PBD_GT_MAX + g];
  // the winners' records are where k_gtbox_pick wrote them: pinned, device-mapped slots f * PBD_GT_MAX + g
  return pck_append(ev, h->h_gt_out, h->cand_stride, PBD_GT_MAX, fnd.data(), nframes, points, scale, ngt);
}

// APK: the frames' detections (frames[f].start / count, in `perm`'s order when given) matched and appended as rows m ...
int apk_append(pbd_eval* ev, const char* rec, size_t stride, const int* perm, std::vector<EvalFrame>& fr, const double* points,
               const double* scale, const int* ngt, int slots) {
  pbd_handle* h = ev->h;
  CallScratch s(h);
  Blob b;
  const PersonTables t = put_persons(b, fr, ev->L.P, points, scale, ngt, slots);
  int total = 0, maxcount = 0;
  for (const EvalFrame& f : fr) { total = std::max(total, f.start + f.count); maxcount = std::max(maxcount, f.count); }
  if (total > 0) {
    const size_t o_ord = b.room(sizeof(int) * (size_t)total);
    int rc = b.upload(s);
    if (rc) return rc;
    EvalApkAddArgs a{};
    a.L = ev->L; a.m0 = ev->m;
    a.rec = rec; a.stride = stride; a.mp = h->max_parts; a.perm = perm;
    a.ord = b.at<int>(o_ord); a.frames = b.at<EvalFrame>(t.frames);
    a.points = b.at<double>(t.points); a.scale = b.at<double>(t.scale);
    a.thresh = ev->thresh;
    launch_eval_apk_add(a, (int)fr.size(), maxcount, h->stream);
    if ((rc = finish(h, "evaluation (APK add): "))) return rc;
  }
  ev->m += total; ev->npos += t.total; ev->frames += (int)fr.size();
  return PBD_OK;
}

int apk_run(pbd_eval* ev, FrameSource s, const double* points, const double* scale, const int* ngt, int slots, int32_t* records, int* needed) {
  pbd_handle* h = ev->h;
  if (!records) return fail(h, PBD_ERR_ARG, "evaluation: records is NULL");
  int rc = check_persons(ev, points, scale, ngt, s.nframes, slots);
  if (rc) return rc;
  if (h->in_group || h->d_gsend) return fail(h, PBD_ERR_UNSUPPORTED, "evaluation: pbd_group members are not supported");
  if (h->zf_on) return fail(h, PBD_ERR_UNSUPPORTED, "evaluation: not with depth pruning on");
  if (h->b3_on) return fail(h, PBD_ERR_UNSUPPORTED, "evaluation: not with 3-D boxes on");
  if (h->cl3_on) return fail(h, PBD_ERR_UNSUPPORTED, "evaluation: not with object clusters on");
  if (h->ps_on) return fail(h, PBD_ERR_UNSUPPORTED, "evaluation: not with per-part scores on");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "previous frame not collected");
  ON_DEVICE(h);
  if ((rc = pbd_i_mine_buffers(h))) return rc;
  if (!h->h_eval_out && (rc = model_alloc(h, &h->h_eval_out, PBD_MAX_BATCH, true, false))) return rc;
  const int B = s.nframes;
  s.eval = true;
  if ((rc = enter_frame(h, s))) return rc;
  hipError_t e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) { h->pf.active = false; return fail(h, PBD_ERR_HIP, std::string("evaluation: ") + hipGetErrorString(e)); }
  const EvalFrameOut* out = h->h_eval_out;
  const int raw = out[0].raw;
  if (raw > h->opt.max_candidates) { std::fill(records, records + B, 0); records[0] = raw; }   // (an overflowed list has no per-frame counts)
  if ((rc = pbd_i_finish_frame(h, raw))) return rc;   // (PBD_ERR_CAPACITY with the plain entries' message; the frame is no longer pending)
  read_stage_times(h);
  std::vector<EvalFrame> fr((size_t)B);
  long long total = 0;
  for (int f = 0; f < B; ++f) {
    records[f] = out[f].count; total += out[f].count;
    fr[f].start = out[f].start; fr[f].count = out[f].count;
  }
  if (needed) *needed = (int)std::min<long long>(ev->m + total, 0x7fffffff);
  if (ev->m + total > ev->L.mcap) return capacity_fail(h, "detections", ev->m + total, ev->L.mcap);
  return apk_append(ev, h->mine_in.p, h->mine_in.stride, h->d_mine_perm, fr, points, scale, ngt, slots);
}
}  // namespace

// behind the route's last post-stage (run_argmin_enqueue): the records' order (RAW: mining's order kernels) and the frames' spans
int pbd_i_eval_enqueue(pbd_handle* h, const FrameRoute& r) {
  EvalSpanArgs a{};
  a.in = h->mine_in = pbd_i_route_records(h, r.final_buf, r.final_count);
  a.nframes = h->batch; a.perm = h->d_mine_perm; a.out = h->h_eval_out;
  if (!a.in.cf) {   // mining's key packs (virtual level, component, root y, root x) into 16 bits each
    if (h->nvl > 65536 || h->md.ncomponents > 65536) return fail(h, PBD_ERR_UNSUPPORTED, "evaluation: more than 65536 (virtual) levels or components");
    for (const Level& L : h->lv)
      if (L.cw > 65536 || L.ch > 65536) return fail(h, PBD_ERR_UNSUPPORTED, "evaluation: a level of more than 65536 cells a side");
    MineArgs m{};
    m.in = a.in; m.nframes = h->batch; m.key = h->d_mine_key; m.perm = h->d_mine_perm;
    launch_qp_mine_order(m, h->stream);
  }
  launch_eval_span(a, h->stream);
  return PBD_OK;
}

#pragma GCC visibility push(default)
extern "C" {

int pbd_eval_create(pbd_handle* h, int nparts, int max_instances, int max_detections, double apk_thresh, pbd_eval** out) {
  if (!h || !out) return PBD_ERR_ARG;
  *out = nullptr;
  if (nparts < 1 || max_instances < 1 || max_detections < 1 || max_detections > (1 << 28) || !std::isfinite(apk_thresh))
    return fail(h, PBD_ERR_ARG, "evaluation: nparts >= 1, max_instances >= 1, 1 <= max_detections <= 2^28, a finite apk_thresh");
  for (int c = 0; c < h->md.ncomponents; ++c)
    if (h->part_offset[c + 1] - h->part_offset[c] != nparts)
      return fail(h, PBD_ERR_ARG, "evaluation: component " + std::to_string(c) + " of the handle's model has " +
                                  std::to_string(h->part_offset[c + 1] - h->part_offset[c]) + " parts, the ledger " + std::to_string(nparts) +
                                  " keypoints: one keypoint per part, in every component");
  if ((long long)nparts * max_detections >= (1LL << 36) || (long long)nparts * max_instances >= (1LL << 36))
    return fail(h, PBD_ERR_ARG, "evaluation: capacity too large");
  ON_DEVICE(h);
  pbd_eval* ev = new pbd_eval;
  ev->h = h; ev->thresh = apk_thresh;
  EvalLedgerDev& L = ev->L;
  L.P = nparts; L.ncap = max_instances; L.mcap = max_detections;
  int n2 = PBD_EVAL_SORT_TILE;
  while (n2 < max_detections) n2 <<= 1;
  ev->n2cap = n2;
  const size_t P = (size_t)nparts, N = (size_t)max_instances, M = (size_t)max_detections;
  int rc;
  if ((rc = ev->alloc(&L.dist, N * P)) || (rc = ev->alloc(&L.scale, N)) || (rc = ev->alloc(&L.score, M)) || (rc = ev->alloc(&L.tp, M * P)) ||
      (rc = ev->alloc(&ev->d_key, (size_t)n2)) || (rc = ev->alloc(&ev->d_tpc, M * P)) || (rc = ev->alloc(&ev->d_sm, M * P)) ||
      (rc = ev->alloc(&ev->d_out, P))) {
    pbd_eval_destroy(ev);
    return rc;
  }
  *out = ev;
  return PBD_OK;
}

void pbd_eval_destroy(pbd_eval* ev) {
  if (!ev) return;
  hipStreamSynchronize(ev->h->stream);   // (like pbd_destroy: the caller's current device is left alone)
  delete ev;
}

int pbd_eval_reset(pbd_eval* ev) {
  if (!ev) return PBD_ERR_ARG;
  ev->n = ev->m = ev->frames = 0; ev->npos = 0;
  return PBD_OK;
}

int pbd_eval_dims(const pbd_eval* ev, int* nparts, int* n, int* m, long long* npos, int* frames) {
  if (!ev) return PBD_ERR_ARG;
  if (nparts) *nparts = ev->L.P;
  if (n) *n = ev->n;
  if (m) *m = ev->m;
  if (npos) *npos = ev->npos;
  if (frames) *frames = ev->frames;
  return PBD_OK;
}

int pbd_eval_get(pbd_eval* ev, double* dist, double* scale, float* score, uint8_t* tp) {
  if (!ev) return PBD_ERR_ARG;
  pbd_handle* h = ev->h;
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  ON_DEVICE(h);
  const size_t P = (size_t)ev->L.P, N = (size_t)ev->n, M = (size_t)ev->m;
  if (dist && N) HIPCHK(h, hipMemcpyAsync(dist, ev->L.dist, sizeof(double) * N * P, hipMemcpyDeviceToHost, h->stream));
  if (scale && N) HIPCHK(h, hipMemcpyAsync(scale, ev->L.scale, sizeof(double) * N, hipMemcpyDeviceToHost, h->stream));
  if (score && M) HIPCHK(h, hipMemcpyAsync(score, ev->L.score, sizeof(float) * M, hipMemcpyDeviceToHost, h->stream));
  if (tp && M) HIPCHK(h, hipMemcpyAsync(tp, ev->L.tp, M * P, hipMemcpyDeviceToHost, h->stream));
  return finish(h, "evaluation (get): ");
}

int pbd_eval_add_pck_records(pbd_eval* ev, const pbd_candidate_head* heads, const int32_t* boxes, const int* found, const double* points,
                             const double* scale, int ngt, int* needed) {
  if (!ev) return PBD_ERR_ARG;
  pbd_handle* h = ev->h;
  int rc = check_persons(ev, points, scale, &ngt, 1, std::max(ngt, 1));
  if (rc) return rc;
  if (ngt > 0 && (!heads || !boxes || !found)) return fail(h, PBD_ERR_ARG, "evaluation: heads / boxes / found is NULL");
  for (int g = 0; g < ngt; ++g)
    if (found[g] && heads[g].nparts != ev->L.P)
      return fail(h, PBD_ERR_ARG, "evaluation: record " + std::to_string(g) + " has " + std::to_string(heads[g].nparts) + " parts, the ledger " +
                                  std::to_string(ev->L.P) + " keypoints: nothing was added");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  if (needed) *needed = ev->n + ngt;
  if ((long long)ev->n + ngt > ev->L.ncap) return capacity_fail(h, "instances", (long long)ev->n + ngt, ev->L.ncap);
  ON_DEVICE(h);
  const int mp = h->max_parts;
  const size_t st = h->cand_stride;
  std::vector<char> rec(st * (size_t)std::max(ngt, 1), 0);
  for (int g = 0; g < ngt; ++g) if (found[g]) pbd_rec_put(rec.data() + st * g, mp, heads, boxes, nullptr, (size_t)g);
  CallScratch s(h);
  char* d_rec = s.dev<char>(ngt > 0 ? rec.size() : 0);
  s.up(d_rec, rec.data(), ngt > 0 ? rec.size() : 0);
  if ((rc = s.status("evaluation: "))) return rc;
  return pck_append(ev, d_rec, st, std::max(ngt, 1), found, 1, points, scale, &ngt);
}

int pbd_eval_add_apk_records(pbd_eval* ev, const pbd_candidate_head* heads, const int32_t* boxes, int count, const double* points,
                             const double* scale, int ngt, int* needed) {
  if (!ev) return PBD_ERR_ARG;
  pbd_handle* h = ev->h;
  int rc = check_persons(ev, points, scale, &ngt, 1, std::max(ngt, 1));
  if (rc) return rc;
  if (count < 0 || (count > 0 && (!heads || !boxes))) return fail(h, PBD_ERR_ARG, "evaluation: heads / boxes / count");
  for (int i = 0; i < count; ++i) {
    if (!std::isfinite(heads[i].score)) return fail(h, PBD_ERR_ARG, "evaluation: non-finite score: its order is undefined");
    if (heads[i].nparts != ev->L.P)
      return fail(h, PBD_ERR_ARG, "evaluation: record " + std::to_string(i) + " has " + std::to_string(heads[i].nparts) + " parts, the ledger " +
                                  std::to_string(ev->L.P) + " keypoints: nothing was added");
  }
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  if (needed) *needed = (int)std::min<long long>((long long)ev->m + count, 0x7fffffff);
  if ((long long)ev->m + count > ev->L.mcap) return capacity_fail(h, "detections", (long long)ev->m + count, ev->L.mcap);
  ON_DEVICE(h);
  const int mp = h->max_parts;
  const size_t st = h->cand_stride;
  std::vector<char> rec(st * (size_t)std::max(count, 1), 0);
  for (int i = 0; i < count; ++i) pbd_rec_put(rec.data() + st * i, mp, heads, boxes, nullptr, (size_t)i);
  CallScratch s(h);
  char* d_rec = s.dev<char>(count > 0 ? rec.size() : 0);
  s.up(d_rec, rec.data(), count > 0 ? rec.size() : 0);
  if ((rc = s.status("evaluation: "))) return rc;
  std::vector<EvalFrame> fr(1);
  fr[0].start = 0; fr[0].count = count;
  return apk_append(ev, d_rec, st, nullptr, fr, points, scale, &ngt, std::max(ngt, 1));
}

int pbd_eval_pck_frame_u8(pbd_eval* ev, const uint8_t* im, int w, int hgt, int cn, int stride, const double* points, const double* scale,
                          int ngt, double overlap, int* found, int* nrecords, int* needed) {
  if (!ev || !im) return PBD_ERR_ARG;
  return pck_run(ev, im, nullptr, 1, w, hgt, cn, stride, points, scale, &ngt, overlap, found, nrecords, needed);
}
int pbd_eval_pck_frame_batch_u8(pbd_eval* ev, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride,
                                const double* points, const double* scale, const int* ngt, double overlap, int* found, int* nrecords,
                                int* needed) {
  if (!ev || !ims) return PBD_ERR_ARG;
  return pck_run(ev, nullptr, ims, nframes, w, hgt, cn, stride, points, scale, ngt, overlap, found, nrecords, needed);
}
int pbd_eval_apk_frame_u8(pbd_eval* ev, const uint8_t* im, int w, int hgt, int cn, int stride, const double* points, const double* scale,
                          int ngt, int* records, int* needed) {
  if (!ev || !im) return PBD_ERR_ARG;
  return apk_run(ev, host_frame(im, w, hgt, cn, stride, PBD_DEPTH_8U), points, scale, &ngt, std::max(ngt, 1), records, needed);
}
int pbd_eval_apk_frame_batch_u8(pbd_eval* ev, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride,
                                const double* points, const double* scale, const int* ngt, int32_t* records, int* needed) {
  if (!ev || !ims) return PBD_ERR_ARG;
  return apk_run(ev, host_batch(ims, nframes, w, hgt, cn, stride), points, scale, ngt, PBD_GT_MAX, records, needed);
}

int pbd_eval_pck(pbd_eval* ev, double thresh, int rule, double* pck) {
  if (!ev) return PBD_ERR_ARG;
  pbd_handle* h = ev->h;
  if (!pck) return fail(h, PBD_ERR_ARG, "evaluation: pck is NULL");
  if (!std::isfinite(thresh)) return fail(h, PBD_ERR_ARG, "evaluation: thresh must be finite");
  if (rule != PBD_EVAL_SCALE_LAST && rule != PBD_EVAL_SCALE_OWN) return fail(h, PBD_ERR_ARG, "evaluation: rule is PBD_EVAL_SCALE_LAST or PBD_EVAL_SCALE_OWN");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  ON_DEVICE(h);
  EvalResultArgs a{};
  a.L = ev->L; a.n = ev->n; a.m = ev->m; a.npos = ev->npos;
  a.out = ev->d_out; a.thresh = thresh; a.rule = rule;
  launch_eval_pck(a, h->stream);
  HIPCHK(h, hipMemcpyAsync(pck, ev->d_out, sizeof(double) * ev->L.P, hipMemcpyDeviceToHost, h->stream));
  return finish(h, "evaluation (PCK): ");
}

int pbd_eval_apk(pbd_eval* ev, double* apk, double* prec, double* rec) {
  if (!ev) return PBD_ERR_ARG;
  pbd_handle* h = ev->h;
  if (!apk) return fail(h, PBD_ERR_ARG, "evaluation: apk is NULL");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  ON_DEVICE(h);
  const size_t P = (size_t)ev->L.P, M = (size_t)ev->m;
  EvalResultArgs a{};
  a.L = ev->L; a.n = ev->n; a.m = ev->m; a.npos = ev->npos;
  a.key = ev->d_key; a.tpc = ev->d_tpc; a.sm = ev->d_sm; a.out = ev->d_out;
  a.n2 = PBD_EVAL_SORT_TILE;
  while (a.n2 < ev->m) a.n2 <<= 1;
  CallScratch s(h);
  const int ncurves = (prec ? 1 : 0) + (rec ? 1 : 0);
  if (ncurves && M) {
    double* d_curves = s.dev<double>(P * M * ncurves);
    int rc = s.status("evaluation (APK): ");
    if (rc) return rc;
    if (prec) a.prec = d_curves;
    if (rec) a.rec = d_curves + (prec ? P * M : 0);
  }
  launch_eval_apk(a, h->stream);
  s.launched();
  s.down(apk, ev->d_out, sizeof(double) * P);
  if (a.prec) s.down(prec, a.prec, sizeof(double) * P * M);
  if (a.rec) s.down(rec, a.rec, sizeof(double) * P * M);
  return s.finish("evaluation (APK): ");
}

}  // extern "C"
#pragma GCC visibility pop
