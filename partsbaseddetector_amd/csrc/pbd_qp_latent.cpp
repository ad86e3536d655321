// pbd_qp_latent.cpp — latent positives (include/pbd_c.h "latent positives"; kernels: k_qp_latent.hip, k_qp.hip's write):
// train.m:166-193's detect(im, model, 0, bbox, overlap, id, 1) with the frame's pose left on the device.  The frame runs as a
// FRAME_LATENT_WRITE job (pbd_route.hpp): a latent frame whose record stays in the device buffer; behind its back-tracking (and the
// candidate filter) the scan is enqueued (pbd_i_latent_write_enqueue), the host reads the scan's pinned block once, and k_qp_write runs
// over the resident records with label +1.  qp.ub does not move and there is no action (detect.m:133,148 are ~latent).
#include <algorithm>
#include "pbd_qp.hpp"

using namespace pbd_qp_detail;

namespace {
const char* const kWhy[] = {"", "a part outside its level or the model", "a column longer than k",
                            "its blocks repeat a dense start index (two of its parts share a filter, def or bias id): qp_write's assertion "
                            "(matlab/learning/qp_write.m:34-35)"};

int latent_write_run(pbd_qp* q, FrameSource s, const int32_t* truth, const int32_t* mix, int component, double overlap,
                     const int32_t* ids, pbd_latent_example* out) {
  pbd_handle* h = q->h;
  if (!out || !ids) return fail(h, PBD_ERR_ARG, "latent positives: out / ids is NULL");
  if (s.nframes < 1 || s.nframes > PBD_MAX_BATCH) return fail(h, PBD_ERR_ARG, "batch: 1..64 frames");
  // (unreachable through the ABI, as the same line in mining is: pbd_qp_create refuses a member, so no cache is ever bound to one; kept so
  //  that the refusal does not depend on that)
  if (h->in_group || h->d_gsend) return fail(h, PBD_ERR_UNSUPPORTED, "latent positives: pbd_group members are not supported");
  if (h->zf_on) return fail(h, PBD_ERR_UNSUPPORTED, "latent positives: not with depth pruning on");
  if (h->b3_on) return fail(h, PBD_ERR_UNSUPPORTED, "latent positives: not with 3-D boxes on");
  if (h->cl3_on) return fail(h, PBD_ERR_UNSUPPORTED, "latent positives: not with object clusters on");
  if (h->ps_on) return fail(h, PBD_ERR_UNSUPPORTED, "latent positives: not with per-part scores on");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "previous frame not collected");
  int rc;
  if ((rc = pbd_i_latent_check(h, truth, mix, s.nframes, component, overlap))) return rc;   // every refusal of the latent entries
  ON_DEVICE(h);
  // (what can be refused from the arguments and the settings alone has been; the compact plan and a bad record are known only once the
  //  frame is planned / has run)
  if ((rc = pbd_i_mine_buffers(h))) return rc;
  if (!h->h_latw_out && (rc = model_alloc(h, &h->h_latw_out, PBD_MAX_BATCH, true, false))) return rc;
  const int B = s.nframes;
  HIPCHK(h, hipStreamSynchronize(h->stream));   // (the pinned staging copy of the ids is read by the copy below)
  std::copy(ids, ids + B, h->h_mine_ids);
  HIPCHK(h, hipMemcpyAsync(h->d_mine_ids, h->h_mine_ids, sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
  h->mine_k = q->dev.k;
  const LatentSource ls{truth, mix, component, overlap};
  s.lat = &ls; s.lat_write = true;
  if ((rc = enter_frame(h, s))) return rc;
  hipError_t e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) { h->pf.active = false; return fail(h, PBD_ERR_HIP, std::string("latent positives: ") + hipGetErrorString(e)); }
  const LatentWriteOut* lo = h->h_latw_out;
  if ((rc = pbd_i_finish_frame(h, lo[0].raw))) return rc;   // (at most one record per frame: never over capacity; the frame is no longer pending)
  read_stage_times(h);
  for (int f = 0; f < B; ++f) {
    pbd_latent_example& o = out[f];
    o.found = lo[f].found; o.written = 0;
    o.component = lo[f].component; o.level = lo[f].level; o.x = lo[f].x; o.y = lo[f].y;
    o.score = lo[f].score;
  }
  // a refused call has written nothing: written = 0 says so
  for (int f = 0; f < B; ++f)
    if (lo[f].found && lo[f].code != MINE_OK)
      return fail(h, PBD_ERR_ARG, "latent positives: the record of frame " + std::to_string(f) + ": " + kWhy[lo[f].code & 3]);
  int total = 0;
  for (int f = 0; f < B; ++f) total += lo[f].found ? 1 : 0;
  int room = q->dev.capacity - q->n;
  const int n = std::min(total, room);   // a full cache is no error (qp_write.m:21-23)
  for (int f = 0; f < B; ++f)
    if (lo[f].found && room > 0) { out[f].written = 1; --room; }
  if (n > 0) {
    QpWriteArgs a{};
    pbd_i_fv_args(h, &a.fv);
    a.fv.in = h->mine_in; a.fv.rec0 = 0; a.fv.n = n;
    a.q = q->dev; a.n0 = q->n;
    a.wreg = q->d_wreg; a.w0 = q->d_w0; a.foff = q->d_foff;
    a.C = q->cpos; a.label = 1; a.id = 0;
    a.perm = h->d_mine_perm; a.ids = h->d_mine_ids; a.nlevels = h->nlevels;
    launch_qp_write(a, h->ts, h->stream);
    LAUNCHCHK(h, "latent positives write");
    for (int i = 0; i < n; ++i) q->overlap[q->slot[q->n + i]] = 0;   // (a record's blocks never overlap: the scan's check)
    q->meta_dirty = true;
    if ((rc = pbd_i_qp_appended(q, q->n, n))) return rc;
    q->n += n;
    if ((rc = finish(h, "latent positives write: "))) return rc;
  }
  return PBD_OK;
}
}  // namespace

// behind the back-tracking and the route's candidate filter (run_argmin_enqueue): the scan of the frames' poses
int pbd_i_latent_write_enqueue(pbd_handle* h, const FrameRoute& r) {
  LatentWriteArgs a{};
  a.in = h->mine_in = pbd_i_route_records(h, r.final_buf, r.final_count);
  a.nframes = h->batch; a.k = h->mine_k;
  pbd_i_fv_args(h, &a.fv);
  a.fv.in = a.in;
  a.noshare = h->d_mine_noshare;
  a.perm = h->d_mine_perm; a.out = h->h_latw_out;
  launch_qp_latent_scan(a, h->stream);
  return PBD_OK;
}

#pragma GCC visibility push(default)
extern "C" {

int pbd_qp_write_latent_u8(pbd_qp* q, const uint8_t* im, int w, int hgt, int cn, int stride, const int32_t* truth, const int32_t* mix,
                           int component, double overlap, int id, pbd_latent_example* out) {
  if (!q || !im) return PBD_ERR_ARG;
  const int32_t ids[1] = {id};
  return latent_write_run(q, host_frame(im, w, hgt, cn, stride, PBD_DEPTH_8U), truth, mix, component, overlap, ids, out);
}
int pbd_qp_write_latent_dev_u8(pbd_qp* q, const void* d_im, int w, int hgt, int cn, int stride, const int32_t* truth, const int32_t* mix,
                               int component, double overlap, int id, pbd_latent_example* out) {
  if (!q || !d_im) return PBD_ERR_ARG;
  const int32_t ids[1] = {id};
  return latent_write_run(q, device_frames(d_im, 1, w, hgt, cn, stride), truth, mix, component, overlap, ids, out);
}
int pbd_qp_write_latent_batch_u8(pbd_qp* q, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride,
                                 const int32_t* truth, const int32_t* mix, int component, double overlap, const int32_t* ids,
                                 pbd_latent_example* out) {
  if (!q || !ims) return PBD_ERR_ARG;
  return latent_write_run(q, host_batch(ims, nframes, w, hgt, cn, stride), truth, mix, component, overlap, ids, out);
}

}  // extern "C"
#pragma GCC visibility pop
