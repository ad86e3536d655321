// pbd_qp_mine.cpp — hard-negative mining (include/pbd_c.h "hard-negative mining"; kernels: k_qp_mine.hip, k_qp.hip's write):
// train.m:99-108's detect(im, model, -1, [], 0, i, -1) with the frame's records left on the device.  The frame runs as a FRAME_MINE
// job (pbd_route.hpp); behind its last post-stage the order and the scan are enqueued (pbd_i_mine_enqueue), the host reads the scan's
// pinned block once, and k_qp_write runs over the resident records.  ub and the action are detect.m:135,148-149,315-324's bookkeeping.
#include <algorithm>
#include <map>
#include "pbd_qp.hpp"

using namespace pbd_qp_detail;

namespace {
// per component: 1 when no two of its parts can share a filter, def or bias id whatever mixtures a pose picks — then no record of it
// can repeat a dense start (qp_write.m:34-35) and the scan skips the pairwise test
std::vector<int> noshare_table(const pbd_handle* h) {
  const int nc = h->md.ncomponents;
  std::vector<int> out((size_t)nc, 1);
  for (int c = 0; c < nc; ++c) {
    const int f0 = h->part_offset[c], np = h->part_offset[c + 1] - f0;
    std::map<int, int> fi, di, bi;   // id -> the part that uses it
    auto claim = [&](std::map<int, int>& m, int id, int p) {
      auto it = m.emplace(id, p).first;
      if (it->second != p) out[c] = 0;
    };
    for (int p = 0; p < np; ++p) {
      const int q = h->parentid[f0 + p];
      const int kq = p > 0 && q >= 0 && q < np ? h->mix_offset[f0 + q + 1] - h->mix_offset[f0 + q] : 1;
      if (p == 0) claim(bi, h->biasid[h->mix_offset[f0]], 0);
      for (int fm = h->mix_offset[f0 + p]; fm < h->mix_offset[f0 + p + 1]; ++fm) {
        claim(fi, h->filterid[fm], p);
        if (p == 0) continue;
        claim(di, h->defid[fm], p);
        for (int m = 0; m < kq; ++m) claim(bi, h->biasid[fm] + m, p);
      }
    }
  }
  return out;
}

// detect.m:148-149, :315-324 on the state the call left.  ub == 0: lb / ub is +-inf or NaN as IEEE has it; NaN > .05 is false, as in MATLAB
int mine_action(const pbd_qp* q) {
  const QpSolveState& S = q->sol;
  if (S.lb < 0 || q->n == q->dev.capacity) return PBD_MINE_OPT;
  return 1 - S.lb / S.ub > .05 ? PBD_MINE_ONE : PBD_MINE_NONE;
}

const char* const kWhy[] = {"", "a part outside its level or the model", "a column longer than k",
                            "its blocks repeat a dense start index (two of its parts share a filter, def or bias id): qp_write's assertion "
                            "(matlab/learning/qp_write.m:34-35)"};

int mine_run(pbd_qp* q, FrameSource s, const int32_t* ids, int32_t* records, int32_t* written, int* action) {
  pbd_handle* h = q->h;
  if (!records || !written || !action || !ids) return fail(h, PBD_ERR_ARG, "mining: records / written / action / ids is NULL");
  if (s.nframes < 1 || s.nframes > PBD_MAX_BATCH) return fail(h, PBD_ERR_ARG, "batch: 1..64 frames");
  if (h->in_group || h->d_gsend) return fail(h, PBD_ERR_UNSUPPORTED, "mining: pbd_group members are not supported");
  if (h->zf_on) return fail(h, PBD_ERR_UNSUPPORTED, "mining: not with depth pruning on");
  if (h->b3_on) return fail(h, PBD_ERR_UNSUPPORTED, "mining: not with 3-D boxes on");
  if (h->cl3_on) return fail(h, PBD_ERR_UNSUPPORTED, "mining: not with object clusters on");
  if (h->ps_on) return fail(h, PBD_ERR_UNSUPPORTED, "mining: not with per-part scores on");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "previous frame not collected");
  ON_DEVICE(h);
  int rc;
  // (what can be refused from the arguments and the settings alone has been; the compact plan, an overflow and a bad record are known
  //  only once the frame has run.  The solver state allocated here starts at a = 0, sv = 1, ub = 0: what any solver entry would find)
  if ((rc = pbd_i_qp_ensure(q)) || (rc = pbd_i_mine_buffers(h))) return rc;
  const int B = s.nframes;
  HIPCHK(h, hipStreamSynchronize(h->stream));   // (the pinned staging copy of the ids is read by the copy below)
  std::copy(ids, ids + B, h->h_mine_ids);
  HIPCHK(h, hipMemcpyAsync(h->d_mine_ids, h->h_mine_ids, sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
  h->mine_k = q->dev.k; h->mine_cneg = q->cneg;
  s.mine = true;
  if ((rc = enter_frame(h, s))) return rc;
  hipError_t e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) { h->pf.active = false; return fail(h, PBD_ERR_HIP, std::string("mining: ") + hipGetErrorString(e)); }
  const MineFrameOut* out = h->h_mine_out;
  const int raw = out[0].raw;
  // a refused call from here on has written nothing: written[] says so; action is left as the caller had it (the state did not move)
  std::fill(written, written + B, 0);
  if (raw > h->opt.max_candidates) { std::fill(records, records + B, 0); records[0] = raw; }   // (an overflowed list has no per-frame counts)
  if ((rc = pbd_i_finish_frame(h, raw))) return rc;   // (PBD_ERR_CAPACITY with the plain entries' message; the frame is no longer pending)
  read_stage_times(h);
  for (int f = 0; f < B; ++f) records[f] = out[f].count;
  for (int f = 0; f < B; ++f)
    if (out[f].bad >= 0)
      return fail(h, PBD_ERR_ARG, "mining: record " + std::to_string(out[f].bad) + " of frame " + std::to_string(f) + ": " + kWhy[out[f].code & 3]);
  long long total = 0;
  for (int f = 0; f < B; ++f) { records[f] = out[f].count; total += out[f].count; }
  int room = q->dev.capacity - q->n;
  const int n = (int)std::min<long long>(total, room);   // a full cache is no error (qp_write.m:21-23)
  for (int f = 0; f < B; ++f) { written[f] = std::min(records[f], room); room -= written[f]; }
  if (n > 0) {
    QpWriteArgs a{};
    pbd_i_fv_args(h, &a.fv);
    a.fv.in = h->mine_in; a.fv.rec0 = 0; a.fv.n = n;
    a.q = q->dev; a.n0 = q->n;
    a.wreg = q->d_wreg; a.w0 = q->d_w0; a.foff = q->d_foff;
    a.C = q->cneg; a.label = -1; a.id = 0;
    a.perm = h->d_mine_perm; a.ids = h->d_mine_ids; a.nlevels = h->nlevels;
    launch_qp_write(a, h->ts, h->stream);
    LAUNCHCHK(h, "mining write");
    for (int i = 0; i < n; ++i) q->overlap[q->slot[q->n + i]] = 0;   // (a record's blocks never overlap: the scan's check)
    q->meta_dirty = true;
    if ((rc = pbd_i_qp_appended(q, q->n, n))) return rc;
    q->n += n;
    if ((rc = finish(h, "mining write: "))) return rc;
  }
  // detect.m:135 for every record of the frame, written or not (qp_write.m:21-23 returns early, :135 still runs): frame after frame
  for (int f = 0; f < B; ++f) q->sol.ub = q->sol.ub + out[f].S;
  *action = mine_action(q);
  return PBD_OK;
}
}  // namespace

// the order, the ids and the per-component noshare flags: model-lifetime buffers, allocated on first use (pbd_qp_latent.cpp shares them)
int pbd_i_mine_buffers(pbd_handle* h) {
  int rc = pbd_i_fv_tables(h);
  if (rc || h->d_mine_perm) return rc;
  const size_t cap = (size_t)h->opt.max_candidates;
  const std::vector<int> ns = noshare_table(h);
  if ((rc = model_alloc(h, &h->d_mine_key, cap)) ||
      (rc = model_alloc(h, &h->d_mine_ids, PBD_MAX_BATCH)) || (rc = model_alloc(h, &h->h_mine_ids, PBD_MAX_BATCH, true, false)) ||
      (rc = model_alloc(h, &h->d_mine_noshare, ns.size())) || (rc = model_alloc(h, &h->h_mine_out, PBD_MAX_BATCH, true, false)) ||
      (rc = model_alloc(h, &h->d_mine_perm, cap)))
    return rc;
  HIPCHK(h, hipMemcpy(h->d_mine_noshare, ns.data(), sizeof(int) * ns.size(), hipMemcpyHostToDevice));
  return PBD_OK;
}

// behind the route's last post-stage (run_argmin_enqueue): the records' order (RAW) and the scan
int pbd_i_mine_enqueue(pbd_handle* h, const FrameRoute& r) {
  MineArgs a{};
  a.in = h->mine_in = pbd_i_route_records(h, r.final_buf, r.final_count);
  a.nframes = h->batch; a.k = h->mine_k; a.cneg = h->mine_cneg;
  pbd_i_fv_args(h, &a.fv);
  a.fv.in = a.in;
  a.noshare = h->d_mine_noshare;
  a.key = h->d_mine_key; a.perm = h->d_mine_perm; a.out = h->h_mine_out;
  if (!a.in.cf) {   // the key packs (virtual level, component, root y, root x) into 16 bits each
    if (h->nvl > 65536 || h->md.ncomponents > 65536) return fail(h, PBD_ERR_UNSUPPORTED, "mining: more than 65536 (virtual) levels or components");
    for (const Level& L : h->lv)
      if (L.cw > 65536 || L.ch > 65536) return fail(h, PBD_ERR_UNSUPPORTED, "mining: a level of more than 65536 cells a side");
    launch_qp_mine_order(a, h->stream);
  }
  launch_qp_mine_scan(a, h->stream);
  return PBD_OK;
}

#pragma GCC visibility push(default)
extern "C" {

int pbd_qp_mine_u8(pbd_qp* q, const uint8_t* im, int w, int hgt, int cn, int stride, int id, int* records, int* written, int* action) {
  if (!q || !im) return PBD_ERR_ARG;
  const int32_t ids[1] = {id};
  return mine_run(q, host_frame(im, w, hgt, cn, stride, PBD_DEPTH_8U), ids, records, written, action);
}
int pbd_qp_mine_dev_u8(pbd_qp* q, const void* d_im, int w, int hgt, int cn, int stride, int id, int* records, int* written, int* action) {
  if (!q || !d_im) return PBD_ERR_ARG;
  const int32_t ids[1] = {id};
  return mine_run(q, device_frames(d_im, 1, w, hgt, cn, stride), ids, records, written, action);
}
int pbd_qp_mine_batch_u8(pbd_qp* q, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride, const int32_t* ids,
                         int32_t* records, int32_t* written, int* action) {
  if (!q || !ims) return PBD_ERR_ARG;
  return mine_run(q, host_batch(ims, nframes, w, hgt, cn, stride), ids, records, written, action);
}
// the same from pyramid-store slots (include/pbd_c.h "pyramid store"): the store's refusals first, then mining's own
int pbd_qp_mine_stored(pbd_qp* q, pbd_pyrstore* s, int slot, int id, int* records, int* written, int* action) {
  if (!q || !s) return PBD_ERR_ARG;
  const int32_t slots[1] = {slot}, ids[1] = {id};
  StoredSource st; FrameSource src;
  int rc = pbd_i_stored_source(q->h, s, slots, 1, &st, &src);
  return rc ? rc : mine_run(q, src, ids, records, written, action);
}
int pbd_qp_mine_batch_stored(pbd_qp* q, pbd_pyrstore* s, const int32_t* slots, int nframes, const int32_t* ids, int32_t* records,
                             int32_t* written, int* action) {
  if (!q || !s || !slots) return PBD_ERR_ARG;
  StoredSource st; FrameSource src;
  int rc = pbd_i_stored_source(q->h, s, slots, nframes, &st, &src);
  return rc ? rc : mine_run(q, src, ids, records, written, action);
}

}  // extern "C"
#pragma GCC visibility pop
