// pbd_pyrstore.cpp — the pyramid store (include/pbd_c.h "pyramid store"; kernels: k_pyrstore.hip): device-resident slots that each hold
// the feature pyramid of one frame as a producer handle's front end wrote it, and the detect entries that start from a slot.  A put is
// pbd_pyramid_u8's front end on the producer (pbd_i_front_end) and one copy of the frame's block of its feature buffer; a consumer
// frame is enter_frame with a StoredSource: planned as the frame that was put, its features loaded by k_pyrstore_load, everything
// behind that the plain frame's.  The mining entries are pbd_qp_mine.cpp's, on the same source.
#include <new>
#include <string>
#include <vector>
#include "pbd_internal.hpp"

struct pbd_pyrstore {
  pbd_handle* producer = nullptr;
  int device = 0, sbin = 0, interval = 0, kind = 0, pad = 0, ts = 4;   // the signature (with PBD_FLEN)
  int nslots = 0, max_w = 0, max_h = 0;
  size_t slot_elems = 0;            // total(max_w, max_h)
  DevBufs mem;
  char* d_mem = nullptr;            // [nslots][slot_elems] of T: mem's one block
  struct Slot { int w = 0, h = 0, cn = 0, nlevels = 0; size_t total = 0; };
  std::vector<Slot> slots;
};

namespace {
size_t slot_bytes(const pbd_pyrstore* s) { return s->slot_elems * (size_t)s->ts; }
char* slot_base(const pbd_pyrstore* s, int slot) { return s->d_mem + slot_bytes(s) * (size_t)slot; }

// the first signature field in which `h` differs from the store, as "<field>: the store has <a>, the handle <b>"; empty: none does
// (the device is the caller's to test: it is refused with another code)
std::string signature_diff(const pbd_pyrstore* s, const pbd_handle* h) {
  const struct { const char* name; int a, b; } f[] = {
      {"sbin", s->sbin, h->md.sbin}, {"interval", s->interval, h->md.interval}, {"pyramid kind", s->kind, h->pyr_kind},
      {"boundary pad", s->pad, h->pad}, {"scalar bytes", s->ts, h->ts}};
  for (const auto& e : f)
    if (e.a != e.b) return std::string(e.name) + ": the store has " + std::to_string(e.a) + ", the handle " + std::to_string(e.b);
  return std::string();
}

// A put's refusals that need no plan; *total = the frame's elements, *nlevels its levels
int put_check(pbd_pyrstore* s, const int32_t* slots, int nframes, int w, int hgt, long long* total, int* nlevels) {
  pbd_handle* h = s->producer;
  for (int f = 0; f < nframes; ++f)
    if (slots[f] < 0 || slots[f] >= s->nslots) return fail(h, PBD_ERR_ARG, "pyramid store put: slot out of range");
  const std::string diff = signature_diff(s, h);
  if (!diff.empty()) return fail(h, PBD_ERR_STATE, "pyramid store put: the producer's settings no longer equal the store's signature — " + diff);
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "pyramid store put: a frame is pending on the producer: collect it first");
  if (h->in_group || h->d_gsend) return fail(h, PBD_ERR_UNSUPPORTED, "pyramid store put: pbd_group members are not supported");
  if (!h->level_set.empty() || h->opt.level_begin > 0 || h->opt.level_end > 0)
    return fail(h, PBD_ERR_UNSUPPORTED, "pyramid store put: the producer processes a subset of the levels (pbd_set_levels / level_begin..level_end)");
  if (pbd_pyrstore_layout(w, hgt, s->sbin, s->interval, s->kind, s->pad, nlevels, nullptr, total))
    return fail(h, PBD_ERR_ARG, "pyramid store put: image too small: the pyramid needs at least `interval` levels");
  if ((size_t)*total > s->slot_elems)
    return fail(h, PBD_ERR_CAPACITY, "pyramid store put: the frame's pyramid (" + std::to_string(*total) + " elements) exceeds the slot (" +
                                     std::to_string(s->slot_elems) + ": " + std::to_string(s->max_w) + " x " + std::to_string(s->max_h) + ")");
  return PBD_OK;
}

// behind the checks: the producer's front end on the frame(s), the copy of frame f's block into slots[f], the slots' records
int put_frames(pbd_pyrstore* s, const int32_t* slots, const FrameSource& src, long long total, int nlevels) {
  pbd_handle* h = s->producer;
  int rc = pbd_i_front_end(h, src);
  if (rc) return rc;
  if (h->compact)
    return fail(h, PBD_ERR_UNSUPPORTED, "pyramid store put: the producer runs the compact memory plan (dp_mode 2, or automatic for large frames and batches)");
  if (h->nlevels != nlevels || h->batch != src.nframes || h->cells * PBD_FLEN != (size_t)total * src.nframes)
    return fail(h, PBD_ERR_STATE, "internal: the producer's plan is not the store's layout of this frame");
  PyrCopyTable t{};
  for (int f = 0; f < src.nframes; ++f) {
    const size_t cell0 = h->lv[(size_t)f * nlevels].cell_off;
    t.j[f] = PyrCopyJob{h->d_feat + cell0 * PBD_FLEN * h->ts, slot_base(s, slots[f]), (unsigned long long)total * h->ts, 0};
  }
  launch_pyrstore_put(t, src.nframes, h->stream);
  LAUNCHCHK(h, "pyramid store put");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int f = 0; f < src.nframes; ++f) {
    pbd_pyrstore::Slot& S = s->slots[slots[f]];
    S.w = src.w; S.h = src.hgt; S.cn = src.cn; S.nlevels = nlevels; S.total = (size_t)total;
  }
  return PBD_OK;
}
}  // namespace

// ---- the consumer side: checks, source, job table (enter_frame) -------------------------------------------------------------------
int pbd_i_stored_source(pbd_handle* h, pbd_pyrstore* s, const int32_t* slots, int nframes, StoredSource* st, FrameSource* out) {
  if (nframes < 1 || nframes > PBD_MAX_BATCH) return fail(h, PBD_ERR_ARG, "batch: 1..64 frames");
  for (int f = 0; f < nframes; ++f)
    if (slots[f] < 0 || slots[f] >= s->nslots) return fail(h, PBD_ERR_ARG, "pyramid store: slot out of range");
  if (h->opt.device != s->device)
    return fail(h, PBD_ERR_UNSUPPORTED, "pyramid store: the store is on device " + std::to_string(s->device) + ", the handle on device " + std::to_string(h->opt.device));
  const std::string diff = signature_diff(s, h);
  if (!diff.empty()) return fail(h, PBD_ERR_ARG, "pyramid store: the handle's settings differ from the store's signature — " + diff);
  if (h->in_group || h->d_gsend) return fail(h, PBD_ERR_UNSUPPORTED, "pyramid store: pbd_group members are not supported");
  if (h->zf_on) return fail(h, PBD_ERR_UNSUPPORTED, "pyramid store: not with depth pruning on");
  if (h->b3_on) return fail(h, PBD_ERR_UNSUPPORTED, "pyramid store: not with 3-D boxes on");
  if (h->cl3_on) return fail(h, PBD_ERR_UNSUPPORTED, "pyramid store: not with object clusters on");
  const pbd_pyrstore::Slot& S0 = s->slots[slots[0]];
  for (int f = 0; f < nframes; ++f) {
    const pbd_pyrstore::Slot& S = s->slots[slots[f]];
    if (S.w == 0) return fail(h, PBD_ERR_STATE, "pyramid store: slot " + std::to_string(slots[f]) + " is empty");
    if (S.w != S0.w || S.h != S0.h || S.cn != S0.cn)
      return fail(h, PBD_ERR_ARG, "pyramid store: the slots of a batch hold frames of different sizes");
  }
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "previous frame not collected");
  *st = StoredSource{s, slots};
  *out = FrameSource{};
  out->on_device = true;
  out->nframes = nframes; out->w = S0.w; out->hgt = S0.h; out->cn = S0.cn; out->stride = S0.w * S0.cn; out->depth = PBD_DEPTH_8U;
  out->stored = st;
  return PBD_OK;
}

int pbd_i_stored_jobs(pbd_handle* h, const StoredSource& st, int nframes, PyrCopyTable* t) {
  const pbd_pyrstore* s = st.store;
  for (int f = 0; f < nframes; ++f) {
    const pbd_pyrstore::Slot& S = s->slots[st.slots[f]];
    // the consumer's plan of (w, hgt) under the shared signature is the producer's: one block of S.total elements per frame
    if (h->nlevels != S.nlevels || h->batch != nframes || h->cells * PBD_FLEN != S.total * nframes)
      return fail(h, PBD_ERR_STATE, "internal: the handle's plan is not the store's layout of this frame");
    const size_t cell0 = h->lv[(size_t)f * h->nlevels].cell_off;
    t->j[f] = PyrCopyJob{slot_base(s, st.slots[f]), h->d_feat + cell0 * PBD_FLEN * h->ts, (unsigned long long)S.total * h->ts, (unsigned long long)cell0};
  }
  return PBD_OK;
}

#pragma GCC visibility push(default)
extern "C" {

int pbd_pyrstore_create(pbd_handle* producer, int slots, int max_w, int max_h, pbd_pyrstore** out) {
  if (!out) return PBD_ERR_ARG;
  *out = nullptr;
  if (!producer) return PBD_ERR_ARG;
  pbd_handle* h = producer;
  if (slots < 1) return fail(h, PBD_ERR_ARG, "pyramid store: at least one slot");
  if (h->in_group || h->d_gsend) return fail(h, PBD_ERR_UNSUPPORTED, "pyramid store: pbd_group members are not supported");
  long long total = 0;
  int nlevels = 0;
  if (pbd_pyrstore_layout(max_w, max_h, h->md.sbin, h->md.interval, h->pyr_kind, h->pad, &nlevels, nullptr, &total) || total <= 0)
    return fail(h, PBD_ERR_ARG, "pyramid store: max_w x max_h is too small for a pyramid of the producer's interval");
  ON_DEVICE(h);
  pbd_pyrstore* s = new (std::nothrow) pbd_pyrstore();
  if (!s) return fail(h, PBD_ERR_ARG, "pyramid store: allocation failed");
  s->producer = h; s->device = h->opt.device;
  s->sbin = h->md.sbin; s->interval = h->md.interval; s->kind = h->pyr_kind; s->pad = h->pad; s->ts = h->ts;
  s->nslots = slots; s->max_w = max_w; s->max_h = max_h; s->slot_elems = (size_t)total;
  s->slots.assign((size_t)slots, pbd_pyrstore::Slot{});
  hipError_t e = s->mem.alloc(&s->d_mem, slot_bytes(s) * (size_t)slots);
  if (e != hipSuccess) {
    delete s;
    return fail(h, PBD_ERR_HIP, pbd_alloc_error("pyramid store: ", e));
  }
  *out = s;
  return PBD_OK;
}

void pbd_pyrstore_destroy(pbd_pyrstore* s) {
  if (!s) return;
  if (s->d_mem) {
    hipSetDevice(s->device);
    hipDeviceSynchronize();   // (a consumer's load may still read a slot on its own stream)
  }
  delete s;
}

int pbd_pyrstore_dims(const pbd_pyrstore* s, int* slots, int* sbin, int* interval, int* kind, int* pad, int* scalar_bytes, size_t* bytes) {
  if (!s) return PBD_ERR_ARG;
  if (slots) *slots = s->nslots;
  if (sbin) *sbin = s->sbin;
  if (interval) *interval = s->interval;
  if (kind) *kind = s->kind;
  if (pad) *pad = s->pad;
  if (scalar_bytes) *scalar_bytes = s->ts;
  if (bytes) *bytes = slot_bytes(s);
  return PBD_OK;
}

int pbd_pyrstore_slot(const pbd_pyrstore* s, int slot, int* w, int* hgt, int* cn, int* nlevels) {
  if (!s || slot < 0 || slot >= s->nslots) return PBD_ERR_ARG;
  const pbd_pyrstore::Slot& S = s->slots[slot];
  if (w) *w = S.w;
  if (hgt) *hgt = S.h;
  if (cn) *cn = S.cn;
  if (nlevels) *nlevels = S.nlevels;
  return PBD_OK;
}

int pbd_pyrstore_put_u8(pbd_pyrstore* s, int slot, const uint8_t* im, int w, int hgt, int cn, int stride) {
  if (!s || !im) return PBD_ERR_ARG;
  const int32_t slots[1] = {slot};
  long long total = 0; int nlevels = 0;
  int rc = put_check(s, slots, 1, w, hgt, &total, &nlevels);
  return rc ? rc : put_frames(s, slots, host_frame(im, w, hgt, cn, stride, PBD_DEPTH_8U), total, nlevels);
}
int pbd_pyrstore_put_dev_u8(pbd_pyrstore* s, int slot, const void* d_im, int w, int hgt, int cn, int stride) {
  if (!s || !d_im) return PBD_ERR_ARG;
  const int32_t slots[1] = {slot};
  long long total = 0; int nlevels = 0;
  int rc = put_check(s, slots, 1, w, hgt, &total, &nlevels);
  return rc ? rc : put_frames(s, slots, device_frames(d_im, 1, w, hgt, cn, stride), total, nlevels);
}
int pbd_pyrstore_put_batch_u8(pbd_pyrstore* s, const int32_t* slots, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride) {
  if (!s || !slots || !ims) return PBD_ERR_ARG;
  if (nframes < 1 || nframes > PBD_MAX_BATCH) return fail(s->producer, PBD_ERR_ARG, "batch: 1..64 frames");
  for (int f = 0; f < nframes; ++f)
    if (!ims[f]) return fail(s->producer, PBD_ERR_ARG, "null frame pointer");
  long long total = 0; int nlevels = 0;
  int rc = put_check(s, slots, nframes, w, hgt, &total, &nlevels);
  return rc ? rc : put_frames(s, slots, host_batch(ims, nframes, w, hgt, cn, stride), total, nlevels);
}

int pbd_pyrstore_get_level(pbd_pyrstore* s, int slot, int level, void* out, size_t out_bytes) {
  if (!s || !out || slot < 0 || slot >= s->nslots) return PBD_ERR_ARG;
  pbd_handle* h = s->producer;
  const pbd_pyrstore::Slot& S = s->slots[slot];
  if (S.w == 0) return fail(h, PBD_ERR_STATE, "pyramid store: slot " + std::to_string(slot) + " is empty");
  if (level < 0 || level >= S.nlevels) return fail(h, PBD_ERR_ARG, "level out of range");
  long long off[PBD_PYRSTORE_MAX_LEVELS + 1], total = 0;
  int n = 0;
  if (pbd_pyrstore_layout(S.w, S.h, s->sbin, s->interval, s->kind, s->pad, &n, off, &total)) return fail(h, PBD_ERR_STATE, "internal: the slot's frame has no layout");
  off[n] = total;
  const size_t bytes = (size_t)(off[level + 1] - off[level]) * s->ts;
  if (out_bytes < bytes) return fail(h, PBD_ERR_CAPACITY, "pbd_pyrstore_get_level: cw * ch * 32 elements of the store's scalar");
  HIPCHK(h, hipSetDevice(s->device));
  HIPCHK(h, hipMemcpy(out, slot_base(s, slot) + (size_t)off[level] * s->ts, bytes, hipMemcpyDeviceToHost));
  return PBD_OK;
}

// ---- detect from a slot: the plain entries on a stored source ----------------------------------------------------------------------
int pbd_detect_stored(pbd_handle* h, pbd_pyrstore* s, int slot, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int capacity, int* count) {
  if (!h || !s) return PBD_ERR_ARG;
  const int32_t slots[1] = {slot};
  StoredSource st; FrameSource src;
  int rc = pbd_i_stored_source(h, s, slots, 1, &st, &src);
  if (!rc) rc = enter_frame(h, src);
  return rc ? rc : pbd_detect_collect(h, heads, boxes, locs, capacity, count);
}
int pbd_detect_batch_stored(pbd_handle* h, pbd_pyrstore* s, const int32_t* slots, int nframes, pbd_candidate_head* heads, int32_t* boxes,
                            int32_t* locs, int capacity, int* counts) {
  if (!h || !s || !slots || !heads || !counts || capacity < 0) return PBD_ERR_ARG;
  StoredSource st; FrameSource src;
  int rc = pbd_i_stored_source(h, s, slots, nframes, &st, &src);
  if (!rc) rc = enter_frame(h, src);
  return rc ? rc : pbd_detect_batch_collect(h, heads, boxes, locs, capacity, counts);
}

}  // extern "C"
#pragma GCC visibility pop
