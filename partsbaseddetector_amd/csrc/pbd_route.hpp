// pbd_route.hpp — what a frame is, where its records go, and what it leaves pending: host only (no HIP include), so the CPU tests
// compile it on its own (tests/tools/route_check.cpp).
//
//   FrameJob      what the frame being enqueued is.  Built once by the entry (enter_frame, or a stage entry) and passed down by
//                 const reference.
//   FrameRoute    route_frame(settings, job): which buffer the back-tracking writes, which post-stages run and what each reads and
//                 writes, how the records reach the host, where the frame's final records are.  Buffers and counts are named by
//                 enum; the executors (run_argmin_enqueue, pbd_i_post_enqueue) map the names to the handle's pointers and launch
//                 what the route lists.  Nothing else decides any of this.
//   PendingFrame  what the collect needs to know about the frame in flight.  Part of the route; assigned whole to the handle, once
//                 per enqueue (begin_pending, pbd_api.cpp).
#pragma once
#include <stddef.h>
#include "../../include/pbd_c.h"

// Frame f's depth image (element type T) at img + f * fbytes, w x h, rows pitch bytes apart; has: frames that carry depth (bit f)
struct DepthFrames {
  const char* img; size_t pitch, fbytes; int w, h; unsigned long long has;
};

enum FrameKind {
  FRAME_PLAIN,
  FRAME_DEPTH,    // RGB-D: the depth-carrying post-stages run (z)
  FRAME_LATENT,   // masked by truth boxes, yields its best pose (its tables: pbd_i_latent_begin)
  FRAME_GTBOX,    // the selection per ground-truth box runs behind the back-tracking (its tables: pbd_i_gt_begin)
  FRAME_STAGE,    // pbd_dp_argmin / pbd_dp_argbest: the back-tracking of resident tables, no frame entry and no post-stage
  FRAME_MINE,     // pbd_qp_mine_*: the final records stay on the device for the example cache's scan and write; only a count comes back
  FRAME_LATENT_WRITE,  // pbd_qp_write_latent_*: a FRAME_LATENT whose pose stays on the device like a mining frame's records
  FRAME_EVAL      // pbd_eval_apk_frame_*: routed as a mining frame; the evaluation ledger matches the final records where they are
};
struct FrameJob {
  FrameKind kind = FRAME_PLAIN;
  DepthFrames z{};                      // FRAME_DEPTH: the depth images, on the device
  const struct PyrCopyTable* stored = nullptr;   // non-null (FRAME_PLAIN / FRAME_MINE): the frame's features come from pyramid-store slots by
                                        // this job table (k_pyrstore_load) instead of from the image pyramid and HOG; the frame runs eagerly
};

// record buffers and count blocks of the handle, by name (pbd_post.cpp: pbd_i_route_buf, pbd_i_route_count)
enum RouteBuf {
  BUF_NONE,
  HOST_OUT,       // h_cand_out: pinned, device-mapped
  DEV_OUT,        // d_cand_out
  DEV_RAW,        // d_cand_raw: the back-tracking's output in front of a post-stage that writes DEV_OUT or reads depth
  DEV_ZF,         // d_zf_out: the depth pruning's output in front of the candidate filter
  DEV_CP_STAGE    // d_cp_stage: the sorted runs in front of the part-wise NMS
};
enum RouteCount {
  CNT_NONE,
  CNT_DEV,        // d_cand_count
  CNT_DEV_ZF,     // d_zf_cnt
  CNT_HOST_CF,    // h_cf_cnt: k_cand_filter's count block, pinned
  CNT_DEV_CF,     // d_cf_cnt
  CNT_DEV_CP      // d_cp_cnt
};
inline bool route_on_host(RouteBuf b) { return b == HOST_OUT; }
inline bool route_on_host(RouteCount c) { return c == CNT_HOST_CF; }
inline bool route_cf_block(RouteCount c) { return c == CNT_HOST_CF || c == CNT_DEV_CF || c == CNT_DEV_CP; }   // a k_cand_filter count block

struct RouteStage {
  bool on;
  RouteBuf in; RouteCount in_count;
  RouteBuf out; RouteCount out_count;
};

struct PendingFrame {
  bool active = false;      // a frame is in flight (the only field anyone but begin_pending writes)
  bool on_host = false;     // every record is on the host once the stream is done: nothing to fetch beyond a first block
  bool filtered = false;    // the records went through k_cand_filter: final order, counts in the cf block
  bool gt = false;          // a gt-box frame: the collect returns the winners, not the records
  bool b3 = false, cl3 = false;   // it computes 3-D boxes (+ object clusters) ...
  unsigned long long b3_has = 0;  // ... of these frames
  bool ps = false;          // it computes per-part scores
  bool ps_compact = false;  // ... it does not because the plan is the compact one (pbd_get_part_scores names it)
  bool dp_timed = false;    // its min() recorded the DP events
};

struct RouteSettings {
  int cand_mode = PBD_CAND_RAW;      // the filter this handle runs (pbd_i_cand_mode)
  int cand_nms = PBD_NMS_PAINTED;
  bool zf_on = false, b3_on = false, cl3_on = false, ps_on = false;
  bool compact = false;              // the plan is the compact one: the raw response planes do not survive min()
  bool member = false;               // an RCCL-gathering pbd_group member (d_gsend): records stay on the device, a send block is packed
  bool zero_copy = true;             // the build's PBD_ARGMIN_ZERO_COPY
  bool ps_compact_was = false;       // what the previous frame left: a FRAME_STAGE job scores nothing and keeps it
  bool dp_timed = false;             // the min() whose tables are back-tracked recorded the DP events
};

struct FrameRoute {
  bool latent = false;               // no hit list from the threshold (+inf root threshold): the mask stage and k_latent_best's one record
  bool gt = false;                   // the gt-box selection reads bt.out; only its winners (pinned slots) and the count reach the host
  RouteStage bt{};                   // the back-tracking (in: the hit list, not a record buffer)
  bool bt_host_count = false;        // ... writes the count into h_cand_count itself, beside the pinned records
  RouteStage zf{};                   // depth pruning
  RouteStage filter{}; int filter_mode = PBD_CAND_RAW;   // k_cand_filter, and the mode it runs in
  RouteStage parts{};                // k_cand_parts behind a filter in SORT mode: writes what the filter would have written
  // how the records reach the host
  RouteCount count_d2h = CNT_NONE;   // this device count is copied into h_cand_count behind the last launch ...
  bool first_d2h = false;            // ... with the first_copy first records of DEV_OUT into HOST_OUT
  RouteCount pack_count = CNT_NONE;  // member: the send block is packed from this count and the first records of DEV_OUT
  // where the frame's final records are: what box3d, cluster3d and the part scores read
  RouteBuf final_buf = BUF_NONE; RouteCount final_count = CNT_NONE;
  PendingFrame pending;
};

// false: a combination the entries refuse (the caller answers an internal error; the entries' own messages stay theirs)
inline bool route_frame(const RouteSettings& s, const FrameJob& job, FrameRoute* out) {
  const FrameKind k = job.kind;
  const bool stage = k == FRAME_STAGE;
  const int cm = stage ? PBD_CAND_RAW : s.cand_mode;
  const bool filtered = cm != PBD_CAND_RAW;
  const bool zf = k == FRAME_DEPTH && s.zf_on;
  const bool post = zf || filtered;
  const bool latw = k == FRAME_LATENT_WRITE;
  const bool mine = k == FRAME_MINE || latw || k == FRAME_EVAL;   // the example cache (the evaluation ledger) reads the final records where they are
  const bool dev = s.member || mine;   // the final records stay in DEV_OUT
  const bool zero_copy = s.zero_copy && !dev;
  if (k == FRAME_GTBOX && (filtered || s.zf_on || s.b3_on || s.cl3_on || s.ps_on)) return false;   // pbd_i_gt_check
  if (s.member && (k == FRAME_DEPTH || k == FRAME_LATENT || k == FRAME_GTBOX || s.b3_on || s.ps_on)) return false;   // the setters and the latent / gt checks
  if (mine && (s.member || s.compact || s.zf_on || s.b3_on || s.cl3_on || s.ps_on)) return false;   // pbd_qp_mine_*'s and pbd_qp_write_latent_*'s own refusals

  FrameRoute r;
  r.latent = k == FRAME_LATENT || latw;
  r.gt = k == FRAME_GTBOX;
  r.bt.on = true;
  r.bt.out_count = CNT_DEV;
  if (r.gt) r.bt.out = DEV_OUT;
  else if (post) r.bt.out = zf || dev ? DEV_RAW : DEV_OUT;
  else if (zero_copy) { r.bt.out = HOST_OUT; r.bt_host_count = true; }
  else r.bt.out = DEV_OUT;
  const RouteStage* last = &r.bt;
  if (zf) {   // kept records straight to the host (the count follows by a copy), or in front of the filter
    r.zf = {true, last->out, last->out_count, filtered ? DEV_ZF : HOST_OUT, CNT_DEV_ZF};
    last = &r.zf;
  }
  if (filtered) {
    const bool parts = cm == PBD_CAND_SORT_NMS && s.cand_nms == PBD_NMS_PARTS;
    const RouteBuf dst = dev ? DEV_OUT : HOST_OUT;
    const RouteCount dst_count = dev ? CNT_DEV_CF : CNT_HOST_CF;
    r.filter_mode = parts ? PBD_CAND_SORT : cm;
    r.filter = {true, last->out, last->out_count, parts ? DEV_CP_STAGE : dst, parts ? CNT_DEV_CP : dst_count};
    last = &r.filter;
    if (parts) { r.parts = {true, DEV_CP_STAGE, CNT_DEV_CP, dst, dst_count}; last = &r.parts; }
  }
  r.final_buf = last->out; r.final_count = last->out_count;
  if (r.gt || mine) r.count_d2h = CNT_DEV;               // nothing of the records themselves is fetched
  else if (s.member) r.pack_count = r.final_count;
  else if (!route_on_host(r.final_buf)) { r.count_d2h = CNT_DEV; r.first_d2h = true; }
  else if (last == &r.zf) r.count_d2h = CNT_DEV_ZF;

  PendingFrame& p = r.pending;
  p.active = true;
  p.on_host = r.gt || mine || route_on_host(r.final_buf);   // (a mining frame: nothing for a collect to fetch)
  p.filtered = filtered;
  p.gt = r.gt;
  p.b3 = k == FRAME_DEPTH && s.b3_on;
  p.cl3 = p.b3 && s.cl3_on;
  p.b3_has = p.b3 ? job.z.has : 0;
  p.ps = s.ps_on && !s.compact && !stage;
  p.ps_compact = stage ? s.ps_compact_was : s.ps_on && s.compact;
  p.dp_timed = s.dp_timed;
  *out = r;
  return true;
}
