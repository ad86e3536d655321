// pbd_internal.hpp — shared declarations of libpbd_hip.so (gfx950 only).
//
// Data layout in HBM for one frame (all buffers owned by the handle, sized on
// the first frame of a given geometry and reused):
//   img      u8   source image, tightly packed w*cn
//   pyr      u8   level images back to back (level l at img_off[l])
//   feat     f32  HOG: level l at feat_off[l], [ch][cw][32]      (cell-major)
//   resp     f32  pdf: level l at resp_off[l], [nfilters][ch][cw] (plane-major)
//   acc      f32  accumulated part scores: level l at acc_off[l], [nslots][ch][cw]
//   ptrk     u8   DP best child mixture Ik: level l at cell_off[l]*nplanes, [nplanes][ch][cw]
//                 (Ix / Iy are composed at back-tracking time from the DT pointer planes dt_ixT / dt_iy)
//   rootv/i  f32/i32  level l at root_off[l], [ncomp][ch][cw]
//   dt_*          per-round scratch of the distance transform
//   cand          device candidate list (count + records)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/pbd_c.h"

#include "pbd_plan.hpp"
#include "pbd_lds.hpp"
#include "pbd_route.hpp"
#include "pbd_mem.hpp"

#ifndef PBD_ARGMIN_ZERO_COPY
#define PBD_ARGMIN_ZERO_COPY 1   // k_backtrack writes candidates straight to the pinned host buffers (handles outside RCCL groups)
#endif
#ifndef PBD_DT_PRIO
#define PBD_DT_PRIO 1            // s_setprio of k_dt_pass's wavefronts (k_dp.hip)
#endif
#ifndef PBD_DT_TASK_PREFETCH
#define PBD_DT_TASK_PREFETCH 256 // k_dt_pass touches the task descriptor this many blocks ahead (k_dp.hip; 0: off)
#endif

struct CandRec { int level, comp, y, x; };

// ---- latent detection (k_latent.hip; include/pbd_c.h "latent detection") ------------------------------------------------------
// One response plane of the mask stage: mixture `mix` of part `part` (local index) of component `comp` at (virtual) level `level`.
struct LatJob {
  void* plane;                   // T [H][W]: the resident response plane, masked in place
  int H, W, level, comp, part, mix;
  int rows;                      // rows of the mixture's filter: the window is rows x rows scaled (k_backtrack's size quirk)
  int flag;                      // index of the (level, component, part) "has an admissible cell" flag
  float scale; int pad;
};
static_assert(sizeof(LatJob) == 48, "LatJob layout");
struct LatPartial { double v; unsigned long long key; };   // a block's best root: score, (level * ncomp + comp) << 32 | cell; key ~0: none
struct LatentMaskArgs {
  const LatJob* jobs; const struct ReduceBlock* blocks;
  const int* truth; const int* mix;   // [frames][max_parts][4]; [frames][max_parts] or null
  int* flags;
  int nlevels, mp, component, org;    // nlevels: levels of ONE frame; org = 1 + boundary pad
  double overlap;
};
struct LatentBestArgs {
  const struct RootJob* jobs; const struct ReduceBlock* blocks; int nblocks;
  const int* flags; const int* nparts;
  int ncomp, mp, nlevels, nframes;
  LatPartial* partial;                // [nblocks]
  int* count; CandRec* rec;           // what k_backtrack consumes: one record per frame that has a pose
};
// one latent frame or batch: a truth set (and mixture set) per frame
struct LatentSource { const int32_t* truth; const int32_t* mix; int component; double overlap; };

// ---- what every post-stage kernel reads (k_cand / k_zfilter / k_box3d / k_cluster3d / k_partscore) ------------------------
// A record is a pbd_candidate_head, then mp * 4 box ints, then mp * 3 loc ints (pbd_rec_bytes).
// The records of a frame or a batch: `count` (device) records at p (count > capacity: the back-tracking overflowed).
struct RecordSet {
  const char* p; size_t stride; int mp;
  const int* count; int capacity;
  const int* cf; int nframes;   // non-null: k_cand_filter's counts; frame f's records at [cf[2+nf+f], +cf[2+f])
  int nlevels;                  // else frame of a record = level / nlevels (0: one frame)
};
#ifdef __HIPCC__
// the frame record i belongs to; -1: none (filtered output beyond every frame's kept records)
__device__ __forceinline__ int record_frame(const RecordSet& r, int i) {
  if (r.cf) {   // filtered output: frame f's records sit at [start_f, start_f + kept_f)
    for (int k = 0; k < r.nframes; ++k)
      if (i >= r.cf[2 + r.nframes + k] && i < r.cf[2 + r.nframes + k] + r.cf[2 + k]) return k;
    return -1;
  }
  return r.nlevels ? ((const pbd_candidate_head*)(r.p + r.stride * (size_t)i))->level / r.nlevels : 0;
}
#endif

// ---- best pose per ground-truth box (k_gtbox.hip; include/pbd_c.h "best pose per ground-truth box") ---------------------------
#define PBD_GT_BLOCK 256                             // threads of a block of either kernel
#define PBD_GT_GRID 64                               // blocks of k_gtbox_centres
#define PBD_GT_SPAN (PBD_GT_GRID * PBD_GT_BLOCK)     // records one pass of its grid covers
struct GtBoxArgs {
  RecordSet in;                 // (cf unused)  nlevels 0: one frame, ties go to the input position; else to (level, component, root y, root x)
  int nframes;
  const double* gt; const int* ngt; double overlap;   // [nframes][PBD_GT_MAX][4] (x1, y1, x2, y2); [nframes]
  double4* cbox; unsigned* key; unsigned long long* rank; int* frame;   // [capacity] each: k_gtbox_centres' planes
  char* out;                    // [nframes * PBD_GT_MAX] record slots: the winners' records (null: none wanted)
  int* found; double* o;        // [nframes * PBD_GT_MAX]
  int* best;                    // [nframes * PBD_GT_MAX] the winner's index in `in`, -1: none (null: not wanted)
};
// one gt-box frame or batch: the boxes of every frame, PBD_GT_MAX slots per frame
struct GtSource { const double* gt; const int* ngt; double overlap; };

// object clusters (k_cluster3d.hip): one record's result in the slot of its record
struct Cl3Res { pbd_cluster3d r; long long off; };   // off: the kept cluster's indices in the pool; -1: they did not fit

struct Cluster3dArgs {
  RecordSet in;
  DepthFrames z; size_t pstride;              // the xyz cloud (points pstride bytes apart), or the depth image (the pinhole model)
  const int* list; int nlist;                 // non-null: only these (record, frame) pairs
  const pbd_box3d* boxes;                     // [capacity] by record
  pbd_camera cam;                             // depth source: the pinhole model
  float tol;
  char* scratch; size_t slot_bytes; int pcap; // one slot of pcap points per workgroup
  Cl3Res* out;                                // [capacity]
  int* pool; unsigned long long pool_cap; unsigned long long* pool_used;
};

struct pbd_handle : HostModel {   // the model (pbd_plan.hpp: validated description, part topology, filter-bank mode)
  std::vector<char> level_set;   // pbd_set_levels: levels this handle processes (empty = all), intersected with [level_begin, level_end)
  std::string err;
  PlanKnobs knobs;               // probe / tune builds: the planner's environment knobs, read at creation

  // device model
  void* d_wT = nullptr;      // T [kh*kw][flen][nfpad] filters transposed (and converted to T) for the conv kernels
  int ncu = 256;
  int nfpad = 0;
  float* d_biasw = nullptr;
  uint8_t* d_hog_lut = nullptr;   // orientation-snap table of HOGFeatures<T>::features (src/HOGFeatures.cpp:243-249), built once per handle on the device
  int* d_parent = nullptr;   // [ncomp][max_parts] parent of each part
  int* d_plane0 = nullptr;   // [ncomp][max_parts] local plane0 of each part
  int* d_nparts = nullptr;
  int* d_mix_rows = nullptr; // [nflat parts][PBD_MAX_MIX] rows of the filter of each mixture (k_backtrack's box size)

  // frame plan
  int fw = 0, fh = 0, fcn = 0, nlevels = 0;     // nlevels: levels of ONE frame
  int dt_geom = 0;                               // distance-transform block geometry of float handles: 0 = the measured rule (plan_frame), 1 = 256 lanes / 40 KB, 2 = 128 lanes / 25 KB (pbd_tune_plan)
  int fdepth = 0, fesz = 1;                      // depth of the planned frame's pixels (PBD_DEPTH_*: cv::Mat::depth()), bytes per element
  int ldepth = 0, lesz = 1;                      // the same of the plan's LEVEL images: the frame's, or PBD_DEPTH_64F under PBD_PYRAMID_MATLAB
  // A batch of B same-sized frames is planned as B x nlevels "virtual levels" (frame f's level l = f * nlevels + l):
  // every stage is driven by per-level tables, so one launch of a stage then covers all frames of the batch — four
  // times the blocks per launch, the thin rounds of the DP fill the chip and launch tails are paid once per batch.
  int batch = 1, nvl = 0;                       // frames per plan, virtual levels = batch * nlevels
  std::vector<Level> lv;                        // [nvl]
  PyrJob* d_pyrjobs = nullptr;                  // resize jobs, then the pyrDown jobs octave by octave
  std::vector<PyrLaunch> pyr_launches;          // [0]: resize, [1..]: pyrDown octave steps
  MatJob* d_matjobs = nullptr; MatRun* d_matruns = nullptr; MatTap* d_mattaps = nullptr;   // PBD_PYRAMID_MATLAB: the jobs pyr_launches index, the resize's tap lists
  size_t cells = 0, pyr_bytes = 0;
  bool have_pyr = false, have_feat = false, have_resp = false, have_dp = false;
  // Compact memory plan only: the DP reuses the feature / response memory, so after min() every plane is stale until it
  // is produced (pyramid / pdf) or handed in (pbd_set_level_*) again: have_feat / have_resp are true only when ALL are.
  std::vector<char> feat_ok, resp_ok;            // [level], [level * nfilters + filter]
  // tables handed in by the caller with no min() of this handle behind them: back-tracking needs every plane and every
  // root table of the active levels before it may run
  bool min_ran = false;                          // this plan's tables (Ik, DT pointer planes, roots) come from run_dp_min
  // Fold plans: min() does not store the Ik planes.  While ik_lazy, the tables are this handle's own and the children's kept scores
  // they are a function of are intact: back-tracking picks Ik from those (k_backtrack), and whoever needs the PLANES — a getter, the
  // stage entry pbd_dp_min, a caller's tables or a response plane about to go on top — has them written first (ensure_ik, pbd_api.cpp).
  bool ik_lazy = false;
  std::vector<char> ext_set, root_set;           // [level * nplanes + plane], [level * ncomp + comp]

  // device frame buffers
  uint8_t* d_img = nullptr; size_t img_cap = 0;
  uint8_t* d_pyr = nullptr;
  char* d_feat = nullptr; char* d_resp = nullptr; char* d_acc = nullptr;   // T data, addressed in bytes (elements * ts)
  uint16_t* d_feat_split = nullptr;   // PBD_CONV_SPLIT: the features as [cell][3 splits][32 channels] bfloat16 (per frame plan)
  bool feat_split_ok = false;         // ... written by k_hog for the features now in d_feat (false: handed in by the caller -> k_feat_split before the bank)
  float* d_split_oscale = nullptr;    // PBD_CONV_SPLIT_F16: [filter] 2^-(12 + e), the responses' scale (e: the filter's weight exponent)
  uint16_t* d_wS = nullptr;           // PBD_CONV_SPLIT: the filters as [tap][2 k-steps][3 splits][n-tile][2 k-groups][32][8] bfloat16 (per model)
  uint8_t* d_pk = nullptr;
  unsigned long long* d_scr_base = nullptr;   // [nlevels][nflat parts] element offset of mixture 0's DT planes (ix / iy / sdt)
  unsigned long long* d_pick = nullptr;       // fold plans, [nvl][nflat parts]: FrameTables::pick
  ReduceBlock* d_ik_blocks = nullptr; unsigned* d_ik_cells = nullptr; int n_ik_blocks = 0;   // k_ik_fill's work table (frame plan)
  std::vector<unsigned long long> scr_base;   // host copy (pbd_get_dp_pointers)
  int* d_flat = nullptr;     // [ncomp][max_parts] flat part index
  int* d_depth = nullptr;    // [ncomp][max_parts] depth of each part in its tree (root = 0)
  int max_depth = 0;
  char* d_rootv = nullptr; int* d_rooti = nullptr;
  char* d_dt_tmpT = nullptr; char* d_dt_sdt = nullptr; void* d_dt_ixT = nullptr; void* d_dt_iy = nullptr; int dt_ptr_bytes = 2;   // the DT pointer planes: dt_ptr_bytes per element (FrameLayout::ptr_bytes)
  size_t dt_cap_elems = 0;
  LevelDev* d_levels = nullptr;
  // boundary padding (pbd_set_boundary_pad; HostModel::pad): k_hog's view of the levels (padded pitch, the interior's first cell; d_levels
  // itself without padding) and the border ring's work table (k_featpad.hip)
  LevelDev* d_hog_levels = nullptr;
  PadJob* d_padjobs = nullptr; ReduceBlock* d_padblocks = nullptr; int n_padblocks = 0;
  HogTile* d_hog_tiles = nullptr; int n_hog_tiles = 0; int hog_tc = 16;
  ConvTile* d_conv_tiles = nullptr; int n_conv_tiles = 0;
  ConvTile* d_conv_tiles_mix = nullptr;   // mixed banks: [group][n_conv_tiles], pad = n0 | (nf_g << 16)
  // DP tables (all rounds back to back)
  DtMap* d_dtmaps = nullptr; DtTask* d_dttasks = nullptr;   // a task carries its group descriptor
  ReduceJob* d_redjobs = nullptr; ReduceBlock* d_redblocks = nullptr; RootJob* d_rootjobs = nullptr; BackLevel* d_back = nullptr;
  size_t dt_lds = 0;                                 // LDS budget of a k_dt_pass block (plan_tables; a launch may take more to be resident at once)
  bool compact = false;                              // memory plan of the current frame geometry (plan_frame)
  FoldJob* d_foldjobs = nullptr;
  unsigned long long* d_foldx = nullptr;             // per fold x task, in task order: the part's raw plane pointers [8] + the first child's plane pointers [8] + its Ik base + the number of children: what
                                                     // the block's loader needs for its first loads, at an address that depends on blockIdx only (k_dt_pass fetches it beside the
                                                     // task descriptor instead of behind it)
  int dt_nt = PBD_DT_NT_DEFAULT;                                   // lanes of a k_dt_pass block (64 or 128)
  std::vector<RoundLaunch> rl;
  int n_rootjobs = 0; unsigned root_cells = 0, root_maxcells = 0;
  uint8_t* d_nms_mask = nullptr;  // [cells * ncomponents]: local maxima of the root planes (same element offsets as d_rootv)
  ReduceBlock* d_rootblocks = nullptr; int n_rootblocks = 0;   // k_root: one 256-thread block per 256 cells of a root job
  // candidates
  int* d_cand_count = nullptr; CandRec* d_cand_rec = nullptr;
  char* d_cand_out = nullptr; char* h_cand_out = nullptr; int* h_cand_count = nullptr;
  size_t cand_stride = 0;
  PendingFrame pf;           // the frame in flight (pbd_route.hpp): assigned whole by begin_pending (pbd_api.cpp), once per enqueue; everyone else flips pf.active
  int first_copy = 0;        // candidate records copied back together with the count (records): starts at PBD_FIRST_COPY per frame of the
                             // plan and grows to 1.25 x the largest count seen, so that the steady state is ONE D2H and no second sync
  char* d_gsend = nullptr;   // set by an RCCL-gathering pbd_group: {count, pad to 16 B, first records} block sent by ncclAllGather

  hipStream_t stream = nullptr;
  bool own_stream = false;
  bool profiling = false;
  hipEvent_t ev[8] = {};
  float stage_ms[6] = {0, 0, 0, 0, 0, 0};
  float warp_ms[3] = {0, 0, 0};      // the last warped-positives call while profiling: resample passes, HOG, write (pbd_debug_warp_ms)
  hipEvent_t ev_dp0 = nullptr, ev_dp1 = nullptr;
  double dp_ms_sum = 0; int dp_frames = 0; bool dp_timer_on = true; bool min_timed = false;   // DP events are recorded only while profiling; min_timed: the last min() recorded them
  hipGraphExec_t gexec = nullptr;   // pbd_options.graph: the frame's launches, captured once per geometry
  int frames_on_plan = 0;           // frames enqueued since the last plan_frame
  // device memory held for the frame plan (dev_alloc: everything freed on re-plan) and for the model (model_alloc: the uploaded model
  // and the post-stages' buffers, held until pbd_destroy); pbd_get_footprint reads their bytes()
  DevBufs frame_allocs, model_allocs;
  // pointer tables handed in by the caller (pbd_set_dp_pointers: a DynamicProgram::argmin fed tables that this handle's
  // min() did not produce): composed Ix / Iy per (level, component, plane), allocated on first use; back-tracking
  // reads them instead of the DT planes until the next min()
  int16_t* d_extx = nullptr; int16_t* d_exty = nullptr; unsigned long long* d_ext_base = nullptr;
  bool ext_ptr = false;
  bool root_dirty = false;   // pbd_set_root since the last min(): argmin re-thresholds the root tables first
  // candidate filter (pbd_set_candidate_filter): Candidate::sort (+ nonMaximaSuppression) by k_cand_filter behind k_backtrack
  int cand_mode = PBD_CAND_RAW; float cand_overlap = 0.f;
  bool in_group = false;     // member of a pbd_group: the group sets the filter
  bool cand_defer = false;   // member of a level-sharded pbd_group_detect_u8: unfiltered, the group filters the union on member 0
  char* d_cand_raw = nullptr;                           // back-tracking output of RCCL-gathering members when filtering
  unsigned long long* d_cf_keys = nullptr; unsigned* d_cf_idx = nullptr; int* d_cf_box = nullptr; uint8_t* d_cf_st = nullptr;
  // k_cand_filter's counts, B = frames of the plan: [0] the back-tracking's device count (all frames, before the filter), [1] kept in frame 0
  // (the device count when that overflowed the capacity: nothing is kept then), [2 + f] kept in frame f, [2 + B + f] frame f's first record.
  // A single-frame collect finds [1] records (pbd_i_found), a batch collect fetches for [0] and splits by [2 + f] / [2 + B + f].
  int* d_cf_cnt = nullptr; int* h_cf_cnt = nullptr;    // [2 + 2 * PBD_MAX_BATCH]; h_: pinned
  unsigned long long* d_cf_mask = nullptr; size_t cf_mask_bytes = 0;   // per-frame masks too large for LDS (frame plan)
  // what the NMS of PBD_CAND_SORT_NMS is (pbd_set_candidate_nms): the painted mask above, or the part-wise rule of nms.m by
  // k_cand_parts behind k_cand_filter in SORT mode, which then writes into d_cp_stage / d_cp_cnt.  Allocated on first use.
  int cand_nms = PBD_NMS_PAINTED; int cand_top = 0;
  char* d_cp_stage = nullptr; int* d_cp_cnt = nullptr;
  int4* d_cp_rect = nullptr; int* d_cp_np = nullptr; unsigned* d_cp_kept = nullptr; unsigned long long* d_cp_bits = nullptr;
  // depth-consistency pruning (pbd_set_depth_filter): k_zfilter.hip behind k_backtrack.  Named z* / zf*: d_depth and max_depth
  // above are the part tree's depth.  Allocated on the first depth-carrying frame with the setting on.
  bool zf_on = false; float zf_factor = 0.f;
  int* d_zf_npart = nullptr; int* d_zf_par = nullptr; double* d_zf_thr = nullptr; float zf_thr_factor = 0.f;   // [ncomp], [ncomp * mp] x 2
  unsigned long long* d_zf_med = nullptr; unsigned* d_zf_large = nullptr;   // [capacity * mp] each
  int* d_zf_cnt = nullptr;          // [0] kept records, [1] boxes listed for k_zmed_large
  char* d_zf_out = nullptr;         // kept records in front of k_cand_filter
  char* d_zimg = nullptr; size_t zimg_bytes = 0;   // host depth images, uploaded
  // 3-D boxes (pbd_set_box3d): k_box3d.hip behind the depth pruning and the candidate filter of depth-carrying frames.  Results
  // land in pinned host buffers indexed by record slot; the collect reorders them like the records it returns.
  bool b3_on = false; pbd_camera b3_cam{};
  pbd_box3d* h_b3 = nullptr; double* h_b3c = nullptr;   // [capacity], [capacity * mp * 3]: pinned
  bool b3_ready = false;            // results of the last collected frame, per frame in the order returned
  std::vector<std::vector<pbd_box3d>> b3_res; std::vector<std::vector<double>> b3_cen; std::vector<char> b3_res_on;
  // object clusters (pbd_set_cluster3d): k_cluster3d.hip right behind k_box3d.  Results per record slot (pinned); the kept
  // clusters' indices in a device pool claimed per record, gathered (and overflowing records run again) by the collect.
  bool cl3_on = false; float cl3_tol = 0.01f;
  Cl3Res* h_cl3 = nullptr;           // [capacity]: pinned
  char* d_cl3_scratch = nullptr; int cl3_slots = 0, cl3_pcap = 0;
  int* d_cl3_pool = nullptr; unsigned long long cl3_pool_cap = 0; unsigned long long* d_cl3_used = nullptr;
  Cluster3dArgs cl3_args{};         // the pending frame's launch (the collect runs overflowing records again with it)
  bool cl3_ready = false;           // results of the last collected frame, per frame in the order returned
  std::vector<std::vector<int>> cl3_slot;   // [frame] the record slots in the order returned
  std::vector<std::vector<pbd_cluster3d>> cl3_res; std::vector<std::vector<int32_t>> cl3_idx; std::vector<char> cl3_res_on;
  // per-part scores (pbd_set_part_scores): k_partscore.hip behind the depth pruning and the candidate filter of EVERY frame (plain
  // and depth-carrying, eager and captured).  Results per record slot (pinned); the collect reorders them like the records.
  bool ps_on = false;
  struct PsMix* d_ps_mix = nullptr; int* d_ps_mix0 = nullptr;   // [flat mixtures], [flat parts + 1]: the model tables of k_partscore
  double* h_ps = nullptr;           // [capacity * mp * 3]: pinned
  bool ps_ready = false;            // results of the last collected frame, per frame in the order returned
  std::vector<std::vector<double>> ps_res; std::vector<char> ps_res_on;
  // feature vectors (pbd_candidates_features*): k_featvec.hip, stand-alone only.  The model table beside k_partscore's, the uploaded
  // records of a call and the host variants' staging buffer: allocated on first use, held until pbd_destroy
  struct FvMix* d_fv_mix = nullptr;                // [flat mixtures]
  char* d_fv_rec = nullptr; size_t fv_rec_cap = 0; // the call's records (bytes)
  char* d_fv_stage = nullptr;                      // PBD_FEATVEC_STAGING_BYTES: a chunk's blocks, then its windows
  // latent detection (pbd_latent_mask / pbd_dp_argbest / pbd_detect_latent_*): k_latent.hip between pdf and min, and in front of the
  // back-tracking.  The work table, the flags and the block partials belong to the frame plan (built on the first latent use of a
  // plan); the truth / mixture tables are model-lifetime buffers, uploaded per frame in the frame's stream.
  bool lat_masked = false;          // the resident responses carry a mask and d_lat_flags its flags (until responses are produced again)
  int lat_component = -1; double lat_overlap = 0.0; bool lat_has_mix = false;
  LatJob* d_lat_jobs = nullptr; ReduceBlock* d_lat_blocks = nullptr; int n_lat_blocks = 0;
  int* d_lat_flags = nullptr; LatPartial* d_lat_partial = nullptr;
  int* d_lat_truth = nullptr; int* h_lat_truth = nullptr;   // [PBD_MAX_BATCH][max_parts][5]: 4 box ints per part of every frame, then the mixtures; h_: pinned
  // best pose per ground-truth box (pbd_detect_gtbox_*): k_gtbox.hip behind k_backtrack, which then writes into d_cand_out.  The planes
  // and the tables are model-lifetime buffers (first use); the winners' records, found and o land in pinned memory, slot f * PBD_GT_MAX + g.
  int gt_max = 0; double gt_overlap = 0.0;   // the largest ngt of the frame's or batch's frames
  double4* d_gt_cbox = nullptr; unsigned* d_gt_key = nullptr; unsigned long long* d_gt_rank = nullptr; int* d_gt_frame = nullptr;   // [capacity]
  double* d_gt = nullptr; double* h_gt = nullptr;   // [PBD_MAX_BATCH][PBD_GT_MAX][4], then the frames' ngt as ints; h_: pinned staging
  char* h_gt_out = nullptr; int* h_gt_found = nullptr; double* h_gt_o = nullptr;   // [PBD_MAX_BATCH * PBD_GT_MAX] slots: pinned
  // hard-negative mining (pbd_qp_mine_*): k_qp_mine.hip behind the back-tracking and the candidate filter, whose records stay in
  // d_cand_out.  Model-lifetime buffers (first use): the records' order, the per-component "no two parts can
  // share an id" flags, the frames' ids and the pinned block the scan answers in.
  unsigned long long* d_mine_key = nullptr; int* d_mine_perm = nullptr;   // [capacity] each
  int* d_mine_ids = nullptr; int* h_mine_ids = nullptr;                   // [PBD_MAX_BATCH] each; h_: pinned staging
  int* d_mine_noshare = nullptr;                                           // [ncomp]
  struct MineFrameOut* h_mine_out = nullptr;                               // [PBD_MAX_BATCH]: pinned
  int mine_k = 0; double mine_cneg = 0.0;   // the calling cache's column length and C, for the scan of the frame being enqueued
  RecordSet mine_in{};                      // where that frame's final records are (its route's final_buf / final_count)
  // latent positives (pbd_qp_write_latent_*): k_qp_latent.hip behind a latent frame's back-tracking; it shares mining's order, ids and
  // noshare buffers and mine_k / mine_in, and answers in a pinned block of its own
  struct LatentWriteOut* h_latw_out = nullptr;                             // [PBD_MAX_BATCH]: pinned
  // evaluation frames (pbd_eval_apk_frame_*): k_eval_span behind the route's last post-stage; they share mining's order buffers and
  // mine_in, and answer in a pinned block of their own
  struct EvalFrameOut* h_eval_out = nullptr;                               // [PBD_MAX_BATCH]: pinned
};
#define PBD_MAX_BATCH 64

// ---- host error plumbing shared by pbd_api.cpp, pbd_post.cpp ---------------------------
#define HIPCHK(h, call)                                                                  \
  do {                                                                                   \
    hipError_t e_ = (call);                                                              \
    if (e_ != hipSuccess) {                                                              \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                      \
      return PBD_ERR_HIP;                                                                \
    }                                                                                    \
  } while (0)

static inline int fail(pbd_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

// Kernel launches return nothing: a launch the runtime rejected (wrong current device, a dynamic-LDS request over
// the opt-in, a bad grid) would otherwise leave the previous frame's buffers in place and detect() would return
// stale candidates with PBD_OK.  Checked after every stage.
#define LAUNCHCHK(h, what)                                                               \
  do {                                                                                   \
    hipError_t e_ = hipGetLastError();                                                   \
    if (e_ != hipSuccess) {                                                              \
      (h)->err = std::string(what) + ": kernel launch failed: " + hipGetErrorString(e_); \
      return PBD_ERR_HIP;                                                                \
    }                                                                                    \
  } while (0)
// hipGetLastError() is the calling THREAD's sticky last error: an unrelated HIP call of the caller that failed
// earlier (or one of ours whose result was deliberately ignored) would be reported as this frame's launch failure.
// Every entry point that launches clears it first, so LAUNCHCHK only ever sees the library's own launches.
#define CLEAR_STICKY() ((void)hipGetLastError())
// every ABI entry that launches or copies runs on the handle's device, whatever the caller's current device is
#define ON_DEVICE(h) do { HIPCHK(h, hipSetDevice((h)->opt.device)); CLEAR_STICKY(); } while (0)

// a captured frame's launches point at the buffers and settings they were captured with: dropped when either changes
static inline void drop_graph(pbd_handle* h) {
  if (h->gexec) { hipGraphExecDestroy(h->gexec); h->gexec = nullptr; }
}

// ---- candidate records ---------------------------------------------------------
inline size_t pbd_rec_bytes(int mp) { return sizeof(pbd_candidate_head) + (size_t)mp * 28; }
inline const int32_t* pbd_rec_locs(const char* r, int mp) { return (const int32_t*)(r + sizeof(pbd_candidate_head)) + (size_t)mp * 4; }
// element i of the caller's heads / boxes / locs -> record r, and back; a null array is skipped
inline void pbd_rec_put(char* r, int mp, const pbd_candidate_head* heads, const int32_t* boxes, const int32_t* locs, size_t i) {
  if (heads) memcpy(r, heads + i, sizeof(pbd_candidate_head));
  if (boxes) memcpy(r + sizeof(pbd_candidate_head), boxes + i * mp * 4, sizeof(int32_t) * mp * 4);
  if (locs) memcpy((char*)pbd_rec_locs(r, mp), locs + i * mp * 3, sizeof(int32_t) * mp * 3);
}
inline void pbd_rec_get(const char* r, int mp, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, size_t i) {
  if (heads) memcpy(heads + i, r, sizeof(pbd_candidate_head));
  if (boxes) memcpy(boxes + i * mp * 4, r + sizeof(pbd_candidate_head), sizeof(int32_t) * mp * 4);
  if (locs) memcpy(locs + i * mp * 3, pbd_rec_locs(r, mp), sizeof(int32_t) * mp * 3);
}
// stable in-place compaction of the caller's arrays: element i stays when keep[i]; returns how many stayed
inline int pbd_rec_compact(pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int count, int mp, const uint8_t* keep) {
  std::vector<char> r(pbd_rec_bytes(mp));
  int k = 0;
  for (int i = 0; i < count; ++i)
    if (keep[i]) { pbd_rec_put(r.data(), mp, heads, boxes, locs, i); pbd_rec_get(r.data(), mp, heads, boxes, locs, k++); }
  return k;
}

// ---- scalar helpers: the reference's std:: overloads resolve on T ---------------
#ifdef __HIPCC__
__device__ __forceinline__ float t_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double t_sqrt(double v) { return sqrt(v); }
__device__ __forceinline__ float t_floor(float v) { return floorf(v); }
__device__ __forceinline__ double t_floor(double v) { return floor(v); }
__device__ __forceinline__ float t_fmin(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double t_fmin(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ int t_round(float v) { return __float2int_rn(v); }    // cvRound: half to even
__device__ __forceinline__ int t_round(double v) { return __double2int_rn(v); }
#endif

// ---- dynamic-LDS opt-in --------------------------------------------------------
// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of a kernel: a process that drives several
// GPUs (pbd_group, or handles created with different pbd_options.device) must set it on each of them.  One
// instance per kernel instantiation; remembers the largest size every device has been given.
#include <mutex>
struct LdsOptIn {
  std::mutex mu;
  size_t cfg[64] = {};
  hipError_t ensure(const void* fn, size_t lds) {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) d = 0;
    std::lock_guard<std::mutex> g(mu);
    if (lds <= cfg[d] && cfg[d]) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) cfg[d] = lds;
    return e;
  }
};

// ---- probes ----------------------------------------------------------------------
// Per-phase wall-clock stamps and the environment tuning knobs are compiled only into the probe build
// (make probes -> libpbd_hip_probes.so, -DPBD_PROBES), which tests/tools_*.py load; the product library carries
// neither (the pbd_debug_* entry points then return PBD_ERR_UNSUPPORTED).
#if defined(PBD_PROBES) || defined(PBD_TUNE)
#define PBD_PROBE_ENV(name) getenv(name)
#else
#define PBD_PROBE_ENV(name) ((const char*)nullptr)
#endif

// ---- frame entry and collect (pbd_detect.cpp), shared with pbd_api.cpp -----------------------------------
// Where a frame or a batch of same-sized frames comes from: host frames are uploaded into the plan's image buffer, device frames read in place
struct DepthSource {              // the depth images of an RGB-D frame or batch (elements of the handle's T)
  bool on_device;                 // read in place, else ONE host image, uploaded
  const void* p; int type;        // PBD_DEPTH_*
  long long stride; size_t fbytes;   // bytes between rows, and between the frames' images of a packed device buffer (0: one frame)
  unsigned long long has;         // frames that carry depth (bit f)
};
struct FrameSource {
  bool on_device;
  const void* one;                // a single frame, or a device batch: one packed buffer, frame after frame
  const uint8_t* const* each;     // or (host batches) a pointer per frame
  int nframes, w, hgt, cn, stride, depth;   // stride: bytes between rows; depth: PBD_DEPTH_* of the pixels
  const DepthSource* z;           // RGB-D: the frame runs with the depth-carrying post-stages; else null
  const LatentSource* lat;        // latent detection: the frame is masked by these boxes and yields its best pose; else null
  const GtSource* gt;             // best pose per ground-truth box: the selection runs behind the back-tracking; else null
  bool mine;                      // hard-negative mining (pbd_qp_mine_*): the final records stay on the device
  bool lat_write;                 // latent positives (pbd_qp_write_latent_*; with lat): the frame's pose stays on the device
  bool eval;                      // an APK evaluation frame (pbd_eval_apk_frame_*): the final records stay on the device like a mining frame's
  const struct StoredSource* stored;   // pyramid store (pbd_detect_stored, pbd_qp_mine_stored): no image — frame f's features are slot slots[f]'s; else null
};
// ---- pyramid store (pbd_pyrstore.cpp, k_pyrstore.hip; include/pbd_c.h "pyramid store") ------------------------------------------
// One streaming copy of `bytes` bytes (a multiple of 128: whole cells of 32 elements), 16-byte aligned at both ends; dst_cell: the
// destination's first cell in the consumer's feature buffer (the split parts' index; the put does not read it)
struct PyrCopyJob { const char* src; char* dst; unsigned long long bytes, dst_cell; };
struct PyrCopyTable { PyrCopyJob j[64]; };   // by value in the kernel's arguments: one job per frame of a batch (PBD_MAX_BATCH)
static_assert(sizeof(PyrCopyJob) == 32 && sizeof(PyrCopyTable) == 2048, "PyrCopyTable layout");
struct StoredSource { const struct pbd_pyrstore* store; const int32_t* slots; };
// enter_frame, on the planned frame: the job table of a stored source (slot f -> the block of frame f's virtual levels); refuses a plan
// whose per-frame block is not the slot's
int pbd_i_stored_jobs(pbd_handle* h, const StoredSource& s, int nframes, PyrCopyTable* t);
// every refusal of a consumer entry that needs no plan, then the source of the frame(s): *st and *out stay the caller's (enter_frame reads them)
int pbd_i_stored_source(pbd_handle* h, struct pbd_pyrstore* s, const int32_t* slots, int nframes, StoredSource* st, FrameSource* out);
// the producer's front end of a put (pbd_api.cpp): enter_frame(.., false), the image pyramid and HOG (+ ring), enqueued on its stream
int pbd_i_front_end(pbd_handle* h, const FrameSource& s);
// njobs jobs, one launch.  load: into feat (the jobs' dst) and, split_parts = 3 / 2, the bank's bfloat16 / binary16 parts of the same
// elements into split ([cell][part][32]) in the same pass; put: the copy alone
void launch_pyrstore_load(const PyrCopyTable& t, int njobs, uint16_t* split, int split_parts, hipStream_t s);
void launch_pyrstore_put(const PyrCopyTable& t, int njobs, hipStream_t s);
// the three shapes of a source, by name (z: see above)
inline FrameSource host_frame(const void* im, int w, int hgt, int cn, int stride, int depth, const DepthSource* z = nullptr) {
  return {false, im, nullptr, 1, w, hgt, cn, stride, depth, z};
}
inline FrameSource host_batch(const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride, const DepthSource* z = nullptr) {
  return {false, nullptr, ims, nframes, w, hgt, cn, stride, PBD_DEPTH_8U, z};
}
inline FrameSource device_frames(const void* d_ims, int nframes, int w, int hgt, int cn, int stride, const DepthSource* z = nullptr) {
  return {true, d_ims, nullptr, nframes, w, hgt, cn, stride, PBD_DEPTH_8U, z};
}
inline DepthSource depth_images(bool on_device, const void* p, int type, long long stride, size_t fbytes, unsigned long long has) {
  return {on_device, p, type, stride, fbytes, has};
}
// validate -> ON_DEVICE -> plan_frame -> upload -> enqueue_all.  detect = false: the stage entry points' way in (pbd_pyramid_*), up to
// the upload — a pending frame is no refusal, nothing is enqueued
int enter_frame(pbd_handle* h, const FrameSource& s, bool detect = true);
// `rows` rows of row_bytes, src_pitch apart -> packed rows, on the handle's stream: one linear copy when the source is packed too, else a 2-D copy
int copy_rows(pbd_handle* h, void* dst, const void* src, size_t src_pitch, size_t row_bytes, size_t rows, hipMemcpyKind kind);
int collect_frame(pbd_handle* h, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int capacity, int* count);   // the pending single frame
// the plan and the stages (pbd_api.cpp)
int plan_frame(pbd_handle* h, int w, int hgt, int cn, int batch = 1, int depth = PBD_DEPTH_8U);   // the frame plan of one geometry, kept while it repeats
void free_frame(pbd_handle* h);                                             // drops the plan: buffers, stage state, captured graph
int enqueue_all(pbd_handle* h, const FrameJob& job, const uint8_t* d_src, int stride);   // all stages + argmin (+ post-stages), eager or as one graph launch
void read_stage_times(pbd_handle* h);
int pbd_i_finish_frame(pbd_handle* h, int found);
int pbd_i_emit(pbd_handle* h, const std::vector<const char*>& recs, pbd_candidate_head* heads, int32_t* boxes,
               int32_t* locs, int capacity, bool ordered = false,    // ordered: the records are in final order already (k_cand_filter)
               std::vector<int>* order_out = nullptr);               // order_out: the record emitted i-th is recs[order[i]]
// latent detection (pbd_api.cpp): the argument checks of every latent entry (nframes truth sets), and — on a planned frame — the work
// table + the upload of the truth / mixture tables in the handle's stream
int pbd_i_latent_check(pbd_handle* h, const int32_t* truth, const int32_t* mix, int nframes, int component, double overlap);
int pbd_i_latent_begin(pbd_handle* h, const LatentSource& s, int nframes);
// best pose per ground-truth box (pbd_post.cpp): the argument checks of every entry (gt boxes of nframes frames; whole: the handle's
// settings too), the buffers + the upload of the boxes in the handle's stream, the launch behind k_backtrack (records in the route's bt.out), and
// the collect's copy of the winners: frame f's at heads[f * PBD_GT_MAX] etc., levels made the frame's own
int pbd_i_gt_check(pbd_handle* h, const double* gt, const int* ngt, int nframes, double overlap, bool whole);
int pbd_i_gt_begin(pbd_handle* h, const GtSource& s, int nframes);
int pbd_i_gt_enqueue(pbd_handle* h, const FrameRoute& r);
void pbd_i_gt_gather(pbd_handle* h, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int* found, double* o);
// hard-negative mining (pbd_qp_mine.cpp): behind the last post-stage of a FRAME_MINE job, the order and the scan of its final records
int pbd_i_mine_enqueue(pbd_handle* h, const FrameRoute& r);
int pbd_i_mine_buffers(pbd_handle* h);   // the order, ids and noshare buffers (first use), shared with the latent positives
// latent positives (pbd_qp_latent.cpp): behind the back-tracking (and the candidate filter) of a FRAME_LATENT_WRITE job, the scan of its poses
int pbd_i_latent_write_enqueue(pbd_handle* h, const FrameRoute& r);
// evaluation (pbd_eval.cpp): behind the last post-stage of a FRAME_EVAL job, the order (RAW) and the per-frame spans of its final records
int pbd_i_eval_enqueue(pbd_handle* h, const FrameRoute& r);
int pbd_i_found(const pbd_handle* h);   // records the pending frame left on the host side (filtered: the kept count)
#define PBD_FIRST_COPY 192   // candidate records fetched (or gathered) together with the count

// ---- the post-stages behind back-tracking (pbd_post.cpp) ----------------------------------
inline int pbd_i_cand_mode(const pbd_handle* h) { return h->cand_defer ? PBD_CAND_RAW : h->cand_mode; }   // the filter this handle runs
// the handle's buffers behind the names of a route (pbd_route.hpp; the route itself: enqueue_all, pbd_api.cpp)
char* pbd_i_route_buf(const pbd_handle* h, RouteBuf b);
int* pbd_i_route_count(const pbd_handle* h, RouteCount c);
RecordSet pbd_i_route_records(const pbd_handle* h, RouteBuf b, RouteCount c);   // the records in b, counted by c, as a kernel reads them
int pbd_i_post_buffers(pbd_handle* h, const FrameRoute& r);   // enqueue_all, outside any capture: the buffers of the route's post-stages
// behind launch_backtrack: the launches of the route's depth pruning and / or candidate filter
int pbd_i_post_enqueue(pbd_handle* h, const FrameJob& job, const FrameRoute& r);
int pbd_i_run_box3d(pbd_handle* h, const FrameJob& job, const FrameRoute& r);   // 3-D boxes (+ object clusters) of the frame's final records
int pbd_i_run_part_scores(pbd_handle* h, const FrameRoute& r);   // per-part scores of the frame's final records
void pbd_i_ps_begin(pbd_handle* h, int nframes);   // the collect: each frame's part scores in the order returned, like the 3-D boxes
void pbd_i_ps_gather(pbd_handle* h, int f, const std::vector<const char*>& recs, const std::vector<int>& order);
// the collect: each frame's 3-D boxes in the order returned (recs[order[i]]), then the clusters of the frames gathered
void pbd_i_b3_begin(pbd_handle* h, int nframes);
void pbd_i_b3_gather(pbd_handle* h, int f, const std::vector<const char*>& recs, const std::vector<int>& order);
int pbd_i_b3_end(pbd_handle* h);
// pbd_candidates_filter without the argument checks: `count` packed records filtered in place (kept ones first, final order)
// (kind / top: pbd_set_candidate_nms, what the NMS of mode 2 is)
int pbd_i_filter_host(pbd_handle* h, int mode, float overlap, int im_w, int im_h, char* recs, int count, int* kept,
                      int kind = PBD_NMS_PAINTED, int top = 0);
int pbd_i_depth_check(pbd_handle* h, int depth_type, long long dstride, int w);   // a depth-carrying frame's depth arguments
// Frame-plan buffers: counted in the frame footprint, freed on re-plan (pbd_api.cpp free_frame)
template <typename T>
int dev_alloc(pbd_handle* h, T** p, size_t n) {
  const hipError_t e = h->frame_allocs.alloc(p, n);
  return e == hipSuccess ? PBD_OK : fail(h, PBD_ERR_HIP, pbd_alloc_error("", e));
}
// Model-lifetime buffers (device, or pinned host): counted in the model footprint (counted = false: not part of it), freed by pbd_destroy
template <typename T>
int model_alloc(pbd_handle* h, T** p, size_t n, bool pinned = false, bool counted = true) {
  const hipError_t e = h->model_allocs.alloc(p, n, pinned, counted);
  return e == hipSuccess ? PBD_OK : fail(h, PBD_ERR_HIP, pbd_alloc_error("", e, pinned));
}
inline void model_free(pbd_handle* h, void* p) { h->model_allocs.release(p); }
// *p holds `have` units; grown (not kept) to `need` units of n elements (n = 0: need elements)
template <typename T, typename C>
int model_grow(pbd_handle* h, T** p, C& have, C need, size_t n = 0) {
  if (need <= have) return PBD_OK;
  if (*p) { model_free(h, *p); *p = nullptr; }
  have = 0;
  int rc = model_alloc(h, p, n ? n : (size_t)need);
  if (!rc) have = need;
  return rc;
}

// ---- kernel launchers (k_*.hip) ----------------------------------------------
void launch_resize(const PyrJob* jobs, int njobs, int maxpix, int cn, int sstride, const uint8_t* src, uint8_t* pyr, hipStream_t s);
void launch_pyrdown(const PyrJob* jobs, int njobs, int maxw, int maxh, int cn, uint8_t* pyr, hipStream_t s);
void launch_hog(const HogTile* tiles, int ntiles, const LevelDev* levels, const uint8_t* pyr, void* feat, int ts,
                int cn, int sbin, int tc, const uint8_t* binlut, uint16_t* split, int split_parts, int depth, hipStream_t s);   // depth: PBD_DEPTH_* of the level images
// PBD_PYRAMID_MATLAB (k_pyramid_mat.hip): job offsets in bytes, sstride in source elements
void launch_resize_area(const MatJob* jobs, int njobs, int maxpix, const MatRun* runs, const MatTap* taps, int cn, int sstride,
                        bool src_f64, const uint8_t* src, uint8_t* pyr, hipStream_t s);
void launch_reduce_f64(const MatJob* jobs, int njobs, int maxpix, int cn, uint8_t* pyr, hipStream_t s);
// the image depths beyond 8 bits (k_pyramid.hip): job offsets in bytes, sstride in bytes
void launch_resize_any(const PyrJob* jobs, int njobs, int maxpix, int cn, int depth, int sstride, const uint8_t* src, uint8_t* pyr, hipStream_t s);
void launch_pyrdown_any(const PyrJob* jobs, int njobs, int maxpix, int cn, int depth, uint8_t* pyr, hipStream_t s);
// the border ring of the boundary padding (k_featpad.hip): 0, and 1 in channel flen - 1, of every ring cell; split: as launch_hog's
void launch_featpad(const PadJob* jobs, const ReduceBlock* blocks, int nblocks, void* feat, int ts, uint16_t* split, int split_parts, hipStream_t s);
size_t hog_binlut_bytes();                                        // orientation-snap table: best_o for every (dx, dy) in [-255, 255]^2
void launch_hog_binlut(uint8_t* lut, int ts, hipStream_t s);      // evaluated in T (ts = sizeof(T)) with the reference's own chain (k_hog.hip)
// split-product filter bank (k_conv_split.hip): fp32 features -> three exact bfloat16 parts; kh x kw x 32 filters, float responses
void launch_feat_split(const float* feat, uint16_t* out, size_t ncells, hipStream_t s);
void launch_conv_split(const ConvTile* tiles, int ntiles, const LevelDev* levels, const uint16_t* feat_split, const uint16_t* wS,
                       float* resp, int nf, int kh, int kw, hipStream_t s, int nf_stride = 0);
void conv_split_filters(const float* filters, int nf, int kh, int kw, std::vector<uint16_t>& out);   // host: the d_wS layout
// PBD_CONV_SPLIT_F16: two scaled binary16 parts per operand, three products (k_conv_split.hip)
void launch_feat_split16(const float* feat, uint16_t* out, size_t ncells, hipStream_t s);
void conv_split16_filters(const float* filters, int nf, int kh, int kw, std::vector<uint16_t>& out, std::vector<float>& oscale);   // oscale[filter]: the response scale
void launch_conv_split16(const ConvTile* tiles, int ntiles, const LevelDev* levels, const uint16_t* feat_split, const uint16_t* wS,
                         float* resp, int nf, int kh, int kw, const float* oscale, hipStream_t s, int nf_stride = 0);
void launch_conv_exact(const ConvTile* tiles, int ntiles, const LevelDev* levels, const void* feat,
                       const void* wT, void* resp, int ts, int nf, int nfpad, int kh, int kw, hipStream_t s, int nf_stride = 0);
// the 16x16x4 MFMA banks (k_conv.hip); w4u: the [tap][group][k][n][u] copy of the filters inside d_wT
void launch_conv_mfma_f64(const ConvTile* tiles, int ntiles, const LevelDev* levels, const double* feat,
                          const double* w4u, double* resp, int nf, int nfpad, int kh, int kw, hipStream_t s, int nf_stride = 0);
void launch_conv_mfma16_f32(const ConvTile* tiles, int ntiles, const LevelDev* levels, const float* feat,
                            const float* w4u, float* resp, int nf, int nfpad, int kh, int kw, hipStream_t s, int nf_stride = 0);
void launch_dt_pass(const DtTask* tasks, int ntasks, const DtMap* maps, const FoldJob* folds, const unsigned long long* foldx, const float* biasw, size_t lds,
                    int ts, int nt, int fm, hipStream_t s);
void launch_reduce(const ReduceJob* jobs, const ReduceBlock* blocks, int nblocks, const float* biasw, int correct_ptr,
                   int ts, hipStream_t s);
void launch_root(const RootJob* jobs, const ReduceBlock* blocks, int nblocks, double thresh, int* count, CandRec* rec,
                 int capacity, int ts, const FoldJob* folds, const float* biasw, int rescan, int fm, const uint8_t* nms_mask,
                 const char* rootv_base, hipStream_t s);
void launch_nms_roots(const RootJob* jobs, int njobs, unsigned maxcells, const char* rootv_base, int ts, int sz, uint8_t* mask, hipStream_t s);
struct BacktrackArgs {   // (k_backtrack's own parameters keep their order: its first eight are preloaded)
  const int* count; const CandRec* rec; int capacity;
  const BackLevel* back; int ncomp;
  const int* parent; const int* plane0; const int* nparts; int max_parts; const int* mix_rows;
  char* out; size_t out_stride;
  const int* flat; const int* depth; int max_depth, nflat;
  const unsigned long long* scr_base;
  const void* ix; const void* iy; int ptr_bytes, correct_ptr;   // ix / iy: the DT's own planes, ptr_bytes wide (FrameLayout::ptr_bytes)
  const int16_t* extx; const int16_t* exty; const unsigned long long* ext_base;
  int* count_out; int pad;      // pad: the boundary padding (box origin)
  const FoldJob* folds; const unsigned long long* pick;   // pick != null: Ik picked from the fold's kept scores (fold_pick.hpp), not read from planes
};
void launch_backtrack(const BacktrackArgs& a, int ts, hipStream_t s);
// fold plans: the Ik planes written from the children's kept scores (k_dp.hip: k_ik_fill); blocks: {index into pick / cells, first cell}
void launch_ik_fill(const FoldJob* folds, const unsigned long long* pick, const ReduceBlock* blocks, int nblocks, const unsigned* cells, int ts, hipStream_t s);
// latent detection (k_latent.hip): the overlap mask of every response plane; the best root over the admissible (level, component) pairs
void launch_latent_mask(const LatentMaskArgs& a, int nblocks, int ts, hipStream_t s);
void launch_latent_best(const LatentBestArgs& a, int ts, hipStream_t s);
void dt_debug_read(unsigned long long* out);
void dt_debug_counters(unsigned long long* out);   // probe build: k_dt_pass path counters, read and reset (zeros elsewhere)
int dt_debug_trace(unsigned long long* t, unsigned* hw, int* nlaunch);   // probe build only
void hog_debug_read(unsigned long long* out);
void conv_debug_read(unsigned long long* out);
void launch_nms_map(const float* src, int rows, int cols, int sz, uint8_t* dst, hipStream_t s);
// candidate sort + painted-box NMS (k_cand.hip): one workgroup per frame
struct CandFilterArgs {
  RecordSet in;                 // (cf unused: one workgroup per frame of nlevels levels)
  const BackLevel* back;        // tie key: root element offset through back[level * ncomp + comp]; null: input position
  const char* rootv_base; int ts, ncomp;
  int nms; double overlap; int im_w, im_h;
  unsigned long long* keys; unsigned* idx;   // [2 * capacity]
  int* box; unsigned char* st;               // [capacity][4], [capacity]
  unsigned long long* gmask;                 // [nframes][cand_filter_mask_bytes / 8] when the mask does not fit LDS
  char* out; int* cnt_out;                   // kept records; counts [2 + 2 * nframes]
};
size_t cand_filter_mask_bytes(int w, int h);
void launch_cand_filter(const CandFilterArgs& a, int nframes, hipStream_t s);
// part-wise overlap NMS (k_cand_parts.hip): one workgroup per frame over the sorted runs k_cand_filter (SORT) left behind
struct CandPartsArgs {
  const char* in; size_t stride; int mp;     // the sorted records, frame f's at in + cnt_in[2 + nf + f] * stride
  const int* cnt_in; int capacity;           // k_cand_filter's count block
  double overlap; int top;
  int4* rect;                                // [mp + 2][capacity]: the restaged rectangles
  int* np; unsigned* kept;                   // [capacity] each: part counts, kept indices
  unsigned long long* gbits;                 // [cand_parts_bits_words]: undecided bits of frames too long for LDS
  char* out; int* cnt_out;                   // kept records; counts [2 + 2 * nframes]
};
size_t cand_parts_bits_words(int capacity, int nframes);
void launch_cand_parts(const CandPartsArgs& a, int nframes, hipStream_t s);
// depth-consistency pruning (k_zfilter.hip)
struct ZFilterArgs {
  RecordSet in;                 // (cf unused)
  DepthFrames z;
  const int* npart; const int* par; const double* thr;   // [ncomp] nparts; [ncomp * mp] parentid, norm(anchor(0)) * zfactor
  unsigned long long* med;      // [capacity * mp] median keys
  unsigned* large; unsigned* nlarge;          // [capacity * mp] boxes for k_zmed_large, their count
  char* out; int* cnt;          // kept records (any order) and their count; or
  unsigned char* flags;         // non-null: a keep flag per record instead (the stand-alone primitive)
};
void launch_zfilter(const ZFilterArgs& a, int ts, hipStream_t s);
// 3-D boxes (k_box3d.hip)
#define PBD_B3_MAXTAPS 35
struct Box3dArgs {
  RecordSet in;
  DepthFrames z;
  int im_w, im_h;
  pbd_camera cam;
  int ntaps; int tap_off[PBD_B3_MAXTAPS]; float tap[PBD_B3_MAXTAPS];   // dog's nonzero taps: offsets from the centre, values
  pbd_box3d* out; double* centres;            // [capacity], [capacity * mp * 3] (centres may be null)
};
void launch_box3d(const Box3dArgs& a, int ts, hipStream_t s);
// per-part scores (k_partscore.hip)
struct PsMix { int filter, bias, ax, ay; float w[4]; };   // one (part, mixture): response plane, bias base, anchor, (-w0, -w1, -w2, -w3) of its deformation (root: zeros)
struct PartScoreArgs {
  RecordSet in;
  const LevelDev* levels; int nvl;              // the plan's (virtual) levels
  const char* resp; int nfilters;               // T: the raw response planes, level l at cell_off[l] * nfilters
  int ncomp, nbias;
  const int* nparts; const int* parent; const int* flat;   // [ncomp]; [ncomp * mp] parent, flat part
  const int* mix0; const PsMix* mix;            // [flat parts + 1] first flat mixture; [flat mixtures]
  const float* biasw;
  double* out;                                  // [capacity][mp][3]: app, def, bias; zero beyond nparts
};
void launch_partscore(const PartScoreArgs& a, int ts, hipStream_t s);
// feature vectors (k_featvec.hip)
struct FvMix { int def, filter, kh, kw; };   // one (part, mixture): its defid, its filter in the CALLER's order and that filter's size
struct FeatVecArgs {
  RecordSet in;                                 // (count / cf unused: records rec0 .. rec0 + n - 1 of in.p)
  int rec0, n;
  const LevelDev* levels; int nvl;              // the plan's (virtual) levels
  const char* feat;                             // T: the feature planes, level l at cell_off[l] * flen, [ch][cw][flen]
  int ncomp, nbias, nfilters;
  const int* nparts; const int* parent; const int* flat;   // [ncomp]; [ncomp * mp] parent, flat part
  const int* mix0; const PsMix* mix; const FvMix* fmix;    // [flat parts + 1] first flat mixture; [flat mixtures] x 2
  int wmax;                                     // elements of a window slot: the bank's largest kh * kw * flen
  pbd_feature_block* blocks;                    // [n][mp]
  void* windows;                                // T [n][mp][wmax], 16-byte aligned
};
void launch_featvec(const FeatVecArgs& a, int ts, hipStream_t s);
// a feature-vector call in two steps (pbd_post.cpp), for the example cache's write: every refusal of pbd_candidates_features_dev with
// nothing touching the device; then the tables and the first `count` (> 0) records on the device — everything of the launch but its
// outputs (the upload synchronises the handle's stream)
int pbd_i_fv_check(pbd_handle* h, const pbd_candidate_head* heads, const int32_t* locs, int count);
int pbd_i_fv_upload(pbd_handle* h, const pbd_candidate_head* heads, const int32_t* locs, int count, FeatVecArgs* a);
// the same launch over records that are on the device already: the tables (built on first use, outside any frame) and everything of
// the launch but its records and its outputs
int pbd_i_fv_tables(pbd_handle* h);
void pbd_i_fv_args(const pbd_handle* h, FeatVecArgs* a);
// training example cache (k_qp.hip, pbd_qp.cpp; include/pbd_c.h "training example cache")
struct QpDev {
  float* x;                 // [capacity][k]: the columns, qp.x verbatim
  int* ids; float* b; double* d;   // [capacity][5], [capacity], [capacity]: by column
  int* tab; int* nblk;      // [capacity][nbmax][3] (0-based dense start, length, offset of the values in the column), [capacity] blocks
  int* slot;                // [capacity]: example -> column (pbd_qp_keep permutes this, no column moves)
  int k, len, capacity, nbmax;
};
struct QpWriteArgs {
  FeatVecArgs fv;           // the gather (blocks / windows unused): records fv.rec0 .. + fv.n - 1
  QpDev q; int n0;          // record r becomes example n0 + r
  const double* wreg; const double* w0; const int* foff;   // [len], [len], [nfilters] dense start of each filter
  double C; int label, id;
  // a mining frame's records, where the back-tracking or the candidate filter left them (pbd_qp_write: all null / 0)
  const int* perm;          // non-null: record fv.rec0 + r of the call is fv.in's record perm[fv.rec0 + r]
  const int* ids;           // non-null: the id of a record of frame f is ids[f] ...
  int nlevels;              // ... f = level / nlevels, and the level word is the frame's own level (0: one frame)
};
void launch_qp_write(const QpWriteArgs& a, int ts, hipStream_t s);
// hard-negative mining (k_qp_mine.hip, pbd_qp_mine.cpp; include/pbd_c.h "hard-negative mining")
enum { MINE_OK = 0, MINE_BAD_RECORD = 1, MINE_BAD_COLUMN = 2, MINE_BAD_REPEAT = 3 };
struct MineFrameOut {       // what the scan answers per frame, in pinned memory
  int count;                // the frame's final records
  int bad, code;            // the first record (in record order) pbd_qp_write would refuse, and why (MINE_*); -1: none
  int raw;                  // the back-tracking's count over all frames, before any filter (> capacity: overflow, nothing else is valid)
  double S;                 // the block sum of the frame's terms cneg * max(1 + score, 0)
};
struct MineArgs {
  RecordSet in;             // the final records of the frame or batch
  int nframes, k;           // k: the cache's column length
  FeatVecArgs fv;           // the model and plan tables of the gather (fv.in = in)
  const int* noshare;       // [ncomp] 1: no two parts of the component can share a filter, def or bias id, whatever the pose picks
  double cneg;
  unsigned long long* key;  // [capacity] RAW: (virtual level, component, root y, root x), 16 bits each
  int* perm;                // [capacity] the records in write order: frame after frame, a frame's in record order
  MineFrameOut* out;        // [nframes]
};
void launch_qp_mine_order(const MineArgs& a, hipStream_t s);   // RAW records only: perm sorts them by key
void launch_qp_mine_scan(const MineArgs& a, hipStream_t s);
// latent positives (k_qp_latent.hip, pbd_qp_latent.cpp; include/pbd_c.h "latent positives")
struct LatentWriteOut {     // what the scan answers per frame, in pinned memory
  int found;                // the frame has a pose
  int code;                 // MINE_*: why pbd_qp_write would refuse its record (MINE_OK: it would not)
  int component, level, x, y;   // the record's head: component, the frame's own level, root cell
  int raw, reserved;        // the back-tracking's count over all frames (at most one record per frame)
  double score;             // the record's score, widened exactly
};
struct LatentWriteArgs {
  RecordSet in;             // the final records of the frame or batch: at most one per frame, not frame-aligned
  int nframes, k;           // k: the cache's column length
  FeatVecArgs fv;           // the model and plan tables of the gather (fv.in = in)
  const int* noshare;       // [ncomp], as MineArgs::noshare
  int* perm;                // [nframes] the found frames' records in frame order: what k_qp_write reads
  LatentWriteOut* out;      // [nframes]
};
void launch_qp_latent_scan(const LatentWriteArgs& a, hipStream_t s);
// evaluation ledger (k_eval.hip, pbd_eval.cpp; include/pbd_c.h "evaluation ledger")
#define PBD_EVAL_ORDER_TILE 256    // keys of a frame's ordering staged in LDS at a time (k_eval_order)
#define PBD_EVAL_SORT_TILE 1024    // keys of the global sort a workgroup orders in LDS; longer runs go through device memory
struct EvalFrameOut { int count, start, raw, reserved; };   // k_eval_span per frame, in pinned memory: its final records are perm[start, start + count)
struct EvalFrame { int start, count, ngt, goff; };           // a frame of an add: its rows [start, start + count) of the call, its persons [goff, goff + ngt)
struct EvalSpanArgs {
  RecordSet in; int nframes;
  int* perm;                // [capacity] RAW: sorted by k_qp_mine_rank; filtered: written here, frame after frame
  EvalFrameOut* out;        // [nframes]
};
struct EvalLedgerDev {
  int P, ncap, mcap;
  double* dist; double* scale;            // [ncap][P], [ncap]
  float* score; unsigned char* tp;        // [mcap], [mcap][P]
};
struct EvalPckAddArgs {
  EvalLedgerDev L; int n0;                // person (f, g) becomes instance n0 + frames[f].goff + g
  const char* rec; size_t stride; int slots;   // its pose: the record at rec + stride * (f * slots + g), if found[f * slots + g]
  const int* found;
  const EvalFrame* frames;
  const double* points; const double* scale;   // [persons][P][2], [persons]: the call's persons back to back
};
struct EvalApkAddArgs {
  EvalLedgerDev L; int m0;                // position j of frame f becomes row m0 + frames[f].start + j
  const char* rec; size_t stride; int mp;
  const int* perm;                        // non-null: position j of frame f is record perm[frames[f].start + j]; else record frames[f].start + j
  int* ord;                               // [rows of the call] ord[start + r] = the position matched r-th (score descending, ties by position)
  const EvalFrame* frames;
  const double* points; const double* scale;
  double thresh;
};
struct EvalResultArgs {
  EvalLedgerDev L; int n, m; long long npos;
  unsigned long long* key; int n2;        // the global sort's keys, n2 = a power of two >= max(m, PBD_EVAL_SORT_TILE)
  int* tpc; double* sm;                   // [P][mcap] each, in sorted order: cumulative true positives, suffix maximum of the precision
  double* out;                            // [P]
  double* prec; double* rec;              // [P][m] or null
  double thresh; int rule;
};
void launch_eval_span(const EvalSpanArgs& a, hipStream_t s);
void launch_eval_pck_add(const EvalPckAddArgs& a, int nframes, hipStream_t s);
void launch_eval_apk_add(const EvalApkAddArgs& a, int nframes, int maxcount, hipStream_t s);   // the order, then the matching
void launch_eval_pck(const EvalResultArgs& a, hipStream_t s);
void launch_eval_apk(const EvalResultArgs& a, hipStream_t s);   // keys, sort, scan, suffix maximum, sum (+ the curves)
// part mixtures (k_kmeans.hip, pbd_kmeans.cpp; include/pbd_c.h "part mixtures"): trial g = p * R + r
struct KmeansArgs {
  const double* def; double* X;            // [P][n][2]
  const int* pa; const int* pb;            // [P]: X of part p = def[pa[p]] - def[pb[p]]
  const int* K;                            // [P]
  int n, P, R, max_iter;
  unsigned long long seed;
  unsigned char* lab;                      // [P * R][n] the trials' labels
  double* tc;                              // [P * R][PBD_CLUSTER_MAX_K][2] the trials' centroids
  double* tsum; int* titers; int* tcap;    // [P * R]
  int* idx; double* centres; double* sumdist; int* best; int* pcap;   // the winners: [P][n], [P][PBD_CLUSTER_MAX_K][2], [P], [P], [P]
};
void launch_kmeans(const KmeansArgs& a, hipStream_t s);   // X, the trials, the winners
// virtual positives (k_augment.hip, pbd_augment.cpp; include/pbd_c.h "virtual positives"): every op of one frame in one launch
struct AugDesc;
struct AugArgs {
  const uint8_t* im; int w, h, cn; unsigned long long stride;   // the source, read in place
  const AugDesc* desc; int nops;                                // [nops] in device memory
  int max_rows, max_cols;                                       // the largest canvas: the grid
};
void launch_augment(const AugArgs& a, hipStream_t s);
// a warped positive's column (train.m:152-161 qp_poswrite): window r of `feat` (T [n][wlen]) becomes example n0 + r with ids (1, ids[r], 0, 0, 0)
struct QpPosArgs {
  QpDev q; int n0, n;
  const void* feat; const int* ids;
  const double* wreg; const double* w0;
  int bias_start, filt_start, wlen;   // dense starts of the two blocks, values of the window
  double C;
};
void launch_qp_poswrite(const QpPosArgs& a, int ts, hipStream_t s);
// warped positives (k_warp.hip, pbd_qp_warp.cpp; include/pbd_c.h "warped positives"): one box's crop + bilinear resize in two passes.
// Tap tables are MatTap [P][n_out] — tap-major, so the lanes of consecutive outputs read consecutive taps —, si the 0-based source index
// inside the crop with the mirror resolved (pbd_warp.cpp)
struct WarpJob {
  unsigned long long scr_off, win_off;   // doubles: the job's intermediate in the scratch, its window in the window buffer
  unsigned long long ytap, xtap;         // first tap of its y table ([Py][oh]) and its x table ([Px][ow])
  int X0, Y0, cw, ch;                    // the crop: the image pixel (0-based, unclamped) of its pixel (0, 0), and its size
  int Py, Px, rows_first, pad;           // rows_first: the intermediate is [oh][cw][3] (y resampled), else [ch][ow][3] (x resampled)
};
struct WarpArgs {
  const WarpJob* jobs; const MatTap* taps;
  const uint8_t* im; int w, h, cn; size_t stride;   // the 8-bit frame on the device, rows `stride` bytes apart
  double* scratch; double* win; int ow, oh;
};
void launch_warp(const WarpArgs& a, int njobs, unsigned max_first, hipStream_t s);   // max_first: elements of the largest intermediate
void launch_qp_score(const QpDev& q, const double* w, const int* inds, int n, double* out, hipStream_t s);
void launch_qp_lincomb(const QpDev& q, const double* a, const int* inds, int n, double* w_out, hipStream_t s);
// the QP solver's device state (k_qp_solve.hip, pbd_qp_solve.cpp; include/pbd_c.h "QP solver")
enum { QP_STAT_L = 0, QP_STAT_WW = 1, QP_STAT_LOSS = 2, QP_STAT_N = 4 };
struct QpSolveDev {
  double* a; unsigned char* sv;   // [capacity] by example
  double* w;                      // [len]
  double* stat;                   // [QP_STAT_N]: l, w'w of the last refresh, the last pass's loss
  double* idC; int* idP; int* idI; double* err; int* order;   // [capacity] the pass's scratch (sumAlpha's tables, by position in order)
  double* scores;                 // [capacity] pbd_qp_loss's scores
};
void launch_qp_pass(const QpDev& q, const QpSolveDev& s, const int* noneg, int p, int n, hipStream_t st);
void launch_qp_clamp_norm(const QpSolveDev& s, const int* noneg, int p, int len, hipStream_t st);
void launch_qp_weights(const double* w, const double* wreg, const double* w0, int len, double* out, hipStream_t st);
// the positives' threshold (k_qp_thresh.hip, pbd_qp_solve.cpp; include/pbd_c.h "one training round")
#define QT_NT 256                 // lanes of a workgroup of every kernel of the file; the rank kernel stages this many scores at a time
struct QpThreshOut { double thresh; int bad; int m; };   // the order statistic; the first example with a non-finite score or -1; the positives
void launch_qp_thresh_weff(const double* w, const double* w0, const double* wreg, int len, double* out, hipStream_t st);
void launch_qp_thresh_select(const QpDev& q, int n, int* sel, QpThreshOut* out, hipStream_t st);             // sel[capacity], out->m
void launch_qp_thresh_scale(double* s, const int* sel, int m, double cpos, QpThreshOut* out, hipStream_t st);   // s /= cpos, out->bad
void launch_qp_thresh_rank(const double* s, int m, int rank, QpThreshOut* out, hipStream_t st);             // out->thresh
// weight updates (k_weights.hip, pbd_weights.cpp; include/pbd_c.h "weight and threshold updates").  stage: the model's float32 weights in
// Model.feature_layout() order; src[n]: where filter n of the bank being packed starts in it
void launch_weights_round(const double* w, int len, float* out, int* bad, hipStream_t s);   // *bad: the first index that is not finite as a float, or -1
void launch_bank_pack(const float* stage, const int* src, int nf, int kh, int kw, int nfpad, void* wT, int ts, hipStream_t s);   // upload_bank's d_wT
void launch_bank_split(const float* stage, const int* src, int nf, int kh, int kw, uint16_t* wS, hipStream_t s);                 // conv_split_filters
void launch_bank_split16(const float* stage, const int* src, int nf, int kh, int kw, uint16_t* wS, float* oscale, hipStream_t s);   // conv_split16_filters
// pbd_set_weights_dev's body, for pbd_qp_apply_weights too: every refusal of include/pbd_c.h, then the update, complete on return
int pbd_i_set_weights_dev(pbd_handle* h, const double* d_w, int len);
int pbd_i_ps_reweigh(pbd_handle* h);   // pbd_post.cpp: k_partscore's mixture table (-defw), if built, written again in place
void launch_gtbox(const GtBoxArgs& a, int gmax, hipStream_t s);   // k_gtbox.hip: gmax = the largest ngt
// object clusters (k_cluster3d.hip)
size_t cluster3d_slot_bytes(int pcap);
// src: 0 = xyz floats (pstride, rstride bytes), 4 / 8 = a depth image of float / double
void launch_cluster3d(const Cluster3dArgs& a, int src, int nblocks, hipStream_t s);
