/*
 * pbd_c.h — C ABI of libpbd_hip.so: the MI355X (gfx950) inference path behind
 * PartsBasedDetector<float>::detect().
 *
 * Every entry point below names the reference interface it replaces
 * (file:line under wg-perception/PartsBasedDetector).  The ABI is plain C:
 * opaque handle, POD structs, raw pointers + sizes, int status codes; no C++
 * exception ever crosses it.  INTEGRATION.md shows the reference-side
 * adaptors (IFeatures / IConvolutionEngine / DynamicProgram / detect()) that
 * bind it.
 *
 * Conventions
 *   - all matrices are dense row-major, "H x W" = rows x cols;
 *   - feature maps are cell-major with `flen` floats contiguous per cell
 *     (the reference's H x (W*flen) cv::Mat, src/HOGFeatures.cpp:178);
 *   - filters are kh x (kw*flen) floats, same interleave
 *     (src/MatlabIOModel.cpp:106-125);
 *   - a handle owns one GPU + one stream; calls on one handle must be
 *     serialised by the caller (the reference detector is not re-entrant
 *     either: src/HOGFeatures.cpp:99,106-107).
 */
#ifndef PBD_C_H_
#define PBD_C_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (reference: assert / CV_Error / bool) */
enum {
  PBD_OK = 0,
  PBD_ERR_ARG = 1,         /* bad pointer / size / index                       */
  PBD_ERR_UNSUPPORTED = 2, /* CV_StsUnsupportedFormat, src/HOGFeatures.cpp:141 */
  PBD_ERR_CAPACITY = 3,    /* output array too small; *count = needed          */
  PBD_ERR_HIP = 4,         /* HIP runtime failure (see pbd_last_error)         */
  PBD_ERR_STATE = 5,       /* stage called before its producer stage           */
  PBD_ERR_RCCL = 6         /* RCCL failure in a pbd_group gather (see pbd_group_last_error) */
};

/* ---- model: POD mirror of include/Model.hpp:49-122 ------------------------
 * Parts of all components are stored back to back ("flat part" index fp);
 * mixtures of all parts are stored back to back ("flat mixture" index fm).
 *   component c owns flat parts  part_offset[c] .. part_offset[c+1]-1
 *   flat part fp owns mixtures   mix_offset[fp] .. mix_offset[fp+1]-1
 * filterid/defid/biasid are 0-based like the C++ Model after zeroIndex
 * (src/MatlabIOModel.cpp:155-166).  For a child part with K mixtures whose
 * parent has L mixtures, bias(mm)[m] = biasw[biasid[fm0+mm] + m]
 * (include/Parts.hpp:172-175), deformation defw[defid[fm0+mm]][0..3] and
 * anchor anchors[defid[fm0+mm]] (include/Parts.hpp:179-183).
 */
typedef struct pbd_model_desc {
  int32_t nfilters;      /* Model::filters().size()                            */
  int32_t kh, kw;        /* filter rows / cols, 1..9, uniform over the bank (pbd_create).  The reference takes a size per
                            filter (src/SpatialConvolutionEngine.cpp:133-159, include/Parts.hpp:185-187), and its own
                            converter writes such models (matlab/modelTransfer.m, VOC path: a root filter per component
                            plus part filters of another size): those go through pbd_create_sized with kh = kw = 0 */
  int32_t flen;          /* Model::flen()  (32)                                */
  int32_t norient;       /* Model::norient() (18)                              */
  int32_t sbin;          /* Model::binsize()                                   */
  int32_t interval;      /* Model::nscales() (levels per octave)               */
  float thresh;          /* Model::thresh()                                    */
  const float* filters;  /* [nfilters][kh][kw*flen] (pbd_create_sized: back to back, each its own size) */
  int32_t ndefs;
  const float* defw;     /* [ndefs][4]  = {wxx, wx, wyy, wy}                   */
  const int32_t* anchors;/* [ndefs][2]  = {x, y}, 0-based                      */
  int32_t nbias;
  const float* biasw;    /* [nbias]                                            */
  int32_t ncomponents;
  const int32_t* part_offset; /* [ncomponents+1]                               */
  const int32_t* parentid;    /* [nparts_total], index local to the component  */
  const int32_t* mix_offset;  /* [nparts_total+1]                              */
  const int32_t* filterid;    /* [nmix_total]                                  */
  const int32_t* defid;       /* [nmix_total] (root: ignored)                  */
  const int32_t* biasid;      /* [nmix_total]                                  */
} pbd_model_desc;

/* ---- options -------------------------------------------------------------- */
enum {
  PBD_CONV_AUTO = 0,  /* banks of fewer than 16 filters: EXACT.  From 16 filters on, any kh x kw: float handles take SPLIT (round 5:
                         ABI version 4; rounds 3-4: MFMA), double handles MFMA.  Neither is bit-identical to the reference's
                         summation order (|delta| <= 2e-5 on HOG features, north_star 1e-4): callers who need the reference's
                         bits ask for PBD_CONV_EXACT.  pbd_get_conv_mode() tells what a handle resolved to.               */
  PBD_CONV_EXACT = 1, /* VALU direct correlation, reference summation order:
                         bit-identical to src/filter.cpp:3899-3922 + pdf+=pdfc */
  PBD_CONV_MFMA = 2,  /* MFMA implicit GEMM (k-ordered fma chain) for any kh x kw: fp32
                         v_mfma_f32_16x16x4_f32 for float handles, fp64
                         v_mfma_f64_16x16x4_f64 for double handles             */
  PBD_CONV_SPLIT = 3, /* float handles, any kh x kw (x 32 channels): the fp32 products on the bf16 matrix units through EXACT
                         three-way splits (x = h + m + l, three bfloat16 of 8 significant bits; the six partial products above
                         2^-24 relative on v_mfma_f32_16x16x32_bf16, fp32 accumulators): fp32 in, fp32 out, errors of the size of
                         PBD_CONV_MFMA's, on hardware the vector ALU does not share.  Weights must be finite
                         and below 3e38 in magnitude (bfloat16's range) — checked by pbd_create —, and so must features
                         handed in through pbd_set_level_features (HOG features are <= 0.4): an out-of-domain or non-finite
                         feature is refused there with PBD_ERR_ARG (PBD_CONV_MFMA / PBD_CONV_EXACT carry such values as
                         ordinary fp32)                                                                          */
  PBD_CONV_SPLIT_F16 = 4 /* opt-in, never what AUTO resolves to.  float handles: TWO binary16 parts per operand (11 significant
                         bits each, operands scaled by powers of two into binary16's range: features by 2^12, a bank's weights to
                         max |w| 2^e in [2^13, 2^14)) and the THREE products above 2^-22 relative on v_mfma_f32_16x16x32_f16, fp32
                         accumulators, responses scaled back exactly — half the matrix instructions of PBD_CONV_SPLIT.  Operands
                         are carried to 23 of their 24 bits; measured errors against fp64 on HOG features: those of
                         PBD_CONV_SPLIT.  Domain: |feature| < 15.99609375 = 65520 / 4096, where the scaled high part
                         would round to binary16's inf (HOG features are <= 1; features handed in
                         through pbd_set_level_features must respect it), weights finite; a feature below 2^-26 or a
                         weight below 2^-27 max |w| loses relative (not absolute) precision.                      */
};
/* Scalar type T of the instantiation (src/PartsBasedDetector.cpp:132-133):
 * PartsBasedDetector<float> (src/demo.cpp:85) or PartsBasedDetector<double>
 * (ros/Node.hpp:121, cells/detect.cpp:93).  Features, responses, scores and
 * the distance transform are computed and stored in T; model weights stay
 * float and are widened where the reference widens them; candidates carry
 * float scores for both (include/Candidate.hpp:72).                          */
enum { PBD_SCALAR_F32 = 0, PBD_SCALAR_F64 = 1 };
/* Depth of an input image: the values of cv::Mat::depth() the reference dispatches on (src/HOGFeatures.cpp:136-146:
 * CV_8U = 0, CV_16U = 2, CV_32F = 5, CV_64F = 6; anything else: CV_Error(StsUnsupportedFormat) -> PBD_ERR_UNSUPPORTED).
 * The *_u8 entry points are the 8-bit case; pbd_detect_image / pbd_pyramid_image take any of the four.             */
enum { PBD_DEPTH_8U = 0, PBD_DEPTH_16U = 2, PBD_DEPTH_32F = 5, PBD_DEPTH_64F = 6 };
typedef struct pbd_options {
  int32_t device;        /* HIP device ordinal                                 */
  int32_t conv_mode;     /* PBD_CONV_*                                         */
  int32_t max_candidates;/* device-side candidate capacity per frame           */
  int32_t dt_correct_ptr;/* 0 = reference pointer composition
                            (include/DistanceTransform.hpp:233-244), 1 = true
                            arg-max composition                                */
  int32_t level_begin;   /* process pyramid levels [level_begin, level_end)    */
  int32_t level_end;     /* <=0: all levels (multi-GPU level sharding)         */
  int32_t scalar_type;   /* PBD_SCALAR_F32 (default) or PBD_SCALAR_F64; a double
                            handle answers the *_f64 stage entry points
                            instead of the float ones                          */
  int32_t graph;         /* 1: capture the ~40 launches of a frame into a hipGraph once per frame geometry and
                            replay it (one hipGraphLaunch per frame instead of ~40 launches); 0: eager launches */
  int32_t reserved[2];   /* [0]: nms_sz — 0 (default, the reference's state: its call site is commented out,
                                 src/PartsBasedDetector.cpp:86): no suppression; sz > 0: nonMaximaSuppression(rootv, sz)
                                 (src/nms.cpp:84-129) of every (level, component) root-score plane ON THE DEVICE between
                                 min() and argmin(): only roots that are above the threshold AND the strict maximum of
                                 their (2 sz + 1)^2 neighbourhood (block rule of nms.cpp) are back-tracked and returned
                                 (ABI version 4; versions <= 3 ignored the slot);
                            [1]: dp_mode — 0: a part's messages are folded by its own x pass wherever the model allows it
                                 (no filter id shared inside a component, <= 8 mixtures per part, <= 8 children per part),
                                 1: the three-kernel structure (x pass, y pass, reduce + accumulated planes) for every model,
                                 2: fold + the compact memory plan (stage buffers that are never live together share
                                    memory; automatic for large frames, e.g. 1920x1080: 1.47 GB instead of 3.3 GB per
                                    handle): after min() / detect() the image, feature and response getters answer
                                    PBD_ERR_STATE                                                                       */
} pbd_options;
/* The layout of pbd_options and pbd_model_desc is frozen from PBD_ABI_VERSION 3 on: new options take a reserved slot
 * or a new entry point, fields are never inserted.  pbd_abi_version() returns the version the LIBRARY was built with;
 * a binding compares it with the header it was compiled against (round 2 inserted `graph` in front of reserved[],
 * which nothing could detect).                                                                                       */
#define PBD_ABI_VERSION 5
int pbd_abi_version(void);
/* Version history: 3 = rounds 3-4.  4 (round 5) = PBD_CONV_AUTO resolves to PBD_CONV_SPLIT for float handles (numerics of
 * AUTO change in the last bits: rounds 3-4 resolved to PBD_CONV_MFMA, and before that to EXACT for banks other than 5 x 5),
 * PBD_CONV_SPLIT, PBD_CONV_SPLIT_F16, pbd_detect_image / pbd_pyramid_image / pbd_get_level_image_raw (PBD_DEPTH_*), pbd_tune_plan, pbd_options.reserved[0] = nms_sz, pbd_get_conv_mode, pbd_get_stage_state, pbd_group_comm_size.  Struct layouts unchanged.
 * Round 6 keeps version 4 (no entry point, layout or result changed); refinements of existing entries: pbd_set_level_features refuses
 * features outside a split bank's domain (PBD_ERR_ARG), pbd_tune_plan drops the handle's plan on return, pbd_detect_image replays a
 * hipGraph under pbd_options.graph.
 * 5 = pbd_create_sized, pbd_group_create_sized, pbd_get_filter_size (filter banks with a size per filter); also marks the round-6
 * refinements above.  Struct layouts unchanged; results of uniform banks unchanged.
 * Version 5 also gains, purely additively (no layout moved, no existing result changed; a binding finds them by symbol): the
 * candidate filter entry points pbd_set_candidate_filter, pbd_group_set_candidate_filter and pbd_candidates_filter; and the
 * depth-pruning entry points pbd_set_depth_filter, pbd_detect_rgbd_u8, pbd_detect_rgbd_enqueue_dev_u8, pbd_detect_batch_rgbd_u8,
 * pbd_detect_batch_rgbd_enqueue_dev_u8 and pbd_candidates_depth_filter; and the 3-D box entry points pbd_set_box3d,
 * pbd_get_box3d and pbd_candidates_box3d (with the structs pbd_camera and pbd_box3d); and the object-cluster entry points
 * pbd_set_cluster3d, pbd_get_cluster3d and pbd_candidates_cluster3d (with the struct pbd_cluster3d); and the per-part score entry
 * points pbd_set_part_scores, pbd_get_part_scores and pbd_candidates_part_scores (with the struct pbd_part_score); and the latent
 * detection entry points pbd_latent_mask, pbd_dp_argbest, pbd_detect_latent_u8, pbd_detect_latent_dev_u8 and
 * pbd_detect_batch_latent_u8; and the feature-vector entry points pbd_feature_window_max, pbd_candidates_features,
 * pbd_candidates_features_f64 and pbd_candidates_features_dev (with the struct pbd_feature_block); and the part-wise NMS entry
 * points pbd_candidates_nms_parts, pbd_set_candidate_nms, pbd_group_set_candidate_nms and pbd_candidates_filter_parts; and the
 * best-pose-per-ground-truth-box entry points pbd_candidates_best_overlap, pbd_candidates_select_gt, pbd_detect_gtbox_u8,
 * pbd_detect_gtbox_dev_u8 and pbd_detect_batch_gtbox_u8 (with PBD_GT_MAX); and the training example cache pbd_qp with its entry
 * points pbd_qp_create, _destroy, _dims, _footprint, _write, _score[_dev], _lincomb[_dev], _keep, _get and _put; and the QP solver
 * over that cache: pbd_qp_noneg, _fix, _state_put, _state_get, _pass, _one, _refresh, _loss, _opt, _prune and _weights; and the
 * warped positives: pbd_warp_geometry, pbd_warp_taps, pbd_warp_windows_u8, pbd_warp_windows_u8_f64, pbd_qp_write_warped_u8 and
 * pbd_debug_warp_ms (with PBD_WARP_SKIPPED / _WRITTEN / _FULL); and the weight and threshold updates pbd_set_weights,
 * pbd_set_weights_dev, pbd_get_weights, pbd_qp_apply_weights, pbd_set_threshold and pbd_get_threshold; and hard-negative mining:
 * pbd_qp_mine_u8, pbd_qp_mine_dev_u8 and pbd_qp_mine_batch_u8 (with PBD_MINE_NONE / _ONE / _OPT); and the latent positives:
 * pbd_qp_write_latent_u8, pbd_qp_write_latent_dev_u8, pbd_qp_write_latent_batch_u8 and pbd_croppos (with the struct
 * pbd_latent_example); and the evaluation ledger pbd_eval: pbd_eval_create, _destroy, _reset, _dims, _get, _add_pck_records,
 * _add_apk_records, _pck_frame_u8, _pck_frame_batch_u8, _apk_frame_u8, _apk_frame_batch_u8, _pck and _apk, with the host-only
 * definitions pbd_eval_keypoint_dist, _pck_host, _apk_match_host and _ap_host (PBD_EVAL_SCALE_LAST / _OWN); and the part mixtures
 * pbd_kmeans_host, pbd_cluster_parts_host and pbd_cluster_parts; and the seams of one training round: pbd_set_interval,
 * pbd_get_interval, pbd_qp_clear and pbd_qp_positive_threshold; and the pyramid store pbd_pyrstore: pbd_pyrstore_create, _destroy,
 * _dims, _slot, _layout, _put_u8, _put_dev_u8, _put_batch_u8 and _get_level, with pbd_detect_stored, pbd_detect_batch_stored,
 * pbd_qp_mine_stored and pbd_qp_mine_batch_stored (PBD_PYRSTORE_MAX_LEVELS); and the virtual positives: pbd_rotate_geometry,
 * pbd_map_rotate_points, pbd_flip_points, pbd_augment_host_u8, pbd_augment_u8, pbd_augment_dev_u8, pbd_augment_last_error and
 * pbd_qp_write_warped_dev_u8 (with the struct pbd_augment_op, PBD_ROT_* and PBD_AUGMENT_MAX_*).                                     */

/* ---- output record: include/Candidate.hpp:56-111 --------------------------
 * One candidate = head + max_parts boxes (x, y, width, height as cv::Rect)
 * + max_parts part locations (x, y, mixture) in cells of its pyramid level.
 * max_parts = pbd_max_parts(handle).  Part confidences are the reference's:
 * root = rootv, every other part 0.0 (src/DynamicProgram.cpp:241-244).  The
 * opt-in step pbd_set_part_scores (below) computes what each part contributes.
 */
typedef struct pbd_candidate_head {
  float score;        /* Candidate::score()                                    */
  int32_t component;  /* Candidate::component()                                */
  int32_t level;      /* pyramid level the root was found at                   */
  int32_t nparts;     /* parts of that component                               */
} pbd_candidate_head;

typedef struct pbd_handle pbd_handle;

/* Restrict the handle to an arbitrary SET of pyramid levels (n = 0: all levels again), intersected with
 * [level_begin, level_end).  Levels never interact (src/DynamicProgram.cpp:83-87 loops over (level,
 * component) pairs independently), so one large frame shards across GPUs by level with no data-path
 * collective: every rank rebuilds the (cheap) image pyramid and runs HOG / pdf / min / argmin on its own
 * cost-balanced level set (SURVEY 8e, configs[3]); the union of the ranks' candidates is the frame's.   */
int pbd_set_levels(pbd_handle* h, const int32_t* levels, int n);
/* PartsBasedDetector<T>::distributeModel (src/PartsBasedDetector.cpp:102-127)
 * incl. SpatialConvolutionEngine::setFilters (src/SpatialConvolutionEngine.cpp:133-159)
 * and Parts construction (include/Parts.hpp:229-235).
 * Filter, bias and deformation weights must be finite (PBD_ERR_ARG).         */
int pbd_create(const pbd_model_desc* model, const pbd_options* opt, pbd_handle** out);
/* A size per filter (SpatialConvolutionEngine::setFilters builds one FilterEngine per filter at its own size).
 * fsize[nfilters][2] = {rows kh, cols kw} of each filter, 1..9 each (else PBD_ERR_UNSUPPORTED); model->filters holds the filters
 * back to back (filter n at offset sum_{i<n} kh_i*kw_i*flen, each kh_i x (kw_i*flen) interleaved); model->kh / kw must be 0 and
 * fsize non-null (else PBD_ERR_ARG).  Validation happens before any HIP call, as in pbd_create.
 * A bank whose filters all have one size is exactly the pbd_create handle of that size (same kernels, same bits).  A mixed bank is
 * run as size groups (filters of one kh x kw), each on the kernel a uniform bank of that size runs in the handle's conv mode; the
 * conv mode resolves from the total filter count as in pbd_create.  The stage entry points (pbd_pdf, pbd_get/set_level_response*,
 * pbd_dp_min, pbd_dp_argmin) keep the caller's filter order.  Part boxes are sized by the filter of the mixture a part chose, with
 * the reference's quirk kept: xsize() and ysize() both return the filter's rows (include/Parts.hpp:185-187), so a box is
 * kh x kh scaled even where kw != kh.                                                                                           */
int pbd_create_sized(const pbd_model_desc* model, const int32_t* fsize, const pbd_options* opt, pbd_handle** out);
/* rows / cols of filter `filter` (caller's order) of a handle made by either constructor */
int pbd_get_filter_size(const pbd_handle* h, int filter, int32_t* kh, int32_t* kw);
int pbd_destroy(pbd_handle* h);
const char* pbd_last_error(const pbd_handle* h);
int pbd_max_parts(const pbd_handle* h);
/* set the stream all work of this handle is enqueued on (hipStream_t as void*) */
int pbd_set_stream(pbd_handle* h, void* hip_stream);

/* PartsBasedDetector<T>::detect(im, candidates) (src/PartsBasedDetector.cpp:69-95).
 * `im` is a host pointer to an 8-bit image, cn = 1 or 3 (BGR interleaved),
 * stride in bytes.  Rows and strides, for every image `stride` and depth-image `dstride` of this header (host and device alike):
 * row y starts at im + y * stride; only its first w * cn * element size bytes are read, so the bytes between rows may
 * hold anything (an ROI of a larger frame, a pitched allocation) and the last row needs no padding: the buffer may end
 * with the last pixel.  The base pointer needs no alignment beyond the element's.  stride < w * cn * element size (a
 * negative one included), or one that is not a multiple of the element size, is PBD_ERR_ARG and leaves no frame pending.
 * Candidates are written in the order of a single-threaded
 * reference run (level, component, row-major root location); at most
 * `capacity`; *count = number found (PBD_ERR_CAPACITY if > capacity).
 * heads[capacity], boxes[capacity][max_parts][4], locs[capacity][max_parts][3]
 * (boxes / locs may be NULL).                                                 */
int pbd_detect_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride,
                  pbd_candidate_head* heads, int32_t* boxes, int32_t* locs,
                  int capacity, int* count);
/* Input depth.  The reference dispatches features<uint8_t|uint16_t|float|double> on im.depth()
 * (src/HOGFeatures.cpp:136-146); its three callers (src/demo.cpp:90, ros/Node.cpp:183,
 * cells/detect.cpp:224) all pass CV_8U BGR, which is what the *_u8 entry points (device-resident images, batches,
 * graph replay, groups) are built and tuned for.  pbd_detect_image takes a host image of any of the four depths
 * (`depth` = PBD_DEPTH_*, stride in BYTES, a multiple of the element size): pyramid levels in the image's own type —
 * cv::resize interpolating in floating point with float coefficients, cv::pyrDown as FltCast<T, 8> (ushort: the
 * integer form), restated from OpenCV 2.4 like the 8-bit pair and equally unpinned (no reference test holds any
 * pyramid value) —, gradients in the pixel type's promoted arithmetic, everything from the histograms on unchanged.
 * Single host frames (replayed as a hipGraph under pbd_options.graph like 8-bit plans, round 6); batches, device-resident entry points
 * and groups stay 8-bit — by design: no caller of the reference hands over anything else, and every further entry point is a surface
 * to test against an oracle that is itself unpinned for these depths.  PBD_DEPTH_8U forwards to pbd_detect_u8.  Any other depth:
 * PBD_ERR_UNSUPPORTED, the counterpart of CV_Error(StsUnsupportedFormat) (:141-145).                               */
int pbd_detect_image(pbd_handle* h, const void* im, int depth, int w, int hgt, int cn, int stride,
                     pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int capacity, int* count);
/* same, image already resident in device memory (tightly packed or strided)  */
int pbd_detect_dev_u8(pbd_handle* h, const void* d_im, int w, int hgt, int cn, int stride,
                      pbd_candidate_head* heads, int32_t* boxes, int32_t* locs,
                      int capacity, int* count);
/* asynchronous halves of pbd_detect_dev_u8: enqueue all kernels + the D2H of
 * the candidate buffer on the handle's stream; collect after the stream (or
 * the caller's event) has completed.  Lets a caller overlap frames.          */
int pbd_detect_enqueue_dev_u8(pbd_handle* h, const void* d_im, int w, int hgt, int cn, int stride);
int pbd_detect_collect(pbd_handle* h, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs,
                       int capacity, int* count);
/* asynchronous pbd_detect_u8: the H2D copy of the host image is enqueued on the handle's stream in
 * front of the kernels (truly asynchronous when `im` is pinned: hipHostMalloc / hipHostRegister; a pageable
 * image is staged by the runtime).  `im` must stay valid until pbd_detect_collect returns.               */
int pbd_detect_enqueue_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride);

/* ---- a batch of same-sized frames on ONE handle (BASELINE configs[2] gives every GPU 4 frames) ----------
 * The frames of a batch go through every stage TOGETHER: one launch (or one chain of launches) per stage for the whole
 * batch — the same kernels with `nframes` times the blocks per launch, which fills the chip in the thin rounds of the DP
 * and pays every launch tail once per batch.  Results per frame are identical to pbd_detect_u8.
 * Frame f's candidates land at heads[f*capacity], boxes[f*capacity*max_parts*4], locs[f*capacity*max_parts*3] (boxes /
 * locs may be NULL), counts[f] = number found; PBD_ERR_CAPACITY if a frame exceeds `capacity` or the batch exceeds
 * pbd_options.max_candidates.  1 <= nframes <= 64; the work tables are re-planned when nframes (or the size) changes.
 * _enqueue_dev_: the frames already in device memory, tightly packed, back to back; collect after either enqueue.   */
int pbd_detect_batch_u8(pbd_handle* h, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride,
                        pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int capacity, int* counts);
int pbd_detect_batch_enqueue_u8(pbd_handle* h, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride);
int pbd_detect_batch_enqueue_dev_u8(pbd_handle* h, const void* d_ims, int nframes, int w, int hgt, int cn);
int pbd_detect_batch_collect(pbd_handle* h, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int capacity, int* counts);

/* ---- one process, several GPUs (SURVEY 8b "Threading", 8e) ------------------
 * The reference's hosts are single processes (src/demo.cpp:85-103, ros/Node.cpp:183, cells/detect.cpp:224).
 * A pbd_group owns one handle per listed device (a device may be listed more than once: several frames in
 * flight on it) and drives them from the calling thread; frames and pyramid levels never interact
 * (src/DynamicProgram.cpp:83-87), so there is no data-path collective, only the gather of the members'
 * candidate buffers:
 *   PBD_GATHER_RCCL  ncclAllGather over the members' devices (RCCL over xGMI; librccl is loaded at run time) of a
 *                    fixed-size block {count, first records}, then ONE D2H on member 0; members holding more
 *                    records than the block hand the remainder over directly;
 *   PBD_GATHER_HOST  one small D2H per member + concatenation on the host (same result; used when librccl is
 *                    missing or a device is listed twice — RCCL wants distinct devices);
 *   PBD_GATHER_AUTO  RCCL when possible, else host.
 * Results are identical to running the frames one after the other on a single handle.                      */
enum { PBD_GATHER_AUTO = 0, PBD_GATHER_HOST = 1, PBD_GATHER_RCCL = 2 };
typedef struct pbd_group pbd_group;
/* opt->device is ignored (devices[] decides); every other option applies to all members                     */
int pbd_group_create(const pbd_model_desc* model, const pbd_options* opt, const int32_t* devices, int ndevices,
                     int gather_mode, pbd_group** out);
/* pbd_group_create with a size per filter: every member is made by pbd_create_sized (same fsize rules) */
int pbd_group_create_sized(const pbd_model_desc* model, const int32_t* fsize, const pbd_options* opt, const int32_t* devices,
                           int ndevices, int gather_mode, pbd_group** out);
int pbd_group_destroy(pbd_group* g);
const char* pbd_group_last_error(const pbd_group* g);
int pbd_group_size(const pbd_group* g);
int pbd_group_gather_mode(const pbd_group* g);          /* PBD_GATHER_HOST or PBD_GATHER_RCCL actually in use   */
int pbd_group_comm_size(const pbd_group* g);            /* ranks of the RCCL communicator (ncclCommCount); 0 = host gather (ABI 4) */
pbd_handle* pbd_group_member(pbd_group* g, int i);     /* borrowed: stage entry points, pbd_get_stage_ms, ...   */
/* BASELINE configs[2]: a batch of same-sized frames, frame f on member f % size, all members busy at once.
 * Frame f's candidates land at heads[f*capacity], boxes[f*capacity*max_parts*4], locs[f*capacity*max_parts*3]
 * (boxes / locs may be NULL), counts[f] = number found; PBD_ERR_CAPACITY if any frame exceeds `capacity`.   */
int pbd_group_detect_batch_u8(pbd_group* g, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride,
                              pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int capacity, int* counts);
/* BASELINE configs[3]: ONE frame, its pyramid levels spread over the members by greedy LPT on the cell counts
 * (every member rebuilds the cheap image pyramid); output in the order a single handle produces.            */
int pbd_group_detect_u8(pbd_group* g, const uint8_t* im, int w, int hgt, int cn, int stride,
                        pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int capacity, int* count);

/* ---- stage entry points (parity testing; same kernels as detect) ----------
 * IFeatures::nscales/scales (include/IFeatures.hpp:54-63) + pyramid geometry
 * of HOGFeatures<T>::pyramid (src/HOGFeatures.cpp:98-127).  Arrays sized
 * >= *nlevels (call with NULL arrays to query).  img_* = level image size,
 * cell_* = feature map size, scales = IFeatures::scales().                   */
int pbd_pyramid_geometry(const pbd_handle* h, int w, int hgt, int* nlevels,
                         int32_t* img_w, int32_t* img_h, int32_t* cell_w, int32_t* cell_h,
                         float* scales);
/* HOGFeatures<T>::pyramid (src/HOGFeatures.cpp:95-151): image pyramid + HOG  */
int pbd_pyramid_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride);
int pbd_get_level_image(pbd_handle* h, int level, uint8_t* out /* img_h*img_w*cn */);
/* HOGFeatures<T>::pyramid for an image of any accepted depth (pbd_detect_image), and a level image in the frame's own pixel
 * type (out_bytes >= img_h * img_w * cn * element size)                                                              */
int pbd_pyramid_image(pbd_handle* h, const void* im, int depth, int w, int hgt, int cn, int stride);
int pbd_get_level_image_raw(pbd_handle* h, int level, void* out, size_t out_bytes);
int pbd_get_level_features(pbd_handle* h, int level, float* out /* cell_h*cell_w*flen */);
/* (a handle on a split-product bank refuses features outside the bank's domain — PBD_CONV_SPLIT: finite, |f| < 3e38;
 *  PBD_CONV_SPLIT_F16: |f| < 15.99609375 (65520 / 4096: f 2^12 must round to a finite binary16) — with PBD_ERR_ARG; nothing is
 *  uploaded then)                                                                                                        */
int pbd_set_level_features(pbd_handle* h, int level, const float* in);
int pbd_get_level_features_f64(pbd_handle* h, int level, double* out);
/* Read-only: the level image (own depth) and the features of ONE frame of the current plan, 0 <= frame < frames of the plan.  Unlike the
 * stage entry points these also answer for a batch plan (pbd_detect_batch_*), where frame f's planes are what the batched launches
 * wrote for it; on a single-frame plan frame is 0 and they equal pbd_get_level_image_raw / pbd_get_level_features.  PBD_ERR_STATE as
 * for those (stage not computed, compact memory plan after min(), level not processed, wrong scalar type).                            */
int pbd_get_frame_level_image_raw(pbd_handle* h, int frame, int level, void* out, size_t out_bytes);
int pbd_get_frame_level_features(pbd_handle* h, int frame, int level, float* out);
int pbd_get_frame_level_features_f64(pbd_handle* h, int frame, int level, double* out);
int pbd_set_level_features_f64(pbd_handle* h, int level, const double* in);
/* declare a frame geometry without running the pyramid (inject features)     */
int pbd_begin_frame(pbd_handle* h, int w, int hgt, int cn);
/* SpatialConvolutionEngine::pdf (src/SpatialConvolutionEngine.cpp:106-124)   */
int pbd_pdf(pbd_handle* h);
int pbd_get_level_response(pbd_handle* h, int level, int filter, float* out /* cell_h*cell_w */);
/* in: finite values only (PBD_ERR_ARG otherwise, the plane is not uploaded): the distance transform's domain, see pbd_dt2d */
int pbd_set_level_response(pbd_handle* h, int level, int filter, const float* in);
int pbd_get_level_response_f64(pbd_handle* h, int level, int filter, double* out);
int pbd_set_level_response_f64(pbd_handle* h, int level, int filter, const double* in);
/* DynamicProgram<T>::min (src/DynamicProgram.cpp:66-173)                      */
int pbd_dp_min(pbd_handle* h);
/* Ix/Iy/Ik[level][component][part][parent mixture] as int32 cell_h*cell_w.
 * A frame entry (pbd_detect_*, pbd_enqueue_*) does not store Ik on the device: its back-tracking picks the mixture at the cells it
 * visits.  The first getter call after such a frame writes the Ik planes of the whole plan from the resident scores (one small launch),
 * later calls read them; the bytes returned are those the reference's min() computes.  pbd_dp_min leaves the planes written. */
int pbd_get_dp_pointers(pbd_handle* h, int level, int component, int part, int parent_mix,
                        int32_t* ix, int32_t* iy, int32_t* ik);
/* Read-only: the same tables of ONE frame of the current plan, 0 <= frame < frames of the plan — also for a batch plan
 * (pbd_detect_batch_*), like pbd_get_frame_level_features; on a single-frame plan frame is 0 and it equals pbd_get_dp_pointers. */
int pbd_get_frame_dp_pointers(pbd_handle* h, int frame, int level, int component, int part, int parent_mix,
                              int32_t* ix, int32_t* iy, int32_t* ik);
int pbd_get_root(pbd_handle* h, int level, int component, float* rootv, int32_t* rooti);
int pbd_get_root_f64(pbd_handle* h, int level, int component, double* rootv, int32_t* rooti);
/* DynamicProgram<T>::argmin takes rootv / rooti / Ix / Iy / Ik as arguments (include/DynamicProgram.hpp:75).  A caller
 * whose tables are not the ones this handle's min() left on the device (another engine's min(), edited tables) hands
 * them over here before pbd_dp_argmin; the next pbd_dp_min / detect goes back to the handle's own tables.  The first
 * pbd_set_dp_pointers after a min() materialises all composed planes once (the planes not handed in keep min()'s).  */
int pbd_set_root(pbd_handle* h, int level, int component, const float* rootv, const int32_t* rooti);
int pbd_set_root_f64(pbd_handle* h, int level, int component, const double* rootv, const int32_t* rooti);
int pbd_set_dp_pointers(pbd_handle* h, int level, int component, int part, int parent_mix,
                        const int32_t* ix, const int32_t* iy, const int32_t* ik);
/* Which stage buffers of the current frame plan hold valid data: state[0] level images, [1] features, [2] responses,
 * [3] the DP tables (what the getters / the next stage would answer PBD_ERR_STATE for when 0).  On a handle with the
 * compact memory plan (reserved[1] = 2, or automatic for large frames) min() reuses the image / feature memory and
 * transforms the responses in place: [0..2] read 0 afterwards, and a response / feature setter makes its stage valid
 * again only once EVERY plane of the active levels has been handed in.  A caller that caches what is resident on the
 * device (host/pbd_host.hpp: content fingerprints) must drop that knowledge when a flag reads 0.                      */
int pbd_get_stage_state(const pbd_handle* h, int32_t state[4]);
/* The filter bank this handle runs (PBD_CONV_EXACT / _MFMA / _SPLIT): what PBD_CONV_AUTO resolved to at pbd_create
 * (SpatialConvolutionEngine is the reference's only engine, src/PartsBasedDetector.cpp:111; the choice here is numerical:
 * see the enum).  Negative: error code.                                                                              */
int pbd_get_conv_mode(const pbd_handle* h);
/* DynamicProgram<T>::argmin (src/DynamicProgram.cpp:189-255).  With tables handed in and NO min() of this handle on the
 * frame, every pointer table and every root table of the handle's levels must have been provided (PBD_ERR_STATE else). */
int pbd_dp_argmin(pbd_handle* h, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs,
                  int capacity, int* count);

/* ---- stand-alone primitives ------------------------------------------------
 * DistanceTransform<T>::compute (include/DistanceTransform.hpp:202-245) with
 * Quadratic(ax,bx), Quadratic(ay,by) and anchor (osx, osy); host arrays.
 * DOMAIN: ax, bx, ay, by finite, ax != 0, ay != 0, every score finite, and the
 * scores of BOTH passes finite (the x pass's a d^2 + b d + y can overflow from
 * finite arguments).  Inside it the result is the reference's bit for bit
 * (scores, Ix, Iy; float and double), whatever the magnitudes.  A NaN or an
 * infinity in the arguments: PBD_ERR_ARG, nothing is launched.  A pass that
 * left the finite range: PBD_ERR_ARG after the run (the kernel ends on any
 * input; out / ix / iy are then not the reference's).  PBD_OK means inside
 * the domain.  DESIGN.md "Input domain of the distance transform".  The score
 * maps and features handed to pbd_set_level_response / pbd_set_level_features
 * (PBD_ERR_ARG, nothing is uploaded) and the weights of a model (pbd_create:
 * PBD_ERR_ARG) must be finite as well; sums that overflow on the device are
 * outside the domain and are not detected on the frame path.               */
int pbd_dt2d(pbd_handle* h, const float* in, int rows, int cols,
             double ax, double bx, double ay, double by, int osx, int osy,
             float* out, int32_t* ix, int32_t* iy);
int pbd_dt2d_f64(pbd_handle* h, const double* in, int rows, int cols,
                 double ax, double bx, double ay, double by, int osx, int osy,
                 double* out, int32_t* ix, int32_t* iy);   /* DistanceTransform<double> */
/* HOGFeatures<T>::features<uint8_t> (src/HOGFeatures.cpp:168-341), one image */
int pbd_hog_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride,
               float* out, int* cell_w, int* cell_h);
int pbd_hog_u8_f64(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride,
                   double* out, int* cell_w, int* cell_h);  /* HOGFeatures<double> */
/* cv::resize(INTER_LINEAR) / cv::pyrDown on 8-bit images as used at
 * src/HOGFeatures.cpp:116,122 (this library's definition)     */
int pbd_resize_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride,
                  uint8_t* out, int ow, int oh);
int pbd_pyrdown_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride,
                   uint8_t* out);
/* The MATLAB pyramid's two stages (PBD_PYRAMID_MATLAB, below), stand-alone: interleaved double images (element (y, x, c) at
 * (y * w + x) * cn + c), cn 1 or 3; `out` sized by the caller for the dimensions stated, which *ow / *oh report.  Bit-exact against
 * the compiled reference files.
 *   pbd_resize_area_f64: resize(im, scale) of matlab/mex/resize.cc:82-106 — area-weighted resampling by resize1dtran's
 *     interpolation cache (:30-66, both `> 1e-3` tests), the rows axis then the columns axis (:101-102), the taps of a destination
 *     index summed in ascending source order from 0.0 (alphacopy :18-24 on zeroed memory :69).  Result size round(hgt * scale) x
 *     round(w * scale), C round() (:94-95).  scale > 1: PBD_ERR_ARG, "Invalid scaling factor" (resize.cc:90).
 *   pbd_reduce_f64: reduce(im) of matlab/mex/reduce.cc:50-70 — the 5-tap binomial of :29 with the edge forms of the first row
 *     (:24), the last row (:42) and the second-to-last row by the parity test dheight * 2 <= sheight (:35-38), rows pass then columns
 *     pass, additions in the written order.  Result size round(hgt * .5) x round(w * .5) (:58-59).  A source dimension below 5
 *     (where the forms would overlap or read outside the image): PBD_ERR_ARG.                                                     */
int pbd_resize_area_f64(pbd_handle* h, const double* im, int w, int hgt, int cn, double scale, double* out, int* ow, int* oh);
int pbd_reduce_f64(pbd_handle* h, const double* im, int w, int hgt, int cn, double* out, int* ow, int* oh);
/* Neubeck-Van Gool block NMS on a score map (src/nms.cpp:84-129)             */
int pbd_nms_map(pbd_handle* h, const float* src, int rows, int cols, int sz, uint8_t* dst);

/* ---- host-side post-processing (include/Candidate.hpp:91-99, 277-304) ------
 * operate in place on the arrays returned by detect; pure host code.         */
int pbd_candidates_sort(pbd_candidate_head* heads, int32_t* boxes, int32_t* locs,
                        int count, int max_parts);
int pbd_candidates_nms(pbd_candidate_head* heads, int32_t* boxes, int32_t* locs,
                       int count, int max_parts, int im_w, int im_h, float overlap, int* kept);

/* ---- the same post-step on the device (ros/Node.cpp:192-196, cells/detect.cpp:237-238) ----------------------------------
 * Modes: PBD_CAND_RAW (default) = detect's output as it is; PBD_CAND_SORT = Candidate::sort; PBD_CAND_SORT_NMS = sort, then
 * nonMaximaSuppression(im, candidates, overlap) with the frame's size.  Every whole-path detect entry point of a handle with a
 * mode set (pbd_detect_u8 / _dev_u8 / _enqueue_* + collect, pbd_detect_image, the pbd_detect_batch_* family; the group's two)
 * returns, per frame, exactly what the two host functions above make of the RAW output; counts become the kept counts.  The
 * step runs on the GPU behind the back-tracking, in the frame's stream and graph.  PBD_ERR_CAPACITY: if the records before
 * filtering overflow pbd_options.max_candidates, as with RAW (count = records needed); if the kept records exceed `capacity`,
 * count = kept.  The stage entry points (pbd_dp_argmin) stay unfiltered.  Applies to frames enqueued after the call; any finite
 * overlap (negative: every non-empty box is rejected).  PBD_ERR_ARG: unknown mode, non-finite overlap; PBD_ERR_STATE: a frame
 * is pending, or the handle is a group member (set it on the group).  A captured graph is dropped and captured again.      */
enum { PBD_CAND_RAW = 0, PBD_CAND_SORT = 1, PBD_CAND_SORT_NMS = 2 };
int pbd_set_candidate_filter(pbd_handle* h, int mode, float overlap);
/* every member; the level-sharded pbd_group_detect_u8 filters the union of the members' records on member 0          */
int pbd_group_set_candidate_filter(pbd_group* g, int mode, float overlap);
/* Stand-alone: the caller's `count` host records (max_parts = the handle's) through the same device kernel, in place, ties
 * broken by input position: bit-identical to pbd_candidates_sort then (mode 2) pbd_candidates_nms(im_w, im_h, overlap);
 * *kept = records left.  PBD_ERR_ARG: non-finite scores (their host order is undefined), nparts outside 0..max_parts in
 * mode 2, boxes NULL or im_w / im_h <= 0 in mode 2.  boxes / locs may be NULL in mode 1.  Synchronous.                  */
int pbd_candidates_filter(pbd_handle* h, int mode, float overlap, int im_w, int im_h, pbd_candidate_head* heads,
                          int32_t* boxes, int32_t* locs, int count, int* kept);

/* ---- part-wise overlap NMS: matlab/detection/nms.m, what testmodel.m:15 runs behind every detect as nms(box, 0.3) ---------
 * A different rule from Candidate::nonMaximaSuppression above: detections are compared part by part and by the box covering
 * all parts, the intersection is divided by the KEPT detection's area, and the list is first cut to the `top` best.
 * Input: records in a given order (sorted by the caller, or by the device step), overlap (finite), top >= 0.
 *  1. Cap (nms.m:18-22): if top > 0 and count > top, only the first `top` records take part; the rest are dropped.
 *  2. Rectangles: a record with nparts = P has rectangles r = 0 .. P-1, its part boxes (x, y, w, h), and rectangle P, the
 *     covering box.  Coordinates are int32, their sums and differences 64-bit integers, so junk coordinates of hand-made records
 *     do not overflow.  A box with w <= 0 or h <= 0 is empty: its area is 0 and it meets nothing.  The covering box is
 *     (min x, min y, max(x + w), max(y + h)) over the non-empty part boxes, empty if there are none.  area = w * h (nms.m:35,42
 *     with x2 = x + w - 1); inter(a, b) = max(0, min(ax1, bx1) - max(ax0, bx0)) * max(0, ... y ...).  Both products are formed
 *     as (double)w * (double)h: the 64-bit product converted to double wherever that product fits 64 bits, and defined beyond.
 *  3. Greedy loop (nms.m:53-70): walk the records in order; a record not yet rejected is kept.  After keeping i, every later
 *     undecided record j is rejected iff for some rectangle — the part rectangles r < min(P_i, P_j), or the two covering boxes —
 *     inter(i_r, j_r) / area(i_r) > (double)overlap, in double.  The divisor is the KEPT record's area; 0 / 0 is NaN and rejects
 *     nothing, as MATLAB's max skips NaN.
 *  4. Output: the kept records in order, *kept = their number.
 * Deviations from nms.m: exactly tied scores keep the order of this library's sort (nms.m's order among ties depends on its
 * emission order and on whether the cap fired); records of components with different part counts compare their common leading
 * parts (nms.m assumes one part count); a kept record always leaves the list (nms.m loops forever for overlap >= 1).
 * Hence overlap >= 1 keeps everything under the cap, and with a negative overlap a kept record rejects every later record
 * that shares a rectangle index with one of its non-empty rectangles (0 / area = 0 > overlap).  Nothing is special-cased.
 * Pure host code, in place, like the two functions above.  PBD_ERR_ARG: heads / boxes / kept NULL, count < 0, max_parts <= 0,
 * top < 0, a non-finite overlap, nparts outside 0..max_parts.                                                              */
int pbd_candidates_nms_parts(pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int count, int max_parts,
                             float overlap, int top, int* kept);
/* What the NMS of PBD_CAND_SORT_NMS is, for frames enqueued afterwards: PBD_NMS_PAINTED (default) = nonMaximaSuppression as
 * above; PBD_NMS_PARTS = the rule above with the overlap of pbd_set_candidate_filter and this `top` (1000 reproduces nms.m,
 * 0 = no cap; PAINTED ignores it).  With PARTS every whole-path entry point (single, _dev, enqueue + collect, pbd_detect_image,
 * the batch family, rgbd, latent; the group's two) returns per frame exactly pbd_candidates_sort then pbd_candidates_nms_parts
 * of its RAW output; capacity errors as with the painted NMS.  The other modes launch what they launched before.
 * PBD_ERR_ARG: unknown kind, top < 0; PBD_ERR_STATE: a frame is pending, or the handle is a group member (set it on the
 * group).  A captured graph is dropped and captured again.                                                                */
enum { PBD_NMS_PAINTED = 0, PBD_NMS_PARTS = 1 };
int pbd_set_candidate_nms(pbd_handle* h, int kind, int top);
/* every member; the level-sharded pbd_group_detect_u8 filters the union of the members' records on member 0          */
int pbd_group_set_candidate_nms(pbd_group* g, int kind, int top);
/* Stand-alone: the caller's `count` host records (max_parts = the handle's) through the same device kernels (the sort of
 * k_cand_filter, ties broken by input position, then k_cand_parts), in place: bit-identical to pbd_candidates_sort then
 * pbd_candidates_nms_parts(overlap, top).  PBD_ERR_ARG: non-finite scores or overlap, nparts outside 0..max_parts, boxes
 * NULL, top < 0.  Synchronous.                                                                                          */
int pbd_candidates_filter_parts(pbd_handle* h, float overlap, int top, pbd_candidate_head* heads, int32_t* boxes,
                                int32_t* locs, int count, int* kept);

/* ---- depth-consistency pruning: SearchSpacePruning<T>::filterCandidatesByDepth (src/SearchSpacePruning.cpp:73-94) -------
 * The reference's detect(im, depth, candidates) has the call commented out (src/PartsBasedDetector.cpp:91-93, zfactor 0.03);
 * here it is an opt-in per-handle step on the GPU, behind the back-tracking and in front of the candidate filter above.
 * A candidate of component c is kept iff nparts(c) >= 2 and for every part p in 1 .. nparts(c) - 1 it is NOT true that
 *   mc > 0 and mp > 0 and (double)|mc - mp| > sqrt((double)ax * ax + (double)ay * ay) * (double)zfactor,
 * mc / mp = median of the depth image over box p / over the box of its parent (parentid), |mc - mp| computed in T, and
 * (ax, ay) = anchors[defid[first mixture of part p]] — anchor(0), mixture 0, NOT the mixture the part chose (include/Parts.hpp:183).
 * Kept from the reference:
 *   - single-part components are always dropped: its descending `p >= 1` loop never reaches the `p == 1` push;
 *   - the median is Math::median<T> (include/Math.hpp:63-72): the element of rank floor(n / 2) in ascending order — the upper
 *     median for even n;
 *   - the break only ends the loop early: the result is the AND over p.
 * Defined here where the reference is undefined: -0.0 == +0.0; NaN pixels order above +inf, and a NaN median fails both > 0.
 * Deviation: each box is intersected with the depth image (the reference's depth(box) throws once a box leaves the image,
 * which boxes of parts near the frame edge routinely do); an empty intersection (or w <= 0 / h <= 0) is "no data", median 0,
 * so the pair is not tested.
 * The depth image's element type is T: PBD_DEPTH_32F for float handles, PBD_DEPTH_64F for double handles (Math::median<T>
 * reads it as T; a 16-bit depth map is converted by the caller first, as src/demo.cpp does); else PBD_ERR_UNSUPPORTED.
 *
 * pbd_set_depth_filter: off by default; any finite zfactor (negative: every pair with both medians > 0 fails), else
 * PBD_ERR_ARG.  PBD_ERR_STATE while a frame is pending; PBD_ERR_UNSUPPORTED for a pbd_group member (groups are out of scope).
 * The depth-carrying entry points below take a depth image of the frame's w x hgt, stride in BYTES.  With the setting off (or
 * a NULL depth: an empty Mat) each is exactly its plain counterpart, depth ignored as in the reference's detect().  With it
 * on, the frame's records are pruned; then, with a candidate filter mode set, sorted (and suppressed) — the result equals
 * pbd_candidates_sort / pbd_candidates_nms of the depth-pruned RAW output.  Counts are kept counts; PBD_ERR_CAPACITY as for
 * the plain entry points (records before pruning over pbd_options.max_candidates; kept records over `capacity`).
 * Depth-carrying frames run their launches eagerly, never through a captured graph (a graph stays for the plain frames), so a
 * change of the setting applies to the next frame.  The plain entry points (and pbd_detect_image: non-8-bit colour frames
 * have no depth-carrying variant) take no depth and are never pruned.  pbd_set_levels handles prune their own records.    */
int pbd_set_depth_filter(pbd_handle* h, int on, float zfactor);
int pbd_detect_rgbd_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, const void* depth, int depth_type,
                       int dstride, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int capacity, int* count);
/* then pbd_detect_collect */
int pbd_detect_rgbd_enqueue_dev_u8(pbd_handle* h, const void* d_im, int w, int hgt, int cn, int stride, const void* d_depth,
                                   int depth_type, int dstride);
/* depths[f] may be NULL: frame f is not pruned */
int pbd_detect_batch_rgbd_u8(pbd_handle* h, const uint8_t* const* ims, const void* const* depths, int nframes, int w, int hgt,
                             int cn, int stride, int depth_type, int dstride, pbd_candidate_head* heads, int32_t* boxes,
                             int32_t* locs, int capacity, int* counts);
/* d_depths: nframes depth images packed back to back (stride w * element size); NULL with the setting on: PBD_ERR_ARG.
 * Then pbd_detect_batch_collect. */
int pbd_detect_batch_rgbd_enqueue_dev_u8(pbd_handle* h, const void* d_ims, const void* d_depths, int nframes, int w, int hgt,
                                         int cn, int depth_type);
/* Stand-alone: the caller's `count` host records (max_parts = the handle's; boxes required, locs may be NULL) against a host
 * depth image of any size dw x dh (NULL only with dw or dh 0: every box is then "no data"), filtered in place, stably, through
 * the same device kernels; *kept = records left.  PBD_ERR_ARG: non-finite zfactor, a component out of range, or an nparts
 * that differs from the handle's model for that component.  Synchronous.                                                   */
int pbd_candidates_depth_filter(pbd_handle* h, float zfactor, const void* depth, int depth_type, int dw, int dh, int dstride,
                                pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int count, int* kept);

/* ---- 3-D bounding boxes: Candidate::boundingBox3D (include/Candidate.hpp:140-215) + PointCloudClusterer::computeBoundingBoxes
 * (include/PointCloudClusterer.hpp:53-150) ------------------------------------------------------------------------------------
 * Per record, with boundingBox() = bb (:105-111, the union of the UNCLIPPED part rects: min of x / y, max of x + w / y + h) and
 * boundingBoxNorm() = bbn (:117-130):
 *   - bbn: centroids cvRound((tl + br) * 0.5) (round half to even) of the nparts rects; cv::meanStdDev in double over them,
 *     mean = sum * (1. / n), std = sqrt(max(sqsum * (1. / n) - mean^2, 0)) (OpenCV 2.4 multiplies by the reciprocal);
 *     Rect(xm - 1.5 sx, ym - 1.5 sy, 3 sx, 3 sy), each argument truncated toward zero;
 *   - boxes: the nparts part rects, then bbn, each & (0, 0, im_w, im_h) (an empty intersection is Rect()), scaled to the
 *     depth image by s = (dw / im_w, dh / im_h) in double, x, y, w and h each truncated;
 *   - points: the depth pixels under the boxes, box by box, with multiplicity where boxes overlap, that are != 0 and not NaN
 *     (negative values and +-inf count).  The record is INVALID when the first box with a non-empty ROI has no such pixel
 *     (the reference's in-loop points.empty() return of NaN).  Deviation: a record none of whose boxes has a non-empty ROI is
 *     invalid too (the reference asserts inside cv::resize there);
 *   - the N sorted points through cv::resize(.., Size(1, 400)), INTER_LINEAR, restated from OpenCV 2.4's resizeGeneric_ for
 *     a float column: N == 400 copies; else for each row dy, scale = 1. / (400. / N) (scale_y = 1. / inv_scale_y),
 *     fy = (float)((dy + 0.5) * scale - 0.5), sy = floor(fy), fy -= sy; rows sy and sy + 1 clamped to [0, N - 1] (fy not
 *     reset at the edges); value = S0 * (1.f - fy) + S1 * fy in float (two products, one add, no FMA);
 *   - dpoints = filter2D(points, dog), dog = filter2D(getGaussianKernel(35, 4, CV_32F), (-1, 0, 1) as a column): direct
 *     correlation over dog's nonzero taps in raster order, a float accumulator from 0.0f, one multiply then one add per tap,
 *     BORDER_REFLECT_101 (getGaussianKernel as OpenCV 2.4: t = exp(-0.5 / 16 * x * x) stored as float, summed in double,
 *     each (float)(cf * (1. / sum)); computed on the host);
 *   - from row 200, the walk up and down while (double)fabs(dpoints[m]) <= 0.035 (:197-208) gives rows dmin / dmax;
 *     zmin = points[dmin], zmax = points[dmax];
 *   - the cube (bb.x, bb.y, zmin) .. (bb.br, zmax) is skipped when it contains a NaN (PointCloudClusterer.hpp:80-87: invalid,
 *     or zmax - zmin NaN, e.g. inf - inf): valid = 0, the Rect3d stays (0, 0, 0, 0, 0, 0), no centres;
 *   - else, with ray(u, v) = ((u - cx - tx) / fx, (v - cy - ty) / fy, 1) in double
 *     (image_geometry::PinholeCameraModel::projectPixelTo3dRay): tl = ray(bb.x, bb.y) * zmin, br = ray(bb.x + bb.w, bb.y + bb.h)
 *     * (zmin + (zmax - zmin)), and Rect3d(tl, br) (include/Rect3.hpp:62-64): x3d, y3d, z3d = tl; width3d, height3d, depth3d
 *     = br - tl;
 *   - part centres (:97-141): each part & (0, 0, im_w, im_h) (empty: Rect()); centre (x + w / 2, y + h / 2) in int; avg = the
 *     double sum of the depth pixels over the reference's TRANSPOSED window — rows x .. x + h - 1, columns y .. y + w - 1,
 *     at image coordinates, not scaled (kept quirk) — divided by w * h when that is nonzero; centre = ray(centre) * avg.
 *     Deviation: window pixels outside the depth image read as 0 and still count in w * h (the reference reads out of bounds).
 *     The sum's order is the device's: equal to the reference's wherever every partial sum is exact.
 * Depth: Mat_<float> reads it: PBD_DEPTH_32F as is, PBD_DEPTH_64F rounded to float first (also for the centres: the reference
 * reinterprets non-float bytes there); anything else PBD_ERR_UNSUPPORTED.  None of the OpenCV 2.4 arithmetic above is pinned
 * by a run of OpenCV.                                                                                            */
typedef struct pbd_camera {
  double fx, fy, cx, cy, tx, ty;   /* image_geometry::PinholeCameraModel: fx(), fy(), cx(), cy(), Tx(), Ty()                   */
} pbd_camera;
typedef struct pbd_box3d {
  int32_t valid;                   /* 0: skipped ("contains nans"): Rect3d zero, centres zero                                  */
  int32_t x, y, width, height;     /* the image-space cube: bb                                                                 */
  float zmin, zmax;                /* points[dmin], points[dmax] (NaN when the record had no points)                           */
  int32_t reserved;
  double x3d, y3d, z3d, width3d, height3d, depth3d;   /* the projected Rect3d                                                  */
} pbd_box3d;                       /* 80 bytes                                                                                 */
/* Stand-alone: the caller's `count` host records (heads + boxes, max_parts = the handle's) against a host depth image of any
 * size dw x dh (NULL only with dw or dh 0: every record is then invalid), for an image of im_w x im_h, through the device
 * kernel; out[count]; centres (may be NULL): 3 * max_parts doubles per record, zero beyond nparts.  PBD_ERR_ARG: a NULL camera,
 * non-finite intrinsics or fx / fy zero, nparts outside 1 .. max_parts, im_w or im_h <= 0.  Synchronous.                    */
int pbd_candidates_box3d(pbd_handle* h, const pbd_camera* cam, const void* depth, int depth_type, int dw, int dh, int dstride,
                         int im_w, int im_h, const pbd_candidate_head* heads, const int32_t* boxes, int count, pbd_box3d* out,
                         double* centres);
/* In-frame step, off by default: with it on, the depth-carrying entry points (pbd_detect_rgbd_u8, pbd_detect_rgbd_enqueue_dev_u8
 * + pbd_detect_collect, pbd_detect_batch_rgbd_u8, pbd_detect_batch_rgbd_enqueue_dev_u8 + pbd_detect_batch_collect) compute one
 * pbd_box3d per returned record, with its centres, on the device, in the frame's stream, behind the depth pruning and the
 * candidate filter, from the depth already resident for the frame (the depth filter need not be on; the image is the frame:
 * im = depth size).  The plain entry points, graphs and every existing result are unchanged.  cam is copied; NULL with on:
 * PBD_ERR_ARG.  PBD_ERR_STATE while a frame is pending; PBD_ERR_UNSUPPORTED for a pbd_group member.
 * pbd_get_box3d: after the detect / collect returned, frame `frame`'s results (entry i = the i-th record returned for that
 * frame; centres as for pbd_candidates_box3d, may be NULL); *count = its records (PBD_ERR_CAPACITY over `capacity`).
 * PBD_ERR_STATE after a frame that did not compute them (a plain frame, pbd_dp_argmin / pbd_dp_argbest, the setting off, a batch frame whose depth was NULL, a
 * frame out of range) or while a frame is pending; PBD_ERR_UNSUPPORTED for a pbd_group member.  Buffers are allocated on first
 * use and count in pbd_get_footprint.                                                                                        */
int pbd_set_box3d(pbd_handle* h, int on, const pbd_camera* cam);
int pbd_get_box3d(pbd_handle* h, int frame, pbd_box3d* out, double* centres, int capacity, int* count);

/* ---- object clusters: PointCloudClusterer::clusterObjects (include/PointCloudClusterer.hpp:156-290) -------------------------
 * Per record, from its Rect3d (x3d .. depth3d of its pbd_box3d; a skipped record has all zeros) and an organized cloud of
 * cw x ch points (point index = row * cw + col):
 *   - crop (:190-215): volume() = width3d * height3d * depth3d >= 1e-6, in double on the UNEXPANDED box (kept quirk: a negative
 *     extent on one axis gives a negative volume and skips the record); failing it the record has no points.  Else the box is
 *     expanded, x -= 0.1 * width3d (y, z alike), then width3d *= 1.2 (height3d, depth3d alike); min = (float)tl() and
 *     max = (float)br(), computed in double then rounded (CropBox's Eigen::Vector4f).  A point is kept iff x, y and z are all
 *     finite and min <= p <= max on every axis as float compares (CropBox, identity transform, inclusive faces; kept quirk: an
 *     axis with min > max keeps nothing);
 *   - Euclidean clusters (:224-245, EuclideanClusterExtraction, min size 1, no max): the connected components of the graph on
 *     the cropped points joining two points iff d2 <= r2, d2 = ((dx * dx) + (dy * dy)) + (dz * dz) in float in that order
 *     without FMA, r2 = tol * tol in float.  Deviation: PCL searches an organized cloud through OrganizedNeighbor, whose window
 *     comes from a projection matrix it estimates from the cloud; this is the exact epsilon-graph that search intends;
 *   - the largest cluster (:250-262).  Defined here: ties go to the cluster with the smallest point index, PCL's discovery
 *     order (PCL leaves them to an unstable std::sort);
 *   - its centroid (:264-278).  Deviation: summed in double (any order), divided by the count, reported in double (PCL sums in
 *     float in index order); NaN when nothing was cropped;
 *   - its point indices, ascending (:283-285, ExtractIndices).
 * None of this PCL behaviour is pinned by a run of PCL.                                                          */
typedef struct pbd_cluster3d {
  int32_t cropped;                 /* points inside the expanded box                                                         */
  int32_t nclusters;               /* Euclidean clusters among them                                                          */
  int32_t size;                    /* points of the kept cluster; 0: none                                                    */
  int32_t first;                   /* its smallest point index; -1: none                                                     */
  double cx, cy, cz;               /* its centroid; NaN when none                                                            */
} pbd_cluster3d;                   /* 40 bytes                                                                               */
/* Stand-alone: the caller's organized host cloud (x, y, z floats at the start of each point; point_stride >= 12 and row_stride
 * in BYTES, both multiples of 4, so PCL PointXYZ (16 B) and PointXYZRGB (32 B) buffers go in as they are) against `count`
 * pbd_box3d through the device kernel; out[count].  indices: the kept clusters' points, record after record, each list
 * ascending, at the exclusive prefix sum of out[].size; *idx_total = their number.  indices NULL: a size query (idx_total may
 * then be NULL too); more than idx_capacity: PBD_ERR_CAPACITY with out[] and *idx_total set.  PBD_ERR_ARG: a non-finite or
 * <= 0 tolerance, a stride below 12 (points) or below (cw - 1) * point_stride + 12 (rows) or not a multiple of 4, a NULL cloud
 * with cw * ch > 0, negative sizes.  Synchronous.                                                                             */
int pbd_candidates_cluster3d(pbd_handle* h, const void* cloud, int cw, int ch, int point_stride, int row_stride,
                             const pbd_box3d* boxes, int count, float tolerance, pbd_cluster3d* out, int32_t* indices,
                             int idx_capacity, int* idx_total);
/* In-frame step, off by default: with it on, the frames that compute 3-D boxes (pbd_set_box3d) also compute one pbd_cluster3d
 * per returned record on the device, in the frame's stream, right behind k_box3d, from the frame's cloud: the frame's depth
 * image (cw x ch = the frame) through the camera given to pbd_set_box3d.  For depth d (PBD_DEPTH_64F rounded to float first):
 * z = d, x = (float)(((u - cx - tx) / fx) * d), y = (float)(((v - cy - ty) / fy) * d) computed in double; d == 0 or a
 * non-finite d gives no point (NaN: depth_image_proc / openni).  The plain entry points, graphs and every existing result are
 * unchanged.  tolerance: the reference's 0.010; PBD_ERR_ARG when on and non-finite or <= 0.  PBD_ERR_STATE while a frame is
 * pending; PBD_ERR_UNSUPPORTED for a pbd_group member.
 * pbd_get_cluster3d: after the detect / collect returned, frame `frame`'s results (entry i = the i-th record returned for that
 * frame; indices as for pbd_candidates_cluster3d); *count = its records (PBD_ERR_CAPACITY over `capacity`, or over
 * idx_capacity with *idx_total set).  PBD_ERR_STATE after a frame that computed no 3-D boxes or clusters (pbd_dp_argmin / pbd_dp_argbest among them), or while a frame is
 * pending; PBD_ERR_UNSUPPORTED for a pbd_group member.  Scratch (one whole frame's points per concurrent record) is allocated
 * on first use and counts in pbd_get_footprint.                                                                               */
int pbd_set_cluster3d(pbd_handle* h, int on, float tolerance);
int pbd_get_cluster3d(pbd_handle* h, int frame, pbd_cluster3d* out, int capacity, int* count, int32_t* indices, int idx_capacity,
                      int* idx_total);

/* ---- per-part scores: the decomposition of a detection's score --------------------------------------------------------------
 * The record promises "bounding box and detection confidence for each part" (include/Candidate.hpp:54-72); the reference stores
 * the root score for part 0 and the literal 0.0 for every other part (src/DynamicProgram.cpp:241-244).  This opt-in step computes,
 * on the GPU, what each part of a returned record contributes.  For a record at level n of component c with part locations
 * (x_p, y_p, m_p) — the locs the detect entry points return — and q the parent of part p:
 *   app_p  = resp[n][filterid[p][m_p]](y_p, x_p): the handle's own response value (type T), widened to double;
 *   def_p  = (a_x * (dx * dx) + b_x * dx) + (a_y * (dy * dy) + b_y * dy) for p >= 1, 0 for the root, with
 *            dx = x_q + anchor_x - x_p, dy = y_q + anchor_y - y_p (ints, squared as ints), (a_x, b_x, a_y, b_y) = (-w0, -w1, -w2,
 *            -w3) of defw[defid[p][m_p]] (negated as float, then widened) and the anchor of the same defid — the CHILD's mixture
 *            selects both; in double, products and sums in the order written, never fused: Quadratic::operator()
 *            (include/DistanceTransform.hpp:102-104) at the displacement the distance transform reads out (:175);
 *   bias_p = biasw[biasid[p][m_p] + m_q] for p >= 1 — the child's mixture picks the base, the PARENT's mixture is the offset
 *            (include/Parts.hpp:172-175, src/DynamicProgram.cpp:138-140); bias_0 = biasw[biasid[0][0]], the root's scalar (:165-170).
 * score_p = app_p + def_p + bias_p and total = the sum of score_p in part order are left to the caller (doubles for both handle
 * types).  With pbd_options.dt_correct_ptr = 1 the total reproduces the record's root score up to the DP's own rounding in T
 * (4 * nparts * eps_T * sum(|app| + |def| + |bias|)); with the reference's pointer composition (0, the default) the returned
 * part locations are not the arg-max, so the total is at most the root score and usually below it.
 *
 * pbd_set_part_scores: off by default.  With it on, EVERY whole-path detect of the handle (pbd_detect_u8 / _dev_u8 / _enqueue_* +
 * collect, pbd_detect_image, the pbd_detect_batch_* family, the *_rgbd_* entry points; eager or a captured graph, which is dropped
 * and captured again when the setting changes) scores the records it returns, behind the depth pruning and the candidate filter,
 * in the frame's stream.  No record, count or struct of detect() changes.  PBD_ERR_STATE while a frame is pending;
 * PBD_ERR_UNSUPPORTED for a pbd_group member.  The stage entry point pbd_dp_argmin scores nothing.
 * The step reads the raw response planes after min().  A frame on the compact memory plan (pbd_options.reserved[1] = 2, or automatic
 * for large frames) has overwritten them: its detect succeeds as ever, the step is skipped, and pbd_get_part_scores answers
 * PBD_ERR_UNSUPPORTED with a message that names the plan (handles that need the scores keep dp_mode 0 or 1).
 * pbd_get_part_scores: after the detect / collect returned, frame `frame`'s results: out[i * max_parts + p] for the i-th record
 * returned for that frame, zero beyond the record's nparts; *count = its records (PBD_ERR_CAPACITY over `capacity`, *count = needed).
 * PBD_ERR_STATE after a frame that did not compute them (setting off, pbd_dp_argmin, a frame out of range) or while a frame is
 * pending.  Buffers (24 bytes per part of max_candidates records, pinned, and two small model tables) are allocated on first use
 * and count in pbd_get_footprint.
 * pbd_candidates_part_scores: stand-alone — the caller's `count` host records (heads + locs, max_parts = the handle's) scored
 * against the response planes now resident for the handle's current frame plan (after a detect, pbd_pdf, or pbd_set_level_response
 * of planes of the caller's own), through the same kernel; out[count * max_parts].  `level` indexes the plan's levels: for a batch
 * plan frame f's level l is f * nlevels + l.  PBD_ERR_ARG, with nothing read, for a component out of range, an nparts that differs
 * from the model's, a level outside the plan or not processed by the handle, or an (x, y, mixture) outside its level's cells / the
 * part's mixtures.  PBD_ERR_STATE without resident responses (a compact plan after min(): the message names the plan) or while a
 * frame is pending.  Synchronous.                                                                                              */
typedef struct pbd_part_score {
  double app, def, bias;           /* appearance (response), deformation, bias of one part                                     */
} pbd_part_score;                  /* 24 bytes                                                                                 */
int pbd_set_part_scores(pbd_handle* h, int on);
int pbd_get_part_scores(pbd_handle* h, int frame, pbd_part_score* out, int capacity, int* count);
int pbd_candidates_part_scores(pbd_handle* h, const pbd_candidate_head* heads, const int32_t* locs, int count, pbd_part_score* out);

/* ---- padded feature pyramid with the boundary-occlusion feature (opt-in, off by default; ABI 5, additive) ------------------
 * The third step PartsBasedDetector::detect()'s author wrote and commented out at the call site (after the score-map NMS,
 * reserved[0], and the depth pruning, pbd_set_depth_filter):
 *   copyMakeBorder(feature, padded, 3, 3, 3*flen_, 3*flen_, BORDER_CONSTANT, 0); boundaryOcclusionFeature(padded, flen_, 3);
 * (src/HOGFeatures.cpp:147-148, body at :57-79).  The models are trained by matlab/detection/featpyramid.m:37-44, which pads every
 * level with zero cells and sets the last HOG channel to 1 there: channel flen - 1 of every filter is a learned "this cell lies
 * outside the image" weight, and only a padded pyramid ever shows it a 1.
 *   * Level l has its interior ih x iw cells as without the step (blocks - 2).  Its planes are (ih + 2 pad) x (iw + 2 pad); interior
 *     cell (y, x) sits at (y + pad, x + pad): copyMakeBorder(..., pad, pad, pad * flen, pad * flen, BORDER_CONSTANT, 0).  A level
 *     without interior cells stays empty.
 *   * Border rule of boundaryOcclusionFeature (src/HOGFeatures.cpp:64-79): rows 0 .. pad - 1 and H - pad .. H - 1, columns
 *     0 .. pad - 1 and W - pad .. W - 1 of the padded plane hold 0 in channels 0 .. flen - 2 and 1 in channel flen - 1.  Interior
 *     cells are untouched (their channel flen - 1 is the HOG truncation feature, 0).
 *   * pad = 3 is the reference's literal; featpyramid.m:11-12 uses max filter size - 2 (3 for 5 x 5 filters, 7 for 9 x 9).
 *     0 <= pad <= 8; anything else is PBD_ERR_ARG.
 *   * Boxes: src/DynamicProgram.cpp:239 becomes xy1 = (Point(x, y) - Point(1 + pad, 1 + pad)) * scale, rounded in T as before; sizes
 *     are unchanged.  This is what matlab/detection/detect.m:266-267 does.  The reference's commented-out C++ lines have no such
 *     compensation, because they were never live: it is the one place where the step follows the MATLAB ancestor, not a C++ line.
 *     Boxes may reach further outside the frame than without the step.
 *   * locs stay coordinates in the level's planes, i.e. PADDED coordinates — the ones the pointer tables and the response getters
 *     use.  pbd_pyramid_geometry reports padded cell_w / cell_h; pbd_get_level_features / _response / pbd_get_root /
 *     pbd_get_dp_pointers and the setters address padded planes; pbd_set_level_features takes a full padded plane and uses the
 *     caller's border as given (the next pbd_pyramid_* / detect writes the rule's border again).
 *   * scales, the level images and the number of levels do not change.  The filter bank, the DP, the root reduction, the score-map
 *     NMS and the back-tracking run on the padded planes with no change of their own; the plan's limits (16-bit pointers, the
 *     distance transform's line length, 2^28 cells per level) are checked on the padded sizes.
 * pbd_set_boundary_pad: every detect path of the handle from the next frame on (single, enqueue / collect, batches, device
 * images, pbd_detect_image, *_rgbd_*, the stage entry points; eager or captured).  A different value drops the handle's frame plan
 * and captured graph, as pbd_tune_plan does on return: stage getters answer PBD_ERR_STATE until the next frame.  PBD_ERR_STATE while
 * an enqueued frame or batch is not collected.  With 0 the handle behaves exactly as one that never had the step on.
 * pbd_group_set_boundary_pad forwards to every member (nothing changes unless the value is valid and no member has a frame pending). */
int pbd_set_boundary_pad(pbd_handle* h, int pad);      /* 0 = off (default) */
int pbd_get_boundary_pad(const pbd_handle* h);
int pbd_group_set_boundary_pad(pbd_group* g, int pad); /* forwards to every member */

/* ---- pyramid kind: the image pyramid of matlab/detection/featpyramid.m (ABI 5, additive) ----------------------------------------
 * PBD_PYRAMID_OPENCV (default): HOGFeatures<T>::pyramid, src/HOGFeatures.cpp:95-127 — cv::resize / cv::pyrDown in the pixel type.
 * PBD_PYRAMID_MATLAB: featpyramid.m:13-34, what the MATLAB side of the reference trains and evaluates on.
 *   * Geometry, all in double: sc = 2^(1 / interval) (:13); nlevels = 1 + floor(log(min(w, h) / (5 sbin)) / log(sc)) (:15), a frame
 *     with fewer than `interval` levels is refused as before; level i < interval has factor s_i = 1 / sc^i (:25) and size
 *     round(hgt * s_i) x round(w * s_i) (resize.cc:94-95, C round(): halves away from zero); level j >= interval has size
 *     round(0.5 * dim) of level j - interval (reduce.cc:58-59); box scale sbin / s_i, doubled per octave (featpyramid.m:27,32,47),
 *     converted to float as the last step; cells per level as features.cc computes them.  pbd_pyramid_geometry answers for the
 *     handle's kind.
 *   * Level images are DOUBLE whatever the frame's depth (:22, nothing is rounded back to 8 bits between the stages), interleaved
 *     and row-major; level 0 is the frame converted (resize with scale 1 is the identity); levels < interval by
 *     pbd_resize_area_f64's definition from the frame, levels >= interval by pbd_reduce_f64's from level j - interval (:25,30).
 *     A one-channel frame stays one channel (featpyramid.m:19-21 replicates it: three equal channels give the same gradients).
 *     pbd_get_level_image_raw / pbd_get_frame_level_image_raw return doubles (iw * ih * cn * 8 bytes); pbd_get_level_image
 *     answers PBD_ERR_STATE.  HOG runs on the double images (the instantiation double frames of pbd_detect_image use).
 *   * Everything behind the features is unchanged; boxes keep this port's 0-based convention, with the scales above.  With
 *     pbd_set_boundary_pad the two together are featpyramid.m.
 *   * 8-bit frames only: pbd_detect_image / pbd_pyramid_image of another depth answer PBD_ERR_UNSUPPORTED, as does pbd_tune_plan
 *     and a geometry whose double level images (all frames of a batch) exceed 2 GiB.  Groups have no setter.
 * pbd_set_pyramid_kind: every path of the handle that takes 8-bit frames, from the next frame on (single, enqueue / collect,
 * batches, device images, *_rgbd_*, latent, the stage entry points; eager or captured).  A different value drops the handle's frame
 * plan and captured graph like pbd_set_boundary_pad; PBD_ERR_STATE while a frame is pending, PBD_ERR_ARG for an unknown kind.  Back
 * at PBD_PYRAMID_OPENCV the handle behaves exactly as one that never left it.                                                     */
#define PBD_PYRAMID_OPENCV 0
#define PBD_PYRAMID_MATLAB 1
int pbd_set_pyramid_kind(pbd_handle* h, int kind);
int pbd_get_pyramid_kind(const pbd_handle* h);

/* ---- latent detection: the best pose overlapping given part boxes (ABI 5, additive) ------------------------------------------
 * detect(im, model, thresh, bbox, overlap) of matlab/detection/detect.m:18-23, 60-101, 115-118, 159-161, 342-376, the MATLAB ancestor
 * the C++ DynamicProgram was ported from: given one box per part (an annotation, a tracker), the single highest-scoring pose whose
 * every part overlaps its box by more than `overlap`.  It is how the models are trained (latent positives) and evaluated with a known
 * person box.  Filtering the thresholded output cannot reproduce it: the constraint acts inside the DP, on every part.
 * Inputs, per frame: truth[max_parts][4] int32 boxes in the convention the detect entries return (x, y, width, height of
 *   cv::Rect(xy1, xy2): the box covers pixels x .. x + width, y .. y + height); optional mix[max_parts] int32 (NULL: all free),
 *   -1 = free, m >= 0 = this part must take mixture m (bbox.m, detect.m:90-93); component, -1 = all; overlap in [0, 1).  Component
 *   c uses the first nparts(c) rows.
 * Window of a cell: for part p, mixture m, level n, cell (x, y) the box pbd_dp_argmin would report there — sz = round(rows * scale)
 *   with the rows of the mixture's filter (rows x rows: the size quirk kept), x1 = round((x - org) * scale), y1 alike, org = 1 +
 *   the boundary pad, products in T rounded half to even — covering pixels x1 .. x1 + sz - 1, y1 .. y1 + sz - 1.
 * Overlap (detect.m:360-376), in float64, operations in the order written, never fused, with x2 = x1 + sz - 1 and the truth's
 *   bx1 = tx, bx2 = tx + tw: w = max(0, min(x2, bx2) - max(x1, bx1) + 1), h alike; inter = h * w; area = sz * sz;
 *   box = (tw + 1) * (th + 1); the cell is admissible iff inter / (area + box - inter) > overlap.  A returned record's own boxes as
 *   truth give overlap exactly 1 at that record's cells.
 * Mask: an inadmissible cell of the response plane of (p, m) becomes (T)-1e10 (detect.m's -INF; exact in float).  With mix[p] = m0
 *   every plane of part p other than m0 becomes -1e10 throughout and only m0 gets the overlap mask: the part's admissible cells are
 *   then those of plane m0.
 * Skip rule (detect.m:60-74): a (level, component) pair in which some part has no admissible cell in any of its mixtures yields
 *   nothing.  DEVIATION from MATLAB: it tests mixture 1 only, on its stated assumption that all mixtures of a part have one size;
 *   this library has a size per mixture (pbd_create_sized) and tests them all.
 * Result: over the remaining pairs the maximum of rootv; ties go to the smallest (level, component, y, x) (MATLAB visits the
 *   components in a random permutation: any fixed rule conforms).  It is back-tracked as pbd_dp_argmin does, honouring
 *   dt_correct_ptr.  *found = 0 with PBD_OK when no pair remains.  The model's threshold plays no part (detect.m:20).
 * Domain: the unmasked terms of a configuration sum to less than 5e9 in magnitude (then every pose with a masked cell scores below
 *   every pose without one); outside that the result is unspecified.
 * Limits, each refused with a message: PBD_ERR_UNSUPPORTED when, among the components searched, a filter id is used by two
 *   different (component, part) slots (the mask is written into the shared plane in place; also two mixtures of a part that is given
 *   a mixture), when the score-map NMS is on (reserved[0] > 0), and for pbd_group members; PBD_ERR_ARG for a negative width or
 *   height, overlap outside [0, 1), mix outside the part's mixtures, component out of range; PBD_ERR_STATE while a frame is pending.
 * All three dp_modes and the compact memory plan work: the mask precedes min().  Latent frames run their launches eagerly, as
 * depth-carrying frames do; plain frames and their captured graph are untouched.
 *
 * Stage entry points.  pbd_latent_mask: after pbd_pdf / pbd_set_level_response, before pbd_dp_min: masks the resident planes
 * (pbd_get_level_response then returns them masked); admissible (may be NULL): [nlevels * ncomponents], 1 where the pair remains.  The
 * mask and its flags hold until responses are produced or handed in again.  pbd_dp_argbest: after pbd_dp_min: the result above, as one
 * record (head, boxes[max_parts][4], locs[max_parts][3]; boxes / locs may be NULL); without a mask on the frame's responses every
 * pair counts.  A later pbd_dp_argmin thresholds the root tables again.
 * Whole-path entry points: pbd_detect_u8 / pbd_detect_dev_u8 / pbd_detect_batch_u8 with a truth set per frame (batch: truth
 * [nframes][max_parts][4], mix [nframes][max_parts] or NULL, heads[nframes], boxes[nframes][max_parts][4], locs alike,
 * found[nframes]).  The handle's post steps (candidate filter, per-part scores) run on the single record unchanged; the per-part
 * scores are three scalars per part — what the pose scored, not what it is made of.  The feature vector of detect.m:272-308, the
 * thing the models are trained from, is pbd_candidates_features below, called after the detect.                                    */
int pbd_latent_mask(pbd_handle* h, const int32_t* truth, const int32_t* mix, int component, double overlap, int32_t* admissible);
int pbd_dp_argbest(pbd_handle* h, pbd_candidate_head* head, int32_t* boxes, int32_t* locs, int* found);
int pbd_detect_latent_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, const int32_t* truth, const int32_t* mix,
                         int component, double overlap, pbd_candidate_head* head, int32_t* boxes, int32_t* locs, int* found);
int pbd_detect_latent_dev_u8(pbd_handle* h, const void* d_im, int w, int hgt, int cn, int stride, const int32_t* truth,
                             const int32_t* mix, int component, double overlap, pbd_candidate_head* head, int32_t* boxes,
                             int32_t* locs, int* found);
int pbd_detect_batch_latent_u8(pbd_handle* h, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride,
                               const int32_t* truth, const int32_t* mix, int component, double overlap, pbd_candidate_head* heads,
                               int32_t* boxes, int32_t* locs, int* found);

/* ---- best pose per ground-truth box: matlab/detection/testmodel_gtbox.m and bestoverlap.m (ABI 5, additive) --------------------
 * The evaluation protocol the models' published numbers come from (testmodel_gtbox.m:17-21): detect at the model's threshold, build
 * the ground-truth box of the annotated key points, and keep bestoverlap(box, gtbox, 0.3) — the highest-scoring pose whose box of
 * part CENTRES covers more than `overlap` of the gt box.  Unlike latent detection nothing is constrained inside the DP: the
 * thresholded output is searched.  On the device only the winners come home, one record per gt box, instead of every record.
 * Input: `count` records (head + boxes[max_parts][4] int32 (x, y, w, h)) in a given order; ngt boxes gt[g] = (x1, y1, x2, y2) as
 * doubles; a double overlap.  Everything below is float64, the operations in the order written, never fused.
 *  1. Centres (bestoverlap.m:11-14): part p < nparts of a record has x2 = x + w - 1, y2 = y + h - 1 (the convention of
 *     pbd_candidates_nms_parts for the same MATLAB boxes); its centre is cx = .5 * x + .5 * x2, cy alike.  The int32 -> double
 *     conversions and the halves are exact: nothing rounds here.  w and h take part whatever their sign (MATLAB knows no empty box).
 *  2. Centre box (:15-18): bx1 = min_p cx, bx2 = max_p cx, by1, by2 alike over the record's nparts parts.  A record with nparts == 0
 *     matches nothing.
 *  3. Overlap (:8-9, :20-28): area = (x2 - x1 + 1) * (y2 - y1 + 1) of the gt box; w = min(x2, bx2) - max(x1, bx1) + 1, w < 0 set
 *     to 0, h alike; inter = w * h; o = inter / area.  Nothing is special-cased: a gt box of area 0 gives 0 / 0 = NaN and matches
 *     nothing, a negative area gives o <= 0.
 *  4. Match (:29): the record matches g iff o > overlap — strict, and NaN is false.
 *  5. Pick (:31-33): among the matching records the one with the largest head.score, compared as the stored float (-0.0 == +0.0);
 *     among exactly equal scores the first record in the given order wins (MATLAB's max).  best[g] = its index, o[g] = its
 *     overlap; with no match best[g] = -1 and o[g] = 0.0 (bestoverlap returns [] then).
 *  6. The boxes of one frame are independent: two gt boxes may pick the same record.
 * DEVIATION: within a frame "the given order" is this library's RAW order — level, component, root row, root column (what every
 * detect entry returns) —, where detect_fast.m's find is column-major within a (level, component).  Only exactly tied scores can
 * tell the two apart.
 * PBD_ERR_ARG: a non-finite gt coordinate or overlap; a non-finite score in caller-supplied records; nparts outside 0..max_parts;
 * ngt outside 0..PBD_GT_MAX; NULL where a size is positive.  ngt == 0 or count == 0: PBD_OK with nothing found.
 *
 * pbd_candidates_best_overlap: the definition, pure host code, callable without a GPU (like pbd_candidates_nms_parts).
 * pbd_candidates_select_gt: the caller's host records (max_parts = the handle's) through the device kernels (k_gtbox.hip), ties
 *   broken by input position: bit-identical to pbd_candidates_best_overlap, best and o alike.  Synchronous; PBD_ERR_STATE while a
 *   frame is pending.
 * Whole-path entry points, modelled on the three latent ones: pbd_detect_u8 / pbd_detect_dev_u8 / pbd_detect_batch_u8 with the gt
 *   boxes of the frame, gt[ngt][4] (batch: gt[nframes][PBD_GT_MAX][4] and ngt[nframes], any of them 0).  The frame runs the ordinary
 *   path at the model's threshold with the back-tracking writing into a device list; the selection runs behind it, and per gt box
 *   the winner's whole record is returned: heads[ngt], boxes[ngt][max_parts][4], locs[ngt][max_parts][3] (either may be NULL),
 *   found[ngt] (1 / 0; the record of an unmatched box is left untouched) and o[ngt] (may be NULL).  Batch outputs carry a leading
 *   [nframes] and are strided by PBD_GT_MAX (heads[nframes][PBD_GT_MAX] ...); the levels returned are the frame's own.  Each result
 *   equals pbd_candidates_best_overlap applied to what pbd_detect_u8 returns for the frame (RAW mode), bit for bit.
 *   *nrecords (may be NULL) = the records in front of the selection (a batch: of all its frames), set before anything can fail:
 *   PBD_ERR_CAPACITY when they overflow pbd_options.max_candidates — the selection would be incomplete — with the needed count
 *   there, as the plain entries report it in *count.
 *   PBD_ERR_UNSUPPORTED, each with a message: a candidate filter mode other than PBD_CAND_RAW, depth pruning, 3-D boxes, object
 *   clusters or per-part scores switched on (the stand-alone pbd_candidates_* entries work on the returned records afterwards), and
 *   pbd_group members.  PBD_ERR_STATE while a frame is pending.  All dp_modes and the compact memory plan work: the selection reads
 *   only the records.  The launches are eager, as those of latent and depth-carrying frames; plain frames and their captured graph
 *   are untouched.                                                                                                                 */
#define PBD_GT_MAX 64
int pbd_candidates_best_overlap(const pbd_candidate_head* heads, const int32_t* boxes, int count, int max_parts, const double* gt,
                                int ngt, double overlap, int32_t* best, double* o);
int pbd_candidates_select_gt(pbd_handle* h, const double* gt, int ngt, double overlap, const pbd_candidate_head* heads,
                             const int32_t* boxes, int count, int32_t* best, double* o);
int pbd_detect_gtbox_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, const double* gt, int ngt,
                        double overlap, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int* found, double* o,
                        int* nrecords);
int pbd_detect_gtbox_dev_u8(pbd_handle* h, const void* d_im, int w, int hgt, int cn, int stride, const double* gt, int ngt,
                            double overlap, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int* found, double* o,
                            int* nrecords);
int pbd_detect_batch_gtbox_u8(pbd_handle* h, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride,
                              const double* gt, const int* ngt, double overlap, pbd_candidate_head* heads, int32_t* boxes,
                              int32_t* locs, int* found, double* o, int* nrecords);

/* ---- feature vectors of detections: what the models are trained from (ABI 5, additive) ------------------------------------------
 * detect(im, model, thresh, bbox, overlap, id, label) of matlab/detection/detect.m collects, while it back-tracks a pose (:272-308),
 * the pose's sparse feature vector ex.blocks — per part a bias block, a deformation block and the HOG window under the part's
 * filter — which qp_write.m stores; its "Crucial DEBUG assertion" (:139-145) checks that the weight vector dotted with that feature
 * reproduces the DP's score.  This is that feature, gathered on the GPU from the planes already resident.
 * For a record at plan level n of component c with part locations (x_p, y_p, m_p) and q the parent of p — the conventions of
 * pbd_part_score above — part p contributes ONE block:
 *   bias_id   = biasid[p][m_p] + m_q (the child's mixture picks the base, the parent's the offset); the root: biasid[0][0].  Value 1.
 *   def_id    = defid[p][m_p]; -1 for the root.
 *   def       = (-(dx * dx), -dx, -(dy * dy), -dy) with dx = x_q + anchor_x - x_p, dy = y_q + anchor_y - y_p, the anchor of the same
 *               defid (the CHILD's mixture selects both).  Integers, negated as integers and widened to double (a level may be
 *               65535 cells wide: dx * dx is no float, and a zero stays +0.0).  The root: zeros.
 *   filter_id = filterid[p][m_p] (the caller's filter order, as pbd_get_filter_size), kh x kw = that filter's size.
 *   window    : win[i][j][ch] = feat[n](y_p - kh / 2 + i, x_p - kw / 2 + j, ch) for i < kh, j < kw, ch < flen, laid out [kh][kw * flen]
 *               like the filter itself.  Integer divisions: the anchor of the filter bank (cv::filter2D's normalizeAnchor).  A cell
 *               outside the level's plane contributes the bank's border value: 0 in channels 0 .. flen - 2 and 1 in channel
 *               flen - 1.  With pbd_set_boundary_pad on, locs and planes are the padded ones and the same rule applies at the
 *               padded plane's edge; nothing else changes.  The values are the handle's own feature values in T, copied, not
 *               recomputed.
 * Then sum_p (filter . win + defw[def_id] . def + biasw[bias_id]) is the pose's score: with pbd_options.dt_correct_ptr = 1 the
 * record's root score up to the rounding of the filter bank and the DP (the bound of pbd_part_score plus the bank's summation
 * error), with the reference's pointer composition at most that.  The dense layout of the weight vector is the binding's business
 * (partsbaseddetector_amd/model.py: Model.weight_vector).
 *
 * pbd_feature_window_max: wmax = the largest kh * kw * flen over the bank (negative: error code).  A record's blocks are
 * blocks[max_parts], its windows windows[max_parts][wmax]: a smaller window sits at the front of its slot, the tail zero; part slots
 * beyond the record's nparts hold ids -1 and zeros.
 * pbd_candidates_features (float windows) / _f64 (double windows; the scalar type must match the handle's, as for
 * pbd_get_level_features[_f64]: PBD_ERR_STATE otherwise): stand-alone and synchronous — the caller's `count` host records (heads +
 * locs, max_parts = the handle's) against the features now resident for the handle's current frame plan: after any detect, a latent
 * or batch detect, pbd_pyramid_*, or pbd_set_level_features.  `level` indexes the plan's levels: on a batch plan frame f's level l
 * is f * nlevels + l (the pbd_candidates_part_scores convention).  blocks[count * max_parts], windows[count * max_parts * wmax].
 * pbd_candidates_features_dev: the same kernel into the caller's DEVICE buffers (d_windows in the handle's T, 16-byte aligned), on
 * the handle's stream: the records are uploaded when it returns, the kernel is enqueued, not finished (synchronise the stream
 * before reading).  A training loop keeps everything on the GPU that way.  The host variants are this one into a handle-owned
 * staging buffer of at most PBD_FEATVEC_STAGING_BYTES plus a copy, chunk by chunk; the staging buffer and the record buffer are
 * allocated on first use and count in pbd_get_footprint.
 * There is no in-frame opt-in step: a person-model record is 83 KB where its part scores are 624 B, callers select records (NMS,
 * latent detection) before they want features, and the stand-alone call behind the detect gathers them in one launch.
 * PBD_ERR_ARG, with nothing written, for a component out of range, an nparts that differs from the model's, a level outside the
 * plan or not processed by the handle, or an (x, y, mixture) outside its level's cells / the part's mixtures; PBD_ERR_STATE
 * without resident features (a compact memory plan after min(): the message names the plan) or while a frame is pending;
 * PBD_ERR_UNSUPPORTED for a pbd_group member.  count == 0 is PBD_OK.                                                              */
typedef struct pbd_feature_block {
  int32_t bias_id, def_id, filter_id, kh, kw, reserved;
  double def[4];
} pbd_feature_block;                                   /* 56 bytes */
#define PBD_FEATVEC_STAGING_BYTES ((size_t)16 << 20)
int pbd_feature_window_max(const pbd_handle* h);
int pbd_candidates_features(pbd_handle* h, const pbd_candidate_head* heads, const int32_t* locs, int count,
                            pbd_feature_block* blocks, float* windows);
int pbd_candidates_features_f64(pbd_handle* h, const pbd_candidate_head* heads, const int32_t* locs, int count,
                                pbd_feature_block* blocks, double* windows);
int pbd_candidates_features_dev(pbd_handle* h, const pbd_candidate_head* heads, const int32_t* locs, int count,
                                pbd_feature_block* d_blocks, void* d_windows);

/* ---- training example cache: qp_write, score and lincomb on the GPU (ABI 5, additive) -------------------------------------------
 * detect(im, model, thresh, bbox, overlap, id, label) of matlab/detection/detect.m hands every back-tracked pose to qp_write(ex)
 * (matlab/learning/train.m:102), which appends it to the QP's cache of block-sparse examples; matlab/mex/score.cc and lincomb.cc sweep
 * that cache.  pbd_qp is that cache, resident on the device: detections are written into it from the feature planes without leaving
 * HBM, it is scored against a weight vector and combined linearly into one.  The coordinate-descent solver over it
 * (matlab/mex/qp_one_sparse.cc, qp_one.m, qp_refresh.m, qp_opt.m with its loss, qp_prune.m, qp_w.m) is the "QP solver" section
 * below: the columns never leave the device.  pbd_qp_get and pbd_qp_put remain for columns made or inspected elsewhere.
 *
 * Dense index space: Model.feature_layout() of the binding — [biasw | defw (ndefs x 4) | the filters back to back in the caller's
 *   order, each [kh][kw * flen]] —, length len.  len >= 2^24 is refused (PBD_ERR_UNSUPPORTED): block bounds are stored as floats,
 *   as in MATLAB (train.m:59, qp.x is single).
 * Example column: qp.x(:,i) verbatim (qp_write.m:46-68), k float32 values: x[0] = number of blocks, then per block i1, i2 (1-based
 *   inclusive bounds into the dense space) and its i2 - i1 + 1 values; the tail is zero.  A column read back can be handed to the
 *   compiled reference files.  k is sparselen of train.m:207-239 — 1 + 2 * blocks + values of a pose —, the maximum over the
 *   components, each part counted at its largest mixture's filter (train.m counts the first mixture's).
 * Block order: detect.m:272-308 — the root's bias, the root's window; then per later part, in part order, bias, deformation, window.
 *   Ids, deformation values and window contents are exactly those of pbd_feature_block above (border rule, padded planes, the
 *   handle's own feature values in T): the same device text gathers both (csrc/featvec_gather.hpp).  The window is laid out
 *   [kh][kw][flen] like this port's filters, not MATLAB's column-major [sizy][sizx][flen].
 * Standardisation (qp_write.m:49-72): C = label > 0 ? cpos : cneg; with label <= 0 every value v is negated first (a zero
 *   becomes -0.0); the stored value is (float)((C * v) / wreg[j]) with v widened to double, evaluated in that order; d is the sum of
 *   the squares of the unrounded double values (C * v) / wreg[j]; b = (float)(C * (1 - sum_blocks w0[j] . v)), v signed and
 *   unscaled (qp_write.m:59 runs before :60).  MATLAB's x'*x has no defined order; this library's is fixed: a block's sum is 64
 *   partial sums (partial t starts at +0.0 and adds the block's terms t, t + 64, ... in that order), folded s[t] += s[t + h] for
 *   h = 32, 16, .. 1; d adds the blocks' sums to 0 in block order, and 1 has the blocks' sums subtracted in block order.  No
 *   product is fused into a sum.  It does not depend on the launch, the capacity or the record's position in the call.
 * Example id: five int32 (label, id, level, x_root, y_root), level and root location as the record carries them.  DEVIATION:
 *   detect.m:273 stores round(x + sizx / 2); this port stores its root cell.  Ids are only ever compared for equality.  The
 *   component is not part of it, as in MATLAB.
 * Defaults (matlab/learning/model2vec.m): wreg = .01 at the root bias of every component, 1 elsewhere; w0 = .01 at elements 0 and 2 of
 *   every deformation, 0 elsewhere.  The caller may pass their own (len doubles each; wreg finite and non-zero).
 * Repeated blocks: a record whose blocks repeat a dense start index (two parts of the pose share a filter, def or bias id) hits
 *   qp_write's assertion (:34-35): checked on the host before any launch, PBD_ERR_ARG with nothing written, for the whole call.
 *
 * pbd_qp is bound to the handle it was created from (model tables, scalar type, stream, device) and must be destroyed before it;
 * pbd_group members are refused (PBD_ERR_UNSUPPORTED).  Indices are 0-based.  Errors are reported through the handle
 * (pbd_last_error).  capacity >= 1 examples.
 * pbd_qp_write: `count` host records (heads + locs, as pbd_candidates_features_dev: same preconditions and refusals) against the
 *   handle's resident feature planes; appends min(count, capacity - n) examples — a full cache is no error (qp_write.m:21-23) —,
 *   *written = that number.  A full cache returns at once: nothing is uploaded.  Otherwise the records' upload synchronises the
 *   handle's stream (earlier work on it is done when the call returns); the kernel is then enqueued on that stream, not finished.
 *   There is no scalar-type refusal (PBD_ERR_STATE of the _f64 entries elsewhere): no pbd_qp entry takes a pointer typed by the
 *   handle's scalar — columns are float32, sums and weights double on float and double handles alike — so a mismatch cannot arise.
 * pbd_qp_score (matlab/mex/score.cc): out[i] = the score of w on example inds[i] — each product rounded, added in storage order,
 *   bit for bit what the compiled reference file computes; inds NULL: examples 0 .. n - 1.  _dev: device pointers, enqueued on the
 *   handle's stream (inds are not range-checked there: the caller's business).
 * pbd_qp_lincomb (matlab/mex/lincomb.cc): w_out = sum_i a[inds[i]] * x(:, inds[i]), w starting at zero, the examples added in the
 *   order of inds (qp_refresh.m:16-17 sorts by a for a reason), each product rounded: bit for bit the reference file's.  a is
 *   indexed by example, capacity doubles.  _dev as above.  No atomics, no tree: qp_one_sparse.cc branches on G > 1e-12 and on
 *   A[i] == 0 && G >= 0, and a solver fed sums that vary with the launch is not reproducible.
 * pbd_qp_keep (qp_prune.m:18-25): with inds strictly ascending, the kept examples become 0 .. n - 1 in that order.  An index table
 *   is permuted; no column moves.
 * pbd_qp_get: examples i0 .. i0 + n - 1 (i0 + n <= capacity: columns behind the cache's n can be read too) — x[n * k],
 *   ids[n * 5], b[n], d[n], each may be NULL.  pbd_qp_put appends n columns made elsewhere (warped positives): every column's block
 *   bounds are validated against len and k (PBD_ERR_ARG, nothing appended); more than 3 * max_parts blocks in a column — more than
 *   any pose has — is PBD_ERR_UNSUPPORTED; beyond the capacity: PBD_ERR_CAPACITY, nothing appended.
 * pbd_qp_footprint: device bytes held by the cache.                                                                               */
typedef struct pbd_qp pbd_qp;
int pbd_qp_create(pbd_handle* h, int capacity, double cpos, double cneg, const double* wreg, const double* w0, pbd_qp** qp);
void pbd_qp_destroy(pbd_qp* qp);
int pbd_qp_dims(const pbd_qp* qp, int* len, int* k, int* capacity, int* n);
int pbd_qp_footprint(const pbd_qp* qp, size_t* bytes);
int pbd_qp_write(pbd_qp* qp, const pbd_candidate_head* heads, const int32_t* locs, int count, int label, int id, int* written);
int pbd_qp_score(pbd_qp* qp, const double* w, const int32_t* inds, int n, double* out);
int pbd_qp_score_dev(pbd_qp* qp, const double* d_w, const int32_t* d_inds, int n, double* d_out);
int pbd_qp_lincomb(pbd_qp* qp, const double* a, const int32_t* inds, int n, double* w_out);
int pbd_qp_lincomb_dev(pbd_qp* qp, const double* d_a, const int32_t* d_inds, int n, double* d_w_out);
int pbd_qp_keep(pbd_qp* qp, const int32_t* inds, int n);
int pbd_qp_get(pbd_qp* qp, int i0, int n, float* x, int32_t* ids, float* b, double* d);
int pbd_qp_put(pbd_qp* qp, int n, const float* x, const int32_t* ids, const float* b, const double* d);

/* ---- QP solver: qp_one_sparse.cc, qp_one.m, qp_refresh.m, qp_opt.m, qp_prune.m and qp_w.m on the cache (ABI 5, additive) ----------
 * detect -> pbd_qp_write -> pbd_qp_opt -> pbd_qp_weights is a closed loop on the device: what crosses PCIe in a solver call is per
 * example (a, sv, ids, b, a score), never a column, and the next model's weights come back once.  The calls are synchronous and
 * finish on the handle's stream.
 *
 * State (device resident, allocated by the first call of this section — pbd_qp_footprint of a cache that never solves is unchanged):
 *   a[capacity] double and sv[capacity] bytes, indexed by EXAMPLE; w[len] double; the scalars l, lb, lb_old, ub; noneg (p dense
 *   indices); nfix (svfix = examples 0 .. nfix - 1).  It starts at a = 0, sv = 1 for the examples held and 0 behind them, w = 0,
 *   scalars 0, no noneg, nfix = 0.  From then on examples appended by pbd_qp_write / pbd_qp_put get a = 0, sv = 1 (qp_write.m:74).
 *   pbd_qp_keep renumbers examples and does NOT move a and sv (its caller does, as before); pbd_qp_prune moves them.
 * pbd_qp_noneg: the dense indices whose weights are clamped at zero (Model.qp_vectors()[3] of the binding); an index outside
 *   [0, len) is PBD_ERR_ARG.  pbd_qp_fix: nfix in [0, n], else PBD_ERR_ARG.
 * pbd_qp_state_put: a and sv of examples 0 .. n - 1 (n <= capacity; either may be NULL).  pbd_qp_state_get: a[capacity],
 *   sv[capacity], w[len], stats[4] = l, lb, lb_old, ub; any may be NULL.
 * pbd_qp_pass: matlab/mex/qp_one_sparse.cc with C = 1 (qp_one.m:15) over the examples `order` — distinct, inside [0, n); a duplicate
 *   or an index out of range is PBD_ERR_ARG, an empty cache PBD_ERR_STATE, a column of pbd_qp_put whose blocks overlap each other
 *   PBD_ERR_UNSUPPORTED (the axpy has one writer per element), each with the state untouched.  *loss = the file's return value.
 *   ONE workgroup runs the whole pass (one CU of the device, by construction: the pass is serial across examples, parallel within
 *   one).  Everything scalar is the file's :171-253 line for line in double, nothing fused, MAX / MIN with the macros' operand order.
 *   sumAlpha (:90-124) runs on the host before the launch: groups in memcmp order of the 20-byte id, ties in the order of `order`.
 *   The sums use this library's order, the block sum stated above for d and b:
 *     score(W, x): a block's products W[j] * (double)x go through the block sum; y starts at 0 and adds the blocks' sums in block order.
 *     dot(x, x2): DEVIATION — the file's merge walk assumes ascending blocks, and this port's columns are in detect.m's order (bias,
 *       window, bias, def, window ...), not ascending in the dense layout.  The library's dot is the complete one: for every block
 *       of x in order, for every block of x2 in order, a non-empty intersection's products (double)x * (double)x2 go through the
 *       block sum and are added to the result, which starts at 0, in that order.  On ascending columns where a block meets at most
 *       one block of the other column this is the file's value in exact arithmetic.
 *     add(W, x, dA): per element one rounded product dA * (double)x and one rounded sum; in the pair branch x, then x2 with -dA,
 *       then the noneg clamp.
 *     loss: err[0] + err[1] + ... left to right.
 *   The result does not depend on the capacity, the columns the examples occupy or the launch.  DEVIATION from the reference in
 *   bits, as for d and b: the file adds strictly left to right; exact comparisons (G > 1e-12, A[i] == 0, Ci >= C) may then fall
 *   differently, so the trajectories are compared through the dual and primal bounds, not element by element.
 * pbd_qp_refresh (qp_refresh.m): I = the examples with a > 0 over the capacity, sorted by a ascending, stable; none: example 0.
 *   l = sum (double)b * a, each product rounded, added left to right in that order; w = pbd_qp_lincomb over I; the noneg clamp;
 *   lb_old = lb; lb = l - w'w * .5.  w'w, which MATLAB leaves to the BLAS, is the block sum over the whole of w.
 * pbd_qp_one (qp_one.m:15-139): the pass, the refresh, sv(svfix) = 1, lb_old = lb (after the refresh moved it, as the file does),
 *   lb = l - w'w * .5, ub = w'w * .5 + loss.
 * pbd_qp_loss (computeloss, qp_opt.m:56-86) over examples 0 .. n - 1: scores by pbd_qp_score; per id the largest slack if positive;
 *   ids in ascending numeric lexicographic order of their five words (sortrows), the ids' terms added left to right.  DEVIATION:
 *   MATLAB computes qp.b(I) - score(...) in single (single - double is single); the library computes (double)b - score in double.
 * pbd_qp_opt (qp_opt.m): the refresh, the true upper bound, sv(0 .. n - 1) = 1, then up to max_iter times pbd_qp_one over a shuffle
 *   of find(sv), the test lb > 0 && 1 - lb / min(qp.ub, ub) < tol, the true-ub check and the sv reset; finally qp.ub = ub.  *passes
 *   = the number of pbd_qp_one calls.  randperm is replaced by a stated generator: find(sv) ascending in v[0 .. m - 1], then
 *   for t = m - 1 .. 1: j = next() mod (t + 1), swap v[t], v[j]; next() is splitmix64 (state += 0x9E3779B97F4A7C15; z = state;
 *   z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31) with state = seed at the
 *   start of the call: one stream through the whole call.
 * pbd_qp_prune (qp_prune.m): if sv is set over the whole capacity, sv = a > 0 and sv(svfix) = 1; I = find(sv) among the n examples
 *   (none: PBD_ERR_STATE, nothing changed); pbd_qp_keep(I); a and sv move with their examples, sv = 1 on them, both 0 behind;
 *   l and w rebuilt in index order (pbd_qp_lincomb with inds NULL), the clamp, lb = l - w'w * .5; lb_old is left alone.  *n = |I|.
 * pbd_qp_weights (qp_w.m): w_out[len] = w ./ wreg + w0.                                                                            */
int pbd_qp_noneg(pbd_qp* qp, const int32_t* idx, int p);
int pbd_qp_fix(pbd_qp* qp, int nfix);
int pbd_qp_state_put(pbd_qp* qp, const double* a, const unsigned char* sv, int n);
int pbd_qp_state_get(pbd_qp* qp, double* a, unsigned char* sv, double* w, double* stats);
int pbd_qp_pass(pbd_qp* qp, const int32_t* order, int n, double* loss);
int pbd_qp_one(pbd_qp* qp, const int32_t* order, int n);
int pbd_qp_refresh(pbd_qp* qp);
int pbd_qp_loss(pbd_qp* qp, double* loss);
int pbd_qp_opt(pbd_qp* qp, double tol, int max_iter, uint64_t seed, double* lb, double* ub, int* passes);
int pbd_qp_prune(pbd_qp* qp, int* n);
int pbd_qp_weights(pbd_qp* qp, double* w_out);

/* ---- warped positives: warppos.m and train.m's poswarp into the example cache (ABI 5, additive) ------------------------------------
 * The first branch a training run executes (trainmodel.m:35, train.m:131-161 with warp = 1): every positive box is cropped with a
 * replicated border, resized to the filter's size plus one cell on every side, its HOG taken and written as a two-block example.
 * Here the crop, the resize, the HOG and the write run on the device: no window, feature plane or column crosses PCIe.
 *
 * Inputs: one 8-bit frame, cn 1 or 3 (a grey frame is replicated to three planes, warppos.m:18-20); n boxes (x1, y1, x2, y2) as
 *   doubles in the .m files' 1-BASED INCLUSIVE pixel coordinates — pixel (1, 1) is im[0, 0]; the rounding below is not
 *   shift-invariant at halves, so the convention is part of the definition —; a filter index of the handle (the caller's order):
 *   kh x kw = pbd_get_filter_size, sbin the model's.
 * Crop (warppos.m:21-27, subarray.m:10-17 with pad = 1), in double, in this order: padx = sbin * (x2 - x1 + 1) / (kw * sbin), pady
 *   alike with kh; X1 = round(x1 - padx), X2 = round(x2 + padx), Y1, Y2 alike, round() rounding halves away from zero.  Window pixel
 *   (i, j) is image pixel (clamp(Y1 + i, 1, H), clamp(X1 + j, 1, W)), widened to double.  The crop is never materialised: it is an
 *   index clamp inside the resize's reads.
 * Resize to oh = (kh + 2) * sbin, ow = (kw + 2) * sbin.  MATLAB's imresize is a binary; the definition is the documented contributions
 *   algorithm, stated here.  Per axis, from n_in to n_out: s = n_out / n_in; width = s < 1 ? 2 / s : 2; P = ceil(width) + 2; for output
 *   x = 1 .. n_out: u = x / s + 0.5 * (1 - 1 / s), left = floor(u - width / 2), taps p = 0 .. P - 1 at ind = left + p with weight
 *   s * max(0, 1 - |s * (u - ind)|) for s < 1 (the antialiased form), max(0, 1 - |u - ind|) otherwise, each divided by the sum of the P
 *   weights added left to right; source index aux[(ind - 1) mod 2 n_in] with aux = [1 .. n_in, n_in .. 1] (MATLAB's mirror).  The
 *   axis with the smaller s goes first, a tie goes to rows (y).  An output element is the sum over ALL P taps, zero weights included:
 *   each product rounded, added to +0.0 in ascending p, never fused.  The result is double, with no clamp.
 *   DEVIATION: MATLAB's own summation order is unknown; this order is the library's.  Octave's imresize is a different function and
 *   is not followed.  The weights are computed once, in double, on the host (pbd_warp_taps) and uploaded: the device multiplies by
 *   exactly the numbers pbd_warp_taps returns.
 * HOG: features(window, sbin) -> kh x kw x 32, by the kernel every pyramid level goes through, over the windows as level images of
 *   PBD_DEPTH_64F, in the handle's scalar T — bit for bit what pbd_pyramid_image + pbd_get_level_features give for that window.
 * Column (train.m:152-161, qp_write.m): two blocks, the bias block [1] at dense index `bias`, then the window [kh][kw][flen] at the
 *   filter's dense start; label 1, so C = cpos; ids (1, id, 0, 0, 0).  Standardisation, d, b and the block sums are exactly those of
 *   pbd_qp_write (the same device text); the solver's state of new examples is a = 0, sv = 1.
 *
 * pbd_warp_geometry, pbd_warp_taps: the planner, pure host code, callable without a GPU.  _geometry: rect[4] = X1, Y1, X2, Y2
 *   (1-based, unclamped), *rows_first = 1 where y is resampled first, *py / *px = P of the axes; outputs may be NULL.  PBD_ERR_ARG: a
 *   non-finite or inverted box (x2 < x1 or y2 < y1), kh / kw / sbin < 1; PBD_ERR_UNSUPPORTED: a crop side beyond 16384 pixels or a
 *   coordinate beyond 2^30 in magnitude.  _taps: one axis — *ntaps = P, and with index / weight non-NULL, [n_out][P] 0-based source
 *   indices inside the crop (mirror resolved) and normalised weights; `capacity` elements each, PBD_ERR_CAPACITY below n_out * P;
 *   n_in, n_out in [1, 16384].
 * pbd_warp_windows_u8 / _u8_f64 (float / double handles, PBD_ERR_STATE on the other): the stand-alone staging entry —
 *   windows[n][oh][ow][3] as doubles and features[n][kh][kw][32] in T of all n boxes (either may be NULL).  Synchronous.
 * pbd_qp_write_warped_u8: poswarp.  Boxes with (x2 - x1 + 1) * (y2 - y1 + 1) < min_area are skipped (train.m:139-143; the caller
 *   computes min_area = prod(maxsize * sbin), train.m:135); of the others the first min(count, capacity - n) are written — a full cache
 *   is no error — in box order; *written = that number; status[i] (may be NULL) = PBD_WARP_WRITTEN, PBD_WARP_SKIPPED or
 *   PBD_WARP_FULL.  ids[i] is box i's id (NULL: i).  Synchronous: the examples are in the cache when the call returns.
 * Refusals, each with a message and nothing written: PBD_ERR_ARG — a non-finite or inverted box, filter or bias out of range, a bad
 *   frame argument, NaN min_area; PBD_ERR_UNSUPPORTED — pbd_group members, a crop side beyond the limit above, a frame of 2^31 bytes
 *   or more, a filter whose window does not fit the cache's column length; PBD_ERR_STATE — a frame pending.  A repeated dense start
 *   (qp_write.m:34-35) cannot arise: the bias block starts below nbias, every filter's at or above it.                              */
#define PBD_WARP_SKIPPED 0
#define PBD_WARP_WRITTEN 1
#define PBD_WARP_FULL 2
int pbd_warp_geometry(const double* box, int kh, int kw, int sbin, int32_t* rect, int32_t* rows_first, int32_t* py, int32_t* px);
int pbd_warp_taps(int n_in, int n_out, int32_t* index, double* weight, int capacity, int32_t* ntaps);
int pbd_warp_windows_u8(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, const double* boxes, int n, int filter,
                        double* windows, float* features);
int pbd_warp_windows_u8_f64(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, const double* boxes, int n, int filter,
                            double* windows, double* features);
int pbd_qp_write_warped_u8(pbd_qp* qp, const uint8_t* im, int w, int hgt, int cn, int stride, const double* boxes, const int32_t* ids,
                           int n, int filter, int bias, double min_area, int32_t* status, int* written);
/* the last pbd_warp_windows_* / pbd_qp_write_warped_u8 call's launches, in ms between events on the handle's stream, while
 * pbd_set_profiling is on (zeros otherwise): [0] the two resample passes, [1] the HOG, [2] the write (0 for pbd_warp_windows_*) */
int pbd_debug_warp_ms(const pbd_handle* h, float ms[3]);

/* ---- weight and threshold updates: vec2model.m on a live handle (ABI 5, additive) ---------------------------------------------------
 * train.m:94,112: model = vec2model(qp_w, model), then detect(im, model, -1, ...) on the negatives with the new weights.  A pbd_qp cache
 * reads the feature planes of the handle it was created on, so the new weights go INTO that handle; the cache's columns are features,
 * not weights, and stay valid.
 *
 * A weight vector has Model.feature_layout()'s order — the order pbd_qp_weights returns and pbd_qp_create derives len from —:
 *   [biasw | defw (ndefs x 4) | the filters back to back in the caller's filter order, each [kh][kw * flen]].
 * The model stores float32: every element becomes (float)w[i], round to nearest even.  After a successful call the handle behaves in
 * every entry point exactly like a handle freshly created from the same model with those weights, the same options and the same
 * setters.  pbd_options.conv_mode's resolution is NOT repeated: pbd_get_conv_mode is constant over a handle's life.  A geometry chosen
 * by pbd_tune_plan survives.  The frame plan is dropped (as after pbd_set_levels): stage getters answer PBD_ERR_STATE until the next frame.
 *
 * pbd_set_weights: a host vector.  pbd_set_weights_dev: a device vector on the handle's device.  pbd_get_weights: the handle's current
 *   float32 weights, widened.  pbd_qp_apply_weights: the solver's resident w ./ wreg + w0 (pbd_qp_weights) into the cache's handle, with
 *   no copy through the host; it needs what every solver entry needs.
 * pbd_set_threshold: replaces the model's thresh for min(), argmin(), the score-map NMS and every detect path; any value but NaN
 *   (train.m uses 0 for latent positives, -1 for mining, then the 5th percentile of the positives' scores).  A min() that is resident
 *   keeps its root tables: the next argmin() thresholds them again.
 * All are synchronous: the update is complete on return.
 * Refusals, each with a message, changing nothing (a detect afterwards returns the bits it returned before):
 *   PBD_ERR_ARG — a NULL argument; len other than the layout's size; an element that is not finite as a float32; a quadratic
 *     deformation weight (elements 0 and 2 of a deformation a non-root part uses) that is zero as a float32; a NaN threshold.
 *   PBD_ERR_UNSUPPORTED — a filter weight with |w| >= 3e38 on a PBD_CONV_SPLIT / PBD_CONV_SPLIT_F16 handle (as at pbd_create); a
 *     pbd_group member.
 *   PBD_ERR_STATE — a frame or batch in flight between enqueue and collect.                                                          */
int pbd_set_weights(pbd_handle* h, const double* w, int len);
int pbd_set_weights_dev(pbd_handle* h, const double* d_w, int len);
int pbd_get_weights(const pbd_handle* h, double* w, int len);
int pbd_qp_apply_weights(pbd_qp* qp);
int pbd_set_threshold(pbd_handle* h, float thresh);
int pbd_get_threshold(const pbd_handle* h, float* thresh);

/* ---- hard-negative mining: detections into the example cache (ABI 5, additive) ---------------------------------------------------------
 * train.m:99-108 runs, once per negative image i, [box, model] = detect(im, model, -1, [], 0, i, -1): every detection above the
 * threshold becomes an example of label -1 (detect.m:127-133 -> qp_write.m), the upper bound grows by its slack (detect.m:135), and the
 * solver runs when the bounds have drifted apart (detect.m:148-149, optimize: 315-325).  pbd_qp_mine_* is that call on the cache's
 * handle with the frame's records left on the device: the image goes in; per frame ONE small block comes out (the record count, the
 * first record the write would refuse, the frame's sum S_f below).  No record crosses PCIe, in either direction.
 *
 * Detection.  The frame is detected exactly as pbd_detect_u8 / pbd_detect_dev_u8 / pbd_detect_batch_u8 would detect it on the cache's
 *   handle: its threshold (pbd_set_threshold; train.m uses -1), candidate mode and NMS, boundary pad and pyramid kind all apply.  The
 *   frame's final records are the ones the plain entry would have returned, in that order: PBD_CAND_RAW by (level, component, root
 *   row, root column); SORT / SORT_NMS / PBD_NMS_PARTS the filter's output.  records[f] = their number for frame f.
 * Write.  Label -1: C = cneg, values negated; id words (-1, id[f], level, x_root, y_root) with the frame's own level.  The first
 *   min(total, capacity - n) records of the call, frame after frame and each frame's in record order, become examples n ...; their
 *   bits — x, ids, b, d, the block table, the solver's a = 0 and sv = 1 — are the ones pbd_qp_write(heads, locs, count, -1, id) gives
 *   for the same records.  written[f] = how many of frame f's records were written.  A full cache is no error (qp_write.m:21-23).
 * Upper bound (detect.m:133-136).  EVERY record of the frame contributes, those a full cache refused included (qp_write.m:21-23
 *   returns early; detect.m:135 still runs): t = cneg * max(1 + (double)score, 0), the sum and the product each rounded, nothing fused.
 *   A frame's terms go through the block sum of the "training example cache" section over the frame's records in record order (64
 *   lane-strided partials starting at +0.0, folded with h = 32 .. 1) to S_f; then ub = ub + S_f, one frame after the other, so a batch
 *   and the same frames one by one give the same bits.  The solver's state is allocated as by any solver entry; its host mirror and
 *   pbd_qp_state_get's stats[3] are current on return.
 * Action (detect.m:148-149, :315-324), evaluated ONCE, after the call, on the state the call left:
 *   lb < 0 || n == capacity -> PBD_MINE_OPT (n == capacity is also part of detect.m's outer trigger, :149); otherwise
 *   1 - lb / ub > .05 -> PBD_MINE_ONE; otherwise PBD_MINE_NONE.  ub == 0 makes lb / ub an infinity or a NaN: IEEE is followed as MATLAB
 *   follows it (a NaN compares false: PBD_MINE_NONE).  The library does not run the solver itself: the caller answers PBD_MINE_OPT with
 *   pbd_qp_opt then pbd_qp_prune, PBD_MINE_ONE with pbd_qp_one, either with pbd_qp_apply_weights.
 *   DEVIATION: detect.m tests after every (level, component) and may change the model in the middle of a frame; here the model is
 *   constant over a call.  DEVIATION: detect.m:36,56 visits levels and components in a random permutation; here the order is the one
 *   stated above.  (train.m:96's model.interval = 2 while mining is pbd_set_interval, "one training round" below.)
 * Validation.  A scan on the device validates every record before anything is written.  A record pbd_qp_write would refuse — a repeated
 *   dense start (qp_write.m:34-35; the test is exact: parts that share an id only in mixtures the pose did not pick are accepted), a
 *   part outside its level, a column longer than k — gets the whole call PBD_ERR_ARG: nothing is written, ub and n are unchanged, the
 *   message names the first such record; records[f] holds the frames' counts, written[f] = 0.  A frame that overflows
 *   pbd_options.max_candidates gets PBD_ERR_CAPACITY with the needed count in records[0], as pbd_detect_u8 reports it; nothing is
 *   written, written[f] = 0.  DEVIATION for a batch: an overflowed list is truncated before the frames are told apart, so the needed
 *   count is that of ALL frames of the batch together, in records[0], and records[1 ..] = 0 (pbd_detect_batch_u8's counts[] are
 *   per frame only while the list did not overflow, too).  A refused call leaves *action as the caller had it.
 * Other refusals, each with a message, changing nothing of the cache (but: a call refused behind its argument and setting checks —
 *   the compact plan, an overflow, a bad record — has allocated the solver's state like any solver entry: a = 0 and sv = 1 for the
 *   examples held, w = 0, l = lb = ub = 0, which is what pbd_qp_state_get answers on a cache that never solved):
 *   PBD_ERR_UNSUPPORTED — pbd_group members; the compact memory plan; depth pruning, 3-D boxes, object clusters or per-part scores
 *     switched on (the refusals of the gt-box frames), beyond what feature vectors already refuse.
 *   PBD_ERR_STATE — a frame pending between enqueue and collect.
 *   PBD_ERR_ARG — NULL arguments; bad frame arguments (as the plain entries); nframes outside 1..64.
 * The call is synchronous.  On return no frame is pending, and the frame's feature planes are resident (the stage getters, and
 *   pbd_candidates_features on records of a plain detect of the same frame, read them).  A caller who wants the mined records
 *   themselves calls the plain detect.  Mining frames run eagerly (no graph replay), like latent and gt-box frames.                      */
#define PBD_MINE_NONE 0
#define PBD_MINE_ONE  1   /* detect.m:322-323: qp_one                         */
#define PBD_MINE_OPT  2   /* detect.m:319-321: qp_opt, then qp_prune          */
int pbd_qp_mine_u8(pbd_qp* qp, const uint8_t* im, int w, int hgt, int cn, int stride, int id,
                   int* records, int* written, int* action);
int pbd_qp_mine_dev_u8(pbd_qp* qp, const void* d_im, int w, int hgt, int cn, int stride, int id,
                       int* records, int* written, int* action);
int pbd_qp_mine_batch_u8(pbd_qp* qp, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride,
                         const int32_t* ids, int32_t* records, int32_t* written, int* action);

/* ---- latent positives: poslatent into the example cache (ABI 5, additive) ----------------------------------------------------------------
 * train.m:166-193 (poslatent) runs, once per positive image i, croppos and then detect(im, model, 0, bbox, overlap, i, 1): the best
 * pose whose every part overlaps its box (detect.m:18-20, 60-101, 115-118) becomes ONE example of label +1 (detect.m:159-164 ->
 * qp_write.m).  It is the path trainmodel.m takes for the final model (warp = 0).  pbd_qp_write_latent_* is that call on the cache's
 * handle with the record left on the device: the image and the truth go in; per frame ONE fixed block comes out (the caller's
 * pbd_latent_example of 32 bytes, filled from a 40-byte pinned slot the device writes).  No record crosses PCIe, in either direction; the example is written straight from the resident feature planes.
 *
 * Detection.  Exactly pbd_detect_latent_u8 / _dev_u8 / pbd_detect_batch_latent_u8 on the cache's handle: everything the "latent
 *   detection" section states applies unchanged — truth convention, mask and skip rule, tie rule, pyramid kind and boundary pad, the
 *   handle's candidate filter on the single record, all three dp_modes.  out[f]'s head fields are those of that entry's record (level:
 *   the frame's own), score its score widened to double (exact).  found = 0 with PBD_OK where a frame has no pose: it writes nothing.
 * Write.  Label +1: C = cpos, no value negated; id words (1, id[f], level, x_root, y_root) with the frame's own level.  The found
 *   frames' records become examples n ..., in frame order, while the cache has room; their bits — x, ids, b, d, the block table, the
 *   solver's a = 0 and sv = 1 — are the ones pbd_qp_write(head, locs, 1, 1, id) gives for the same record on the same resident planes.
 *   written = 1 where the frame became an example; found = 1 with written = 0: the cache was full, which is no error (qp_write.m:21-23).
 *   qp.ub does not move and there is no action to answer (detect.m:133,148 are ~latent).  Fixing the positives as permanent support
 *   vectors (train.m:90-91) stays the caller's pbd_qp_fix.
 * Validation.  A scan on the device validates every record before anything is written, by hard-negative mining's rule and with its
 *   device text: a record pbd_qp_write would refuse — a repeated dense start (two parts of the pose sharing a def or bias id;
 *   qp_write.m:34-35), a part outside its level, a column longer than k — gets the whole call PBD_ERR_ARG: nothing is written, n is
 *   unchanged, the message names the frame; out[f].found and the head fields are filled, written = 0.
 * Other refusals, each with a message and leaving the cache as it was — the union of latent detection's and mining's:
 *   PBD_ERR_UNSUPPORTED — pbd_group members; the score-map NMS (reserved[0] > 0); a filter id shared between (component, part) slots
 *     among the components searched; the compact memory plan (its min() reuses the memory of the feature planes the example is read
 *     from); depth pruning, 3-D boxes, object clusters or per-part scores switched on.
 *   PBD_ERR_STATE — a frame pending between enqueue and collect.
 *   PBD_ERR_ARG — NULL arguments; the latent entries' bad arguments (negative width or height, overlap outside [0, 1), mix outside the
 *     part's mixtures, component out of range); bad frame arguments (as the plain entries); nframes outside 1..64.
 * The call is synchronous.  On return no frame is pending, and the frame's feature planes are resident (pbd_candidates_features on the
 *   returned head reads them); the response planes carry the mask, as after any latent frame, and a plain detect afterwards is
 *   untouched by it.  Latent frames run eagerly (no graph replay); plain frames and their captured graph are untouched.
 * Batch: truth [nframes][max_parts][4], mix [nframes][max_parts] or NULL, ids [nframes], out [nframes]; frames of one size, as every
 *   batch entry takes them.  The examples are those of the frames written one by one, in bits.
 *
 * pbd_croppos is croppos.m, host code like pbd_warp_geometry (no GPU is initialised).  truth: [nparts][4] in this ABI's convention,
 *   (x, y, width, height), 0-based, covering x .. x + width.  In MATLAB's 1-based terms, in double, with MATLAB's round (halves away
 *   from zero; pad is a multiple of 0.5): X1 = min x + 1, X2 = max(x + width) + 1, Y alike; pad = 0.5 * ((X2 - X1 + 1) + (Y2 - Y1 + 1));
 *   x1 = max(1, round(X1 - pad)), x2 = min(w, round(X2 + pad)), y alike.  roi = (x1 - 1, y1 - 1, x2 - x1 + 1, y2 - y1 + 1): 0-based
 *   corner, width and height in pixels of the crop.  truth_out (may be NULL, may be truth): the truth with x -= roi[0], y -= roi[1];
 *   widths and heights unchanged.  An empty ROI (the truth wholly outside the w x hgt frame) is PBD_ERR_ARG, as are NULL truth / roi,
 *   nparts < 1 and a negative width or height.  The crop itself is a view: im + roi[1] * stride + roi[0] * cn with the same stride.    */
typedef struct pbd_latent_example {   /* 32 bytes */
  int32_t found;      /* 1: the frame has a pose (pbd_detect_latent_u8's *found)                                       */
  int32_t written;    /* 1: it became an example; 0 with found = 1: the cache was full, or the call was refused         */
  int32_t component;  /* the record's head: component ...                                                              */
  int32_t level;      /* ... pyramid level (the frame's own) ...                                                       */
  int32_t x, y;       /* ... and root cell (locs[0][0], locs[0][1])                                                    */
  double  score;      /* the record's score, widened exactly                                                           */
} pbd_latent_example;
int pbd_qp_write_latent_u8(pbd_qp* qp, const uint8_t* im, int w, int hgt, int cn, int stride, const int32_t* truth, const int32_t* mix,
                           int component, double overlap, int id, pbd_latent_example* out);
int pbd_qp_write_latent_dev_u8(pbd_qp* qp, const void* d_im, int w, int hgt, int cn, int stride, const int32_t* truth,
                               const int32_t* mix, int component, double overlap, int id, pbd_latent_example* out);
int pbd_qp_write_latent_batch_u8(pbd_qp* qp, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride,
                                 const int32_t* truth, const int32_t* mix, int component, double overlap, const int32_t* ids,
                                 pbd_latent_example* out /* [nframes] */);
int pbd_croppos(const int32_t* truth, int nparts, int w, int hgt, int32_t roi[4], int32_t* truth_out);   /* host only */

/* ---- evaluation ledger: matlab/evaluation/eval_pck.m, eval_apk.m and VOCap.m (ABI 5, additive) ---------------------------------------------
 * What turns the output of the two test protocols — testmodel_gtbox.m (pbd_detect_gtbox_*) and testmodel.m (detect + nms.m,
 * PBD_NMS_PARTS) — into the numbers a model is judged by.  A pbd_eval is bound to a handle as the example cache is: test frames go in with
 * their annotated keypoints, per-instance keypoint distances (PCK) and per-detection true-positive flags (APK) accumulate on the device,
 * per frame only counts and found flags come back, and at the end P doubles per metric: train -> pbd_qp_apply_weights -> evaluate on one
 * handle.  Everything below is float64, the operations in the order written, never fused.  P = the ledger's number of keypoints; the
 * keypoints of a pose are its P parts, in part order.
 * Keypoint.  Part p of a record has box (x, y, w, h); its keypoint is the box centre of rule 1 of "best pose per ground-truth box":
 *   x2 = x + w - 1, cx = .5 * x + .5 * x2, cy alike; exact.  (The reference tree holds no boxes-to-points conversion — the callers of
 *   eval_pck / eval_apk were not vendored; this centre is the one bestoverlap.m:11-14 uses.)
 * Distance (eval_pck.m:10, eval_apk.m:21): dx = cx - gx, dy = cy - gy; s = dx * dx + dy * dy (two rounded products, one rounded sum,
 *   the x term first); d = sqrt(s), correctly rounded.
 * PCK (eval_pck.m).  Instance n = 0 .. N-1 is one annotated person.  With a selected pose dist[n][p] = d of the pose's part p against
 *   the person's point p; without one dist[n][p] = +Inf (our rule: eval_pck.m would fault on an empty box; the instance misses every
 *   keypoint and stays in the denominator).  hit = dist[n][p] < thresh * s_n, strict, the product rounded once;
 *   pck[p] = (double)hits_p / (double)N; N == 0: 0 / 0 = NaN.  Two scale rules, chosen when the result is asked for:
 *   PBD_EVAL_SCALE_LAST: s_n = scale[N-1] for every n — eval_pck.m:13 taken literally, where gt(n) is read after the loop has ended;
 *   PBD_EVAL_SCALE_OWN:  s_n = scale[n].
 *   (eval_pck.m:3-5 and eval_apk.m:3-5 test nargin < 4 on three-argument functions: the reference's threshold is always 0.5.  Here it
 *   is the caller's.)
 * APK matching (eval_apk.m:14-36), independently per keypoint p and per frame.  The frame's detections are taken in the order (score
 *   descending as the stored float, -0.0 == +0.0; ties by the given record order): MATLAB's stable sort(..., 'descend') restricted to the
 *   frame.  For each detection: ngt == 0 -> false positive; else q_g = d(point_p, gtpoint[g][p]) / scale[g] (a rounded division), jmin =
 *   the first index of the minimum; if q_jmin <= thresh and gt jmin is not yet taken for this p the detection is a true positive and gt
 *   jmin becomes taken; in every other case it is a false positive.  A frame's flags depend on nothing outside the frame.
 * APK result (eval_apk.m:7,38-43, VOCap.m).  All M detections of the ledger ordered by (score descending, sequence ascending; sequence =
 *   frames in the order added, within a frame the given order); tpc, fpc the integer cumulative sums (fp = 1 - tp); npos = the sum of ngt
 *   over every frame added, frames without detections included; rec = tpc / npos, prec = tpc / (fpc + tpc), one division each;
 *   mrec = [0; rec; 1], mpre = [0; prec; 0] with the suffix maximum applied; ap = sum_{i=1..M+1} (mrec(i) - mrec(i-1)) * mpre(i) over ALL
 *   i — a term whose mrec did not change is exactly +0.0, so this is the value of VOCap.m:8-9 — in the block-sum order of the "training
 *   example cache" section (64 lane-strided partials starting at +0.0, i ascending, folded h = 32 .. 1).  M == 0: ap = 0.  npos == 0: IEEE
 *   is followed as MATLAB follows it (rec = 0 / 0 = NaN, ap = NaN).
 * Arguments.  Points, scales and thresholds must be finite, every scale > 0, ngt in 0..PBD_GT_MAX; scores of caller-supplied records
 *   finite (their order is undefined otherwise): PBD_ERR_ARG.
 *
 * Host-only definitions (no GPU; pure host code like pbd_candidates_nms_parts):
 *   pbd_eval_keypoint_dist   one record's boxes[nparts][4] against points[nparts][2] -> d[nparts].
 *   pbd_eval_pck_host        dist[n][nparts] (+Inf allowed, NaN refused), scale[n], thresh, rule -> pck[nparts].
 *   pbd_eval_apk_match_host  one frame: heads[count], boxes[count][max_parts][4] in the given order, points[ngt][nparts][2], scale[ngt]
 *                            -> tp[count][nparts] (bytes, by given position).  A record with nparts != the argument: PBD_ERR_ARG.
 *   pbd_eval_ap_host         score[m], tp[m][nparts], npos -> apk[nparts], and prec / rec [nparts][m] in sorted order (either may be NULL).
 * The ledger.  pbd_eval_create(h, nparts, max_instances, max_detections, apk_thresh): PBD_ERR_ARG unless EVERY component of the handle's
 *   model has nparts parts.  The matching threshold is the ledger's; the PCK threshold is an argument of pbd_eval_pck.  Device memory:
 *   8 (P + 1) bytes per instance, 4 + 13 P bytes per detection, 8 per sort slot (max_detections rounded up to a power of two).
 *   pbd_eval_reset empties it; pbd_eval_dims reports P, N, M, npos and the frames added; pbd_eval_get copies the ledger out for tests and
 *   tools: dist[N][P], scale[N], score[M], tp[M][P] (any may be NULL).  pbd_eval_destroy before pbd_destroy.
 * Adds.  Every add answers *needed (may be NULL) = the instances (PCK) or detections (APK) the ledger would hold after the call.  A call
 *   that would overflow max_instances / max_detections adds NOTHING and answers PBD_ERR_CAPACITY: an evaluation that silently drops
 *   detections is wrong (unlike qp_write.m's full cache).  Append positions are deterministic: the host knows ngt, a device scan
 *   answers the frames' detection counts; no atomics.  All adds are synchronous.
 *   pbd_eval_add_pck_records: the caller's ngt host records (heads[ngt], boxes[ngt][max_parts][4], max_parts = the handle's;
 *     found[ngt]: person g has a pose) through the device kernels, appended as ngt instances.  pbd_eval_add_apk_records: ONE frame's
 *     `count` records in the given order, matched against its ngt persons and appended as `count` rows.  A record (with a pose) whose
 *     nparts != P refuses the whole call: PBD_ERR_ARG, nothing is added.
 *   pbd_eval_pck_frame_u8 / _batch_u8: the frame runs exactly as pbd_detect_gtbox_u8 / pbd_detect_batch_gtbox_u8 would, with its
 *     refusals, on the gt box [min x, min y, max x, max y] of every person's points (testmodel_gtbox.m:18-20; exact); a kernel behind the
 *     selection reads the winners where it left them and appends the persons' columns in (frame, person) order.  found[g] = person g
 *     has a pose; *nrecords as there.  Batch layout: points[nframes][PBD_GT_MAX][P][2], scale[nframes][PBD_GT_MAX], ngt[nframes],
 *     found[nframes][PBD_GT_MAX].
 *   pbd_eval_apk_frame_u8 / _batch_u8: the frame runs as pbd_detect_u8 / pbd_detect_batch_u8 would on the handle — its threshold,
 *     candidate mode and NMS apply (testmodel.m: PBD_CAND_SORT_NMS with PBD_NMS_PARTS at 0.3) —, its final records stay on the device and
 *     are reached by the route mining reads; RAW records are put into the plain entries' order by mining's order kernels; the matching
 *     kernel appends the frame's (score, tp[P]) rows.  records[f] = the frame's final records.  Refusals are those of the mining entries
 *     (group members, the compact memory plan, depth pruning, 3-D boxes, object clusters, per-part scores: PBD_ERR_UNSUPPORTED; a frame
 *     pending: PBD_ERR_STATE; an overflow of pbd_options.max_candidates: PBD_ERR_CAPACITY with the needed count in records[0]).
 *   Both kinds launch eagerly; like every special frame they leave plain frames and their captured graph untouched.  A _dev_u8 form is
 *   not provided.
 * Results.  pbd_eval_pck(ev, thresh, rule, pck[P]): one kernel counts per keypoint, for any threshold, with no re-detection.
 *   pbd_eval_apk(ev, apk[P], prec, rec): prec / rec [P][M] in sorted order, either may be NULL.  Both equal the host definitions on
 *   pbd_eval_get's arrays bit for bit.                                                                                                   */
#define PBD_EVAL_SCALE_LAST 0
#define PBD_EVAL_SCALE_OWN  1
typedef struct pbd_eval pbd_eval;
int pbd_eval_keypoint_dist(const int32_t* boxes, int nparts, const double* points, double* d);                      /* host only */
int pbd_eval_pck_host(const double* dist, const double* scale, int n, int nparts, double thresh, int rule, double* pck);   /* host only */
int pbd_eval_apk_match_host(const pbd_candidate_head* heads, const int32_t* boxes, int count, int max_parts, int nparts,
                            const double* points, const double* scale, int ngt, double thresh, uint8_t* tp);         /* host only */
int pbd_eval_ap_host(const float* score, const uint8_t* tp, int m, int nparts, long long npos, double* apk, double* prec,
                     double* rec);                                                                                     /* host only */
int pbd_eval_create(pbd_handle* h, int nparts, int max_instances, int max_detections, double apk_thresh, pbd_eval** ev);
void pbd_eval_destroy(pbd_eval* ev);
int pbd_eval_reset(pbd_eval* ev);
int pbd_eval_dims(const pbd_eval* ev, int* nparts, int* n, int* m, long long* npos, int* frames);
int pbd_eval_get(pbd_eval* ev, double* dist, double* scale, float* score, uint8_t* tp);
int pbd_eval_add_pck_records(pbd_eval* ev, const pbd_candidate_head* heads, const int32_t* boxes, const int* found, const double* points,
                             const double* scale, int ngt, int* needed);
int pbd_eval_add_apk_records(pbd_eval* ev, const pbd_candidate_head* heads, const int32_t* boxes, int count, const double* points,
                             const double* scale, int ngt, int* needed);
int pbd_eval_pck_frame_u8(pbd_eval* ev, const uint8_t* im, int w, int hgt, int cn, int stride, const double* points, const double* scale,
                          int ngt, double overlap, int* found, int* nrecords, int* needed);
int pbd_eval_pck_frame_batch_u8(pbd_eval* ev, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride,
                                const double* points, const double* scale, const int* ngt, double overlap, int* found, int* nrecords,
                                int* needed);
int pbd_eval_apk_frame_u8(pbd_eval* ev, const uint8_t* im, int w, int hgt, int cn, int stride, const double* points, const double* scale,
                          int ngt, int* records, int* needed);
int pbd_eval_apk_frame_batch_u8(pbd_eval* ev, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride,
                                const double* points, const double* scale, const int* ngt, int32_t* records, int* needed);
int pbd_eval_pck(pbd_eval* ev, double thresh, int rule, double* pck);
int pbd_eval_apk(pbd_eval* ev, double* apk, double* prec, double* rec);

/* ---- part mixtures: matlab/learning/k_means.m and clusterparts.m (ABI 5, additive) ----------------------------------------------------------
 * What a training run starts from (trainmodel.m:13-15): every part's positives are clustered by the part's offset from its parent, and the
 * cluster of a positive is the part's mixture label there — the `mix` the latent entries take, the K of the model that buildmodel.m lays out
 * (Model.build_model of the binding).  clusterparts.m runs R = 100 independent k-means per part from random starts and keeps the best: P * R
 * small independent problems.  pbd_cluster_parts runs them on the device, one wavefront each, and needs no handle.
 * k-means (k_means.m:71-114), float64, the operations in the order written, never fused.  X[n][m] points, c[k][m] centroids, labels 0-based.
 *   One pass: D(i, t) = d with d = 0; d = d + (X(i, s) - c(t, s))^2, s ascending; [z, label] = min(D, [], 2) — NaN is ignored, the first of
 *   equal minima wins; then c(t, :) = the mean of the points labelled t, each coordinate's sum divided by the count, and NaN in every
 *   coordinate for a centroid without a point: it can never win again.  The loop runs while the labels changed, the labels before the
 *   first pass being ones no pass gives (g0 = ones, gIdx = zeros): at least one pass, and two unless the cap ends it.  sumdist = sum(z) of
 *   the last pass: measured against the centroids BEFORE that pass's update, as in the file; c is the file's, after it.
 * DEVIATIONS from the file, each stated:
 *   Sums.  The per-cluster coordinate sums and sum(z) use the block sum of the "training example cache" section over the point index i:
 *     element i goes to partial i mod 64, i ascending, the partials start at +0.0, a point of another cluster adds nothing, folded
 *     s[t] += s[t + h], h = 32 .. 1.  The file's sum and mean add left to right.  On data whose sums are exact (small integers) both give
 *     the same bits.  The result does not depend on the launch.
 *   Random starts.  X(ceil(rand(k,1)*n),:) becomes k draws row = next() mod n, c(t, :) = X(row, :), t ascending, next() the splitmix64 of
 *     the "QP solver" section.  The stream of part p, trial r starts at state = seed ^ (0xD1B54A32D192ED03 * (uint64)(p * R + r + 1)).
 *     Rows may repeat, as in the file: two equal centroids leave the later one without a point, and the NaN path above is taken.
 *   Iteration cap.  max_iter in [1, PBD_CLUSTER_MAX_ITER], else PBD_ERR_ARG; k_means.m has none.  A trial whose labels still changed in
 *     pass max_iter stops there, keeps its labels, centroids and sumdist, competes like any other, and is counted in *capped.
 *   A cluster of one point.  k_means.m:103 is mean(X(gIdx==t,:)): for a single point (with m > 1) MATLAB's mean runs ALONG the 1 x m row,
 *     and the scalar — the mean of the point's coordinates — is spread over c(t,:).  Here the centroid is the per-coordinate mean for any
 *     count, so a cluster of one point has that point as its centroid.
 * pbd_kmeans_host: one k-means.  c0[k][m] non-NULL: the k_means(X, C) form; NULL: the start is drawn from the generator at state0.
 *   -> idx[n], and (each may be NULL) c[k][m], *sumdist, *iters = the passes run.  Any m >= 1.
 * pbd_cluster_parts_host (clusterparts.m): def[P][n][2] = part p's position in positive i (Model.data_def of the binding); parent[P] 0-based,
 *   -1 at part 0 only, parent < child; K[P] clusters per part.  X of part p = def[p] - def[parent[p]]; of the root: def[c] - def[0], c its
 *   first child.  R trials per part with m = 2; the winner is the FIRST trial at the minimal sumdist (min as above).  -> idx[P][n], and (each
 *   may be NULL) centres[P][PBD_CLUSTER_MAX_K][2] (the winner's centroids, NaN included; rows from K[p] on are +0.0), sumdist[P],
 *   best_trial[P], trial_sumdist[P * R], trial_iters[P * R], *capped = capped trials over all parts.
 * pbd_cluster_parts: the same on HIP device `device`: def goes up once, X is formed there (the subtraction is exact IEEE either way), a
 *   wavefront per (part, trial) walks its points lane-strided — lane j owns partial j of the block sum — and a second launch picks the
 *   winners; only idx, the centres and the per-part and per-trial scalars come back.  No workgroup waits on another and every loop is
 *   bounded by max_iter.  Synchronous; the calling thread's current device is restored.  Every output equals pbd_cluster_parts_host bit
 *   for bit.  PBD_ERR_HIP: no such device, or a HIP failure.
 * Refusals, nothing computed: PBD_ERR_ARG — NULL def / parent / K / idx (X / idx), n < 1, P < 1, R < 1, m < 1, k or K[p] < 1, a parent
 *   array not as above, a root without a child (the file's while loop runs off the end), a non-finite def, c0 or X, max_iter out of range;
 *   PBD_ERR_UNSUPPORTED — k or K[p] > PBD_CLUSTER_MAX_K; P * R > PBD_CLUSTER_MAX_TRIALS (the device keeps 512 bytes of
 *   centroids per trial: at most 512 MiB); P * R * n > PBD_CLUSTER_MAX_LABELS (the label bytes of all trials: below 2 GiB).  Beside these two
 *   the device holds def and X (32 P n bytes), idx (4 P n) and 20 bytes per trial.                                                       */
#define PBD_CLUSTER_MAX_K 32
#define PBD_CLUSTER_MAX_ITER 10000
#define PBD_CLUSTER_MAX_TRIALS 1048576
#define PBD_CLUSTER_MAX_LABELS 2147483647ll
int pbd_kmeans_host(const double* X, int n, int m, int k, const double* c0, uint64_t state0, int max_iter, int32_t* idx, double* c,
                    double* sumdist, int* iters);                                                                         /* host only */
int pbd_cluster_parts_host(const double* def, int n, int P, const int32_t* parent, const int32_t* K, int R, uint64_t seed, int max_iter,
                           int32_t* idx, double* centres, double* sumdist, int32_t* best_trial, double* trial_sumdist,
                           int32_t* trial_iters, int32_t* capped);                                                        /* host only */
int pbd_cluster_parts(int device, const double* def, int n, int P, const int32_t* parent, const int32_t* K, int R, uint64_t seed,
                      int max_iter, int32_t* idx, double* centres, double* sumdist, int32_t* best_trial, double* trial_sumdist,
                      int32_t* trial_iters, int32_t* capped);

/* ---- one training round: what train.m still needed around the entries above (ABI 5, additive) ------------------------------------------------
 * train.m:73-121 is: qp.n = 0; the positives; fix, prune, opt, vec2model; model.interval = 2; mine the negatives; opt, vec2model; the
 * threshold from the positives' scores; the interval back.  The sections above are its bodies.  These three are its seams, on the device:
 * with them a round is the binding's train() (PartsBasedDetector<T>::train of the host layer) and moves no per-example data over PCIe.
 *
 * pbd_set_interval / pbd_get_interval (train.m:95-96,121: interval0 = model.interval; model.interval = 2; ...; model.interval = interval0).
 *   interval in 1..16, the bound pbd_create checks.  The handle's model gets the new interval; the frame plan and any captured graph are
 *   dropped, as pbd_set_weights and pbd_set_levels drop them (stage getters answer PBD_ERR_STATE until the next frame).  After a
 *   successful call the handle behaves in every entry point exactly like a handle freshly created from the same model with that
 *   interval, the same weights, threshold, options and setters: the results are the same in bits.  pbd_options.conv_mode's resolution is
 *   NOT repeated; a geometry chosen by pbd_tune_plan survives (the rule of pbd_set_weights).  A bound pbd_qp or pbd_eval stays valid:
 *   their columns and ledgers hold features and records, not geometry.  A frame with too few levels for the new interval is refused by
 *   the next frame entry, with the message a fresh handle gives.  Setting the interval the handle has is PBD_OK and drops nothing.
 *   Refusals, changing nothing (a detect afterwards returns the bits it returned before): PBD_ERR_ARG — an interval out of range;
 *   PBD_ERR_UNSUPPORTED — a pbd_group member; PBD_ERR_STATE — a frame or batch in flight between enqueue and collect.
 *   pbd_get_interval: the handle's current interval (0 for NULL).
 * pbd_qp_clear (train.m:75: qp.n = 0).  The cache keeps its capacity, footprint, wreg, w0, cpos / cneg, noneg and binding, and holds no
 *   example: columns, ids, b, d and the example -> column map are what pbd_qp_create left (pbd_qp_get behind n reads zeros again), and
 *   the solver's state, where a solver entry has allocated it, is what pbd_qp_state_get answers on a cache that never solved: a = 0,
 *   sv = 0, w = 0, l = lb = lb_old = ub = 0, nfix = 0.  A refill's bits are a new cache's.  Synchronous.
 *   DEVIATION: train.m:75 resets qp.n alone, so MATLAB's iterations after the first start from stale qp.a, qp.sv and bounds; here the
 *   cache is clean.  trainmodel.m only ever runs iter = 1, where the two agree.
 * pbd_qp_positive_threshold (train.m:116-118 with qp_scorepos, :198-204): r = sort(score(qp.w + qp.w0 .* qp.wreg, qp.x, find(qp.i(1, 1:n)
 *   == 1)) / qp.Cpos); thresh = r(ceil(length(r) * q)) — the threshold a trained model ships with (train.m: q = .05), from the resident
 *   columns and the solver's resident w.  Steps, all on the device (k_qp_thresh.hip):
 *     the examples whose first id word is 1, in ascending index order — a stream compaction, no atomic decides an order —, m of them;
 *     w_eff[j] = w[j] + w0[j] * wreg[j], the product rounded, then the sum, nothing fused;
 *     the selection's scores by the kernel pbd_qp_score_dev launches: the bits pbd_qp_score(w_eff, I) returns;
 *     each score divided by cpos, one rounded division;
 *     the element of ascending rank max(ceil(m * q), 1) - 1, the product in double (Model.positive_threshold's rule of the binding).  The
 *       rank of a score is an exact count: the strictly smaller scores plus the equal scores at a smaller position.  Ties cannot change
 *       the value.  (-0.0 and +0.0 compare equal, as in MATLAB's sort; which of the two zeros is returned is the position's.)
 *       The count is O(m^2) comparisons for any m up to the capacity, as mining's record order is.
 *   *thresh = that score, *npos = m: one double and one int come back (m once in between, for the launch sizes).  The cache, the
 *   solver's a, sv, w and bounds are not changed.  It needs what every solver entry needs (the state is allocated if it is not).
 *   Refusals: PBD_ERR_ARG — NULL thresh / npos, q outside (0, 1] or NaN, a score that is not finite (the message names the example's
 *   index; the smallest one); PBD_ERR_STATE — m == 0 (an empty cache included).                                                        */
int pbd_set_interval(pbd_handle* h, int interval);
int pbd_get_interval(const pbd_handle* h);
int pbd_qp_clear(pbd_qp* qp);
int pbd_qp_positive_threshold(pbd_qp* qp, double q, double* thresh, int* npos);

/* ---- pyramid store: detect and mine from resident feature pyramids (ABI 5, additive) -----------------------------------------------------
 * A frame's HOG pyramid depends on (w, hgt, sbin, interval, pyramid kind, boundary pad, scalar type) and on nothing of the model's
 * filters; a training of sum(K) + 2 rounds (trainmodel.m) mines the same negatives at interval 2 in every round, and two models with
 * equal sbin / interval on one camera frame compute two identical pyramids.  A pbd_pyrstore is a device-resident array of slots, each
 * holding the feature pyramid of ONE frame as the producer handle's front end (image pyramid, HOG, boundary ring) wrote it: level l's
 * [ch][cw][32] block at level_off[l] elements, the levels back to back (pbd_pyrstore_layout) — the very block of the producer's
 * feature buffer.  Any handle with the store's signature detects or mines from a slot instead of from an image.
 *
 * Signature: (device, sbin, interval, pyramid kind, boundary pad, scalar bytes 4 / 8, 32 channels), taken from `producer` at create
 *   and fixed for the life of the store.  slot_bytes = total(max_w, max_h) * scalar bytes.  The store must be destroyed before its
 *   producer; a consumer is bound to nothing.
 * pbd_pyrstore_layout: host only, no GPU.  The geometry of the planner (HOGFeatures<T>::pyramid or featpyramid.m by `kind`, then the
 *   padding): *nlevels, level_off[l] = the level's first element (level_off: NULL, or room for PBD_PYRSTORE_MAX_LEVELS), *total = all
 *   elements = the sum of cw * ch * 32.  PBD_ERR_ARG: a frame too small for `interval` levels, or arguments out of the setters' ranges.
 * Put (synchronous): the producer's own front end on the image, as pbd_pyramid_u8 runs it, then k_pyrstore_put copies the frame's
 *   block into the slot and the slot records (w, hgt, cn).  Refused with the slot unchanged: PBD_ERR_CAPACITY — the frame's total
 *   exceeds the slot; PBD_ERR_STATE — the producer's settings no longer equal the signature (the message names the field), or a frame
 *   is pending on it; PBD_ERR_UNSUPPORTED — the producer is a pbd_group member, runs the compact memory plan or a level subset.
 *   A batch put takes same-sized frames through the producer as one batch; frame f goes to slots[f].
 * Consume: pbd_detect_stored / pbd_detect_batch_stored / pbd_qp_mine_stored / pbd_qp_mine_batch_stored are pbd_detect_u8 /
 *   pbd_detect_batch_u8 / pbd_qp_mine_u8 / pbd_qp_mine_batch_u8 on the frame that was put, planned as the (w, hgt, cn) the put
 *   recorded: ONE launch of k_pyrstore_load (features into the consumer's buffer, and the split banks' parts in the same pass) stands
 *   where the image pyramid and HOG stood; everything behind it is the plain frame's.  The result equals the image entry's on the same
 *   handle with the same image in every bit — records, counts, cache columns, ids, b, d, ub, records[], written[], action and the
 *   error codes of an overflow or a bad record.  Model, bank, threshold, candidate mode, NMS and part scores are the consumer's own.
 *   Stored frames run eagerly and leave a captured graph as it is.  Afterwards features, responses and min() are set and the level
 *   images are NOT (pbd_get_level_image: PBD_ERR_STATE); the feature planes are resident for the getters and pbd_candidates_features.
 *   The same slot may appear twice in a batch.
 * Refusals, each with a message on the consumer, changing nothing:
 *   PBD_ERR_ARG — NULL arguments; a slot out of range; nframes outside 1..64; slots of a batch that differ in (w, hgt, cn); a
 *     signature field (sbin, interval, kind, pad, scalar) that differs: the message names the field and both values.
 *   PBD_ERR_STATE — an empty slot; a frame pending.
 *   PBD_ERR_UNSUPPORTED — pbd_group members; the compact memory plan; depth pruning, 3-D boxes, object clusters; another device.
 * Not provided: latent, gt-box, evaluation, RGB-D and enqueue / collect entries from a store; puts of other than 8-bit frames.            */
#define PBD_PYRSTORE_MAX_LEVELS 128
typedef struct pbd_pyrstore pbd_pyrstore;
int  pbd_pyrstore_create(pbd_handle* producer, int slots, int max_w, int max_h, pbd_pyrstore** out);
void pbd_pyrstore_destroy(pbd_pyrstore* s);
int  pbd_pyrstore_dims(const pbd_pyrstore* s, int* slots, int* sbin, int* interval, int* kind, int* pad, int* scalar_bytes, size_t* slot_bytes);
int  pbd_pyrstore_slot(const pbd_pyrstore* s, int slot, int* w, int* hgt, int* cn, int* nlevels);   /* w = 0: empty */
int  pbd_pyrstore_layout(int w, int hgt, int sbin, int interval, int kind, int pad, int* nlevels, long long* level_off, long long* total);  /* host only */
int  pbd_pyrstore_put_u8(pbd_pyrstore* s, int slot, const uint8_t* im, int w, int hgt, int cn, int stride);
int  pbd_pyrstore_put_dev_u8(pbd_pyrstore* s, int slot, const void* d_im, int w, int hgt, int cn, int stride);
int  pbd_pyrstore_put_batch_u8(pbd_pyrstore* s, const int32_t* slots, const uint8_t* const* ims, int nframes, int w, int hgt, int cn, int stride);
int  pbd_pyrstore_get_level(pbd_pyrstore* s, int slot, int level, void* out, size_t out_bytes);
int  pbd_detect_stored(pbd_handle* h, pbd_pyrstore* s, int slot, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int capacity, int* count);
int  pbd_detect_batch_stored(pbd_handle* h, pbd_pyrstore* s, const int32_t* slots, int nframes, pbd_candidate_head* heads, int32_t* boxes, int32_t* locs, int capacity, int* counts);
int  pbd_qp_mine_stored(pbd_qp* qp, pbd_pyrstore* s, int slot, int id, int* records, int* written, int* action);
int  pbd_qp_mine_batch_stored(pbd_qp* qp, pbd_pyrstore* s, const int32_t* slots, int nframes, const int32_t* ids, int32_t* records, int32_t* written, int* action);

/* ---- virtual positives: mirrored and rotated frames with their keypoints (ABI 5, additive) ---------------------------------------------
 * The recipe trainmodel.m was written for takes every annotated image as it is, mirrored with the left and right parts swapped, and all
 * of these rotated by a few angles, the keypoints carried along (matlab/globals.m:18-23 creates the imrotate/ and imflip/ caches,
 * train.m:130,165: "we create virtual examples by flipping each image left to right").  matlab/learning/map_rotate_points.m maps the
 * keypoints; the image side is a gather over pixels.  Both are defined here, once, in double: every operation below is one IEEE
 * operation in the order written, never fused.
 *
 * Frame of reference: pixel index k (0-based) of an axis sits at coordinate k.  map_rotate_points.m is coordinate-agnostic (a point at
 *   hiA maps to hiB); this is the frame in which image and points agree exactly, and every function of this section works in it.
 *   DEVIATION from a caller who passes the .m files' 1-based keypoints straight in: subtract 1 before and add 1 after (the binding's
 *   augment_positives does).
 * pbd_rotate_geometry (map_rotate_points.m:21-35 as the file computes it): phi = (deg * pi) / 180, c = cos phi, s = sin phi by the
 *   host's libm, once, on the host: the device never evaluates a trigonometric function, it multiplies by the numbers this call returns.
 *   hiA = ((hgt - 1) / 2, (w - 1) / 2) as (row, col), loA = -hiA.  The forward map of a (row, col) pair (u, v) is
 *   (u*c - v*s, u*s + v*c).  Of the file's two corners (loA_r, hiA_c) and (hiA_r, hiA_c): hiB_k = ceil(max |.| / 2) * 2 per axis k;
 *   the canvas has 2 hiB_r + 1 rows and 2 hiB_c + 1 columns.  -> *out_w, *out_h, m[6] = {c, s, hiA_r, hiA_c, hiB_r, hiB_c}; each
 *   may be NULL.  The file's quirks are kept: hiB is the extent rounded UP to an even number, so at 0 degrees an even side gets a
 *   larger canvas with the image a fraction of a pixel off the grid (640 x 480 -> 641 x 481; a side of 30 -> 33), and an odd side n
 *   keeps its size only where (n - 1) / 2 is even (29 -> 29, 31 -> 33); at +-90, 180 and 360 degrees cos and sin are not exactly
 *   0 or +-1, and an extent one ulp above an even number adds two to hiB, four to the canvas side (37 x 29 at 90 degrees: 33 x 37,
 *   not 29 x 37).
 * pbd_map_rotate_points (map_rotate_points.m:37-46): pts[n][2] rows of (x, y) -> out[n][2] (out may be pts).  PBD_ROT_ORI2NEW:
 *   u = y - hiA_r, v = x - hiA_c, out = (x: (u*s + v*c) + hiB_c, y: (u*c - v*s) + hiB_r).  PBD_ROT_NEW2ORI: u = y - hiB_r,
 *   v = x - hiB_c, out = (x: (v*c - u*s) + hiA_c, y: (u*c + v*s) + hiA_r).  DEVIATION: tforminv inverts the matrix numerically; here
 *   the inverse is the transpose.
 * pbd_flip_points: out[p] = (w - 1 - x[mirror[p]], y[mirror[p]]): the mirrored frame's part p is the original's part mirror[p] (left
 *   and right swapped).  mirror must be a permutation of 0..n-1; NULL is the identity.  out may be pts.
 * The image: struct pbd_augment_op {flip, method, deg, rotate}; the mirror comes first, then the rotation.
 *   Flip: F[y][x][ch] = in[y][w - 1 - x][ch] (flip == 0: F = in).  rotate == 0: the output is F, hgt rows of w pixels.
 *   Rotation by deg: for output pixel (r, q) of the canvas, u = r - hiB_r, v = q - hiB_c, source row sr = (u*c + v*s) + hiA_r, source
 *   column sc = (v*c - u*s) + hiA_c — NEW2ORI of the pixel.
 *   PBD_ROT_NEAREST (imrotate's default): F at (floor(sr + 0.5), floor(sc + 0.5)); pixels outside the source are 0 (black).
 *   PBD_ROT_BILINEAR: y0 = floor(sr), fy = sr - y0, x0 = floor(sc), fx = sc - x0; taps a00 = F[y0][x0], a01 = F[y0][x0 + 1],
 *   a10 = F[y0 + 1][x0], a11 = F[y0 + 1][x0 + 1], a tap outside the source counting as 0.0;
 *   value = (1 - fy) * ((1 - fx) * a00 + fx * a01) + fy * ((1 - fx) * a10 + fx * a11); byte = min(255, floor(value + 0.5)).
 *   DEVIATION: imrotate's bilinear kernel and its fill are MATLAB binaries; this definition is the library's.
 * pbd_augment_host_u8: the definition, on the host, one thread.  im: hgt rows of w pixels of cn channels, `stride` bytes apart;
 *   outs[i]: op i's canvas, out_strides[i] bytes between rows.  Bytes of an output row beyond the canvas row are left untouched.
 * pbd_augment_u8: the same on HIP device `device`, host in, host out.  pbd_augment_dev_u8: device in, device out: d_im is read in
 *   place, d_outs is a HOST array of device pointers, written in place.  Both need no handle, are synchronous, and restore the calling
 *   thread's device.  One launch of k_augment.hip serves all ops of the frame: a workgroup is one 64 x 4 output tile of one op, the
 *   op's descriptor is wave-uniform, a lane does one pixel with all its channels; the result equals pbd_augment_host_u8 in every byte
 *   (the same text, augment_core.hpp).  PBD_ERR_HIP: no such device, or a HIP failure (after the refusals below).
 *   Streams: pbd_augment_dev_u8 reads d_im and writes d_outs on a non-blocking stream of its own, which waits for no other stream.
 *   Whatever produced d_im, or still uses the d_outs buffers, on the caller's streams must be COMPLETE before the call (synchronise
 *   the producing stream or the device); on return the canvases are complete and any stream may read them.
 * Refusals, each with a message (pbd_augment_last_error: the calling thread's last one) and nothing written: PBD_ERR_ARG — NULL
 *   pointers, cn other than 1 or 3, w or hgt < 1, a stride below w * cn, a non-finite deg, an unknown method of a rotating op, a
 *   dir other than the two, a mirror that is no permutation, nops outside 1..PBD_AUGMENT_MAX_OPS, an out_stride below the canvas
 *   row; PBD_ERR_UNSUPPORTED — a canvas side beyond PBD_AUGMENT_MAX_SIDE.
 * pbd_qp_write_warped_dev_u8: pbd_qp_write_warped_u8 ("warped positives") with the frame read from device memory on the cache's
 *   device: the upload becomes a device-to-device copy of the same rows; every refusal and every written bit is the same.  With it
 *   and pbd_qp_write_latent_dev_u8 a virtual positive never has to leave the device.  Both read d_im on the handle's stream: the
 *   caller's work that produces the frame must be complete before the call, as above.
 * Not built: rotated negatives, other fills than black, 16-bit frames.                                                              */
#define PBD_ROT_ORI2NEW 0
#define PBD_ROT_NEW2ORI 1
#define PBD_ROT_NEAREST 0
#define PBD_ROT_BILINEAR 1
#define PBD_AUGMENT_MAX_OPS 64
#define PBD_AUGMENT_MAX_SIDE 16384
typedef struct pbd_augment_op {
  int32_t flip;      /* != 0: mirror left to right first                        */
  int32_t method;    /* PBD_ROT_NEAREST / PBD_ROT_BILINEAR (read when rotating)  */
  double deg;        /* the angle in degrees, map_rotate_points.m's `ang`        */
  int32_t rotate;    /* 0: no rotation (the canvas is the frame's), != 0: by deg */
  int32_t reserved;  /* 0                                                        */
} pbd_augment_op;
int pbd_rotate_geometry(int w, int hgt, double deg, int* out_w, int* out_h, double* m);                                  /* host only */
int pbd_map_rotate_points(const double* pts, int n, int w, int hgt, double deg, int dir, double* out);                   /* host only */
int pbd_flip_points(const double* pts, int n, int w, const int32_t* mirror, double* out);                                /* host only */
int pbd_augment_host_u8(const uint8_t* im, int w, int hgt, int cn, int stride, const pbd_augment_op* ops, int nops, uint8_t* const* outs,
                        const int* out_strides);                                                                         /* host only */
int pbd_augment_u8(int device, const uint8_t* im, int w, int hgt, int cn, int stride, const pbd_augment_op* ops, int nops,
                   uint8_t* const* outs, const int* out_strides);
int pbd_augment_dev_u8(int device, const void* d_im, int w, int hgt, int cn, int stride, const pbd_augment_op* ops, int nops,
                       void* const* d_outs, const int* out_strides);
const char* pbd_augment_last_error(void);
int pbd_qp_write_warped_dev_u8(pbd_qp* qp, const void* d_im, int w, int hgt, int cn, int stride, const double* boxes, const int32_t* ids,
                               int n, int filter, int bias, double min_area, int32_t* status, int* written);

/* ---- instrumentation --------------------------------------------------------
 * GPU time (ms, hipEvent) of the stages of the last synchronous detect:
 * [0] image pyramid [1] HOG [2] pdf [3] dp min [4] argmin [5] total            */
int pbd_get_stage_ms(const pbd_handle* h, float ms[6]);
/* enable per-stage events (adds host syncs between stages; off by default)   */
int pbd_set_profiling(pbd_handle* h, int on);
/* algorithmic bytes / flops of the last frame geometry (SURVEY §8d formulas):
 * [0] B_hog [1] B_pdf [2] F_pdf [3] B_dp [4] cells [5] dt_elements
 * (filter taps: the sum of kh_i * kw_i over the filters, for mixed banks too) */
int pbd_get_work(const pbd_handle* h, double work[6]);
/* device memory held by the handle: the buffers and work tables of the current frame geometry (everything a
 * re-plan frees) and the model-sized allocations made at create.  Either pointer may be NULL.                     */
int pbd_get_footprint(const pbd_handle* h, size_t* frame_bytes, size_t* model_bytes);
/* device and pinned host memory the library holds in this process right now, over every handle, cache, ledger, store, group and
 * call: the number of live buffers and their bytes (buffers that pbd_get_footprint leaves out included).  Compiled into every build.
 * A call that keeps nothing leaves both where they were; destroying every object brings both back to zero.  Either pointer may be NULL. */
int pbd_debug_live_allocs(long long* buffers, long long* bytes);
/* Measure the planner's distance-transform block geometry on the caller's own frames instead of trusting its rule (float handles:
 * 256 lanes / 40 KB against 128 lanes / 25 KB per block; results are bit-identical under either): `batch` copies of the host image
 * per call (1 = single frames, the reference's call shape; > 1 = pbd_detect_batch_u8), 2 warm-up + 3 timed calls per geometry, the
 * dp_min stage's GPU time.  The faster one is kept for every later plan of this handle; *chosen = 1 / 2 (0: nothing to choose —
 * double handles), ms[0..1] = the two medians.  im == NULL: back to the rule.  Synchronous; costs ten calls.  The handle's plan is
 * dropped on return (as after pbd_set_levels): stage getters answer PBD_ERR_STATE until the next frame; pbd_get_stage_ms keeps the
 * caller's last figures.  Refused (PBD_ERR_STATE) on a member of an RCCL-gathering pbd_group and while a frame is pending.          */
int pbd_tune_plan(pbd_handle* h, const uint8_t* im, int w, int hgt, int cn, int stride, int batch, int* chosen, double ms[2]);
/* average GPU ms of the DP-min kernels alone over frames since the last reset
 * (HIP events on the handle's stream around the DP stage)                    */
int pbd_dp_timer(pbd_handle* h, int reset, double* avg_ms, int* nframes);
/* The pbd_debug_* entry points below report something only in the probe build of the library
 * (make -C partsbaseddetector_amd/csrc probes -> libpbd_hip_probes.so, -DPBD_PROBES: per-phase stamps inside
 * the kernels + environment tuning knobs); the product library compiles neither and returns
 * PBD_ERR_UNSUPPORTED.
 * debug: 100 MHz wall-clock stamps of block 0 of the last distance-transform launch at its six
 * phase boundaries (setup, line load, envelope scan, read-out, pointer store, end)            */
int pbd_debug_dt_stamps(unsigned long long out[8]);
/* debug: how often k_dt_pass took its rare paths since the last call (the call resets them): [0] blocks that entered validation
 * rounds, [1] rounds run (summed over blocks), [2] the most rounds in one block, [3] stitches redone, [4] boundaries judged stale
 * only because their left neighbour's F moved, [5] lines flagged in a local scan (suspect quotient), [6] lines flagged in a
 * speculative or redone stitch (lost invariant / suspect quotient), [7] lines redone sequentially                            */
int pbd_debug_dt_counters(unsigned long long out[8]);
/* same for the HOG kernel: tile staging, gradient, histogram, energy+normalisers, features */
int pbd_debug_hog_stamps(unsigned long long out[8]);
/* same for the MFMA filter bank: tile staging, K loop, barrier, epilogue                    */
int pbd_debug_conv_stamps(unsigned long long out[8]);

#ifdef __cplusplus
}
#endif
#endif /* PBD_C_H_ */
