// pbd_plan.hpp — the frame planner of libpbd_hip.so: the work tables the kernels read, the host model they are built from, and the
// two pure phases that build them for one frame geometry (plan_layout: geometry and buffers; plan_tables: every table, from the
// buffers' base addresses).  Host-only: compiles with plain g++ (no HIP runtime); pbd_api.cpp allocates and uploads.
#pragma once
#include <cmath>
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/pbd_c.h"

#define PBD_MAX_LEVELS 128
#define PBD_FLEN 32
#define PBD_NORIENT 18
#define PBD_MAX_MIX 16

struct Level {
  int iw, ih;      // level image size
  int bw, bh;      // HOG blocks
  int cw, ch;      // cells (feature map / response size)
  float scale;     // IFeatures::scales()[l]
  size_t img_off;  // bytes into pyr
  size_t cell_off; // prefix sum of cells (over all levels)
  int active;      // within [level_begin, level_end)
};

// ---- kernel work tables -----------------------------------------------------
// one image of the pyramid: level image (frame f, level l) from the frame itself (cv::resize, first octave) or from
// level l - interval (cv::pyrDown); tables in device memory, one launch covers every job of a stage
struct PyrJob { unsigned long long soff, doff; int sw, sh, dw, dh; };
// PBD_PYRAMID_MATLAB (k_pyramid_mat.hip): one level image, in double, from the 8-bit frame by the area resize of matlab/mex/resize.cc
// (first octave) or from level l - interval by the 5-tap reduce of matlab/mex/reduce.cc.  The resize reads resize1dtran's
// interpolation cache (resize.cc:35-66), built here on the host in double: run yrun0 + dy / xrun0 + dx of the run table lists the
// taps of destination row dy / column dx, `count` taps from tap `first`, in the order the reference's loop appends them.
struct MatTap { double alpha; int si, pad; };
struct MatRun { int first, count; };
struct MatJob { unsigned long long soff, doff; int sw, sh, dw, dh, yrun0, xrun0; };   // soff / doff: bytes
struct HogTile { int level, cy0, cx0, pad; };
struct LevelDev {    // per level, device copy
  int iw, ih, bw, bh, cw, ch;
  unsigned long long img_off, cell_off;
};
// pad: 0 in a uniform bank's tile list.  Mixed banks (pbd_create_sized) keep one copy of the list per size group with
// pad = n0 | (nf_g << 16): the group writes response planes n0 .. n0 + nf_g - 1 of the level's block (the MIX kernel
// instantiations read it; their `nf` argument is then the level block's plane count, the whole bank's)
struct ConvTile { int level, y0, x0, pad; };
// boundary padding (pbd_set_boundary_pad, k_featpad.hip): the border ring of one level — the cells of its cw x ch plane outside the
// interior (cw - 2 pad) x (ch - 2 pad), nring of them, in row-major order
struct PadJob { unsigned long long cell_off; int cw, ch, pad, nring; };
#define PBD_FEATPAD_CPB 64   // ring cells per block of k_featpad (ReduceBlock{job, first ring cell})

// Score data is T = float or double (the handle's instantiation, pbd_options.scalar_type); the work
// tables carry untyped pointers and the kernels are instantiated for both.
struct DtMap {       // one 1-D pass over one score map
  const void* src;   // T: lines contiguous: line i at src + i*len
  void* dst;         // T: transposed out: element q of line i at dst + q*nlines + i
  void* ptr;         // uint8_t where the plan's lines all fit byte links (DT_G_PTR8 on every group: FrameLayout::ptr_bytes == 1), else int16_t.
                     // Same layout as dst, in BOTH passes: element q of line i at ptr + q*nlines + i.  An x pass's plane (lines = rows) is therefore
                     // stored [column][row] with the level's row count as its pitch — k_backtrack and pbd_get_dp_pointers address it so, from the level's
                     // H alone; a y pass's (lines = columns) comes out [row][column]
  double a, b;       // Quadratic(a, b)
  double r2a;        // RN(1 / (2a)), IEEE division on the host (dt_core.hpp: the reciprocal of an intersection's denominator)
  int os, ptr_natural;  // ptr_natural: 1 on an x pass's map.  No kernel reads it: up to round 6 it chose a row-major [line][q] pointer plane (one 2-byte
                        // write per lane and store); the host replay of a block (tests/tools/dt_replay.cpp) still lays out its private planes by it
};
// One group = the maps of one launch that share a geometry: nmaps maps of nlines lines of len elements.
//   plain:  line gi of the group = line gi % nlines of map gi / nlines (map-major); a block = lpb consecutive lines.
//   fold:   the group is ONE part at one level (nmaps = its K mixtures, the lines of a row are its K mixtures): a
//           block = nrows consecutive rows x K mixtures, and its loader builds the lines on the fly from the part's raw
//           responses and its children's distance-transformed scores (FoldJob).
// The block's index arithmetic divides by wave-uniform numbers (lines per block, lines per map, segments per line): the plan
// supplies them as multiply-high constants — a division by a run-time value is ~20 vector instructions per lane, and vector
// instruction issue is what bounds k_dt_pass.  magic_d = ceil(2^32 / d): x / d == umulhi(x, magic_d) exactly for x * d < 2^32.
struct DtGroup {
  int map0, nmaps, nlines, len, stride, lpb, fold;   // stride: LDS elements per line (odd); lpb: lines per block; fold: FoldJob index or -1
  int nsub;                  // lanes per line = block lanes / lpb
  int P;                     // segments per line = dt_segments(nsub, len)
  int chunk;                 // read-out: outputs per lane = ceil(len / nsub)
  unsigned magic_lpb;        // lane / lpb              (lane < 2^8)
  unsigned magic_nlines;     // (l0 + lane) / nlines    (numerator < nlines + 2^8, nlines < 2^15)
  unsigned magic_P;          // (p * len) / P           (p * len < 2^21, P <= 64)
  int fused;                 // bit 0 — float maps only: every map of the group has weights that are converted floats, len and len + |os| <= DT_FUSE_MAXLEN: the
                             // intersection's and the read-out's products are exact and fuse into their additions (dt_core.hpp: dt_isect);
                             // bit 1 — the group is an x pass (DtMap::ptr_natural of every map of the group).  No kernel reads it since the x pass writes its
                             // pointers transposed like every other output of the chain; the planner keeps setting it on exactly the x passes, which the plan
                             // check (tests/tools/plan_check.cpp) pins
};
#define DT_G_FUSED 1
#define DT_G_NATURAL 2
#define DT_G_PTR8 4          // bit 2 — the group's pointer planes are bytes (plan-wide: dt_mark_ptr8), else int16_t
struct DtTask { int g0, nl, m0, l0; DtGroup g;     // g0: first line (plain) / first row (fold); nl: lines of this block; plain: g0 = m0 * nlines + l0
                                                    // (first map of the block, first line inside it); the group travels with the task
  const void* src0; };                              // plain: the block's first line when its nl lines are CONTIGUOUS in memory (consecutive maps of a group
                                                    // back to back — the y pass's input always, plan_frame), else null: the loader then needs no map descriptor
static inline unsigned dt_magic(unsigned d) { return d > 1 ? 0xFFFFFFFFu / d + 1u : 0u; }   // d == 1: the quotient is the numerator itself (callers test)
#define PBD_MAX_CH 8   // children of one parent folded into one reduce job
struct ReduceChild {     // one child part's distance-transformed mixtures
  const void* sdt;       // T [K][H][W] distance-transformed child scores
  uint8_t* ok;           // output: best child mixture per parent mixture, [L][H][W].  The x / y pointers of the
                         // winning mixture are NOT materialised: the DT pointer planes stay in HBM for the frame and
                         // the few back-tracked candidates compose them on the fly (k_backtrack)
  int K, pad;
  int bias_off[PBD_MAX_MIX];  // biasw index of bias(mm)[0] for each child mixture mm
};
// fold mode: the children of one (level, part), descending child index (src/DynamicProgram.cpp:95); read by the loader
// of the part's x pass (k_dt_pass<T, true>) and, for a root, by k_root
#define PBD_FOLDX_QW 18     // quad-words of a fold x task's extension record (pbd_handle::d_foldx)
#define PBD_FOLD_MAXMIX 8   // fold mode keeps one value per parent mixture / child mixture in registers: K, L <= 8
struct FoldChild {
  const void* sdt[PBD_FOLD_MAXMIX];   // T [H][W]: distance-transformed scores of child mixture k (one pointer per plane: the planes may
                                      // be the child's own response planes, overwritten in place by its y pass)
  uint8_t* ok;                        // Ik: best child mixture per parent mixture, [L][H][W].  The fold itself does not write it: k_backtrack picks the
                                      // mixture again at the cells it visits, k_ik_fill writes the planes when a caller asks for the tables (fold_pick.hpp)
  int K, L;                           // mixtures of the child, of its parent
  float bias[PBD_FOLD_MAXMIX][PBD_FOLD_MAXMIX];   // bias(k)[m] = biasw[biasid[k] + m] (include/Parts.hpp:172-175), dense: rows beyond K / columns
                                                  // beyond L repeat the last valid one, so the kernel fetches whole rows with wide scalar loads
};
struct FoldJob { int nch, pad; FoldChild ch[PBD_MAX_CH]; };
#define PBD_NO_PICK (~0ull)
struct ReduceJob {       // one (level, parent): fold the messages of nch children, in the reference's order
  int H, W, L, nch;
  const void* par_in[PBD_MAX_MIX];   // T: parent mixture m: current score (resp plane or acc slot)
  void* par_out[PBD_MAX_MIX];        // T: parent mixture m: acc slot
  ReduceChild ch[PBD_MAX_CH];        // descending child index (src/DynamicProgram.cpp:95)
};
struct ReduceBlock { int job; unsigned cell0; };  // one 256-thread block of k_reduce
struct RootJob {
  const void* score[PBD_MAX_MIX];  // T: root mixture m current score (entries beyond K repeat mixture K - 1)
  void* rootv; int* rooti;         // rootv: T
  int H, W, K, level, comp;
  float bias;
  unsigned cell0;
  int fold, pad;                   // FoldJob of the root part (score[] are then its raw responses) or -1
};
struct BackLevel {   // per (level, comp) info for backtracking
  const uint8_t* pk;   // best-mixture plane 0 of this comp at this level
  const void* rootv; const int* rooti;   // rootv: T
  int H, W; float scale;
};

// The kernels read these tables byte for byte: their layouts are pinned.
static_assert(sizeof(Level) == 56, "Level layout");
static_assert(sizeof(PyrJob) == 32, "PyrJob layout");
static_assert(sizeof(MatTap) == 16 && sizeof(MatRun) == 8 && sizeof(MatJob) == 40, "MatTap / MatRun / MatJob layout");
static_assert(sizeof(HogTile) == 16, "HogTile layout");
static_assert(sizeof(LevelDev) == 40, "LevelDev layout");
static_assert(sizeof(ConvTile) == 16, "ConvTile layout");
static_assert(sizeof(PadJob) == 24, "PadJob layout");
static_assert(sizeof(DtMap) == 56, "DtMap layout");
static_assert(sizeof(DtGroup) == 56, "DtGroup layout");
static_assert(sizeof(DtTask) == 80, "DtTask layout");
static_assert(sizeof(FoldChild) == 336, "FoldChild layout");
static_assert(sizeof(FoldJob) == 2696, "FoldJob layout");
static_assert(sizeof(ReduceChild) == 88, "ReduceChild layout");
static_assert(sizeof(ReduceJob) == 976, "ReduceJob layout");
static_assert(sizeof(ReduceBlock) == 8, "ReduceBlock layout");
static_assert(sizeof(RootJob) == 184, "RootJob layout");
static_assert(sizeof(BackLevel) == 40, "BackLevel layout");

#ifndef PBD_DT_NT_DEFAULT
#define PBD_DT_NT_DEFAULT 128   // lanes of a k_dt_pass block
#endif

// ---- host model -------------------------------------------------------------
struct PartInfo {
  int comp, p, parent;       // local indices
  int K;                     // #mixtures
  std::vector<int> filterid, defid, biasid;
  std::vector<int> slot;     // acc slot per mixture (global slot id)
  int plane0;                // first pointer plane (global plane id), parent's L planes
  bool leaf;
};

// one size group of a mixed bank: filters of one kh x kw, contiguous in the handle's internal filter order (planes n0 .. n0 + nf - 1);
// its weights in the layouts a uniform bank of those filters has (nfpad, the wT copies, the split parts and scales)
struct SizeGroup {
  int kh = 0, kw = 0, n0 = 0, nf = 0, nfpad = 0;
  void* d_wT = nullptr; uint16_t* d_wS = nullptr; float* d_oscale = nullptr;
};


// The model as the planner sees it: the caller's description validated and copied, the part trees' topology (slots, pointer
// planes, the round schedule of the DP) and the handle options that shape the plan.  pbd_handle derives from it.
struct HostModel {
  pbd_model_desc md;         // pointers into the vectors below
  std::vector<float> filters, defw, biasw;
  std::vector<int> anchors, part_offset, parentid, mix_offset, filterid, defid, biasid;
  pbd_options opt;
  int ts = 4;                // sizeof(T): 4 = PartsBasedDetector<float>, 8 = PartsBasedDetector<double>
  int conv_mode = PBD_CONV_EXACT;   // resolved: never PBD_CONV_AUTO
  int split_parts = 0;       // 3: PBD_CONV_SPLIT (bfloat16 parts), 2: PBD_CONV_SPLIT_F16 (binary16 parts), 0: no split bank
  int pad = 0;               // pbd_set_boundary_pad: cells of padding around every level's feature map (0: off, the reference's state)
  int pyr_kind = PBD_PYRAMID_OPENCV;   // pbd_set_pyramid_kind: PBD_PYRAMID_MATLAB = the pyramid of matlab/detection/featpyramid.m:13-34 (double level images)
  int nms_sz = 0;            // pbd_options.reserved[0]: window of the score-map NMS in front of the back-tracking (0: off, the reference's state)
  int max_parts = 0, nslots = 0, nplanes = 0;
  std::vector<PartInfo> parts;                 // flat parts
  std::vector<std::vector<int>> rounds;        // flat part ids whose DT runs in round r
  std::vector<std::vector<std::vector<int>>> red_rounds;  // [round][wave] -> flat child part ids reduced (grouped by parent at plan time)
  std::vector<int> comp_plane0;
  bool unique_filters = false;                 // every filter id belongs to exactly one (component, part, mixture)
  bool fold = false;                           // DP structure: messages folded by the parent's x pass (no k_reduce, no acc planes)
  int fold_mix = 0;                            // largest mixture count of a part (the fold kernels' register-array bound)
  // mixed banks (pbd_create_sized with more than one filter size): md.kh = md.kw = 0, the filters sorted by size internally
  // (stable: size groups in order of (kh, kw)); filterid / filters / response planes are in the INTERNAL order, the stage entry
  // points translate the caller's filter index with fperm
  bool mixed = false;
  std::vector<int> fkh, fkw;     // [internal filter] rows / cols
  std::vector<int> fperm;        // [caller filter] -> internal filter (empty: identity)
  std::vector<SizeGroup> groups; // size groups (kh, kw, n0, nf); the device fields are filled by the upload
};
// The distance transform's input domain: FINITE scores and FINITE quadratics (DESIGN.md "Input domain of the distance transform").  Every
// entry point that takes score maps or weights from the host scans them with this before anything reaches k_dt_pass: a NaN or an
// infinity makes the reference's own loop compare unordered values, and can keep a speculative stitch of dt_core.hpp from ending.
// Returns the index of the first non-finite element, or n.
template <typename T>
static inline size_t pbd_first_nonfinite(const T* v, size_t n) {
  size_t i = 0;
  while (i < n && std::isfinite(v[i])) ++i;
  return i;
}
// pbd_create (sized = false) / pbd_create_sized up to the device: options, model validation and topology, the filter-bank mode.
// PBD_OK, or an error code with its message in *err.
int plan_model(HostModel& hm, const pbd_model_desc* model, const int32_t* fsize, bool sized, const pbd_options* opt, std::string* err);

// Tuning knobs of the DT geometry (the probe and tune builds read them from the environment, pbd_api.cpp; product builds keep these)
struct PlanKnobs {
  int dt_nt = 0;                 // PBD_DT_NT: lanes of a k_dt_pass block (0: the rule)
  int dt_seg = 0;                // PBD_DT_SEG: target segment length of the DT scans (0: as many lines per block as fit)
  long long dt_budget_kb = -1;   // PBD_DT_BUDGET_KB: LDS budget of a DT block (-1: the rule)
  long long dt_budget_b = -1;    // PBD_DT_BUDGET_B: the same in bytes (wins over _KB)
  int xcd_chunk = 16;            // PBD_DT_XCD_CHUNK: consecutive k_dt_pass tasks kept on one XCD (0: table order)
};

// ---- phase 1: frame geometry and buffers ----------------------------------------------------------------------------------------
struct FrameSpec {
  int w = 0, h = 0, cn = 3, batch = 1, depth = PBD_DEPTH_8U;
  std::vector<char> level_set;   // pbd_set_levels (empty: all), intersected with [level_begin, level_end)
};
enum FrameBuf { FB_IMG, FB_PYR, FB_FEAT, FB_RESP, FB_PK, FB_ROOTV, FB_ROOTI, FB_NMS_MASK, FB_DT_TMPT, FB_DT_SDT, FB_DT_IXT, FB_DT_IY,
                FB_ACC, FB_FEAT_SPLIT, FB_COUNT };
struct BufPlace { int region = -1; size_t offset = 0, bytes = 0; };   // region -1: the plan has no such buffer
struct FrameLayout {
  int nlevels = 0, batch = 1, nvl = 0, esz = 1;   // nlevels: levels of ONE frame; nvl = batch * nlevels virtual levels; esz: bytes per element of the LEVEL images
  int src_esz = 1;                               // bytes per element of the frame itself (PBD_PYRAMID_MATLAB: 8-bit frames, double level images; else esz)
  std::vector<Level> lv;                         // [nvl]
  size_t cells = 0, pyr_bytes = 0;
  size_t act_cells = 0;                          // cells of the active levels
  size_t maxK = 1;                               // maps transformed in the fullest round (per level)
  size_t dt_cap_elems = 0;                       // elements of the per-map DT planes
  int ptr_bytes = 2;                             // bytes per element of the DT pointer planes: 1 where every line of the plan has a stride <= 256 (an
                                                 // element index < 255, k_dt_pass's own byte links), else 2 — one width for the whole plan
  bool compact = false;
  BufPlace buf[FB_COUNT];
  std::vector<size_t> regions;                   // bytes of each region: one allocation each
};
// PBD_OK, or an error code (PBD_ERR_ARG: too small for the pyramid; PBD_ERR_UNSUPPORTED: a level or the frame too large) and *err
int plan_layout(const HostModel& hm, const FrameSpec& f, FrameLayout& out, std::string* err);

// ---- phase 2: work tables -------------------------------------------------------------------------------------------------------
struct FrameBases { char* p[FB_COUNT]; };       // base address of every buffer (null where the plan has none)
FrameBases frame_bases(const FrameLayout& lay, char* const* regions);

struct PyrLaunch { int job0, njobs, maxpix, maxw, maxh; };   // maxpix / maxw / maxh: the largest destination level of the launch
struct ReduceWave { int blk0, nblks; };
struct RoundLaunch { int xtask0, nxtasks, ytask0, nytasks; size_t lds_x, lds_y; int fold_x; std::vector<ReduceWave> waves;
                     size_t foldx0 = 0; };             // fold x launch: its first record in foldx (PBD_FOLDX_QW quad-words per task)
struct FrameTables {
  std::vector<PyrJob> pyrjobs;                   // resize jobs, then the pyrDown jobs octave by octave
  std::vector<PyrLaunch> pyr_launches;           // [0]: resize, [1..]: pyrDown octave steps
  // PBD_PYRAMID_MATLAB (pyrjobs then empty; pyr_launches index matjobs): area-resize jobs, then the reduce jobs octave by octave
  std::vector<MatJob> matjobs;
  std::vector<MatRun> matruns;
  std::vector<MatTap> mattaps;
  std::vector<LevelDev> levels;
  // boundary padding only (else empty): the levels as k_hog addresses them — cw is the padded pitch and cell_off the interior's first
  // cell (cell_off + pad * cw + pad), so the kernel's store needs no offset of its own — and the border ring's jobs / blocks
  std::vector<LevelDev> hog_levels;
  std::vector<PadJob> padjobs;
  std::vector<ReduceBlock> padblk;               // k_featpad: one block per PBD_FEATPAD_CPB ring cells of a job
  int hog_tc = 16;
  std::vector<HogTile> hog_tiles;
  std::vector<ConvTile> conv_tiles, conv_tiles_mix;   // mixed banks: [group][conv tile], pad = n0 | (nf_g << 16)
  int dt_nt = PBD_DT_NT_DEFAULT;
  size_t dt_lds = 0;                             // LDS budget of a k_dt_pass block
  std::vector<DtMap> maps;
  std::vector<DtTask> tasks;                     // all rounds back to back
  std::vector<FoldJob> folds;
  std::vector<unsigned long long> foldx;         // per fold x task: the loader's first addresses (PBD_FOLDX_QW quad-words)
  std::vector<ReduceJob> red;
  std::vector<ReduceBlock> redblk;
  std::vector<RoundLaunch> rl;
  std::vector<RootJob> rootjobs;
  std::vector<ReduceBlock> rootblk;              // k_root: one 256-thread block per 256 cells of a root job
  std::vector<BackLevel> back;                   // [nvl][ncomponents]
  std::vector<unsigned long long> scr_base;      // [nvl][nflat parts] element offset of mixture 0's DT planes (ix / iy / sdt)
  std::vector<unsigned long long> pick;          // fold plans, [nvl][nflat parts]: byte offset in `folds` of the FoldChild that carries the part's message at the
                                                 // level — its kept score planes and its bias block, what the mixture choice is picked from —, PBD_NO_PICK: none
  unsigned root_cells = 0, root_maxcells = 0;
};
// dt_geom: pbd_tune_plan's DT block geometry of float handles (0 = the measured rule, 1 = 256 lanes / 40 KB, 2 = 128 lanes / 25 KB);
// ncu: compute units of the device.  Only computes addresses: nothing behind `b` is read.
int plan_tables(const HostModel& hm, const FrameSpec& f, const FrameLayout& lay, const FrameBases& b, int ncu, int dt_geom,
                const PlanKnobs& kn, FrameTables& out, std::string* err);

// ---- DT task lists (also pbd_dt2d's) ----------------------------------------------------------------------------------------------
int dt_stride_for(int len);
// natural: the group is an x pass (DT_G_NATURAL: a marker, see DtGroup::fused); fold >= 0: the group is one part at
// one level, a block = whole rows of its nmaps mixtures; round_lanes: plain groups only — the largest lines-per-block <= the fit that
// leaves no lane idle
DtGroup dt_group(int map0, int nmaps, int nlines, int len, size_t budget, int ts, int nt, int seg, bool natural, int fold = -1,
                 bool round_lanes = true);
void dt_add_tasks(const DtGroup& g, std::vector<DtTask>& out, const std::vector<DtMap>* maps = nullptr, int ts = 4);
void dt_mark_fused(std::vector<DtTask>& tasks, const DtMap* maps, int ts);
DtMap dt_map(const void* src, void* dst, void* ptr, float wq, float wl, int os, int natural);
int dt_ptr_bytes_for(int maxlen);                      // width of the pointer planes of a plan whose longest line has maxlen elements (1 or 2)
void dt_mark_ptr8(std::vector<DtTask>& tasks);         // DT_G_PTR8 on every group (a plan of dt_ptr_bytes_for(...) == 1)

// pyramid geometry of one frame (HOGFeatures<T>::pyramid): 0, or -1 when the frame has fewer than `interval` or more than PBD_MAX_LEVELS levels
int compute_geometry(int w, int h, int sbin, int interval, int* nlevels, Level* lv);
// PBD_PYRAMID_MATLAB: the same for matlab/detection/featpyramid.m:13-34 (levels in double arithmetic, sizes by C round(), box scale
// sbin / s_i doubled per octave); also -1 where a reduce would read a level with a dimension below 5
int compute_geometry_matlab(int w, int h, int sbin, int interval, int* nlevels, Level* lv);
// resize1dtran's interpolation cache for one axis (matlab/mex/resize.cc:30-66): appends dlen runs and their taps; false
// where a tap's source index falls outside [0, slen) (the reference asserts it cannot)
bool resize_taps(int slen, int dlen, std::vector<MatRun>& runs, std::vector<MatTap>& taps);
#define PBD_MATPYR_MAX_BYTES ((size_t)1 << 31)   // PBD_PYRAMID_MATLAB: the level images of a plan (all frames of a batch), in double
// boundary padding: every level that has cells grows by `pad` cells on each side (copyMakeBorder(feature, padded, pad, pad, pad * flen,
// pad * flen, ...), src/HOGFeatures.cpp:147); bw / bh stay the HOG blocks, the interior is (bw - 2) x (bh - 2)
void pad_geometry(int pad, int nlevels, Level* lv);
int depth_esz(int depth);   // bytes per element of a PBD_DEPTH_* image; 0: unsupported
