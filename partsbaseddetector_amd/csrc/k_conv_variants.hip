// k_conv_variants.hip — the filter-bank kernels and configurations that were measured and NOT adopted, with what they measured.
// Linked into the tuning and probe libraries only (libpbd_hip_tune.so, libpbd_hip_probes.so): the product library holds the
// kernels of k_conv.hip and nothing else.  launch_conv_variant (called from run_pdf in those builds) takes the bank over when one
// of PBD_MFMA_VARIANT, PBD_CONV_LDS_KB, PBD_SPLIT_VARIANT or, in the probe build alone, PBD_MFMA64_QUARTERS / PBD_CONV_PRIO is set.
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include "pbd_internal.hpp"

void launch_conv_split_variant(const pbd_handle* h, int variant);   // k_conv_split_variants.hip

namespace conv_variants {   // own instantiations of the shared templates: no kernel handle or stamp buffer shared with k_conv.hip
#include "k_conv_mfma16.hpp"
#define CSTR 33      // LDS floats per cell of k_conv_mfma (32 + 1 pad: conflict-free across x)

#ifdef PBD_PROBES
// k_conv_glds: per-phase sums over the units of one workgroup (wave 0 lane 0), slots: 0 = barrier waits before the K loops, 1 = both K loops, 2 = barrier before the epilogue, 4 = shader cycles of both K loops (s_memtime), 5 = epilogue; 6 = units; 7 = life
#define GLDS_T(var) const unsigned long long var = wall_clock64()
#define GLDS_C(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define GLDS_ACC(i, a, b) do { if (blockIdx.x == gridDim.x / 2 + 3 && threadIdx.x == 0) pbd_conv_dbg[i] += (b) - (a); } while (0)
#define GLDS_INIT() do { if (blockIdx.x == gridDim.x / 2 + 3 && threadIdx.x == 0) for (int q_ = 0; q_ < 8; ++q_) pbd_conv_dbg[q_] = 0; } while (0)
#else
#define GLDS_T(var) do { } while (0)
#define GLDS_C(var) do { } while (0)
#define GLDS_ACC(i, a, b) do { } while (0)
#define GLDS_INIT() do { } while (0)
#endif

// ---------------------------------------------------------------------------
// fp32 MFMA implicit GEMM (v_mfma_f32_32x32x2_f32), M = cells, N = filters, K = kh*kw*32.
// Workgroup = 256 threads = 4 waves: tile = 16x16 cells (M = 256) x ONE 32-filter n-tile; the
// grid is (tiles, nfpad/32), so work units are small (3 resident per CU, ~12 per CU for the person
// model) and the tail of the launch is short.  Wave w owns cell rows 4w..4w+3 = two 32-row MFMA
// M-tiles (2 cell rows x 16 cols each): 2 accumulators of 16 VGPRs.
//  * A (features): the 20x20-cell tile with halo is staged once in LDS, cell stride 33 floats, so
//    the 32 lanes of an M-tile read conflict-free; lane l holds A[i = l&31][k = l>>5].
//  * B (weights, [tap][channel][nfpad]): 512 KB for the whole bank, L2-resident.  A lane's B
//    operand is ONE float per MFMA (B[k = l>>5][j = l&31]); the 16 values of a tap are loaded
//    straight from L2 into registers a whole tap (2048 MFMA cycles) ahead of use — no weight LDS,
//    no barrier anywhere in the K loop.
//  * K order: tap-major, channel-minor; the accumulation is a k-ordered fp32 fma chain.
// ---------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int KH, int KW>
__global__ __launch_bounds__(256) void k_conv_mfma(const ConvTile* __restrict__ tiles,
                                                   const LevelDev* __restrict__ levels,
                                                   const float* __restrict__ feat, const float* __restrict__ wT,
                                                   float* __restrict__ resp, int nf, int nfpad) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TW = CT + KW - 1;
  float* ft = (float*)smem;                 // [TH][TW][CSTR]
  CONV_STAMP(0);
  const ConvTile t = tiles[blockIdx.x];
  const LevelDev lv = levels[t.level];
  const int H = lv.ch, W = lv.cw;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nbase = blockIdx.y * 32;
  const float* F = feat + lv.cell_off * PBD_FLEN;
  // A operand: lane l holds A[i = l&31][k = l>>5]; M-tile m of this wave: cell rows 4*wave + 2*m + (ai>>4), col ai&15
  const int ai = lane & 31, ak = lane >> 5;
  // B operand: B[k = l>>5][j = l&31] -> wT[(tap*32 + c + ak)*nfpad + nbase + (l&31)]
  const float* bsrc = wT + (size_t)ak * nfpad + nbase + (lane & 31);
  // two register sets in explicit ping-pong (the tap loop is unrolled by two): while one set feeds
  // the 32 MFMAs of a tap, the other receives the next tap's 16 values.  With a single pair of
  // arrays and a copy hipcc merges them and ends up loading the next tap AFTER the last MFMA that
  // reads the registers, then waits vmcnt(0) at the loop tail: a full L2 round trip per tap.
  float b0[16], b1[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) b0[u] = bsrc[(size_t)(2 * u) * nfpad];  // tap 0, issued before the tile staging
  constexpr int NB = ((CT + KH - 1) * (CT + KW - 1) * 8 + 255) / 256;   // every batch of loads in flight
  stage_tile<float, PBD_FLEN, CSTR, NB>(ft, F, t.y0, t.x0, H, W, KH, KW, 0, true, tid);
  __syncthreads();
  CONV_STAMP(1);

  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
  const int arow0 = 4 * wave + (ai >> 4), acol = ai & 15;
  const float* abase0 = ft + (arow0 * TW + acol) * CSTR + ak;
  const float* abase1 = ft + ((arow0 + 2) * TW + acol) * CSTR + ak;
  constexpr int NTAP = KH * KW;

  auto load_tap = [&](float (&dst)[16], int tap) {
    const float* bs = bsrc + (size_t)min(tap, NTAP - 1) * PBD_FLEN * nfpad;
#pragma unroll
    for (int u = 0; u < 16; ++u) dst[u] = bs[(size_t)(2 * u) * nfpad];
  };
  auto mma_tap = [&](const float (&bw)[16], int tap) {
    const int ti = tap / KW, tj = tap - ti * KW;
    const float* a0 = abase0 + (ti * TW + tj) * CSTR;
    const float* a1 = abase1 + (ti * TW + tj) * CSTR;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const float av0 = a0[2 * u], av1 = a1[2 * u];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, bw[u], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, bw[u], acc1, 0, 0, 0);
    }
  };
  for (int tap = 0; tap < NTAP; tap += 2) {
    load_tap(b1, tap + 1);
    mma_tap(b0, tap);
    if (tap + 1 < NTAP) {
      load_tap(b0, tap + 2);
      mma_tap(b1, tap + 1);
    }
  }
  CONV_STAMP(2);
  __syncthreads();  // all waves are done reading the feature tile: reuse it for the epilogue
  CONV_STAMP(3);
  // Epilogue.  C/D layout 32x32: col(j) = lane&31, row(i) = (reg&3) + 8*(reg>>2) + 4*(lane>>5),
  // i.e. a lane holds ONE filter and 16 scattered cells: storing that directly would be 4-byte
  // scatters across 32 response planes.  Transpose the wave's 64-cell x 32-filter slab through the
  // (now free) feature-tile LDS so lanes run along cells: every store instruction then writes
  // four 64-B row segments of one plane.
  float* R = resp + lv.cell_off * nf;
  float* tr = ft + wave * (32 * 65);  // per-wave [32 filters][64 cells + 1]
  const int py = t.y0 + 4 * wave + (lane >> 4), pxx = t.x0 + (lane & 15);
  const bool pvalid = (py < H && pxx < W);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    tr[(lane & 31) * 65 + i] = acc0[r];
    tr[(lane & 31) * 65 + 32 + i] = acc1[r];
  }
  __syncthreads();
  for (int j = 0; j < 32; ++j) {
    const int fn = nbase + j;
    if (fn < nf && pvalid) R[(size_t)fn * H * W + (size_t)py * W + pxx] = tr[j * 65 + lane];
  }
  CONV_STAMP(4);
}

static void launch_conv_mfma(const ConvTile* tiles, int ntiles, const LevelDev* levels, const float* feat,
                             const float* wT, float* resp, int nf, int nfpad, hipStream_t s) {
  const size_t lds = sizeof(float) * (CT + 4) * (CT + 4) * CSTR;
  static LdsOptIn optin;
  optin.ensure((const void*)k_conv_mfma<5, 5>, lds);
  dim3 grid(ntiles, (nf + 31) / 32);
  hipLaunchKernelGGL((k_conv_mfma<5, 5>), grid, dim3(256), lds, s, tiles, levels, feat, wT, resp, nf, nfpad);
}

static int env_int(const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; }
// The knobs of the probe build alone: PBD_CONV_PRIO travels in the upper half of nfpad, which only a kernel compiled with PBD_PROBES
// strips again — the tuning library (this unit compiled without it) must never read it; PBD_MFMA64_QUARTERS was a probe-build knob too
#ifdef PBD_PROBES
static int probe_env_int(const char* name, int unset) { return env_int(name, unset); }
#else
static int probe_env_int(const char*, int unset) { return unset; }
#endif

// k_conv_mfma16 with the tuning knobs: PBD_CONV_LDS_KB (an occupancy cap by LDS request; uniform banks only — a mixed bank's launches
// are the product's) and, probe build, PBD_CONV_PRIO
template <typename T, int NHALF, int WPE, int NTW = 1, bool B4 = false, int KH_T = 5, int KW_T = 5>
static void launch_v(const ConvTile* tiles, int ntiles, const LevelDev* levels, const T* feat,
                     const T* wT, T* resp, int nf, int nfpad, hipStream_t s, int kh = 5, int kw = 5) {
  static const int lds_req_kb = env_int("PBD_CONV_LDS_KB", 0), prio_mode = probe_env_int("PBD_CONV_PRIO", 0);
  launch_conv_mfma16_t<T, NHALF, WPE, NTW, B4, KH_T, KW_T>(tiles, ntiles, levels, feat, wT, resp, nf, nfpad, s, kh, kw, 0, (size_t)lds_req_kb * 1024, prio_mode);
}

// ---------------------------------------------------------------------------
// k_conv_glds: the fp32 filter bank as a PERSISTENT, double-buffered workgroup.  k_conv_mfma16 runs the MFMA pipe at
// ~93 % while its K loops run, but every workgroup first stages its tile (global -> registers -> LDS, 9 + 5 us of a
// 75 us life) and ends with an epilogue, and co-resident workgroups run those phases in step: over the whole kernel
// the pipe is ~66 % busy.  Here a workgroup loops over work units (tile, pair of 16-filter n-tiles) and the NEXT
// channel half (of this unit, or half 0 of the next unit) streams into the other LDS buffer with
// global_load_lds_dwordx4 (LDS-DMA: no staging registers, no ds_write pass) while the MFMAs of the current half
// run.  LDS image of a half: [cell 0..399][16 channels], 64 B per cell, lane-linear as the DMA writes it (piece p =
// cells 16 p .. 16 p + 15, lane = 4 (cell & 15) + 16-byte chunk); border cells are DMA'd from a constant cell
// (0, and 1 for the truncation channel 31, src/SpatialConvolutionEngine.cpp:147-155).  A operand: lane (i, k) reads ONE
// ds_read_b128 per M-tile and tap = channels 4k .. 4k+3 of its cell, which feed k-steps s = 0..3 (k-step s contracts
// channels {s, 4+s, 8+s, 12+s}; the B rows are picked to match) -- the 16 cells of a full-width M-tile are 1 KB
// contiguous: conflict-free without padding.  Units of XCD x: tile positions 8 g + x (same convention as
// k_conv_mfma16, so the plan's neighbour pairing holds), n-pairs minor: the n-pairs of one tile are taken by adjacent
// workgroups of the XCD at the same time (one HBM fetch of the tile, L2 hits for the others).
// ---------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void pbd_lds_void;
typedef __attribute__((address_space(1))) const void pbd_glb_cvoid;

// PERSIST = false: the same operand paths (LDS-DMA staging, 16-byte A and B reads) without the persistent loop: one unit per
// workgroup, ONE 25.6 KB buffer (stage half, barrier, K loop, barrier, ...), grid and XCD mapping of k_conv_mfma16.
template <int WPE, bool PERSIST = true>
__global__ __launch_bounds__(256, WPE) void k_conv_glds(const ConvTile* __restrict__ tiles, const LevelDev* __restrict__ levels,
                                                        const float* __restrict__ feat, const float* __restrict__ wT,
                                                        float* __restrict__ resp, int nf, int nfpad, int ntiles,
                                                        const float* __restrict__ border) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TW = CT + 4, NCELL = TW * TW, NTAP = 25, NTW = 2, CH = 16, CELLB = CH * 4, BUFB = NCELL * CELLB, NPIECE = NCELL / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ai = lane & 15, ak = lane >> 4;
  const int np = (nf + 16 * NTW - 1) / (16 * NTW);
  // persistent: workgroup j of XCD blockIdx.x % 8 takes units j, j + nwx, ... of that XCD's tile positions xcd, xcd + 8, ...;
  // else: groups of 8 tiles x np n-pairs, all n-pairs of a tile on one XCD (k_conv_mfma16's mapping), one unit per workgroup
  const int xcd = blockIdx.x & 7;
  const int grp_ = (int)blockIdx.x / (8 * np), rem_ = (int)blockIdx.x - grp_ * (8 * np);
  const int j = PERSIST ? (int)(blockIdx.x >> 3) : grp_ * np + (rem_ >> 3);
  const int nwx = PERSIST ? (int)(gridDim.x >> 3) : (1 << 30);
  const int ntx = ntiles > xcd ? (ntiles - xcd + 7) >> 3 : 0;     // tile positions xcd, xcd + 8, ...
  const int nunits = ntx * np;
  char* const buf0 = smem;
  char* const buf1 = smem + BUFB;

  // one wave's share of the LDS-DMA pieces of channel half `half` of the tile at (y0, x0) of a W x H level: 16 cells x 64 B per piece
  auto issue_stage = [&](int y0, int x0, int W, int H, size_t cell_off, int half, char* buf) {
    const float* F = feat + cell_off * PBD_FLEN + half * CH + 4 * (lane & 3);
    const float* bz = border + half * CH + 4 * (lane & 3);
    for (int p = wave; p < NPIECE; p += 4) {
      const int cell = 16 * p + (lane >> 2);
      const int ty = cell / TW, tx = cell - ty * TW;
      const int y = y0 + ty - 2, x = x0 + tx - 2;
      const bool inside = (y >= 0 && y < H && x >= 0 && x < W);
      const float* src = inside ? F + ((size_t)y * W + x) * PBD_FLEN : bz;
      __builtin_amdgcn_global_load_lds((pbd_glb_cvoid*)src, (pbd_lds_void*)(buf + p * 1024), 16, 0, 0);
    }
  };

  int v = j;
  if (v >= nunits) return;
  int y0, x0, W, H;
  size_t cell_off;
  {
    const ConvTile t = tiles[xcd + 8 * (v / np)];
    const LevelDev lv = levels[t.level];
    y0 = t.y0; x0 = t.x0; W = lv.cw; H = lv.ch; cell_off = lv.cell_off;
  }
  GLDS_INIT();
  GLDS_T(tl0);
  if (PERSIST) issue_stage(y0, x0, W, H, cell_off, 0, buf0);
  while (v < nunits) {
    GLDS_T(t0_);
    // the next unit's descriptor (after the last unit: this unit again, its half 0 is then re-staged into the free buffer —
    // the DMA issue stays unconditional: under a condition hipcc drains the whole load queue at every tap pair of the next K loop)
    const int vn = PERSIST ? v + nwx : nunits;
    int y0n, x0n, Wn, Hn;
    size_t cell_offn;
    {
      const ConvTile tn = tiles[xcd + 8 * ((vn < nunits ? vn : v) / np)];
      const LevelDev lvn = levels[tn.level];
      y0n = tn.y0; x0n = tn.x0; Wn = lvn.cw; Hn = lvn.ch; cell_offn = lvn.cell_off;
    }
    const int nbase = (v % np) * (16 * NTW);
    const int vw = min(CT, W - x0), vh = min(CT, H - y0), ncell = vw * vh;
    const int nmt = (ncell + 15) >> 4;
    const int mvalid = __builtin_amdgcn_readfirstlane(max(0, min(4, (nmt - wave + 3) >> 2)));
    int aoff[4];   // byte offset of the lane's 16-byte A chunk (tap 0) per M-tile
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int c = min(16 * (wave + 4 * m) + ai, ncell - 1);
      const int cy = c / vw, cx = c - cy * vw;
      aoff[m] = (cy * TW + cx) * CELLB + 16 * ak;
    }
    f32x4 acc[NTW][4];
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[nt][m][r] = 0.f;
    const float* bsrc = wT + ((size_t)ak * nfpad + nbase + ai) * 4;   // w4[tap 0][half 0][k = ak][filter nbase + ai][s = 0..3]

    // MV = 4: all four M-tiles of the wave hold valid cells (the common case: no branch in the K loop); MV = 0: decided per M-tile at run time
    auto kloop = [&](const char* buf, int half, auto mv_tag) {
      constexpr int MV = decltype(mv_tag)::value;
      const float* bh = bsrc + (size_t)half * 16 * nfpad;
      f32x4 b0[NTW], b1[NTW];
      f32x4 a0[4], a1[4];
      auto load_b = [&](f32x4 (&dst)[NTW], int tap) {
        const float* bs = bh + (size_t)tap * PBD_FLEN * nfpad;
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) dst[nt] = *(const f32x4*)(bs + 64 * nt);
      };
      auto load_a = [&](f32x4 (&dst)[4], int tap) {
        const int ti = tap / 5, tj = tap - ti * 5;
        const char* a = buf + (ti * TW + tj) * CELLB;
#pragma unroll
        for (int m = 0; m < 4; ++m) dst[m] = *(const f32x4*)(a + aoff[m]);
      };
      auto mma = [&](const f32x4 (&av)[4], const f32x4 (&bw)[NTW]) {
#pragma unroll
        for (int s_ = 0; s_ < 4; ++s_)
#pragma unroll
          for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
            for (int m = 0; m < 4; ++m)
              if (MV == 4 || m < mvalid) acc[nt][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m][s_], bw[nt][s_], acc[nt][m], 0, 0, 0);
      };
      load_b(b0, 0);
      load_a(a0, 0);
      // vmcnt(0): the wave's DMA pieces of the NEXT buffer (issued just before) and tap 0's B have landed.  hipcc cannot count
      // past an LDS-DMA in flight: left pending it waits vmcnt(0) at the first MFMA of every tap pair (exposing the B latency
      // 12 times per K loop); drained here once (~1 us, the co-resident workgroup's waves keep the pipe busy) the loop gets
      // exact counted waits.
      __builtin_amdgcn_s_waitcnt(0x0F70);
      // taps in pairs, operands in explicit ping-pong: the next tap's B (global, L2-resident) and A (LDS) are in flight while
      // this tap's 32 MFMAs issue.  No condition inside the loop (hipcc sinks loads into a conditional use); tap 24 is peeled.
      _Pragma("unroll 1") for (int tap = 0; tap < NTAP - 1; tap += 2) {
        load_b(b1, tap + 1);
        load_a(a1, tap + 1);
        __builtin_amdgcn_sched_barrier(0);
        mma(a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        load_b(b0, tap + 2);
        load_a(a0, tap + 2);
        __builtin_amdgcn_sched_barrier(0);
        mma(a1, b1);
        __builtin_amdgcn_sched_barrier(0);
      }
      mma(a0, b0);
    };

    // two channel halves through ONE K-loop instance: half h computes on buffer h while the DMA fills buffer 1 - h with
    // half 1 of this unit (h = 0) or half 0 of the next unit (h = 1)
    _Pragma("unroll 1") for (int half = 0; half < 2; ++half) {
      GLDS_T(ta_);
      if (!PERSIST) {
        if (half) __syncthreads();                        // every wave is done with half 0
        issue_stage(y0, x0, W, H, cell_off, half, buf0);
      }
      __syncthreads();          // buffer `half` has landed (the DMA queue is drained before the barrier); every wave is done with buffer 1 - half
      GLDS_T(tb_);
      GLDS_C(cb_);
      char* const cur = (PERSIST && half) ? buf1 : buf0;
      if (PERSIST) {
        if (half == 0) issue_stage(y0, x0, W, H, cell_off, 1, buf1);
        else issue_stage(y0n, x0n, Wn, Hn, cell_offn, 0, buf0);
      }
      if (mvalid == 4) kloop(cur, half, std::integral_constant<int, 4>()); else kloop(cur, half, std::integral_constant<int, 0>());
      GLDS_T(tc_);
      GLDS_C(cc_);
      GLDS_ACC(0, ta_, tb_); GLDS_ACC(1, tb_, tc_); GLDS_ACC(4, cb_, cc_);
    }
    GLDS_T(t4_);
    __syncthreads();            // every wave is done reading buf1: its first 16.6 KB become the four waves' transposition slabs
    GLDS_T(t5_);
    {
      float* R = resp + cell_off * nf;
      float* tr = (float*)(PERSIST ? buf1 : buf0) + wave * (16 * 65);           // per-wave [16 filters][64 cells + 1]
      const int pc = 16 * (wave + 4 * (lane >> 4)) + (lane & 15);
      const int pcy = pc / vw, py = y0 + pcy, pxx = x0 + (pc - pcy * vw);
      const bool pvalid = pc < ncell;
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int r = 0; r < 4; ++r) tr[ai * 65 + m * 16 + 4 * ak + r] = acc[nt][m][r];   // D[i = 4 ak + r][j = ai] of M-tile m
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (int jf = 0; jf < 16; ++jf) {
          const int fn = nbase + 16 * nt + jf;
          if (fn < nf && pvalid) R[(size_t)fn * H * W + (size_t)py * W + pxx] = tr[jf * 65 + lane];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      }
    }
    GLDS_T(t6_);
    GLDS_ACC(2, t4_, t5_); GLDS_ACC(5, t5_, t6_);
    GLDS_ACC(6, 0ull, 1ull); GLDS_ACC(7, tl0 * 0ull + t0_, t6_);
    v = vn;
    y0 = y0n; x0 = x0n; W = Wn; H = Hn; cell_off = cell_offn;
  }
}

void launch_conv_glds_f32(const ConvTile* tiles, int ntiles, const LevelDev* levels, const float* feat, const float* wT,
                          float* resp, int nf, int nfpad, const float* border, int wg_per_cu, int ncu, hipStream_t s) {
  if (ntiles <= 0) return;
  const size_t lds = 2 * (size_t)(CT + 4) * (CT + 4) * 64;
  const int nwx = std::max(1, ncu / 8) * wg_per_cu;          // workgroups per XCD
  if (wg_per_cu <= 0) {    // one unit per workgroup, single buffer
    const int np = (nf + 31) / 32;
    static LdsOptIn optin;
    optin.ensure((const void*)k_conv_glds<3, false>, lds / 2);
    hipLaunchKernelGGL((k_conv_glds<3, false>), dim3((ntiles + 7) / 8 * 8 * np), dim3(256), lds / 2, s, tiles, levels, feat, wT, resp, nf, nfpad, ntiles, border);
  } else if (wg_per_cu >= 3) {
    static LdsOptIn optin;
    optin.ensure((const void*)k_conv_glds<3>, lds);
    hipLaunchKernelGGL((k_conv_glds<3>), dim3(8 * nwx), dim3(256), lds, s, tiles, levels, feat, wT, resp, nf, nfpad, ntiles, border);
  } else {
    static LdsOptIn optin;
    optin.ensure((const void*)k_conv_glds<2>, lds);
    hipLaunchKernelGGL((k_conv_glds<2>), dim3(8 * nwx), dim3(256), lds, s, tiles, levels, feat, wT, resp, nf, nfpad, ntiles, border);
  }
}

// float instantiations of k_conv_mfma16, by PBD_MFMA_VARIANT.  20 is the product's (k_conv.hip): 16x16x4 MFMA, tile staged in two
// channel halves, TWO 16-filter n-tiles per workgroup, B operand by 16-byte loads.  Two n-tiles per workgroup: alone the same time
// as one, but every tile is staged half as often and with frames in flight that VALU / LDS time goes to the other frames' DT blocks
// (1 392 vs 1 331 frames/s, batches of 4 on 3 handles).  16-byte B loads: 0.339 vs 0.388 ms sequential, 1 419 vs 1 391 frames/s (eight
// global_load_dword per 32 MFMAs cost the MFMA pipe a quarter of its issue rate: tests/tools/mfma_rate_probe.hip).
// 0 = the older 32x32x2 kernel, 1 = whole tile (0.42 ms), 2 = halves at 5 waves/SIMD (8 spilled registers), 3 = one n-tile, halves at
// 3+ waves per SIMD (0.39 ms), 4 = channel quarters, 5-9 = n-tile counts with 4-byte B loads, 10 / 11 / 19 / 18 = k_conv_glds at 2 / 3 /
// 1 workgroups per CU / one unit per workgroup (0.354 ms sequential, 1 353-1 378 frames/s), 21-27 = n-tile counts and register
// allocations with 16-byte B loads.  Tried and dropped: a persistent
// variant keeping the tile resident across a chunk of n-tiles with a register-direct epilogue (0.49 ms vs
// 0.44 ms, and long-running workgroups hurt the overlap with other frames' kernels); capping the kernel at
// two workgroups per CU to leave LDS and wave slots to co-running DT kernels (716 vs 751 frames/s); staging
// once for 2 or 5 n-tiles with a register-direct epilogue (one unaligned 16-byte store per M-tile and lane:
// 0.48-0.52 ms vs 0.43 ms — the LDS-transposed epilogue writes whole 64-byte row segments and is faster);
// double-buffered staging (next channel group prefetched into registers across the K loop, second LDS buffer):
// 0.51-0.71 ms vs 0.39 ms.
static void launch_variant_f32(const pbd_handle* h, int variant) {
  const pbd_model_desc& m = h->md;
  const ConvTile* tiles = h->d_conv_tiles;
  const LevelDev* levels = h->d_levels;
  const int ntiles = h->n_conv_tiles, nf = m.nfilters, nfpad = h->nfpad, kh = m.kh, kw = m.kw;
  // d_wT: [tap][channel][nfpad], the border cell, the [tap][half][k][n][s] copy (k_conv_glds), the [tap][half][k][n][u] copy (16-byte B loads)
  const size_t wt_n = (size_t)kh * kw * m.flen * nfpad;
  const float* feat = (const float*)h->d_feat, *wT = (const float*)h->d_wT, *border = wT + wt_n, *w4s = border + m.flen, *w4u = w4s + wt_n;
  float* resp = (float*)h->d_resp;
  hipStream_t s = h->stream;
  if (ntiles <= 0) return;
  if (variant >= 10 && variant < 20 && kh == 5 && kw == 5 && m.flen == PBD_FLEN)
    launch_conv_glds_f32(tiles, ntiles, levels, feat, w4s, resp, nf, nfpad, border, variant == 19 ? 1 : variant == 18 ? 0 : variant - 8, h->ncu, s);
  else if (kh != 5 || kw != 5)   // any other filter size: the default configuration with a run-time tap loop, whatever the variant
    launch_v<float, 2, 3, 2, true, 0, 0>(tiles, ntiles, levels, feat, w4u, resp, nf, nfpad, s, kh, kw);
  else if (variant == 0) launch_conv_mfma(tiles, ntiles, levels, feat, wT, resp, nf, nfpad, s);
  else if (variant == 20) launch_v<float, 2, 3, 2, true>(tiles, ntiles, levels, feat, w4u, resp, nf, nfpad, s);   // two n-tiles per workgroup, 16-byte B loads
  else if (variant == 21) launch_v<float, 2, 3, 1, true>(tiles, ntiles, levels, feat, w4u, resp, nf, nfpad, s);   // one n-tile, 16-byte B loads
  else if (variant == 22) launch_v<float, 2, 2, 2, true>(tiles, ntiles, levels, feat, w4u, resp, nf, nfpad, s);   // two n-tiles, 2 waves/SIMD allocation
  else if (variant == 23) launch_v<float, 2, 2, 5, true>(tiles, ntiles, levels, feat, w4u, resp, nf, nfpad, s);   // five n-tiles (80 filters), 16-byte B loads
  else if (variant == 24) launch_v<float, 2, 2, 3, true>(tiles, ntiles, levels, feat, w4u, resp, nf, nfpad, s);   // three n-tiles (48 filters)
  else if (variant == 25) launch_v<float, 2, 4, 2, true>(tiles, ntiles, levels, feat, w4u, resp, nf, nfpad, s);   // two n-tiles, register allocation for 4 waves per SIMD
  else if (variant == 26) launch_v<float, 2, 4, 1, true>(tiles, ntiles, levels, feat, w4u, resp, nf, nfpad, s);   // one n-tile, 4 waves per SIMD
  else if (variant == 27) launch_v<float, 2, 5, 1, true>(tiles, ntiles, levels, feat, w4u, resp, nf, nfpad, s);   // one n-tile, 5 waves per SIMD
  else if (variant == 5) launch_v<float, 2, 3, 2>(tiles, ntiles, levels, feat, wT, resp, nf, nfpad, s);        // two n-tiles (32 filters) per workgroup
  else if (variant == 6) launch_v<float, 2, 2, 2>(tiles, ntiles, levels, feat, wT, resp, nf, nfpad, s);
  else if (variant == 7) launch_v<float, 1, 2, 2>(tiles, ntiles, levels, feat, wT, resp, nf, nfpad, s);   // whole tile, 32 filters
  else if (variant == 8) launch_v<float, 2, 2, 5>(tiles, ntiles, levels, feat, wT, resp, nf, nfpad, s);   // five n-tiles (80 filters) per workgroup
  else if (variant == 9) launch_v<float, 2, 3, 5>(tiles, ntiles, levels, feat, wT, resp, nf, nfpad, s);
  else if (variant == 2) launch_v<float, 2, 5>(tiles, ntiles, levels, feat, wT, resp, nf, nfpad, s);
  else if (variant == 3) launch_v<float, 2, 3>(tiles, ntiles, levels, feat, wT, resp, nf, nfpad, s);
  else if (variant == 4) launch_v<float, 4, 3>(tiles, ntiles, levels, feat, wT, resp, nf, nfpad, s);
  else launch_v<float, 1, 3>(tiles, ntiles, levels, feat, wT, resp, nf, nfpad, s);
}

// double: PBD_MFMA64_QUARTERS 1 (the product's) = four 8-channel passes with 16-byte B loads, 2 = the same with 8-byte B loads, 0 = two
// 16-channel halves (54 KB of LDS; the quarters measured 7 % faster)
static void launch_variant_f64(const pbd_handle* h, int q) {
  const pbd_model_desc& m = h->md;
  const size_t wt_n = (size_t)m.kh * m.kw * m.flen * h->nfpad;
  const double* feat = (const double*)h->d_feat, *wT = (const double*)h->d_wT, *w4u = wT + wt_n + m.flen;
  double* resp = (double*)h->d_resp;
  if (h->n_conv_tiles <= 0) return;
  if (m.kh != 5 || m.kw != 5) launch_v<double, 4, 2, 1, true, 0, 0>(h->d_conv_tiles, h->n_conv_tiles, h->d_levels, feat, w4u, resp, m.nfilters, h->nfpad, h->stream, m.kh, m.kw);
  else if (q == 2) launch_v<double, 4, 2>(h->d_conv_tiles, h->n_conv_tiles, h->d_levels, feat, wT, resp, m.nfilters, h->nfpad, h->stream);
  else if (q) launch_v<double, 4, 2, 1, true>(h->d_conv_tiles, h->n_conv_tiles, h->d_levels, feat, w4u, resp, m.nfilters, h->nfpad, h->stream);
  else launch_v<double, 2, 2>(h->d_conv_tiles, h->n_conv_tiles, h->d_levels, feat, wT, resp, m.nfilters, h->nfpad, h->stream);
}

static bool g_variant_ran = false;
}   // namespace conv_variants

// The bank of a tuning / probe build: true when it is uniform, a knob is set and it has been launched here.  The probe build's
// conv_debug_read follows the handle's LAST bank launch: this unit's stamps after a variant, k_conv.hip's after a product kernel.
bool launch_conv_variant(const pbd_handle* h) {
  using conv_variants::env_int;
  using conv_variants::probe_env_int;
  static const int mfma = env_int("PBD_MFMA_VARIANT", -1), quarters = probe_env_int("PBD_MFMA64_QUARTERS", -1), split = env_int("PBD_SPLIT_VARIANT", -1);
  static const bool knobs = env_int("PBD_CONV_LDS_KB", 0) > 0 || probe_env_int("PBD_CONV_PRIO", 0) != 0;
  conv_variants::g_variant_ran = false;
  if (h->mixed) return false;
  if (h->conv_mode == PBD_CONV_SPLIT || h->conv_mode == PBD_CONV_SPLIT_F16) {
    if (split < 0) return false;
    launch_conv_split_variant(h, split);
  } else if (h->conv_mode == PBD_CONV_MFMA && h->ts == 8) {
    if (quarters < 0 && !knobs) return false;
    conv_variants::launch_variant_f64(h, quarters < 0 ? 1 : quarters);
  } else if (h->conv_mode == PBD_CONV_MFMA) {
    if (mfma < 0 && !knobs) return false;
    conv_variants::launch_variant_f32(h, mfma < 0 ? 20 : mfma);
  } else return false;
  conv_variants::g_variant_ran = true;
  return true;
}

#ifdef PBD_PROBES
bool conv_variants_debug_read(unsigned long long* out) {
  if (conv_variants::g_variant_ran) hipMemcpyFromSymbol(out, HIP_SYMBOL(conv_variants::pbd_conv_dbg), sizeof(unsigned long long) * 8);
  return conv_variants::g_variant_ran;
}
#endif
