// k_conv_mfma16.hpp — what the filter-bank units share: the tile staging (stage_tile, the ONE place that holds the reference's border
// rule) and the 16x16x4 MFMA kernel template with its launcher.  Included by k_conv.hip (the kernels a product handle launches) and,
// inside a namespace of its own, by k_conv_variants.hip (tune and probe libraries only): an instantiation made there never shares a
// kernel handle or a stamp buffer with the product's.  No include guard on purpose (a guard would
// silently drop the second of two inclusions under different namespaces): textual inclusion, once per unit, after pbd_internal.hpp and
// <algorithm>; everything it defines is a declaration that lands in the including namespace, CONV_STAMP the one macro.

// debug: per-phase wall-clock stamps (100 MHz) of one workgroup of the unit's last stamped launch
#ifdef PBD_PROBES
static __device__ unsigned long long pbd_conv_dbg[8];
#define CONV_STAMP(i) do { if (blockIdx.x == 300 && blockIdx.y == 2 && threadIdx.x == 0) pbd_conv_dbg[i] = wall_clock64(); } while (0)
#else
#define CONV_STAMP(i) do { } while (0)
#endif

constexpr int CT = 16;   // spatial tile side (cells)

// Stage channels c0 .. c0 + CPP - 1 of the (CT+KH-1) x (CT+KW-1) cell tile with halo into LDS ([cell][CS]).  CPP / (16 / sizeof(T)) lanes
// fetch one cell's channels as 16-byte vectors (coalesced); BATCH independent loads are in flight before the first wait (a caller with a
// compile-time size that wants every load in flight passes the tile's number of batches).  Clamped addresses, the border value is selected
// after the load: 0, or 1 for the truncation channel = the pass's last channel when `trunc` (src/SpatialConvolutionEngine.cpp:147-155).
template <typename T, int CPP, int CS, int BATCH>
__device__ __forceinline__ void stage_tile(T* __restrict__ ft, const T* __restrict__ F, int y0, int x0, int H, int W,
                                           int KH, int KW, int c0, bool trunc, int tid) {
  constexpr int EPV = 16 / (int)sizeof(T), LPC = CPP / EPV;         // elements per 16-byte vector, lanes per cell
  struct alignas(16) V { T e[EPV]; };
  const int TW = CT + KW - 1, TH = CT + KH - 1, N = TH * TW * LPC, NB = (N + 255) / 256;
  for (int j0 = 0; j0 < NB; j0 += BATCH) {
    V r[BATCH];
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int i = min(tid + (j0 + j) * 256, N - 1);
      const int cell = i / LPC, q = i - cell * LPC;
      const int ty = cell / TW, tx = cell - ty * TW;
      const int y = min(max(y0 + ty - KH / 2, 0), H - 1), x = min(max(x0 + tx - KW / 2, 0), W - 1);
      r[j] = *(const V*)(F + ((size_t)y * W + x) * PBD_FLEN + c0 + q * EPV);
    }
    __builtin_amdgcn_sched_barrier(0);   // every load of the batch is issued before the first store waits for one
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int i = tid + (j0 + j) * 256;
      if (i < N) {
        const int cell = i / LPC, q = i - cell * LPC;
        const int ty = cell / TW, tx = cell - ty * TW;
        const int y = y0 + ty - KH / 2, x = x0 + tx - KW / 2;
        const bool inside = (y >= 0 && y < H && x >= 0 && x < W);
        T* d = ft + cell * CS + q * EPV;
#pragma unroll
        for (int k = 0; k < EPV; ++k) d[k] = inside ? r[j].e[k] : (T)((trunc && q == LPC - 1 && k == EPV - 1) ? 1 : 0);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// 16x16x4 MFMA implicit GEMM, instantiated for double (v_mfma_f64_16x16x4_f64: the filter bank of the
// double instantiation) and for float (v_mfma_f32_16x16x4_f32).  M = cells, N = filters, K = kh*kw*32.
// Measured on MI355X (tests/tools/mfma64_probe.hip, mfma16_probe.hip): f64 64 cycles per instruction and
// SIMD = 72 TFLOP/s; operand layout A[i = l&15][k = l>>4], B[k = l>>4][j = l&15] for both; result
// D[i = 4*reg + (l>>4)][j = l&15] (f64) / D[i = 4*(l>>4) + reg][j = l&15] (f32).
// Workgroup = 4 waves: 16x16 cells x ONE 16-filter n-tile, grid = (tiles, nfpad/16).  The VALID cells of the tile
// (levels are ragged: the last tile of a row / column is cut by the level's edge) are numbered row-major and cut
// into 16-cell M-tiles; wave w owns M-tiles w, w + 4, w + 8, w + 12 = up to four accumulators, and an M-tile beyond
// the last valid cell issues no MFMAs (13 % of the MFMA work of a 640x480 pyramid was padding when an M-tile was a
// fixed 16-cell row segment).  The 20x20-cell feature tile is staged in
// NHALF channel groups (double: two 16-channel halves, 54 KB -> three workgroups per CU), cell stride
// CH+1 elements (conflict-free across the 16 cells of an M-tile).  B: one element per lane and k-step, a
// whole tap loaded from the L2-resident [tap][channel][nfpad] array one tap ahead, ping-pong registers.
// Accumulation is a k-ordered fma chain (half, tap, channel): not the reference's order, tolerance-based.
// ---------------------------------------------------------------------------
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <typename T> struct Mfma16;
template <> struct Mfma16<double> {
  typedef f64x4 acc_t;
  static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int drow(int reg, int ak) { return 4 * reg + ak; }
};
template <> struct Mfma16<float> {
  typedef f32x4 acc_t;
  static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int drow(int reg, int ak) { return 4 * ak + reg; }
};

// B4 (float, two channel halves; double, four 8-channel groups): wT is the [tap][group][k][nfpad][u] copy of the filters (channel
// CH group + 4 u + k): a lane reads the k-steps of a tap and n-tile with ONE 16-byte load instead of four global_load_dword (which cost the MFMA pipe a quarter of its
// issue rate with two waves per SIMD: tests/tools/mfma_rate_probe.hip)
// KH_T / KW_T > 0: compile-time filter size (the 5x5 bank of the person / face models: tap loops and tile geometry fold);
// 0: the size comes from the kernel arguments (any kh x kw <= 9 x 9, src/SpatialConvolutionEngine.cpp:133-159 takes any).
// MIX: a size group of a mixed bank, as in k_conv_exact_generic (run-time size only).
template <typename T, int KH_T, int KW_T, int NHALF, int WPE, int NTW = 1, bool B4 = false, bool MIX = false>   // WPE: waves per SIMD the register allocation must allow; NTW: 16-filter n-tiles per workgroup
__global__ __launch_bounds__(256, WPE) void k_conv_mfma16(const ConvTile* __restrict__ tiles,
                                                     const LevelDev* __restrict__ levels,
                                                     const T* __restrict__ feat, const T* __restrict__ wT,
                                                     T* __restrict__ resp, int nf, int nfpad, int ntiles_total, int kh_rt, int kw_rt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef Mfma16<T> MM;
  const int KH = KH_T > 0 ? KH_T : kh_rt, KW = KW_T > 0 ? KW_T : kw_rt;
  const int TW = CT + KW - 1, NTAP = KH * KW;
  // channels per pass, LDS cell stride, k-steps per tap.  Float: stride CH + 2 = 18 dwords: the 32 lanes of one LDS
  // access group (16 cells x 2 channels) then hit 32 different banks (16 * 18 mod 32 are the 16 even residues); with
  // 17 the cell 15 / channel 1 lane fell on cell 0's bank (SQ_LDS_BANK_CONFLICT was twice SQ_ACTIVE_INST_LDS)
  constexpr int CH = PBD_FLEN / NHALF, CS = CH + (sizeof(T) == 4 ? 2 : 1), KS = CH / 4;
  constexpr int EPV = 16 / (int)sizeof(T);                          // elements per 16-byte vector
  struct alignas(16) V { T e[EPV]; };
  T* ft = (T*)smem;                         // [TH][TW][CS]
  CONV_STAMP(0);
#ifdef PBD_PROBES
  {  // probe: issue priority by workgroup index, to pull co-resident workgroups out of phase
    const unsigned lin_ = blockIdx.x + blockIdx.y * gridDim.x;
    const int mode = nfpad >> 16;
    const unsigned pr = mode == 1 ? (lin_ & 3u) : mode == 2 ? ((lin_ >> 8) & 3u) : mode == 3 ? ((lin_ >> 3) & 3u) : mode == 4 ? ((lin_ >> 10) & 3u) : mode == 5 ? (blockIdx.y & 3u) : 0u;
    if (pr == 1) __builtin_amdgcn_s_setprio(1); else if (pr == 2) __builtin_amdgcn_s_setprio(2); else if (pr == 3) __builtin_amdgcn_s_setprio(3);
  }
  nfpad &= 0xffff;
#endif
  // XCD-aware workgroup -> (tile, n-tile) mapping.  Workgroup b runs on XCD b % 8 and every XCD has its own L2; the
  // ny n-tile workgroups of one spatial tile all stage the same 20x20-cell feature tile.  With (tile, n-tile) =
  // (blockIdx.x, blockIdx.y) they were 604 workgroups apart and on 8 different XCDs: the tile came from HBM ~10
  // times (FETCH 5.9x the algorithmic bytes, r01).  Here groups of 8 tiles x ny n-tiles are laid out so that all
  // n-tiles of a tile share b % 8 and are dispatched within 8 * ny consecutive workgroups: one HBM fetch, ny - 1 L2 hits.
  const int ny = gridDim.y;                      // n-tiles (the launch keeps the 2-D grid shape; only the roles are permuted)
  const int lin = blockIdx.x + blockIdx.y * gridDim.x;
  const int grp = lin / (8 * ny), rem = lin - grp * (8 * ny);
  const int tile_i = grp * 8 + (rem & 7), ntile_i = rem >> 3;
  if (tile_i >= ntiles_total) return;            // the grid is padded to a multiple of 8 tiles
  const ConvTile t = tiles[tile_i];
  const LevelDev lv = levels[t.level];
  const int H = lv.ch, W = lv.cw;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nbase = ntile_i * (16 * NTW);
  const T* F = feat + lv.cell_off * PBD_FLEN;
  const int ai = lane & 15, ak = lane >> 4;
  static_assert(!B4 || (sizeof(T) == 4 && NHALF == 2) || (sizeof(T) == 8 && NHALF == 4), "16-byte B loads: the k-steps of a channel group fill one 16-byte vector");
  const T* bsrc = B4 ? wT + ((size_t)ak * nfpad + nbase + ai) * KS     // w4[tap 0][group 0][k = ak][filter nbase + ai][u = 0..KS-1]
                     : wT + (size_t)ak * nfpad + nbase + ai;           // B[k = ak][j = ai] of k-step 0, tap 0, half 0, n-tile 0 (n-tile nt: + 16 nt)
  typename MM::acc_t acc[NTW][4];
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[nt][m][r] = (T)0;
  // packed M-tiles: valid cell c = 16 * (wave + 4 m) + ai of the vh x vw valid region -> (c / vw, c % vw); cells past the
  // last one repeat it (their products are never stored)
  const int vw = min(CT, W - t.x0), vh = min(CT, H - t.y0), ncell = vw * vh;
  const int nmt = (ncell + 15) >> 4;                                                        // M-tiles of the tile
  const int mvalid = __builtin_amdgcn_readfirstlane(max(0, min(4, (nmt - wave + 3) >> 2)));   // M-tiles of this wave
  // c / vw for c < 256, vw <= 16 as a multiply: floor(c * ceil(2^16 / vw) / 2^16) is exact there (error < c (vw - 1) / (vw 2^16) < 1 / vw);
  // one wave-uniform division for the constant instead of a full 32-bit division sequence per lane and M-tile
  const unsigned vw_magic = 65535u / (unsigned)vw + 1u;
  int aoff[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int c = min(16 * (wave + 4 * m) + ai, ncell - 1);
    const int cy = (int)(((unsigned)c * vw_magic) >> 16), cx = c - cy * vw;
    aoff[m] = (cy * TW + cx) * CS + ak;
  }

#pragma unroll 1
  for (int half = 0; half < NHALF; ++half) {
    if (half) __syncthreads();
    const T* bh = bsrc + (size_t)(half * CH) * nfpad;
    T b0[NTW][KS], b1[NTW][KS];
    auto load_tap = [&](T (&dst)[NTW][KS], int tap) {
      const T* bs = bh + (size_t)min(tap, NTAP - 1) * PBD_FLEN * nfpad;
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) {
        if constexpr (B4) {
          const V w = *(const V*)(bs + 16 * KS * nt);
#pragma unroll
          for (int u = 0; u < KS; ++u) dst[nt][u] = w.e[u];
        } else {
#pragma unroll
          for (int u = 0; u < KS; ++u) dst[nt][u] = bs[(size_t)(4 * u) * nfpad + 16 * nt];
        }
      }
    };
    load_tap(b0, 0);   // tap 0, issued before the staging
    // stage CH channels of every cell (a tighter register allocation stages in smaller batches)
    stage_tile<T, CH, CS, (WPE >= 4 ? 4 : 7)>(ft, F, t.y0, t.x0, H, W, KH, KW, half * CH, half == NHALF - 1, tid);
    __syncthreads();
    CONV_STAMP(1 + 2 * half);
    // The K loop of one channel group, instantiated per number of M-tiles the wave owns (MV = 1..4, wave-uniform: a ragged
    // tile leaves some waves with fewer).  With the count tested inside the loop (`if (m < mvalid)`) hipcc guarded EVERY MFMA
    // with its own scalar branch — 32 branches per tap between instructions that should issue back to back.
    auto k_loop = [&](auto mv_tag) {
      constexpr int MV = decltype(mv_tag)::value;
      auto mma_tap = [&](const T (&bw)[NTW][KS], int tap) {
        const int ti = tap / KW, tj = tap - ti * KW;
        const T* a = ft + (ti * TW + tj) * CS;
#pragma unroll
        for (int u = 0; u < KS; ++u) {
          T av[MV];
#pragma unroll
          for (int m = 0; m < MV; ++m) av[m] = a[aoff[m] + 4 * u];    // one A element per M-tile, shared by the workgroup's n-tiles
#pragma unroll
          for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
            for (int m = 0; m < MV; ++m) acc[nt][m] = MM::mma(av[m], bw[nt][u], acc[nt][m]);
        }
      };
      auto tap_pair = [&](int tap) {
        load_tap(b1, tap + 1);
        mma_tap(b0, tap);
        if (tap + 1 < NTAP) {
          load_tap(b0, tap + 2);
          mma_tap(b1, tap + 1);
        }
      };
      if constexpr (NHALF == 1 && NTW == 1 && KH_T > 0) {
        for (int tap = 0; tap < NTAP; tap += 2) tap_pair(tap);
      } else {   // with half the k-steps per tap hipcc would unroll all taps and run out of registers
        _Pragma("unroll 1") for (int tap = 0; tap < NTAP; tap += 2) tap_pair(tap);
      }
    };
    if (mvalid == 4) k_loop(std::integral_constant<int, 4>());
    else if (mvalid == 3) k_loop(std::integral_constant<int, 3>());
    else if (mvalid == 2) k_loop(std::integral_constant<int, 2>());
    else if (mvalid == 1) k_loop(std::integral_constant<int, 1>());   // (0: M-tiles past the tile's last valid cell: no MFMA work)
    CONV_STAMP(2 + 2 * half);
  }
  __syncthreads();  // all waves are done reading the feature tile: reuse it for the epilogue
  CONV_STAMP(5);
  // Epilogue: transpose the wave's 64-cell x 16-filter slab of each n-tile through LDS so lanes run along cells
  // (a store instruction then writes whole 64-B row segments of one response plane).  The slab is private to the
  // wave and a wave's LDS operations execute in order, so the n-tiles simply follow each other.
  T* R = resp + lv.cell_off * nf;
  int nfw = nf;   // planes this launch writes
  if constexpr (MIX) { R += (size_t)(t.pad & 0xFFFF) * H * W; nfw = t.pad >> 16; }
  T* tr = ft + wave * (16 * 65);           // per-wave [16 filters][64 cells + 1]
  // lane -> slot (M-tile lane >> 4, row lane & 15) -> packed cell -> (row, column) of the level
  const int pc = 16 * (wave + 4 * (lane >> 4)) + (lane & 15);
  const int pcy = (int)(((unsigned)pc * vw_magic) >> 16), py = t.y0 + pcy, pxx = t.x0 + (pc - pcy * vw);   // (pc < 256)
  const bool pvalid = pc < ncell;
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) tr[ai * 65 + m * 16 + MM::drow(r, ak)] = acc[nt][m][r];   // D[i][j = ai] of M-tile m
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // (plane base wave-uniform, the lane's cell a 32-bit offset: a store is one LDS read + one store instruction, no address
    // arithmetic per filter — it was seven vector instructions per store)
    if (pvalid) {
      const unsigned cellb = (unsigned)(py * W + pxx) * (unsigned)sizeof(T);      // < 2^31 (plan_frame: a level has < 2^28 cells)
      for (int j = 0; j < 16; ++j) {
        const int fn = nbase + 16 * nt + j;
        if (fn < nfw) {
          char* plane = (char*)(R + (size_t)fn * H * W);
          *(T*)(plane + cellb) = tr[j * 65 + lane];
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  CONV_STAMP(6);
}

// KH_T = KW_T = 5: the compile-time 5x5 instantiation; 0: any kh x kw (run-time tap loop).  lds_min, prio: k_conv_variants.hip's knobs (an
// occupancy cap by LDS request; the probe build's issue-priority mode, carried in the upper half of nfpad) — the product passes neither
template <typename T, int NHALF, int WPE, int NTW = 1, bool B4 = false, int KH_T = 5, int KW_T = 5, bool MIX = false>
static void launch_conv_mfma16_t(const ConvTile* tiles, int ntiles, const LevelDev* levels, const T* feat, const T* wT, T* resp, int nf,
                                 int nfpad, hipStream_t s, int kh = 5, int kw = 5, int nf_stride = 0, size_t lds_min = 0, int prio = 0) {
  // a channel group of the tile with halo, or the four waves' transposition slabs of the epilogue
  const size_t lds = std::max({sizeof(T) * (CT + kh - 1) * (CT + kw - 1) * (PBD_FLEN / NHALF + (sizeof(T) == 4 ? 2 : 1)), sizeof(T) * 4 * 16 * 65, lds_min});
  static LdsOptIn optin;   // one per instantiation
  optin.ensure((const void*)k_conv_mfma16<T, KH_T, KW_T, NHALF, WPE, NTW, B4, MIX>, lds);
  dim3 grid((ntiles + 7) / 8 * 8, (nf + 16 * NTW - 1) / (16 * NTW));   // tiles padded to a multiple of 8 (XCD-aware mapping in the kernel)
  hipLaunchKernelGGL((k_conv_mfma16<T, KH_T, KW_T, NHALF, WPE, NTW, B4, MIX>), grid, dim3(256), lds, s, tiles, levels, feat, wT, resp, MIX ? nf_stride : nf,
                     nfpad | (prio << 16), ntiles, kh, kw);
}
