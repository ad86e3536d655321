// k_conv_split32_m32.hpp — the split-product bank's kernel template on v_mfma_f32_32x32x16 (32-cell M-tiles, 32-filter n-tiles) and its
// launchers: the product's kernel until its K loop moved to 16x16x32 (k_conv_split32.hpp), kept as it was measured for
// k_conv_split_variants.hip, which includes it inside a namespace of its own (the tuning variants: tune and probe libraries only).
// No include guard on purpose: textual inclusion, once per unit, after pbd_internal.hpp, <type_traits> and conv_split_ntiles().
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// NT: 32-filter n-tiles per workgroup (1..5); NW: wavefronts per workgroup (2: a 16 x 8 half of a ConvTile, 4: the whole 16 x 16 tile)
// PIN: the K loop's schedule for ONE wavefront per SIMD (see the loop): 1 = the next k-step's loads as a block in front of this k-step's MFMAs,
// 2 = the same loads dealt out between the MFMAs (sched_group_barrier); 0: hipcc's own schedule at two wavefronts per SIMD
// NS: parts per operand — 3: bfloat16 parts, six products (PBD_CONV_SPLIT); 2: scaled binary16 parts, three products (PBD_CONV_SPLIT_F16, below)
// MIX: one size group of a mixed bank (pbd_create_sized): the tile's pad = n0 | (nf_g << 16) — planes n0 .. n0 + nf_g - 1 of a level block
// of `nf` planes; filt / oscale are the group's own (ConvTile, pbd_internal.hpp)
template <int NT, int NW, int PIN, int NS = 3, bool MIX = false>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(1, PIN ? 1 : 2))) void k_conv_split32(const ConvTile* __restrict__ tiles, const LevelDev* __restrict__ levels,
                                                             const uint16_t* __restrict__ feat, const uint16_t* __restrict__ filt,
                                                             float* __restrict__ resp, int nf, int ntl_bank, int ntile0, int ngroups,
                                                             int ntiles_total, int kh, int kw, const float* __restrict__ oscale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using opnd = std::conditional_t<NS == 3, bf16x8, f16x8>;
  constexpr int ROWS = 4 * NW, NHALVES = 16 / ROWS, NTHR = 64 * NW, PPC = 4 * NS;   // PPC: 16-byte pieces per cell
  const int TW = 16 + kw - 1, TH = ROWS + kh - 1, NC = TW * TH, PLANE = NC * 64;
  // workgroup -> (tile, role = (half, n-group)): tile position 8 g + x runs on XCD x (the plan pairs horizontal neighbours on that
  // convention); the roles of a tile share lin % 8 (one XCD: the halves' common halo rows and the n-groups' common tile come from
  // HBM once) and are dispatched 8 workgroups apart
  const int R = NHALVES * ngroups;
  const int lin = blockIdx.x;
  const int grp = lin / (8 * R), rem = lin - grp * (8 * R);
  const int tile_i = grp * 8 + (rem & 7), role = rem >> 3;
  if (tile_i >= ntiles_total) return;
  const int half = role & (NHALVES - 1), ngroup = role / NHALVES;
  const ConvTile t = tiles[tile_i];
  const LevelDev lv = levels[t.level];
  const int H = lv.ch, W = lv.cw;
  const int ty0 = t.y0 + ROWS * half, tx0 = t.x0;
  if (ty0 >= H) return;                                  // the lower half of a tile on the level's last rows
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint16_t* F = feat + lv.cell_off * (NS * PBD_FLEN);
  {  // stage the halo tile: 4 NS 16-byte pieces per cell (piece = 4 split + channel group), batches of independent loads; outside the
     // level: zeros, and 1.0 (0x3F80, exact in bfloat16: part h; binary16 parts: 2^12 = 0x6C00) in the truncation channel = element 7 of piece 3 (:147-155)
    const int NPC = NC * PPC, oy = ty0 - kh / 2, ox = tx0 - kw / 2;
    constexpr unsigned ONE = NS == 3 ? 0x3F800000u : 0x6C000000u;
    auto cell_of = [](int i) { return NS == 3 ? (int)(((unsigned)i * 43691u) >> 19) : i >> 3; };     // i / 12 (exact for i < 2^17), i / 8
    const unsigned magic_tw = 0xFFFFFFFFu / (unsigned)TW + 1u;     // cell / TW = umulhi(cell, magic) (cell * TW < 2^32)
    constexpr int BATCH = 12;
    for (int i0 = 0; i0 < NPC; i0 += NTHR * BATCH) {
      u32x4 v[BATCH];
#pragma unroll
      for (int j = 0; j < BATCH; ++j) {
        const int i = min(i0 + j * NTHR + tid, NPC - 1);
        const int cell = cell_of(i), piece = i - cell * PPC;
        const int cy = (int)__umulhi((unsigned)cell, magic_tw), cx = cell - cy * TW;
        const int y = min(max(oy + cy, 0), H - 1), x = min(max(ox + cx, 0), W - 1);
        v[j] = *(const u32x4*)(F + ((size_t)(y * W + x) * (NS * PBD_FLEN) + piece * 8));
      }
#pragma unroll
      for (int j = 0; j < BATCH; ++j) {
        const int i = i0 + j * NTHR + tid;
        if (i < NPC) {
          const int cell = cell_of(i), piece = i - cell * PPC;
          const int cy = (int)__umulhi((unsigned)cell, magic_tw), cx = cell - cy * TW;
          const int y = oy + cy, x = ox + cx;
          const bool inside = y >= 0 && y < H && x >= 0 && x < W;
          const u32x4 border = u32x4{0u, 0u, 0u, piece == 3 ? ONE : 0u};
          const int q = piece & 3;
          *(u32x4*)(smem + (piece >> 2) * PLANE + cell * 64 + ((q ^ ((cell >> 2) & 3)) << 4)) = inside ? v[j] : border;
        }
      }
    }
  }
  __syncthreads();
  // lane -> (cell position inside a 32-cell M-tile, k-group).  ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27},
  // {4-11, 16-19, 28-31} (+32): positions are dealt so that each group is 16 consecutive positions = one row of a full-width unit
  const int c = lane & 31, kg = lane >> 5;
  const int mid = ((c & 15) >= 4 && (c & 15) < 12) ? 1 : 0;
  const int pos = (c & 15) + 16 * (mid ^ (c >> 4));
  // packed M-tiles: valid cell number 32 j + pos of the vh x vw valid region, j = wave + NW m (round robin: a ragged unit's
  // M-tiles spread over the wavefronts); positions past the last cell repeat it (never stored)
  const int vw = min(16, W - tx0), vh = min(ROWS, H - ty0), ncell = vw * vh;
  const int nmt = (ncell + 31) >> 5;
  const int mvalid = __builtin_amdgcn_readfirstlane(max(0, min(2, (nmt - wave + NW - 1) / NW)));
  const unsigned vw_magic = 65535u / (unsigned)vw + 1u;   // idx / vw for idx < 256 (k_conv_mfma16)
  int cl0[2], cofs[2];
  bool cval[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int idx = 32 * (wave + NW * m) + pos;
    cval[m] = idx < ncell;
    const int ic = min(idx, ncell - 1);
    const int cy = (int)(((unsigned)ic * vw_magic) >> 16), cx = ic - cy * vw;
    cl0[m] = cy * TW + cx;
    cofs[m] = (ty0 + cy) * W + tx0 + cx;
  }
  const int ntb = ntile0 + ngroup * NT;                  // first n-tile of this workgroup
  f32x16 acc[NT][2];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nt][m][r] = 0.f;
  const uint16_t* bl = filt + (size_t)ntb * 512 + lane * 8;
  const size_t bs_split = (size_t)ntl_bank * 512, bs_kstep = NS * bs_split;
  const int nkstep = 2 * kh * kw;
#ifdef PBD_BANK_PRIO   // experiment builds only: the K loop's wavefronts at a raised issue priority against the other batches' kernels on the SIMD
  __builtin_amdgcn_s_setprio(PBD_BANK_PRIO);
#endif

  auto k_loop = [&](auto mv_tag) __attribute__((always_inline)) {
    constexpr int MV = decltype(mv_tag)::value;
    auto load_b = [&](opnd (&b)[NT][NS], int kstep) __attribute__((always_inline)) {
      const uint16_t* p = bl + (size_t)min(kstep, nkstep - 1) * bs_kstep;
#pragma unroll
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) b[nt][s] = *(const opnd*)(p + s * bs_split + nt * 512);
    };
    auto load_a = [&](opnd (&a)[2][NS], int tapofs, int ks) __attribute__((always_inline)) {     // tapofs = ti * TW + tj
#pragma unroll
      for (int m = 0; m < MV; ++m) {
        const int cl = cl0[m] + tapofs;
        const char* p = smem + cl * 64 + (((2 * ks + kg) ^ ((cl >> 2) & 3)) << 4);
#pragma unroll
        for (int s = 0; s < NS; ++s) a[m][s] = *(const opnd*)(p + s * PLANE);
      }
    };
    auto mma = [&](const opnd (&a)[2][NS], const opnd (&b)[NT][NS]) __attribute__((always_inline)) {
      // products outermost (consecutive MFMAs go to different accumulators: an accumulator is touched every 2 NT instructions)
      auto sweep = [&](int sa, int sb) __attribute__((always_inline)) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int m = 0; m < MV; ++m) {
            if constexpr (NS == 3) acc[nt][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[nt][sb], a[m][sa], acc[nt][m], 0, 0, 0);
            else acc[nt][m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(b[nt][sb], a[m][sa], acc[nt][m], 0, 0, 0);
          }
      };
      // feature part x filter part, the small products of a k-step before its large one: m m, h l, l h (2^-16), h m, m h (2^-8), h h
      // (binary16 parts: h m, m h (2^-11), h h)
      if constexpr (NS == 3) { sweep(1, 1); sweep(0, 2); sweep(2, 0); }
      sweep(0, 1); sweep(1, 0); sweep(0, 0);
    };
    int ti = 0, tj = 0;
    const int ntap = kh * kw;
    // (binary16 parts: a k-step is 30 MFMAs = 960 cycles, and SQ_WAIT_INST_ANY reads 32 % of the wavefronts' cycles.  The filters TWO k-steps
    //  ahead — three register sets in rotation, a body of three taps — measured the same pdf time, 0.141 vs 0.139-0.141 ms per frame, at 430
    //  registers: no distance-transform wavefront beside it, 2 150 vs 2 225-2 277 frames/s; r05 session 15.  Not latency: the operand traffic.)
    opnd a0[2][NS], a1[2][NS], b0[NT][NS], b1[NT][NS];
    load_b(b0, 0);
    load_a(a0, 0, 0);
#pragma unroll 1
    for (int tap = 0; tap < ntap; ++tap) {
      // operands in explicit ping-pong, the schedule pinned: the next k-step's 15 filter loads + 6 LDS reads are ISSUED before this
      // k-step's 60 MFMAs (1 920 cycles) and waited for after them.  Left alone, hipcc's scheduler sinks every load to just in front
      // of its first use to save registers (80 VGPRs) — an L2 round trip in front of every other MFMA, with one wavefront per SIMD
      const int tapofs = ti * TW + tj;
      auto deal = [&]() {   // PIN == 2: one load per three MFMAs, then one LDS read per two (the MFMA pipe never waits for an issue burst)
        if constexpr (PIN == 2) {
#pragma unroll
          for (int i = 0; i < NS * NT; ++i) { __builtin_amdgcn_sched_group_barrier(0x8, NS == 3 ? (MV == 2 ? 3 : 1) : MV, 0); __builtin_amdgcn_sched_group_barrier(0x20, 1, 0); }
#pragma unroll
          for (int i = 0; i < NS * MV; ++i) { __builtin_amdgcn_sched_group_barrier(0x8, 2, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); }
        }
      };
      if (PIN) __builtin_amdgcn_sched_barrier(0);
      load_b(b1, 2 * tap + 1);
      load_a(a1, tapofs, 1);
      if (PIN == 1) __builtin_amdgcn_sched_barrier(0);
      mma(a0, b0);
      deal();
      if (PIN) __builtin_amdgcn_sched_barrier(0);
      if (++tj == kw) { tj = 0; ++ti; }
      const int nextofs = tap + 1 < ntap ? ti * TW + tj : tapofs;   // (past the last tap: this tap again, never used)
      load_b(b0, 2 * tap + 2);
      load_a(a0, nextofs, 0);
      if (PIN == 1) __builtin_amdgcn_sched_barrier(0);
      mma(a1, b1);
      deal();
      if (PIN) __builtin_amdgcn_sched_barrier(0);
    }
  };
  if (mvalid == 2) k_loop(std::integral_constant<int, 2>());
  else if (mvalid == 1) k_loop(std::integral_constant<int, 1>());
  if (mvalid == 0) return;

  // D[i = filter 32 nt + (r & 3) + 8 (r >> 2) + 4 kg][j = cell pos of M-tile m]
  float* Rl = resp + lv.cell_off * nf;
  const size_t HW = (size_t)H * W;
  int nfw = nf;                                          // planes this launch writes
  if constexpr (MIX) { Rl += (size_t)(t.pad & 0xFFFF) * HW; nfw = t.pad >> 16; }
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    if (m < mvalid && cval[m]) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        float* pl = Rl + (size_t)(32 * (ntb + nt) + 4 * kg) * HW + cofs[m];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int fo = (r & 3) + 8 * (r >> 2);
          if (32 * (ntb + nt) + 4 * kg + fo < nfw) pl[(size_t)fo * HW] = NS == 3 ? acc[nt][m][r] : acc[nt][m][r] * oscale[32 * (ntb + nt) + 4 * kg + fo];   // (a power of two: exact)
        }
      }
    }
  }
}

// MIX: a size group of a mixed bank (nf: the group's filters, nf_stride: the planes of a level block; tiles: the group's list)
template <int NT, int NW, int PIN, int NS = 3, bool MIX = false>
static void launch_conv_split_t(const ConvTile* tiles, int ntiles, const LevelDev* levels, const uint16_t* feat_split, const uint16_t* wS,
                                float* resp, int nf, int ntl_bank, int ntile0, int ngroups, int kh, int kw, hipStream_t s, const float* oscale = nullptr,
                                int nf_stride = 0) {
  constexpr int ROWS = 4 * NW, NHALVES = 16 / ROWS;
  const size_t lds = (size_t)(16 + kw - 1) * (ROWS + kh - 1) * 64 * NS;
  static LdsOptIn optin;
  optin.ensure((const void*)k_conv_split32<NT, NW, PIN, NS, MIX>, lds);
  const int grid = (ntiles + 7) / 8 * 8 * NHALVES * ngroups;
  hipLaunchKernelGGL((k_conv_split32<NT, NW, PIN, NS, MIX>), dim3(grid), dim3(64 * NW), lds, s, tiles, levels, feat_split, wS, resp, MIX ? nf_stride : nf,
                     ntl_bank, ntile0, ngroups, ntiles, kh, kw, oscale);
}
// groups of G = five n-tiles (160 filters: the person bank's 156 in one pass), then the remainder with its own instantiation
// (G = 4 / 3: tuning variants — fewer accumulators per wavefront, two wavefronts per SIMD, every tile staged once per group)
// (banks of more than 160 filters: balanced groups — 208 filters as 4 + 3 n-tiles instead of 5 + 2 — measured the same, 0.300 vs 0.302 ms per frame: what a
//  second group costs is staging every tile again and a second launch tail, not the smaller register block; session 11)
template <int NW, int PIN, int NS, bool MIX = false>
static void launch_conv_split_groups(const ConvTile* tiles, int ntiles, const LevelDev* levels, const uint16_t* feat_split, const uint16_t* wS,
                                     float* resp, int nf, int kh, int kw, const float* oscale, hipStream_t s, int nf_stride = 0, int G = 5) {
  const int ntl = conv_split_ntiles(nf), full = ntl / G, rest = ntl - G * full;
  auto go = [&](int nt, int ntile0, int ngroups) {
    switch (nt) {
      case 1: launch_conv_split_t<1, NW, PIN, NS, MIX>(tiles, ntiles, levels, feat_split, wS, resp, nf, ntl, ntile0, ngroups, kh, kw, s, oscale, nf_stride); break;
      case 2: launch_conv_split_t<2, NW, PIN, NS, MIX>(tiles, ntiles, levels, feat_split, wS, resp, nf, ntl, ntile0, ngroups, kh, kw, s, oscale, nf_stride); break;
      case 3: launch_conv_split_t<3, NW, PIN, NS, MIX>(tiles, ntiles, levels, feat_split, wS, resp, nf, ntl, ntile0, ngroups, kh, kw, s, oscale, nf_stride); break;
      case 4: launch_conv_split_t<4, NW, PIN, NS, MIX>(tiles, ntiles, levels, feat_split, wS, resp, nf, ntl, ntile0, ngroups, kh, kw, s, oscale, nf_stride); break;
      case 5: launch_conv_split_t<5, NW, PIN, NS, MIX>(tiles, ntiles, levels, feat_split, wS, resp, nf, ntl, ntile0, ngroups, kh, kw, s, oscale, nf_stride); break;
      default: break;
    }
  };
  if (full) go(G, 0, full);
  if (rest) go(rest, G * full, 1);
}
