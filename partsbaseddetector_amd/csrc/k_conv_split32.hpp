// k_conv_split32.hpp — the split-product bank's kernel template on v_mfma_f32_16x16x32 (16-cell M-tiles, 16-filter tiles) and its
// launchers: what k_conv_split.hip's product handles launch.  The template on 32x32x16 that it replaced, and that every tuning variant
// was measured on, is k_conv_split32_m32.hpp (k_conv_split_variants.hip: tune and probe libraries only); name, signature, launchers,
// grid, staging, LDS image and filter layout are the same in both.
// No include guard on purpose: textual inclusion, once per unit, after pbd_internal.hpp, <type_traits> and conv_split_ntiles().
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// NT: 32-filter n-tiles per workgroup (1..5); NW: wavefronts per workgroup (2: a 16 x 8 half of a ConvTile, 4: the whole 16 x 16 tile)
// PIN: kept from the 32x32x16 template, where it chose the K loop's schedule; here the loop has ONE schedule (loads pinned between the MFMA
// statements, see the loop) and PIN only sets the occupancy bound: != 0 one wavefront per SIMD (the product's 2), 0 up to two
// NS: parts per operand — 3: bfloat16 parts, six products (PBD_CONV_SPLIT); 2: scaled binary16 parts, three products (PBD_CONV_SPLIT_F16, below)
// MIX: one size group of a mixed bank (pbd_create_sized): the tile's pad = n0 | (nf_g << 16) — planes n0 .. n0 + nf_g - 1 of a level block
// of `nf` planes; filt / oscale are the group's own (ConvTile, pbd_internal.hpp)
template <int NT, int NW, int PIN, int NS = 3, bool MIX = false>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(1, PIN ? 1 : 2))) void k_conv_split32(const ConvTile* __restrict__ tiles, const LevelDev* __restrict__ levels,
                                                             const uint16_t* __restrict__ feat, const uint16_t* __restrict__ filt,
                                                             float* __restrict__ resp, int nf, int ntl_bank, int ntile0, int ngroups,
                                                             int ntiles_total, int kh, int kw, const float* __restrict__ oscale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
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
  // lane -> (column of a 16-cell M-tile, channel group kb = 8 channels).  One MFMA takes a tap's 32 channels: the lane holds row / column
  // lane & 15 and the channels 8 kb .. 8 kb + 7 of both operands.  ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27},
  // {4-11, 16-19, 28-31} (+32): every group holds columns 0-3, 12-15 of one channel group and columns 4-11 of its neighbour kb ^ 1, whose
  // XOR swizzle lands on the 16-byte slots of the cells 4 away.  Columns are therefore dealt to cell positions by position & 3: columns
  // 4-11 take the positions = 0, 1 (mod 4), the others 2, 3 (mod 4) — in 16 consecutive cells the two halves of a group then differ in
  // (cell & 3), the upper two bits of the slot, whatever the tap's offset: conflict-free on every row of a full-width unit
  const int col = lane & 15, kb = lane >> 4;
  const bool inner = col >= 4 && col < 12;
  const int kk = inner ? col - 4 : col < 4 ? col : col - 8;     // 0..7 inside either set of eight columns
  const int pos = ((kk >> 1) << 2) + (inner ? 0 : 2) + (kk & 1);
  // packed M-tiles: valid cell number 16 j + pos of the vh x vw valid region, j = wave + NW m (round robin: a ragged unit's
  // M-tiles spread over the wavefronts); positions past the last cell repeat it (never stored)
  const int vw = min(16, W - tx0), vh = min(ROWS, H - ty0), ncell = vw * vh;
  const int nmt = (ncell + 15) >> 4;
  const int mvalid = __builtin_amdgcn_readfirstlane(max(0, min(4, (nmt - wave + NW - 1) / NW)));
  const unsigned vw_magic = 65535u / (unsigned)vw + 1u;   // idx / vw for idx < 256 (k_conv_mfma16)
  int cl0[4], cofs[4];
  bool cval[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int idx = 16 * (wave + NW * m) + pos;
    cval[m] = idx < ncell;
    const int ic = min(idx, ncell - 1);
    const int cy = (int)(((unsigned)ic * vw_magic) >> 16), cx = ic - cy * vw;
    cl0[m] = cy * TW + cx;
    cofs[m] = (ty0 + cy) * W + tx0 + cx;
  }
  const int ntb = ntile0 + ngroup * NT;                  // first n-tile of this workgroup
  // filters [tap][k-step][split][n-tile][k-group][32][8]: channel group kb is k-step kb >> 1, k-group kb & 1; the 16-filter half h of an
  // n-tile is + 128 h elements
  const size_t bs_split = (size_t)ntl_bank * 512, bs_kstep = NS * bs_split, bs_tap = 2 * bs_kstep;
  const uint16_t* bl = filt + (size_t)ntb * 512 + (size_t)(kb >> 1) * bs_kstep + (kb & 1) * 256 + col * 8;
#ifdef PBD_BANK_PRIO   // experiment builds only: the K loop's wavefronts at a raised issue priority against the other batches' kernels on the SIMD
  __builtin_amdgcn_s_setprio(PBD_BANK_PRIO);
#endif

  // D (16 filters x 16 cells) += filters (A: row lane & 15, channels 8 kb ..) x cells (B: column lane & 15, channels 8 kb ..), K = 32.
  // The products of a tap, feature part x filter part, the small ones before the large one: m m, h l, l h (2^-16), h m, m h (2^-8), h h
  // (binary16 parts: h m, m h (2^-11), h h), adjacent on their accumulator.  Three products to a statement (hipcc puts a wait state
  // between two statements that share an accumulator, none inside one): the small three (bfloat16 parts only), then the large three;
  // fb / fa = the filter's / the cell's parts
  constexpr int NTRI = NS == 3 ? 2 : 1;
  auto mfma3 = [](int tri, f32x4& d, const u32x4 (&fb)[NS], const u32x4 (&fa)[NS]) __attribute__((always_inline)) {
    if constexpr (NS == 3) {
      if (tri == 0)
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0\n\tv_mfma_f32_16x16x32_bf16 %0, %3, %4, %0\n\tv_mfma_f32_16x16x32_bf16 %0, %5, %6, %0"
                     : "+a"(d) : "v"(fb[1]), "v"(fa[1]), "v"(fb[2]), "v"(fa[0]), "v"(fb[0]), "v"(fa[2]));
      else
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0\n\tv_mfma_f32_16x16x32_bf16 %0, %3, %4, %0\n\tv_mfma_f32_16x16x32_bf16 %0, %3, %2, %0"
                     : "+a"(d) : "v"(fb[1]), "v"(fa[0]), "v"(fb[0]), "v"(fa[1]));
    } else {
      asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0\n\tv_mfma_f32_16x16x32_f16 %0, %3, %4, %0\n\tv_mfma_f32_16x16x32_f16 %0, %3, %2, %0"
                   : "+a"(d) : "v"(fb[1]), "v"(fa[0]), "v"(fb[0]), "v"(fa[1]));
    }
  };

  auto k_loop = [&](auto mv_tag) __attribute__((always_inline)) {
    // A step = (tap, n-tile): the 2 x MV accumulators of the n-tile's two 16-filter halves, 3 NTRI adjacent MFMAs each (a dependent chain
    // runs at the rate of independent ones on this shape), half 0 of every M-tile before half 1.  The filters sit in a ring of two n-tile
    // slots (2 halves x NS parts x 4 registers): step t's MFMAs read one slot while the 2 NS loads of step t + 1 fill the other, LPT loads
    // behind each of the step's first statements — a step (768 cycles at MV = 4) ahead of their use.  The cells are single-buffered:
    // in a tap's last step the parts of M-tile m are read again for the next tap right after the last MFMA that takes them, 4 accumulators
    // (384 cycles at MV = 4) ahead.  Operands reach the MFMAs only from loads (hipcc waits for its own loads in front of an asm statement
    // that takes them, but pads no VALU -> MFMA hazard there), and sched_barrier(0) fences pin every load between two statements.
    constexpr int MV = decltype(mv_tag)::value, NU = 2 * MV * NTRI, NLD = 2 * NS, LPT = (NLD + NU - 2) / (NU - 1);
    static_assert(NU >= 2 && LPT * (NU - 1) >= NLD, "a step's statements carry the next step's filter loads");
    u32x4 a[4][NS], b[2][2][NS];                           // a[M-tile][part]; b[slot][half][part]
    // D[filter][cell]: 2 NT 16-filter tiles x MV M-tiles of 4 registers, in the accumulator file (the MFMAs are inline assembly with the
    // accumulator tied, "+a": with the builtin hipcc rotates the 40 accumulators through VGPRs at the loop's back edge, 140-250 moves a body).
    // Zeroed, multiplied and stored inside ONE instantiation: accumulators that meet behind the switch are copied to VGPRs there, all at once
    f32x4 acc[2 * NT][MV];
#pragma unroll
    for (int ft = 0; ft < 2 * NT; ++ft)
#pragma unroll
      for (int m = 0; m < MV; ++m) acc[ft][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    // hipcc pads no hazard of an asm statement: wait states between a write of the accumulators outside the K loop (the zeros above, the
    // loop's last MFMAs) and whatever reads them next: 8 states in a statement of its own per accumulator, in the order the loop writes
    // them (the last one written has every other statement in front of its own).  Once per workgroup on either side of the loop.
    auto pad_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int ft = 0; ft < 2 * NT; ++ft)
#pragma unroll
        for (int m = 0; m < MV; ++m) asm volatile("s_nop 7" : "+a"(acc[ft][m]));
    };
    auto ld_a = [&](int m, int tapofs) __attribute__((always_inline)) {     // tapofs = ti * TW + tj
      const int cl = cl0[m] + tapofs;
      const char* p = smem + cl * 64 + ((kb ^ ((cl >> 2) & 3)) << 4);
#pragma unroll
      for (int s = 0; s < NS; ++s) a[m][s] = *(const u32x4*)(p + s * PLANE);
    };
    // one tap with the ring at parity P: pt / pn = this / the next tap's filters, nextofs = the next tap's offset
    auto tap_body = [&](auto p_tag, const uint16_t* pt, const uint16_t* pn, int nextofs) __attribute__((always_inline)) {
      constexpr int P = decltype(p_tag)::value;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int slot = (P + nt) & 1;
        const bool last = nt == NT - 1;
        const uint16_t* pl = last ? pn : pt + (nt + 1) * 512;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int m = 0; m < MV; ++m) {
#pragma unroll
            for (int q = 0; q < NTRI; ++q) {
              const int u = (h * MV + m) * NTRI + q;
              mfma3(q + 2 - NTRI, acc[2 * nt + h][m], b[slot][h], a[m]);
              if (u * LPT < NLD) {
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = u * LPT; k < (u + 1) * LPT && k < NLD; ++k)
                  b[slot ^ 1][k / NS][k % NS] = *(const u32x4*)(pl + (k % NS) * bs_split + (k / NS) * 128);
                __builtin_amdgcn_sched_barrier(0);
              }
            }
            if (last && h == 1) {
              __builtin_amdgcn_sched_barrier(0);
              ld_a(m, nextofs);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
      }
    };
    const int ntap = kh * kw;
#pragma unroll
    for (int k = 0; k < NLD; ++k) b[0][k / NS][k % NS] = *(const u32x4*)(bl + (k % NS) * bs_split + (k / NS) * 128);
#pragma unroll
    for (int m = 0; m < MV; ++m) ld_a(m, 0);
    pad_acc();
    int ti = 0, tj = 0;
    const uint16_t* pt = bl;
    // (past the last tap: this tap's filters and offset 0 once more, never used)
    auto one_tap = [&](auto p_tag, int tap) __attribute__((always_inline)) {
      if (++tj == kw) { tj = 0; ++ti; }
      const bool more = tap + 1 < ntap;
      const uint16_t* pn = more ? pt + bs_tap : pt;
      tap_body(p_tag, pt, pn, more ? ti * TW + tj : 0);
      pt = pn;
    };
#pragma unroll 1
    for (int tap = 0; tap < ntap; tap += 1 + (NT & 1)) {   // an odd number of n-tiles turns the ring once per tap: a body of two taps
      one_tap(std::integral_constant<int, 0>(), tap);
      if constexpr (NT & 1) {
        if (tap + 1 >= ntap) break;
        one_tap(std::integral_constant<int, 1>(), tap + 1);
      }
    }
    pad_acc();

    // D[i = filter 16 ft + 4 kb + r][j = column of M-tile m]
    float* Rl = resp + lv.cell_off * nf;
    const size_t HW = (size_t)H * W;
    int nfw = nf;                                          // planes this launch writes
    if constexpr (MIX) { Rl += (size_t)(t.pad & 0xFFFF) * HW; nfw = t.pad >> 16; }
#pragma unroll
    for (int m = 0; m < MV; ++m) {
      if (cval[m]) {
#pragma unroll
        for (int ft = 0; ft < 2 * NT; ++ft) {
          const int f0 = 32 * ntb + 16 * ft + 4 * kb;
          float* pl = Rl + (size_t)f0 * HW + cofs[m];
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (f0 + r < nfw) pl[(size_t)r * HW] = NS == 3 ? acc[ft][m][r] : acc[ft][m][r] * oscale[f0 + r];   // (a power of two: exact)
        }
      }
    }
  };
  switch (mvalid) {   // (a wavefront issues no MFMAs for an M-tile without a valid cell)
    case 4: k_loop(std::integral_constant<int, 4>()); break;
    case 3: k_loop(std::integral_constant<int, 3>()); break;
    case 2: k_loop(std::integral_constant<int, 2>()); break;
    case 1: k_loop(std::integral_constant<int, 1>()); break;
    default: return;
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
