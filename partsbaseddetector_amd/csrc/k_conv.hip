// k_conv.hip — SpatialConvolutionEngine::pdf as one batched filter-bank
// correlation over all pyramid levels (reference
// src/SpatialConvolutionEngine.cpp:70-124, Filter2D src/filter.cpp:3879-3924).
//
//   resp[l][n](y,x) = sum_c sum_{i,j} w_n[i][j][c] * F_l(y+i-kh/2, x+j-kw/2, c)
//   "same" size, correlation (no flip), constant border: 0 for c<flen-1,
//   1 for the last (truncation) channel (:147-155).
//
// The kernels of this unit are the ones a product handle launches:
//  * k_conv_exact / k_conv_exact_f64 / k_conv_exact_generic — VALU, reproduce the reference's summation order bit for
//    bit: per channel a tap-ordered (row-major) chain of separately rounded mul + add starting from 0
//    (filter.cpp:3914-3918), then the channel partials are added in channel order (`pdf += pdfc`, :92).  Compiled with
//    -ffp-contract=off so hipcc cannot fuse the mul/add.
//  * k_conv_mfma16 (k_conv_mfma16.hpp) — 16x16x4 MFMA implicit GEMM (M = cells, N = filters, K = kh*kw*flen = 800): a
//    k-ordered fma chain, |delta| ~1e-6 vs the reference order; the fast path when nfilters*flen is a real dense contraction.
//    Its default configuration per scalar type, as the 5x5, run-time-size and mixed-bank forms; every other configuration
//    that was measured lives in k_conv_variants.hip (tune and probe libraries only).
// All stage a (T+kh-1)x(T+kw-1)-cell feature tile with halo in LDS once per workgroup and channel group (stage_tile;
// float k_conv_exact: stage_feature_tile below — border values materialised there) and write plane-major outputs.
#include <algorithm>
#include <vector>
#include <cstring>
#include "pbd_internal.hpp"
#include <type_traits>
#include "k_conv_mfma16.hpp"

#ifdef PBD_PROBES
bool conv_variants_debug_read(unsigned long long* out);   // k_conv_variants.hip: true once a variant kernel has been the bank
void conv_debug_read(unsigned long long* out) {
  if (!conv_variants_debug_read(out)) hipMemcpyFromSymbol(out, HIP_SYMBOL(pbd_conv_dbg), sizeof(unsigned long long) * 8);
}
#else
void conv_debug_read(unsigned long long* out) { for (int i = 0; i < 8; ++i) out[i] = 0; }
#endif

#define CSTR 33      // LDS floats per cell (32 + 1 pad: conflict-free across x)
#define NFG 8        // filters held in registers per pass (exact kernel)

// k_conv_exact's own staging of the whole 32-channel tile, the one caller stage_tile does not serve: here ALL NB batches of loads are
// in flight before the first wait.  Through stage_tile<float, 32, CSTR, NB> hipcc sinks the half-filled last batch into its `i < N`
// branch (12 of 13 in flight, one more exposed round trip for half of the workgroup); this form compiles to the instructions the
// kernel has always had.  Same rule as stage_tile: clamped addresses, border value selected after the load (0, or 1 for the last channel).
template <int KH, int KW>
__device__ __forceinline__ void stage_feature_tile(float* __restrict__ ft, const float* __restrict__ F, int y0, int x0,
                                                   int H, int W, int tid) {
  constexpr int TW = CT + KW - 1, TH = CT + KH - 1, N = TH * TW * 8, NB = (N + 255) / 256;
  float4 r[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int i = min(tid + j * 256, N - 1);
    const int cell = i >> 3, q = i & 7;
    const int ty = cell / TW, tx = cell - ty * TW;
    const int y = min(max(y0 + ty - KH / 2, 0), H - 1), x = min(max(x0 + tx - KW / 2, 0), W - 1);
    r[j] = *(const float4*)(F + ((size_t)y * W + x) * PBD_FLEN + q * 4);
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int i = tid + j * 256;
    if (i < N) {
      const int cell = i >> 3, q = i & 7;
      const int ty = cell / TW, tx = cell - ty * TW;
      const int y = y0 + ty - KH / 2, x = x0 + tx - KW / 2;
      float4 v = r[j];
      if (!(y >= 0 && y < H && x >= 0 && x < W)) v = make_float4(0.f, 0.f, 0.f, q == 7 ? 1.f : 0.f);
      float* d = ft + cell * CSTR + q * 4;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
  }
}

// SpatialConvolutionEngine(CV_32F), compile-time filter size (the double instantiation, CV_64F, is k_conv_exact_f64 below)
template <int KH, int KW>
__global__ __launch_bounds__(256) void k_conv_exact(const ConvTile* __restrict__ tiles,
                                                    const LevelDev* __restrict__ levels,
                                                    const float* __restrict__ feat, const float* __restrict__ wT,
                                                    float* __restrict__ resp, int nf, int nfpad, int groups_per_wg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef float T;
  T* ft = (T*)smem;  // [(CT+KH-1)][(CT+KW-1)][CSTR]
  const ConvTile t = tiles[blockIdx.x];
  const LevelDev lv = levels[t.level];
  const int H = lv.ch, W = lv.cw;
  const int TW = CT + KW - 1;
  const int tid = threadIdx.x;
  const T* F = feat + lv.cell_off * PBD_FLEN;
  // stage the tile: 8 lanes x float4 per cell -> coalesced 128 B per cell, every batch of loads in flight before the first wait
  stage_feature_tile<KH, KW>(ft, F, t.y0, t.x0, H, W, tid);
  __syncthreads();
  const int ly = tid >> 4, lx = tid & 15;
  const int oy = t.y0 + ly, ox = t.x0 + lx;
  const bool valid = (oy < H && ox < W);
  const T* fbase = ft + (ly * TW + lx) * CSTR;
  T* R = resp + lv.cell_off * nf;  // level base, plane n at + n*H*W
  const int g0 = blockIdx.y * groups_per_wg;
  for (int g = g0; g < g0 + groups_per_wg; ++g) {
    const int n0 = g * NFG;
    if (n0 >= nf) break;
    T tot[NFG];
#pragma unroll
    for (int n = 0; n < NFG; ++n) tot[n] = (T)0;
    for (int c = 0; c < PBD_FLEN; ++c) {
      T acc[NFG];
#pragma unroll
      for (int n = 0; n < NFG; ++n) acc[n] = (T)0;
#pragma unroll
      for (int i = 0; i < KH; ++i) {
#pragma unroll
        for (int j = 0; j < KW; ++j) {
          const T f = fbase[(i * TW + j) * CSTR + c];
          const T* w = wT + ((size_t)(i * KW + j) * PBD_FLEN + c) * nfpad + n0;  // wave-uniform
#pragma unroll
          for (int n = 0; n < NFG; ++n) acc[n] += w[n] * f;
        }
      }
#pragma unroll
      for (int n = 0; n < NFG; ++n) tot[n] += acc[n];
    }
    if (valid) {
#pragma unroll
      for (int n = 0; n < NFG; ++n)
        if (n0 + n < nf) R[(size_t)(n0 + n) * H * W + (size_t)oy * W + ox] = tot[n];
    }
  }
}

// double instantiation of the exact filter bank.  A 20x20-cell tile of 32 doubles is 105 KB of LDS (one
// workgroup per CU), so the tile is staged in two 16-channel halves (53 KB: three workgroups per CU).  The
// reference's order survives: channels are still visited 0..31, each channel's tap chain starts from
// zero and the channel partials are added to the running total in channel order (`pdf += pdfc`, :92);
// the totals of the workgroup's GPW filter groups simply stay in registers across the two halves.
#define CHALF 16     // channels staged per pass
#define CSTRH 17     // LDS doubles per cell and pass (16 + 1 pad)
template <int KH, int KW, int GPW>
__global__ __launch_bounds__(256) void k_conv_exact_f64(const ConvTile* __restrict__ tiles,
                                                        const LevelDev* __restrict__ levels,
                                                        const double* __restrict__ feat, const double* __restrict__ wT,
                                                        double* __restrict__ resp, int nf, int nfpad) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* ft = (double*)smem;  // [(CT+KH-1)][(CT+KW-1)][CSTRH]
  const ConvTile t = tiles[blockIdx.x];
  const LevelDev lv = levels[t.level];
  const int H = lv.ch, W = lv.cw;
  constexpr int TW = CT + KW - 1;
  const int tid = threadIdx.x;
  const double* F = feat + lv.cell_off * PBD_FLEN;
  const int ly = tid >> 4, lx = tid & 15;
  const int oy = t.y0 + ly, ox = t.x0 + lx;
  const bool valid = (oy < H && ox < W);
  const double* fbase = ft + (ly * TW + lx) * CSTRH;
  double* R = resp + lv.cell_off * nf;
  const int g0 = blockIdx.y * GPW;
  double tot[GPW][NFG];
#pragma unroll
  for (int g = 0; g < GPW; ++g)
#pragma unroll
    for (int n = 0; n < NFG; ++n) tot[g][n] = 0.0;
  for (int half = 0; half < PBD_FLEN / CHALF; ++half) {
    if (half) __syncthreads();   // everyone is done with the previous half
    // stage 16 channels of every cell: 8 lanes x double2 per cell
    stage_tile<double, CHALF, CSTRH, 7>(ft, F, t.y0, t.x0, H, W, KH, KW, half * CHALF, half == PBD_FLEN / CHALF - 1, tid);
    __syncthreads();
#pragma unroll
    for (int g = 0; g < GPW; ++g) {
      const int n0 = (g0 + g) * NFG;
      if (n0 >= nf) break;
      for (int cc = 0; cc < CHALF; ++cc) {
        const int c = half * CHALF + cc;
        double acc[NFG];
#pragma unroll
        for (int n = 0; n < NFG; ++n) acc[n] = 0.0;
#pragma unroll
        for (int i = 0; i < KH; ++i) {
#pragma unroll
          for (int j = 0; j < KW; ++j) {
            const double f = fbase[(i * TW + j) * CSTRH + cc];
            const double* w = wT + ((size_t)(i * KW + j) * PBD_FLEN + c) * nfpad + n0;  // wave-uniform
#pragma unroll
            for (int n = 0; n < NFG; ++n) acc[n] += w[n] * f;
          }
        }
#pragma unroll
        for (int n = 0; n < NFG; ++n) tot[g][n] += acc[n];
      }
    }
  }
  if (valid) {
#pragma unroll
    for (int g = 0; g < GPW; ++g) {
      const int n0 = (g0 + g) * NFG;
#pragma unroll
      for (int n = 0; n < NFG; ++n)
        if (n0 + n < nf) R[(size_t)(n0 + n) * H * W + (size_t)oy * W + ox] = tot[g][n];
    }
  }
}

// generic-size fallback (runtime kh, kw <= 9).  MIX: a size group of a mixed bank (pbd_create_sized) — the tile's pad = n0 | (nf_g << 16):
// planes n0 .. n0 + nf_g - 1 of a level block of `nf` planes, wT the group's own (ConvTile, pbd_internal.hpp)
template <typename T, bool MIX = false>
__global__ __launch_bounds__(256) void k_conv_exact_generic(const ConvTile* __restrict__ tiles,
                                                            const LevelDev* __restrict__ levels,
                                                            const T* __restrict__ feat,
                                                            const T* __restrict__ wT, T* __restrict__ resp,
                                                            int nf, int nfpad, int KH, int KW) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* ft = (T*)smem;
  const ConvTile t = tiles[blockIdx.x];
  const LevelDev lv = levels[t.level];
  const int H = lv.ch, W = lv.cw;
  const int TW = CT + KW - 1, TH = CT + KH - 1;
  const int tid = threadIdx.x;
  const T* F = feat + lv.cell_off * PBD_FLEN;
  for (int i = tid; i < TH * TW * PBD_FLEN; i += 256) {
    const int cell = i >> 5, c = i & 31;
    const int ty = cell / TW, tx = cell - ty * TW;
    const int y = t.y0 + ty - KH / 2, x = t.x0 + tx - KW / 2;
    const bool inside = (y >= 0 && y < H && x >= 0 && x < W);
    const T v = F[((size_t)min(max(y, 0), H - 1) * W + min(max(x, 0), W - 1)) * PBD_FLEN + c];
    ft[cell * CSTR + c] = inside ? v : (T)(c == PBD_FLEN - 1 ? 1 : 0);
  }
  __syncthreads();
  const int ly = tid >> 4, lx = tid & 15;
  const int oy = t.y0 + ly, ox = t.x0 + lx;
  const bool valid = (oy < H && ox < W);
  const T* fbase = ft + (ly * TW + lx) * CSTR;
  T* R = resp + lv.cell_off * nf;
  int nfw = nf;   // planes this launch writes
  if constexpr (MIX) { R += (size_t)(t.pad & 0xFFFF) * H * W; nfw = t.pad >> 16; }
  for (int n = blockIdx.y; n < nfw; n += gridDim.y) {
    T tot = (T)0;
    for (int c = 0; c < PBD_FLEN; ++c) {
      T acc = (T)0;
      for (int i = 0; i < KH; ++i)
        for (int j = 0; j < KW; ++j)
          acc += wT[((size_t)(i * KW + j) * PBD_FLEN + c) * nfpad + n] * fbase[(i * TW + j) * CSTR + c];
      tot += acc;
    }
    if (valid) R[(size_t)n * H * W + (size_t)oy * W + ox] = tot;
  }
}

template <typename T>
static void launch_conv_exact_t(const ConvTile* tiles, int ntiles, const LevelDev* levels, const T* feat,
                                const T* wT, T* resp, int nf, int nfpad, int kh, int kw, hipStream_t s, int nf_stride) {
  const size_t lds = sizeof(T) * (CT + kh - 1) * (CT + kw - 1) * CSTR;
  if (nf_stride > 0) {   // a size group of a mixed bank: the run-time-size kernel for every size (the reference's summation order whatever the size)
    static LdsOptIn optinm;
    optinm.ensure((const void*)k_conv_exact_generic<T, true>, lds);
    dim3 grid(ntiles, nf < 16 ? nf : 16);
    hipLaunchKernelGGL((k_conv_exact_generic<T, true>), grid, dim3(256), lds, s, tiles, levels, feat, wT, resp, nf_stride, nfpad, kh, kw);
    return;
  }
  if (kh == 5 && kw == 5) {
    const int groups = (nf + NFG - 1) / NFG;
    constexpr int GPW = 4;
    dim3 grid(ntiles, (groups + GPW - 1) / GPW);
    static LdsOptIn optin;   // one per instantiation
    if constexpr (sizeof(T) == 8) {
      const size_t ldsh = sizeof(double) * (CT + 4) * (CT + 4) * CSTRH;
      optin.ensure((const void*)k_conv_exact_f64<5, 5, GPW>, ldsh);
      hipLaunchKernelGGL((k_conv_exact_f64<5, 5, GPW>), grid, dim3(256), ldsh, s, tiles, levels, feat, wT, resp, nf, nfpad);
    } else {
      optin.ensure((const void*)k_conv_exact<5, 5>, lds);
      hipLaunchKernelGGL((k_conv_exact<5, 5>), grid, dim3(256), lds, s, tiles, levels, feat, wT, resp, nf, nfpad, GPW);
    }
  } else {
    static LdsOptIn opting;
    opting.ensure((const void*)k_conv_exact_generic<T>, lds);
    dim3 grid(ntiles, nf < 16 ? nf : 16);
    hipLaunchKernelGGL(k_conv_exact_generic<T>, grid, dim3(256), lds, s, tiles, levels, feat, wT, resp, nf, nfpad, kh, kw);
  }
}

// ts = sizeof(T): 4 -> SpatialConvolutionEngine(CV_32F), 8 -> CV_64F
void launch_conv_exact(const ConvTile* tiles, int ntiles, const LevelDev* levels, const void* feat, const void* wT,
                       void* resp, int ts, int nf, int nfpad, int kh, int kw, hipStream_t s, int nf_stride) {
  if (ntiles <= 0) return;
  if (ts == 8) launch_conv_exact_t<double>(tiles, ntiles, levels, (const double*)feat, (const double*)wT, (double*)resp, nf, nfpad, kh, kw, s, nf_stride);
  else launch_conv_exact_t<float>(tiles, ntiles, levels, (const float*)feat, (const float*)wT, (float*)resp, nf, nfpad, kh, kw, s, nf_stride);
}

// The 16x16x4 MFMA bank (k_conv_mfma16.hpp).  double: four 8-channel passes (27 KB of LDS per workgroup; measured 7 % faster
// than two 16-channel halves, 54 KB), 16-byte B loads from the [tap][group][k][n][u] copy of the filters (w4u)
void launch_conv_mfma_f64(const ConvTile* tiles, int ntiles, const LevelDev* levels, const double* feat,
                          const double* w4u, double* resp, int nf, int nfpad, int kh, int kw, hipStream_t s, int nf_stride) {
  if (ntiles <= 0) return;
  if (nf_stride > 0)   // a size group of a mixed bank: the run-time-size configuration for every size
    launch_conv_mfma16_t<double, 4, 2, 1, true, 0, 0, true>(tiles, ntiles, levels, feat, w4u, resp, nf, nfpad, s, kh, kw, nf_stride);
  else if (kh != 5 || kw != 5)   // any other filter size: the same kernel with a run-time tap loop
    launch_conv_mfma16_t<double, 4, 2, 1, true, 0, 0>(tiles, ntiles, levels, feat, w4u, resp, nf, nfpad, s, kh, kw);
  else
    launch_conv_mfma16_t<double, 4, 2, 1, true>(tiles, ntiles, levels, feat, w4u, resp, nf, nfpad, s);
}

// float: the tile staged in two channel halves (27 KB of LDS per workgroup, so DT blocks of other frames co-reside on the CU),
// 3+ waves per SIMD, TWO 16-filter n-tiles per workgroup, 16-byte B loads from the [tap][half][k][n][u] copy of the filters
// (w4u): 0.339 ms sequential and the best throughput with other frames' kernels co-resident.  What it was measured against:
// k_conv_variants.hip.
void launch_conv_mfma16_f32(const ConvTile* tiles, int ntiles, const LevelDev* levels, const float* feat,
                            const float* w4u, float* resp, int nf, int nfpad, int kh, int kw, hipStream_t s, int nf_stride) {
  if (ntiles <= 0) return;
  if (nf_stride > 0)   // a size group of a mixed bank: the run-time-size configuration for every size
    launch_conv_mfma16_t<float, 2, 3, 2, true, 0, 0, true>(tiles, ntiles, levels, feat, w4u, resp, nf, nfpad, s, kh, kw, nf_stride);
  else if (kh != 5 || kw != 5)   // any other filter size (3x3 .. 9x9): the same kernel with a run-time tap loop
    launch_conv_mfma16_t<float, 2, 3, 2, true, 0, 0>(tiles, ntiles, levels, feat, w4u, resp, nf, nfpad, s, kh, kw);
  else
    launch_conv_mfma16_t<float, 2, 3, 2, true>(tiles, ntiles, levels, feat, w4u, resp, nf, nfpad, s);
}
