// k_conv_split.hip — PBD_CONV_SPLIT: SpatialConvolutionEngine::pdf (reference src/SpatialConvolutionEngine.cpp:70-124,
// Filter2D src/filter.cpp:3879-3924) with the fp32 products carried by the bf16 matrix units through EXACT splits.
//
// An fp32 number is the sum of three bfloat16 (8 significant bits each): x = h + m + l, h = RN16(x), m = RN16(x - h),
// l = RN16(x - h - m), every subtraction exact.  A product of two bfloat16 is exact in an fp32 accumulator; the six partial
// products above 2^-24 relative (hh, hm, mh, hl, lh, mm) reproduce the fp32 product to fp32's own rounding
// (tests/tools_split_products_study.py: max error against fp64 3.1e-7 on the person bank, 9.1e-7 for the fp32 MFMA chain of
// k_conv_mfma16).  Why: fp32 MFMAs execute at the vector ALU's rate (157.3 TF is both peaks), so the bank and the distance
// transforms queue for one pipe; the bf16 MFMAs run on the matrix cores at 16x that rate.  The shape is v_mfma_f32_16x16x32_bf16:
// the bank runs at the chip's power limit on real operands, and the chip holds a higher clock on this shape than on 32x32x16 at the
// same cycles per product (the 32x32x16 template is k_conv_split32_m32.hpp, tuning builds only).
//
// Implicit GEMM D[filter][cell] = sum over (tap, channel, product) — filters are the MFMA's A operand (rows), cells its B
// operand (columns): an accumulator register then holds 16 cells of ONE response plane, and a store writes 64-byte row segments
// without an LDS transpose.  One MFMA takes a tap's 32 channels (K = 32).
//   * features: [cell][split][32 channels] bfloat16 in HBM (192 B per cell: k_feat_split, or k_hog's epilogue);
//   * filters:  [tap][k-step (16 channels)][split][32-filter n-tile][k-group (8 channels)][32 filters][8] bfloat16 (host, once per
//     model; L2-resident) — the layout of the 32x32x16 kernel, shared with k_weights.hip and the tuning variants: a lane loads the
//     16 bytes of (filter lane & 15 of a 16-filter half, channel group lane >> 4 = k-step, k-group), a wavefront four 256-byte segments;
//   * a workgroup = NW wavefronts = a 16 x 4 NW cell unit of a ConvTile (default NW = 4: the whole tile); every wavefront owns four
//     16-cell M-tiles x 2 NT (<= 10) 16-filter tiles = up to 160 accumulator registers (40 accumulators of 4, in the accumulator
//     file), ONE wavefront per SIMD (the register file is the occupancy bound): per tap 30 filter loads + 12 LDS reads feed 240
//     MFMAs of 16 cycles — the 64 x 160 register block of the 32x32x16 kernel and the same 3 840 cycles;
//   * the unit's halo tile sits in LDS as [split][cell][64 B], the four 16-byte channel groups of a cell XOR-swizzled with
//     bits 2-3 of the cell index.  A ds_read_b128 lane group ({0-3, 12-15, 20-27}, ...: MI355X_MICROARCH.md, LDS) holds eight
//     columns of one channel group and eight of its neighbour: the columns of an M-tile are dealt to its cells by (cell & 3), so
//     that the group's 16 reads fall on 16 different 16-byte bank slots on every row of a full-width unit (k_conv_split32.hpp);
//   * the valid cells of a ragged unit are packed into M-tiles (level edges issue no MFMAs for an M-tile without a valid cell).
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>
#include <cstring>
#include "pbd_internal.hpp"
#include "pbd_split.hpp"

int conv_split_ntiles(int nf);
#include "k_conv_split32.hpp"

// ---- features -> three exact bfloat16 parts ([cell][split][32]); one thread = 8 consecutive channels of a cell ----
__global__ __launch_bounds__(256) void k_feat_split(const float* __restrict__ feat, uint16_t* __restrict__ out, size_t ngroups) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;    // (cell, channel group g = i & 3)
  if (i >= ngroups) return;
  const f32x4 a = *(const f32x4*)(feat + i * 8), b = *(const f32x4*)(feat + i * 8 + 4);
  float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  unsigned part[3][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float r = v[e];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      part[s][e] = bf16_rn_bits(__float_as_uint(r));
      r = r - __uint_as_float(part[s][e] << 16);               // exact: the difference has at most 16 (then 8) significant bits
    }
  }
  const size_t cell = i >> 2, g = i & 3;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    u32x4 w;
#pragma unroll
    for (int d = 0; d < 4; ++d) w[d] = part[s][2 * d] | (part[s][2 * d + 1] << 16);
    *(u32x4*)(out + (cell * 3 + s) * PBD_FLEN + g * 8) = w;
  }
}
void launch_feat_split(const float* feat, uint16_t* out, size_t ncells, hipStream_t s) {
  const size_t ngroups = ncells * 4;
  if (!ngroups) return;
  hipLaunchKernelGGL(k_feat_split, dim3((unsigned)((ngroups + 255) / 256)), dim3(256), 0, s, feat, out, ngroups);
}

// ---- filters -> [tap][k-step][split][n-tile][k-group][32][8] bfloat16 (host) ----
int conv_split_ntiles(int nf) { return (nf + 31) / 32; }
void conv_split_filters(const float* filters, int nf, int kh, int kw, std::vector<uint16_t>& out) {
  const int ntap = kh * kw, NTL = conv_split_ntiles(nf);
  out.assign((size_t)ntap * 2 * 3 * NTL * 512, 0);
  for (int fn = 0; fn < nf; ++fn)
    for (int tap = 0; tap < ntap; ++tap)
      for (int c = 0; c < PBD_FLEN; ++c) {
        float r = filters[((size_t)fn * ntap + tap) * PBD_FLEN + c];
        const int ks = c >> 4, kg = (c >> 3) & 1, e = c & 7;
        for (int s = 0; s < 3; ++s) {
          unsigned u; memcpy(&u, &r, 4);
          const unsigned hb = bf16_rn_bits(u);
          out[((((size_t)(tap * 2 + ks) * 3 + s) * NTL + fn / 32) * 2 + kg) * 256 + (size_t)(fn % 32) * 8 + e] = (uint16_t)hb;
          const unsigned back = hb << 16; float hf; memcpy(&hf, &back, 4);
          r -= hf;                                              // exact
        }
      }
}

// ---------------------------------------------------------------------------------------------------------------------
// PBD_CONV_SPLIT_F16 (opt-in): TWO binary16 parts per operand and THREE products.  binary16 carries 11 significant bits: with
// x 2^e = h + m (h = RN16(x 2^e), m = RN16(x 2^e - h), the subtraction exact) two parts hold 22-23 of an fp32 number's 24 bits,
// every product of two parts is exact in an fp32 accumulator, and h h + h m + m h leaves out terms of 2^-22 relative — against
// 2^-24 for the six bfloat16 products, but far under what the fp32 ACCUMULATION of 800 terms loses either way: measured against
// fp64 on the person bank (tests/tools_split_products_study.py) max 3.2e-7 / rms 4.1e-8, the six-product bank 3.1e-7 / 3.2e-8,
// the fp32 MFMA chain 9.1e-7 / 8.2e-8.  Half the matrix instructions of the six-product bank.
// binary16's range is the price: operands are scaled by powers of two (exact) to sit high in it — features by 2^12 (HOG features
// are <= 1: the truncation channel; |feature| must stay below 65520 / 4096 = 15.99609375, where the high part would round to inf), every filter's weights by its own 2^e with max |w| 2^e in
// [2^13, 2^14) — and a part below 2^-14 (scaled) is a binary16 subnormal of absolute precision 2^-25: an absolute error of 2^-37
// per feature, 2^-38 of the filter's max |w| per weight.  A filter's responses are multiplied by 2^-(12 + e) on the way out (exact).  Not the default and not what
// PBD_CONV_AUTO resolves to: the operands are represented to 23 bits, not 24 — bench.py reports it beside the benched bank.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_feat_split16(const float* __restrict__ feat, uint16_t* __restrict__ out, size_t ngroups) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;    // (cell, channel group g = i & 3)
  if (i >= ngroups) return;
  const f32x4 a = *(const f32x4*)(feat + i * 8), b = *(const f32x4*)(feat + i * 8 + 4);
  const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  f16x8 hi, lo;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float x = v[e] * (float)(1 << SPLIT16_FEXP);
    hi[e] = (_Float16)x;                                        // round to nearest even
    lo[e] = (_Float16)(x - (float)hi[e]);                       // (the subtraction is exact)
  }
  const size_t cell = i >> 2, g = i & 3;
  *(f16x8*)(out + (cell * 2 + 0) * PBD_FLEN + g * 8) = hi;
  *(f16x8*)(out + (cell * 2 + 1) * PBD_FLEN + g * 8) = lo;
}
void launch_feat_split16(const float* feat, uint16_t* out, size_t ncells, hipStream_t s) {
  const size_t ngroups = ncells * 4;
  if (!ngroups) return;
  hipLaunchKernelGGL(k_feat_split16, dim3((unsigned)((ngroups + 255) / 256)), dim3(256), 0, s, feat, out, ngroups);
}
// filters -> [tap][k-step][part (2)][n-tile][k-group][32][8] binary16 of w 2^e(filter); oscale[filter] = the response scale 2^-(12 + e)
void conv_split16_filters(const float* filters, int nf, int kh, int kw, std::vector<uint16_t>& out, std::vector<float>& oscale) {
  const int ntap = kh * kw, NTL = conv_split_ntiles(nf);
  out.assign((size_t)ntap * 2 * 2 * NTL * 512, 0);
  oscale.assign((size_t)NTL * 32, 1.f);
  for (int fn = 0; fn < nf; ++fn) {
    const float* wf = filters + (size_t)fn * ntap * PBD_FLEN;
    float wmax = 0.f;
    for (int i = 0; i < ntap * PBD_FLEN; ++i) wmax = std::max(wmax, std::fabs(wf[i]));
    int x = 0;
    if (wmax > 0.f) std::frexp(wmax, &x);                     // wmax = f 2^x, f in [0.5, 1)
    const int e = wmax > 0.f ? std::min(100, std::max(-110, 14 - x)) : 0;
    oscale[fn] = std::ldexp(1.0f, -(SPLIT16_FEXP + e));
    for (int tap = 0; tap < ntap; ++tap)
      for (int c = 0; c < PBD_FLEN; ++c) {
        float r = std::ldexp(filters[((size_t)fn * ntap + tap) * PBD_FLEN + c], e);
        const int ks = c >> 4, kg = (c >> 3) & 1, el = c & 7;
        for (int s = 0; s < 2; ++s) {
          const _Float16 hv = (_Float16)r;
          uint16_t bits; memcpy(&bits, &hv, 2);
          out[((((size_t)(tap * 2 + ks) * 2 + s) * NTL + fn / 32) * 2 + kg) * 256 + (size_t)(fn % 32) * 8 + el] = bits;
          r -= (float)hv;                                       // exact
        }
      }
  }
}

// The form a product handle launches — four wavefronts per workgroup = one 16 x 16 cell ConvTile, ONE workgroup per CU (304 registers per
// wavefront: 144 + 160 accumulators; two 104-register distance-transform wavefronts still fit on the SIMD), the next step's filter loads
// pinned between this step's MFMAs, groups of five n-tiles.  On the 16x16x32 shape, alternating with the 32x32x16 form on one MI355X
// (profiles/split_bank_16x16x32/): 0.166-0.170 against 0.174-0.182 ms of pdf per frame in batches of 16, 2 540-2 571 against 2 411-2 450
// frames/s with three batches in flight.  One workgroup per CU leaves the CU's other LDS half and a quarter of its
// registers to a distance-transform block of another batch in flight, whose integer / fp64 vector work issues beside bf16 MFMAs
// (tests/tools/mfma_valu_overlap_probe.hip: 0.5-0.75 of the shorter one hidden; fp32 FMAs: none).  What the 32x32x16 form was measured
// against: k_conv_split_variants.hip (tune and probe libraries only; its variant 9 is that form itself).
// nf_stride > 0: a size group of a mixed bank (nf: the group's filters, nf_stride: the planes of a level block; tiles: the group's list)
void launch_conv_split(const ConvTile* tiles, int ntiles, const LevelDev* levels, const uint16_t* feat_split, const uint16_t* wS,
                       float* resp, int nf, int kh, int kw, hipStream_t s, int nf_stride) {
  if (ntiles <= 0) return;
  if (nf_stride > 0) launch_conv_split_groups<4, 2, 3, true>(tiles, ntiles, levels, feat_split, wS, resp, nf, kh, kw, nullptr, s, nf_stride);
  else launch_conv_split_groups<4, 2, 3>(tiles, ntiles, levels, feat_split, wS, resp, nf, kh, kw, nullptr, s);
}
// PBD_CONV_SPLIT_F16: the same form over two parts
void launch_conv_split16(const ConvTile* tiles, int ntiles, const LevelDev* levels, const uint16_t* feat_split, const uint16_t* wS,
                         float* resp, int nf, int kh, int kw, const float* oscale, hipStream_t s, int nf_stride) {
  if (ntiles <= 0) return;
  if (nf_stride > 0) launch_conv_split_groups<4, 2, 2, true>(tiles, ntiles, levels, feat_split, wS, resp, nf, kh, kw, oscale, s, nf_stride);
  else launch_conv_split_groups<4, 2, 2>(tiles, ntiles, levels, feat_split, wS, resp, nf, kh, kw, oscale, s);
}
