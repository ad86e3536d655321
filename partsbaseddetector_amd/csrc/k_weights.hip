// k_weights.hip — a live handle's weights replaced on the device (include/pbd_c.h "weight and threshold updates"; host side:
// pbd_weights.cpp).  A weight vector arrives as doubles in Model.feature_layout() order; k_weights_round makes the model's float32
// values of it (the staging vector, which also becomes the host mirror), and the pack kernels gather from the staging vector into
// every layout upload_bank (pbd_api.cpp) writes at create, in place.  Runs once per solver round: written for exactness — every
// kernel reproduces the host function's integer and exact-float operations —, one thread per 16-byte destination vector.
#include "pbd_internal.hpp"
#include "pbd_split.hpp"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---- doubles -> the staging vector: (float)w[i], round to nearest even; *bad = the first index that is not finite then (else ~0u = -1) ----
__global__ __launch_bounds__(256) void k_weights_round(const double* __restrict__ w, int len, float* __restrict__ out, unsigned* __restrict__ bad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  const float f = (float)w[i];
  out[i] = f;
  if ((__float_as_uint(f) & 0x7F800000u) == 0x7F800000u) atomicMin(bad, (unsigned)i);
}
void launch_weights_round(const double* w, int len, float* out, int* bad, hipStream_t s) {
  hipMemsetAsync(bad, 0xFF, sizeof(int), s);
  if (len > 0) hipLaunchKernelGGL(k_weights_round, dim3((len + 255) / 256), dim3(256), 0, s, w, len, out, (unsigned*)bad);
}

// ---- d_wT of one bank (upload_bank): three regions of wt_n = ntap * 32 * nfpad elements of T, a border cell of 32 elements (which
// carries no weight and is left alone) behind the first.  Region 0: [tap][c][nfpad].  float — region 1: [tap][half][k][nfpad][s],
// c = 16 half + 4 k + s; region 2: [tap][half][s][nfpad][u], c = 16 half + 4 u + s.  double — region 1: [tap][group][k][nfpad][u],
// c = 8 group + 4 u + k; region 2: the float region 2, widened (no kernel reads it).  Lanes n >= nf are 0.
// src[n]: where the bank's filter n ([tap][c]) starts in the staging vector.
template <typename T>
__global__ __launch_bounds__(256) void k_bank_pack(const float* __restrict__ stage, const int* __restrict__ src, int nf, int ntap, int nfpad,
                                                   T* __restrict__ wT) {
  constexpr int V = 16 / (int)sizeof(T);
  const unsigned wt_n = (unsigned)ntap * PBD_FLEN * (unsigned)nfpad;     // a multiple of 160 * 32: no vector straddles two regions
  const unsigned v = blockIdx.x * 256u + threadIdx.x;
  if (v >= 3u * wt_n / V) return;
  const unsigned i0 = v * V, region = i0 / wt_n;
  T val[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const unsigned r = i0 + e - region * wt_n;
    unsigned n, tap, c;
    if (region == 0) { n = r % nfpad; c = (r / nfpad) % PBD_FLEN; tap = r / nfpad / PBD_FLEN; }
    else if (sizeof(T) == 8 && region == 1) {
      const unsigned u = r & 1, q = (r >> 1) / nfpad;
      n = (r >> 1) % nfpad; c = 8 * ((q >> 2) & 3) + 4 * u + (q & 3); tap = q >> 4;
    } else {
      const unsigned lo = r & 3, q = (r >> 2) / nfpad, mid = q & 3, half = (q >> 2) & 1;
      n = (r >> 2) % nfpad; tap = q >> 3;
      c = region == 1 ? 16 * half + 4 * mid + lo : 16 * half + 4 * lo + mid;
    }
    val[e] = n < (unsigned)nf ? (T)stage[(size_t)src[n] + tap * PBD_FLEN + c] : (T)0;
  }
  T* dst = wT + (region ? PBD_FLEN : 0) + i0;
  if constexpr (sizeof(T) == 8) *(double2*)dst = double2{val[0], val[1]};
  else *(float4*)dst = float4{val[0], val[1], val[2], val[3]};
}
void launch_bank_pack(const float* stage, const int* src, int nf, int kh, int kw, int nfpad, void* wT, int ts, hipStream_t s) {
  const size_t nvec = (size_t)3 * kh * kw * PBD_FLEN * nfpad / (16 / ts);
  if (!nvec) return;
  const dim3 grid((unsigned)((nvec + 255) / 256));
  if (ts == 8) hipLaunchKernelGGL(k_bank_pack<double>, grid, dim3(256), 0, s, stage, src, nf, kh * kw, nfpad, (double*)wT);
  else hipLaunchKernelGGL(k_bank_pack<float>, grid, dim3(256), 0, s, stage, src, nf, kh * kw, nfpad, (float*)wT);
}

// ---- d_wS of a PBD_CONV_SPLIT bank: conv_split_filters (k_conv_split.hip) — [tap][k-step][split][n-tile][k-group][32][8] bfloat16,
// c = 16 k-step + 8 k-group + e; one thread = the 8 channels of one (tap, k-step, split, filter, k-group) ----
__global__ __launch_bounds__(256) void k_bank_split(const float* __restrict__ stage, const int* __restrict__ src, int nf, int ntap, int ntl,
                                                    uint16_t* __restrict__ wS) {
  const unsigned v = blockIdx.x * 256u + threadIdx.x;
  if (v >= (unsigned)ntap * 6u * ntl * 64u) return;
  const unsigned lane = v & 31, kg = (v >> 5) & 1, q = v >> 6, tile = q % ntl, s = (q / ntl) % 3, ks = (q / ntl / 3) & 1, tap = q / ntl / 6;
  const unsigned fn = tile * 32 + lane;
  unsigned part[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    part[e] = 0;
    if (fn >= (unsigned)nf) continue;
    float r = stage[(size_t)src[fn] + tap * PBD_FLEN + ks * 16 + kg * 8 + e];
    for (unsigned k = 0; k <= s; ++k) {
      part[e] = bf16_rn_bits(__float_as_uint(r));
      r = r - __uint_as_float(part[e] << 16);                  // exact
    }
  }
  u32x4 w;
#pragma unroll
  for (int d = 0; d < 4; ++d) w[d] = (part[2 * d] & 0xFFFFu) | (part[2 * d + 1] << 16);
  *(u32x4*)(wS + (size_t)v * 8) = w;
}
void launch_bank_split(const float* stage, const int* src, int nf, int kh, int kw, uint16_t* wS, hipStream_t s) {
  const int ntl = (nf + 31) / 32;
  const size_t nvec = (size_t)kh * kw * 6 * ntl * 64;
  if (nvec) hipLaunchKernelGGL(k_bank_split, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, s, stage, src, nf, kh * kw, ntl, wS);
}

// ---- d_wS and d_oscale of a PBD_CONV_SPLIT_F16 bank: conv_split16_filters — per filter e = clamp(14 - x), max |w| = f 2^x with f in
// [0.5, 1) as frexp gives it, oscale = 2^-(12 + e), and the two binary16 parts of w 2^e in [tap][k-step][part][n-tile][k-group][32][8].
// One wavefront per filter slot of the n-tiles (slots >= nf: zero parts, oscale 1). ----
__global__ __launch_bounds__(64) void k_bank_split16(const float* __restrict__ stage, const int* __restrict__ src, int nf, int ntap, int ntl,
                                                     uint16_t* __restrict__ wS, float* __restrict__ oscale) {
  const unsigned fn = blockIdx.x, lane = threadIdx.x;          // fn < ntl * 32: the grid
  const bool real = fn < (unsigned)nf;
  const float* wf = real ? stage + src[fn] : nullptr;
  const int nw = ntap * PBD_FLEN;
  float wmax = 0.f;
  if (real) for (int i = lane; i < nw; i += 64) wmax = fmaxf(wmax, fabsf(wf[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, o, 64));
  int e = 0;
  if (wmax > 0.f) {   // frexp's exponent of a finite positive float, by its bits: normal 2^(E - 127) 1.m = 2^(E - 126) 0.1m; subnormal m 2^-149
    const unsigned b = __float_as_uint(wmax), E = (b >> 23) & 0xFFu, m = b & 0x7FFFFFu;
    const int x = E ? (int)E - 126 : (31 - __clz((int)m)) - 148;
    e = min(100, max(-110, 14 - x));
  }
  if (lane == 0) oscale[fn] = real ? __uint_as_float((unsigned)(127 - SPLIT16_FEXP - e) << 23) : 1.f;
  const float scale = __uint_as_float((unsigned)(127 + e) << 23);   // 2^e: w 2^e is ldexp(w, e), one rounding where the result is subnormal
  for (int g = lane; g < ntap * 4; g += 64) {                       // (tap, k-step, k-group): 8 channels
    const unsigned tap = g >> 2, ks = (g >> 1) & 1, kg = g & 1;
    unsigned hi[8], lo[8];
#pragma unroll
    for (int el = 0; el < 8; ++el) {
      hi[el] = lo[el] = 0;
      if (!real) continue;
      const float r = wf[tap * PBD_FLEN + ks * 16 + kg * 8 + el] * scale;
      const _Float16 hv = (_Float16)r;                              // round to nearest even
      const _Float16 lv = (_Float16)(r - (float)hv);                // (the subtraction is exact)
      hi[el] = __builtin_bit_cast(unsigned short, hv);
      lo[el] = __builtin_bit_cast(unsigned short, lv);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const unsigned* p = s ? lo : hi;
      const u32x4 w = {p[0] | (p[1] << 16), p[2] | (p[3] << 16), p[4] | (p[5] << 16), p[6] | (p[7] << 16)};
      *(u32x4*)(wS + ((((size_t)(tap * 2 + ks) * 2 + s) * ntl + fn / 32) * 2 + kg) * 256 + (size_t)(fn % 32) * 8) = w;
    }
  }
}
void launch_bank_split16(const float* stage, const int* src, int nf, int kh, int kw, uint16_t* wS, float* oscale, hipStream_t s) {
  const int ntl = (nf + 31) / 32;
  if (ntl > 0) hipLaunchKernelGGL(k_bank_split16, dim3((unsigned)ntl * 32), dim3(64), 0, s, stage, src, nf, kh * kw, ntl, wS, oscale);
}
