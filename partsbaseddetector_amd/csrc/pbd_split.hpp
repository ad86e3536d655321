// pbd_split.hpp — a feature's operands for the split-product filter banks (k_conv_split.hip), one definition for every kernel that
// writes features on the device: k_hog's epilogue (the interior cells) and k_featpad (the border ring of the boundary padding).
#pragma once
#include <stdint.h>
// PBD_CONV_SPLIT_F16: features are carried as two binary16 parts of f 2^SPLIT16_FEXP.  binary16 rounds to inf from 65520 on (its largest
// finite value 65504 plus half a unit in the last place), so the bank's domain is |f| < SPLIT16_FMAX = 15.99609375: from there on the high
// part is inf and the low part, x - inf, NaN.
constexpr int SPLIT16_FEXP = 12;
constexpr float SPLIT16_FMAX = 65520.0f / (float)(1 << SPLIT16_FEXP);
// fp32 bits -> bfloat16 bits, round to nearest even (finite, below bfloat16's overflow threshold): the one definition of the features'
// parts (k_feat_split), the filters' on the host (conv_split_filters) and the filters' on the device (k_bank_split, k_weights.hip)
#ifdef __HIPCC__
__host__ __device__
#endif
static inline unsigned bf16_rn_bits(unsigned u) { return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16; }
#ifdef __HIPCC__
// PBD_CONV_SPLIT: v = h + m + l, three exact bfloat16 parts (round to nearest even, every subtraction exact); part q at sp[q * stride]
__device__ __forceinline__ void feat_split_bf16(float v, uint16_t* sp, int stride) {
  float r = v;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const unsigned u = __float_as_uint(r);
    const unsigned hb = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
    sp[q * stride] = (uint16_t)hb;
    r = r - __uint_as_float(hb << 16);
  }
}
// PBD_CONV_SPLIT_F16: two binary16 parts of v 2^SPLIT16_FEXP (k_feat_split16); part q at sp[q * stride]
__device__ __forceinline__ void feat_split_f16(float v, _Float16* sp, int stride) {
  const float x = v * (float)(1 << SPLIT16_FEXP);
  const _Float16 hv = (_Float16)x;
  sp[0] = hv;
  sp[stride] = (_Float16)(x - (float)hv);
}
#endif
