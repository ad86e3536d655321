// fold_pick.hpp — the ONE statement of a message's mixture choice (src/DynamicProgram.cpp:139-150, Math::reduceMax,
// include/Math.hpp:108-185): for one cell, one child and one parent mixture m,
//   weighted[k] = sdt_k + bias(k)[m]                                  (:139)
//   (maxv, maxi) = reduceMax(weighted): starts from -inf, strict >, the FIRST maximum wins — a NaN leaves -inf, index 0;
//   K == 1: the shortcut copies (Math.hpp:154-158): maxv = the one weighted map, NaN and -inf included, maxi = 0.
// The value is what the parent's score accumulates (k_dp.hip: fold_children); the index is Ik (:150).  The index is a pure
// function of the children's kept y-pass outputs and the model's biases, so nothing stores it per cell: k_backtrack picks it for
// the cells it visits, k_ik_fill for whole planes when a caller asks for the tables — the same adds and compares on the same
// stored values, hence the same index bit for bit.  tests/test_fold_pick_cpu.py states it in numpy against the oracle; the GPU tests run this header.
//
// fold_max is the VALUE alone, for the consumers that drop the index (the fold itself): a plain maximum of the weighted entries seeded
// with -inf.  maxNum skips a (quiet) NaN exactly as the strict > does — the sums are results of additions, hence never signalling —, equal
// maxima have equal bits, so the maximum is fold_pick's value bit for bit EXCEPT when it is a zero: of tied zeros of both signs the reference
// keeps the first, a maximum instruction the positive one.  fold_max_sure(r) = `|r| > 0` is the test for that doubt; it is also false for
// a NaN, which only the K == 1 copy yields and both forms copy alike, so sending one to fold_pick changes nothing.  fold_max = fold_max_fast,
// and fold_pick where the result is not sure: the per-value statement, which tests/test_fold_max_cpu.py compares with fold_pick bitwise.
// The kernel (k_dp.hip: fold_children) does not call fold_max: it runs the same fold_max_fast and the same fold_pick, but decides per CHILD and
// WAVEFRONT — fold_max_sure on the smallest |r| of a child's results (a NaN-skipping minimum: zeros only), any lane — so that the branch is
// wave-uniform; that aggregation is checked on the GPU (tests/test_gpu_fold_max.py), the two building blocks on the host.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define FP_HD __host__ __device__ __forceinline__
#else
#define FP_HD static inline
#endif

template <typename T> struct FoldPick { T v; int i; };

// sd[k]: the child's distance-transformed score of mixture k at the cell; bias_col[k] = bias(k)[m].
// N = 0: the arrays hold K entries.  N > 0: register arrays of N >= K entries whose entries beyond K repeat entry K - 1 (the
// plan pads them so): the loop runs to the compile-time N with no `k < K` test — a repeat cannot be strictly greater than the
// maximum it has already been folded into — and the K == 1 shortcut is a select, not a branch (k_dp.hip says why).
template <typename T, int N = 0>
FP_HD FoldPick<T> fold_pick(const T* sd, const float* bias_col, int K) {
  const int n = N > 0 ? N : K;
  // k = 0 first: Math::reduceMax starts from -inf and takes strict > (first maximum wins): a NaN score leaves -inf
  const T w0 = sd[0] + bias_col[0];                    // DynamicProgram.cpp:139
  T v = w0 > (T)-INFINITY ? w0 : (T)-INFINITY;
  int bi = 0;
#ifdef __HIPCC__
#pragma unroll
#endif
  for (int k = 1; k < n; ++k) {
    const T wv = sd[k] + bias_col[k];
    const bool take = wv > v;                          // strict >: first max wins
    bi = take ? k : bi;
    v = take ? wv : v;
  }
  return FoldPick<T>{K == 1 ? w0 : v, bi};             // (K == 1: entries beyond 0 repeat entry 0, bi stays 0)
}

FP_HD float fold_maxnum(float a, float b) { return __builtin_fmaxf(a, b); }
FP_HD double fold_maxnum(double a, double b) { return __builtin_fmax(a, b); }
FP_HD float fold_abs(float a) { return __builtin_fabsf(a); }
FP_HD double fold_abs(double a) { return __builtin_fabs(a); }

// the maximum alone: fold_pick's value wherever fold_max_sure(result), sd / bias_col / N / K as in fold_pick
template <typename T, int N = 0>
FP_HD T fold_max_fast(const T* sd, const float* bias_col, int K) {
  const int n = N > 0 ? N : K;
  const T w0 = sd[0] + bias_col[0];                    // DynamicProgram.cpp:139
  T v = fold_maxnum((T)-INFINITY, w0);
#ifdef __HIPCC__
#pragma unroll
#endif
  for (int k = 1; k < n; ++k) v = fold_maxnum(v, (T)(sd[k] + bias_col[k]));   // (a repeat of entry K - 1 changes no maximum)
  return K == 1 ? w0 : v;
}
template <typename T> FP_HD bool fold_max_sure(T r) { return fold_abs(r) > (T)0; }   // false for a zero and for a NaN

// fold_pick(sd, bias_col, K).v, bit for bit, for every input
template <typename T, int N = 0>
FP_HD T fold_max(const T* sd, const float* bias_col, int K) {
  const T r = fold_max_fast<T, N>(sd, bias_col, K);
  return fold_max_sure(r) ? r : fold_pick<T, N>(sd, bias_col, K).v;
}
