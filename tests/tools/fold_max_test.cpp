// fold_max against fold_pick(...).v (csrc/fold_pick.hpp), bitwise, on the host: tests/test_fold_max_cpu.py builds and runs this program, once
// plain and once with -fsanitize=address,undefined.  For T in {float, double}, N in {0, 1, 4, 6, 8} and every K from 1 to N (N = 0: K from 1 to 8,
// the arrays hold K entries):
//   random   10^6 vectors in all: normal values, values quantised so that sums tie, and vectors salted with +-0, +-inf and NaN;
//   zeros    every arrangement of {-0, +0, a negative value, -inf} over K <= 4 positions, under biases that make the sums tie exactly
//            (all +0, all -0, alternating signs, and a pair +c / -c on the first two entries);
//   nan      a NaN in each position, among finite values, among -inf, and alone;
//   copy     K == 1: NaN, -inf, +inf, -0, +0 are copied;
//   padded   N > K: entries beyond K repeat entry K - 1 (the form the kernels use) — compared with the K-entry form too.
// Prints one line of counts; exit status 1 and the first mismatches on stderr if any pair of results differs in a bit.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
#include "fold_pick.hpp"

static long g_checked = 0, g_bad = 0, g_unsure = 0;

template <typename T> struct Bits;
template <> struct Bits<float> { typedef uint32_t U; };
template <> struct Bits<double> { typedef uint64_t U; };
template <typename T> static typename Bits<T>::U bits(T v) { typename Bits<T>::U u; memcpy(&u, &v, sizeof(u)); return u; }

// one vector of K entries through form N (padded to N entries by repeats when N > 0) and, for N > 0, through the K-entry form as well
template <typename T, int N>
static void check(const T* sd, const float* bias, int K, const char* what) {
  T s[8]; float b[8];
  const int n = N > 0 ? N : K;
  for (int k = 0; k < n; ++k) { s[k] = sd[k < K ? k : K - 1]; b[k] = bias[k < K ? k : K - 1]; }
  const T want = fold_pick<T, N>(s, b, K).v, got = fold_max<T, N>(s, b, K);
  const T want0 = fold_pick<T, 0>(sd, bias, K).v;
  ++g_checked;
  if (!fold_max_sure(fold_max_fast<T, N>(s, b, K))) ++g_unsure;
  if (bits(want) != bits(got) || bits(want0) != bits(got)) {
    if (g_bad++ < 10) {
      fprintf(stderr, "MISMATCH %s T%zu N %d K %d: fold_pick %a (K-entry form %a) fold_max %a; w =", what, sizeof(T), N, K, (double)want, (double)want0, (double)got);
      for (int k = 0; k < K; ++k) fprintf(stderr, " %a+%a", (double)sd[k], (double)bias[k]);
      fprintf(stderr, "\n");
    }
  }
}
template <typename T>
static void check_all_forms(const T* sd, const float* bias, int K, const char* what) {
  check<T, 0>(sd, bias, K, what);
  if (K <= 1) check<T, 1>(sd, bias, K, what);
  if (K <= 4) check<T, 4>(sd, bias, K, what);
  if (K <= 6) check<T, 6>(sd, bias, K, what);
  check<T, 8>(sd, bias, K, what);
}

template <typename T>
static void run_random(long nvec, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> uni(-4.0, 4.0);
  const T inf = std::numeric_limits<T>::infinity(), nan = std::numeric_limits<T>::quiet_NaN();
  const T special[6] = {(T)-0.0, (T)0.0, -inf, inf, nan, (T)-1.0};
  for (long i = 0; i < nvec; ++i) {
    const int K = 1 + (int)(rng() % 8), kind = (int)(rng() % 4);
    T sd[8]; float bias[8];
    for (int k = 0; k < K; ++k) {
      if (kind == 0) { sd[k] = (T)uni(rng); bias[k] = (float)uni(rng); }                                        // no ties
      else if (kind == 1) { sd[k] = (T)((int)(rng() % 9) - 4) * (T)0.25; bias[k] = (float)((int)(rng() % 9) - 4) * 0.25f; }   // exact ties, zero sums
      else if (kind == 2) { sd[k] = rng() % 3 ? (T)((int)(rng() % 5) - 2) : special[rng() % 6]; bias[k] = (float)((int)(rng() % 3) - 1); }
      else { sd[k] = special[rng() % 6]; bias[k] = rng() % 2 ? 0.0f : -0.0f; }                                    // specials only, signed-zero biases
    }
    // one form per vector, every form in turn (the forms' totals add up to nvec)
    switch (i % 5) {
      case 0: check<T, 0>(sd, bias, K, "random"); break;
      case 1: check<T, 1>(sd, bias, 1, "random"); break;
      case 2: check<T, 4>(sd, bias, 1 + (K - 1) % 4, "random"); break;
      case 3: check<T, 6>(sd, bias, 1 + (K - 1) % 6, "random"); break;
      default: check<T, 8>(sd, bias, K, "random"); break;
    }
  }
}

template <typename T>
static void run_zeros() {
  const T inf = std::numeric_limits<T>::infinity();
  const T vals[4] = {(T)-0.0, (T)0.0, (T)-1.5, -inf};
  for (int K = 1; K <= 4; ++K) {
    int npos = 1;
    for (int k = 0; k < K; ++k) npos *= 4;
    for (int a = 0; a < npos; ++a) {
      T sd[4];
      for (int k = 0, r = a; k < K; ++k, r /= 4) sd[k] = vals[r % 4];
      for (int bk = 0; bk < 5; ++bk) {
        float bias[4];
        for (int k = 0; k < K; ++k)
          bias[k] = bk == 0 ? 0.0f : bk == 1 ? -0.0f : bk == 2 ? ((k & 1) ? -0.0f : 0.0f) : bk == 3 ? ((k & 1) ? 0.0f : -0.0f) : 0.0f;
        T sdb[4];
        for (int k = 0; k < K; ++k) sdb[k] = sd[k];
        if (bk == 4) {   // entries 0 and 1 shifted by +c / -c under biases -c / +c: the sums tie exactly where the entries did
          bias[0] = -1.5f; sdb[0] = sd[0] + (T)1.5;
          if (K > 1) { bias[1] = 1.5f; sdb[1] = sd[1] - (T)1.5; }
        }
        check_all_forms<T>(sdb, bias, K, "zeros");
      }
    }
  }
}

template <typename T>
static void run_nan() {
  const T inf = std::numeric_limits<T>::infinity(), nan = std::numeric_limits<T>::quiet_NaN();
  for (int K = 1; K <= 8; ++K)
    for (int pos = 0; pos < K; ++pos)
      for (int bg = 0; bg < 4; ++bg) {   // the other entries: ascending finite, descending finite, -inf, zeros of both signs
        T sd[8]; float bias[8];
        for (int k = 0; k < K; ++k) {
          sd[k] = bg == 0 ? (T)(k - 3) : bg == 1 ? (T)(3 - k) : bg == 2 ? -inf : ((k & 1) ? (T)0.0 : (T)-0.0);
          bias[k] = bg == 3 ? 0.0f : 0.5f;
        }
        sd[pos] = nan;
        check_all_forms<T>(sd, bias, K, "nan");
        sd[pos] = inf; bias[pos] = -std::numeric_limits<float>::infinity();   // inf + -inf: the sum itself is the NaN
        check_all_forms<T>(sd, bias, K, "nan-sum");
      }
  for (int K = 1; K <= 8; ++K) {         // all NaN: -inf is left (K == 1: the NaN is copied)
    T sd[8]; float bias[8];
    for (int k = 0; k < K; ++k) { sd[k] = nan; bias[k] = 0.25f; }
    check_all_forms<T>(sd, bias, K, "all-nan");
  }
}

template <typename T>
static void run_copy() {
  const T inf = std::numeric_limits<T>::infinity(), nan = std::numeric_limits<T>::quiet_NaN();
  const T vals[7] = {nan, -inf, inf, (T)-0.0, (T)0.0, (T)1.25, (T)-1.25};
  const float biases[4] = {0.0f, -0.0f, 0.5f, -1.25f};
  for (T v : vals)
    for (float b : biases) {
      const T sd[1] = {v};
      const float bias[1] = {b};
      check_all_forms<T>(sd, bias, 1, "copy");
      const T want = v + (T)b;           // K == 1: the one weighted entry itself
      const T sd8[8] = {v, v, v, v, v, v, v, v};
      const float bias8[8] = {b, b, b, b, b, b, b, b};
      if (bits(fold_max<T, 8>(sd8, bias8, 1)) != bits(want)) {
        ++g_bad;
        fprintf(stderr, "MISMATCH copy T%zu: %a + %a is not copied\n", sizeof(T), (double)v, (double)b);
      }
    }
}

int main(int argc, char** argv) {
  const long nrand = argc > 1 ? atol(argv[1]) : 1000000;
  run_random<float>(nrand / 2, 11u);
  run_random<double>(nrand - nrand / 2, 12u);
  const long nr = g_checked;
  run_zeros<float>(); run_zeros<double>();
  const long nz = g_checked - nr;
  run_nan<float>(); run_nan<double>();
  const long nn = g_checked - nr - nz;
  run_copy<float>(); run_copy<double>();
  const long nc = g_checked - nr - nz - nn;
  printf("fold_max: %ld random, %ld zeros, %ld nan, %ld copy checks; %ld took the fold_pick path; %ld mismatches\n", nr, nz, nn, nc, g_unsure, g_bad);
  return g_bad ? 1 : 0;
}
