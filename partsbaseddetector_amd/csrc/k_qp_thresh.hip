// k_qp_thresh.hip — the threshold a trained model ships with (include/pbd_c.h "one training round"): train.m:116-118 with qp_scorepos
// (:198-204) on the resident columns.  gfx950 only.
//
// k_qp_thresh_weff: w_eff[j] = w[j] + w0[j] * wreg[j], one thread per dense element; the product is rounded, then the sum.
// k_qp_thresh_select: find(qp.i(1, 1:n) == 1) as a stream compaction.  ONE workgroup walks the examples in chunks of QT_NT in ascending
//   order; inside a chunk a lane's position is the number of selected lanes below it (a ballot and a popcount per wavefront, the
//   wavefronts' counts through LDS), in front of it the running total of the earlier chunks, which every thread carries in a register.
//   The order is the examples' by construction: no atomic takes part.  O(n / QT_NT) rounds of one id word per thread.
// (the scores are k_qp.hip's k_qp_score over the selection: the device text pbd_qp_score_dev runs)
// k_qp_thresh_scale: s[t] = s[t] / cpos, one rounded division, and the first position whose quotient is not finite (the selection is
//   ascending, so the first position is the smallest example index).  ONE workgroup, lane-strided; the minimum is folded through LDS.
// k_qp_thresh_rank: the order statistic by an exact count, for any m.  A thread owns score i and counts the scores that sort in front
//   of it — strictly smaller, or equal with a smaller position — over all m, which the workgroup stages through LDS QT_NT at a time
//   (every lane reads the same LDS word in a step: a broadcast, no bank conflict).  The counts of m finite scores are a permutation of
//   0 .. m - 1, so exactly one thread of the grid holds `rank` and stores its score: equal scores store equal values, ties cannot
//   change the result.  The count is O(m^2) comparisons, as mining's record order is: 4e6 at m = 2000, a few microseconds of one CU
//   row; a selection network would not be simpler to state exactly.
// Plain vector stores only.
#include "pbd_internal.hpp"

__global__ void __launch_bounds__(QT_NT) k_qp_thresh_weff(const double* __restrict__ w, const double* __restrict__ w0,
                                                         const double* __restrict__ wreg, int len, double* __restrict__ out) {
  const int j = blockIdx.x * QT_NT + threadIdx.x;
  if (j < len) out[j] = __dadd_rn(w[j], __dmul_rn(w0[j], wreg[j]));
}

__global__ void __launch_bounds__(QT_NT) k_qp_thresh_select(QpDev q, int n, int* __restrict__ sel, QpThreshOut* __restrict__ out) {
  __shared__ int s_wave[QT_NT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;                                    // selected examples of the chunks walked so far (uniform over the workgroup)
  for (int c0 = 0; c0 < n; c0 += QT_NT) {
    const int i = c0 + threadIdx.x;
    const bool pos = i < n && q.ids[(size_t)q.slot[i] * 5] == 1;
    const unsigned long long bal = __ballot(pos);
    if (lane == 0) s_wave[wave] = __popcll(bal);
    __syncthreads();
    int off = base, tot = 0;
#pragma unroll
    for (int v = 0; v < QT_NT / 64; ++v) { const int c = s_wave[v]; off += v < wave ? c : 0; tot += c; }
    if (pos) sel[off + __popcll(bal & ((1ull << lane) - 1ull))] = i;
    base += tot;
    __syncthreads();                               // s_wave is rewritten by the next chunk
  }
  if (threadIdx.x == 0) out->m = base;
}

__global__ void __launch_bounds__(QT_NT) k_qp_thresh_scale(double* __restrict__ s, const int* __restrict__ sel, int m, double cpos,
                                                          QpThreshOut* __restrict__ out) {
  __shared__ int s_bad[QT_NT];
  int bad = m;
  for (int t = threadIdx.x; t < m; t += QT_NT) {
    const double v = __ddiv_rn(s[t], cpos);
    s[t] = v;
    if (!(v - v == 0.0) && t < bad) bad = t;       // (v - v is NaN for an infinity and for a NaN)
  }
  s_bad[threadIdx.x] = bad;
  __syncthreads();
  for (int h = QT_NT / 2; h >= 1; h >>= 1) {
    if (threadIdx.x < h && s_bad[threadIdx.x + h] < s_bad[threadIdx.x]) s_bad[threadIdx.x] = s_bad[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) out->bad = s_bad[0] < m ? sel[s_bad[0]] : -1;
}

__global__ void __launch_bounds__(QT_NT) k_qp_thresh_rank(const double* __restrict__ s, int m, int rank, QpThreshOut* __restrict__ out) {
  __shared__ double s_t[QT_NT];
  const int i = blockIdx.x * QT_NT + threadIdx.x;
  const double v = i < m ? s[i] : 0.0;
  int cnt = 0;
  for (int c0 = 0; c0 < m; c0 += QT_NT) {
    const int j = c0 + threadIdx.x;
    s_t[threadIdx.x] = j < m ? s[j] : 0.0;
    __syncthreads();
    const int lim = m - c0 < QT_NT ? m - c0 : QT_NT;
    for (int u = 0; u < lim; ++u) {
      const double x = s_t[u];
      cnt += (x < v || (x == v && c0 + u < i)) ? 1 : 0;
    }
    __syncthreads();
  }
  if (i < m && cnt == rank) out->thresh = v;
}

void launch_qp_thresh_weff(const double* w, const double* w0, const double* wreg, int len, double* out, hipStream_t st) {
  hipLaunchKernelGGL(k_qp_thresh_weff, dim3((len + QT_NT - 1) / QT_NT), dim3(QT_NT), 0, st, w, w0, wreg, len, out);
}
void launch_qp_thresh_select(const QpDev& q, int n, int* sel, QpThreshOut* out, hipStream_t st) {
  hipLaunchKernelGGL(k_qp_thresh_select, dim3(1), dim3(QT_NT), 0, st, q, n, sel, out);
}
void launch_qp_thresh_scale(double* s, const int* sel, int m, double cpos, QpThreshOut* out, hipStream_t st) {
  hipLaunchKernelGGL(k_qp_thresh_scale, dim3(1), dim3(QT_NT), 0, st, s, sel, m, cpos, out);
}
void launch_qp_thresh_rank(const double* s, int m, int rank, QpThreshOut* out, hipStream_t st) {
  hipLaunchKernelGGL(k_qp_thresh_rank, dim3((m + QT_NT - 1) / QT_NT), dim3(QT_NT), 0, st, s, m, rank, out);
}
