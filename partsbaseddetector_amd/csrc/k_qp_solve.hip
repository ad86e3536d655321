// k_qp_solve.hip — the QP solver's kernels (include/pbd_c.h "QP solver"): matlab/mex/qp_one_sparse.cc's coordinate-descent pass
// over the device-resident example cache, the non-negativity clamp with w'w, and qp_w.m.  gfx950 only.
//
// k_qp_pass: ONE workgroup runs the whole pass, one launch per pass: the pass is a serial chain through w across examples, but a
//   step is a sparse dot of about k values with w, a handful of scalar decisions and an axpy of about k values into w, and those are
//   spread over the workgroup's lanes.  No cooperative launch, no grid barrier, no spin-wait: within one CU __syncthreads() orders the
//   workgroup's global stores and loads of w.  Every barrier is reached by all threads: thread 0's decisions (which branch, dA, i2)
//   go through LDS and the branches around barriers are uniform.  The arrays the kernel writes (w, a, idC, idI, err, sv) are plain
//   pointers, neither const nor __restrict__, read with ordinary vector loads.
//   Everything scalar is qp_one_sparse.cc:171-253 line for line, by thread 0, in double with explicit __dadd_rn / __dmul_rn /
//   __ddiv_rn (nothing fused); MAX / MIN keep the macros' operand order (MAX(W, 0) keeps -0.0 and NaN).
//   The vector parts use the library's stated order: a block's products go through the block sum (qp_fold.hpp) by one wavefront,
//   the blocks' sums are added in block order by thread 0; the dot of two columns is the complete one (every intersecting pair of
//   blocks, x's blocks outer, x2's inner); the axpy rounds one product and one sum per element.
#include "pbd_internal.hpp"
#include "qp_fold.hpp"

#define QPS_NT 1024
#define QPS_WAVES (QPS_NT / 64)

// the reference's macros, operand order kept
__device__ __forceinline__ double qp_MAX(double A, double B) { return A < B ? B : A; }
__device__ __forceinline__ double qp_MIN(double A, double B) { return A > B ? B : A; }

struct QpCol { const float* x; const int* tab; int nb; };
__device__ __forceinline__ QpCol qp_col(const QpDev& q, int col) {
  QpCol c;
  c.x = q.x + (size_t)q.k * col; c.tab = q.tab + (size_t)col * q.nbmax * 3; c.nb = q.nblk[col];
  return c;
}

// score(W, x), the blocks' part: block b's sum to out[b], one wavefront per block
__device__ __forceinline__ void qp_score_blocks(double* W, const QpCol& c, double* out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int b = wave; b < c.nb; b += QPS_WAVES) {
    const int st = c.tab[b * 3], ln = c.tab[b * 3 + 1], xo = c.tab[b * 3 + 2];
    double s = 0.0;
    for (int e = lane; e < ln; e += 64) s = __dadd_rn(s, __dmul_rn(W[st + e], (double)c.x[xo + e]));
    s = qp_fold(s);
    if (lane == 0) out[b] = s;
  }
}

// add(W, x, a): blocks of one column do not overlap (checked on the host), so every element has one writer
__device__ __forceinline__ void qp_add(double* W, const QpCol& c, double a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int b = wave; b < c.nb; b += QPS_WAVES) {
    const int st = c.tab[b * 3], ln = c.tab[b * 3 + 1], xo = c.tab[b * 3 + 2];
    for (int e = lane; e < ln; e += 64) W[st + e] = __dadd_rn(W[st + e], __dmul_rn(a, (double)c.x[xo + e]));
  }
}

__device__ __forceinline__ void qp_clamp(double* W, const int* noneg, int p) {
  for (int d = threadIdx.x; d < p; d += blockDim.x) W[noneg[d]] = qp_MAX(W[noneg[d]], 0.0);
}

static size_t qp_pass_lds(int nbmax) { return sizeof(double) * 4 * (size_t)nbmax + sizeof(int) * ((size_t)nbmax + 1); }

__global__ void __launch_bounds__(QPS_NT) k_qp_pass(QpDev q, QpSolveDev s, const int* noneg, int p, int n) {
  extern __shared__ double s_dyn[];
  double* s_bs = s_dyn;                        // [nbmax] block sums of score(W, x)
  double* s_bs2 = s_bs + q.nbmax;              // [nbmax] of score(W, x2)
  double* s_ps = s_bs2 + q.nbmax;              // [2 nbmax] sums of the intersecting block pairs, in the dot's order
  int* s_cnt = (int*)(s_ps + 2 * (size_t)q.nbmax);   // [nbmax] pairs of x's block t, then their exclusive prefix
  __shared__ double s_err[QPS_NT];
  __shared__ double s_dA;
  __shared__ int s_branch, s_i2, s_go, s_P;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const double C = 1.0;                        // qp_one.m:15
  double* W = s.w; double* A = s.a;
  double L = 0.0, G = 0.0, Ai = 0.0, Ci = 0.0; // thread 0's
  if (tid == 0) L = s.stat[QP_STAT_L];
  for (int cnt = 0; cnt < n; ++cnt) {
    const int i = s.order[cnt], j = s.idP[cnt] - 1;
    const int col = q.slot[i];
    const QpCol x = qp_col(q, col);
    qp_score_blocks(W, x, s_bs);
    __syncthreads();
    if (tid == 0) {
      double y = 0.0;
      for (int b = 0; b < x.nb; ++b) y = __dadd_rn(y, s_bs[b]);
      const double Bi = (double)q.b[col];
      Ai = qp_MAX(qp_MIN(A[i], C), 0.0);
      A[i] = Ai;
      Ci = qp_MAX(qp_MIN(s.idC[j], C), Ai);
      G = __dsub_rn(y, Bi);
      double PG = G;
      if ((Ai == 0 && G >= 0) || (Ci >= C && G <= 0)) PG = 0;
      if (-G > s.err[j]) s.err[j] = -G;
      if (Ai == 0 && G > 0) s.sv[i] = 0;
      const int ii = s.idI[j];
      int branch = 0;
      if (Ci >= C && G < -1e-12 && Ai < C && ii - 1 != i && ii > 0) {
        branch = 2;
        s_i2 = ii - 1;
      } else if (PG > 1e-12 || PG < -1e-12) {
        branch = 1;
        double dA = Ai;
        const double maxA = __dsub_rn(C, __dsub_rn(Ci, dA));
        Ai = qp_MIN(qp_MAX(__dsub_rn(Ai, __ddiv_rn(G, q.d[col])), 0.0), maxA);
        A[i] = Ai;
        dA = __dsub_rn(Ai, dA);
        L = __dadd_rn(L, __dmul_rn(dA, Bi));
        s.idC[j] = qp_MIN(qp_MAX(__dadd_rn(Ci, dA), 0.0), C);
        s_dA = dA;
      }
      s_branch = branch;
    }
    __syncthreads();
    const int branch = s_branch;               // (uniform)
    if (branch == 2) {
      const int i2 = s_i2, col2 = q.slot[i2];
      const QpCol x2 = qp_col(q, col2);
      qp_score_blocks(W, x2, s_bs2);
      for (int t = tid; t < x.nb; t += QPS_NT) {   // how many of x2's blocks x's block t meets
        const int st = x.tab[t * 3], en = st + x.tab[t * 3 + 1];
        int c = 0;
        for (int u = 0; u < x2.nb; ++u) {
          const int st2 = x2.tab[u * 3], en2 = st2 + x2.tab[u * 3 + 1];
          c += (st > st2 ? st : st2) < (en < en2 ? en : en2);
        }
        s_cnt[t] = c;
      }
      __syncthreads();
      if (tid == 0) {
        double y2 = 0.0;
        for (int b = 0; b < x2.nb; ++b) y2 = __dadd_rn(y2, s_bs2[b]);
        G = __dsub_rn(G, __dsub_rn(y2, (double)q.b[col2]));
        if (Ai == 0 && G > 0) { G = 0; s.sv[i] = 0; }
        const int go = G > 1e-12 || G < -1e-12;
        if (go) {
          int run = 0;
          for (int t = 0; t < x.nb; ++t) { const int c = s_cnt[t]; s_cnt[t] = run; run += c; }
          s_P = run;                           // <= nb + nb2 - 1: neither column's blocks overlap each other
        }
        s_go = go;
      }
      __syncthreads();
      if (s_go) {                              // (uniform)
        for (int t = wave; t < x.nb; t += QPS_WAVES) {
          const int st = x.tab[t * 3], en = st + x.tab[t * 3 + 1], xo = x.tab[t * 3 + 2];
          int idx = s_cnt[t];
          for (int u = 0; u < x2.nb; ++u) {
            const int st2 = x2.tab[u * 3], en2 = st2 + x2.tab[u * 3 + 1], xo2 = x2.tab[u * 3 + 2];
            const int j1 = st > st2 ? st : st2, j2 = en < en2 ? en : en2;
            if (j1 >= j2) continue;
            double v = 0.0;
            for (int e = j1 + lane; e < j2; e += 64)
              v = __dadd_rn(v, __dmul_rn((double)x.x[xo + (e - st)], (double)x2.x[xo2 + (e - st2)]));
            v = qp_fold(v);
            if (lane == 0) s_ps[idx] = v;
            ++idx;
          }
        }
        __syncthreads();
        if (tid == 0) {
          double res = 0.0;
          const int P = s_P;
          for (int t = 0; t < P; ++t) res = __dadd_rn(res, s_ps[t]);
          const double Bi = (double)q.b[col], B2 = (double)q.b[col2], A2 = A[i2];
          double dA = __ddiv_rn(-G, __dsub_rn(__dadd_rn(q.d[col], q.d[col2]), __dmul_rn(2.0, res)));
          if (dA > 0) dA = qp_MIN(qp_MIN(dA, __dsub_rn(C, Ai)), A2);
          else dA = qp_MAX(qp_MAX(dA, -Ai), __dsub_rn(A2, C));
          Ai = __dadd_rn(Ai, dA);
          A[i] = Ai;
          A[i2] = __dsub_rn(A2, dA);
          L = __dadd_rn(L, __dmul_rn(dA, __dsub_rn(Bi, B2)));
          s_dA = dA;
        }
        __syncthreads();
        const double dA = s_dA;
        qp_add(W, x, dA);
        __syncthreads();                       // x first, then x2: their blocks may share elements
        qp_add(W, x2, -dA);
        __syncthreads();
        qp_clamp(W, noneg, p);
      }
    } else if (branch == 1) {
      qp_add(W, x, s_dA);
      __syncthreads();
      qp_clamp(W, noneg, p);
    }
    if (tid == 0 && Ai > 0) s.idI[j] = i + 1;
    __syncthreads();                           // w, and the LDS tables, before the next step
  }
  // loss = err[0] + err[1] + ... left to right
  double sum = 0.0;
  for (int c0 = 0; c0 < n; c0 += QPS_NT) {
    if (c0 + tid < n) s_err[tid] = s.err[c0 + tid];
    __syncthreads();
    if (tid == 0) {
      const int m = n - c0 < QPS_NT ? n - c0 : QPS_NT;
      for (int t = 0; t < m; ++t) sum = __dadd_rn(sum, s_err[t]);
    }
    __syncthreads();
  }
  if (tid == 0) { s.stat[QP_STAT_L] = L; s.stat[QP_STAT_LOSS] = sum; }
}

void launch_qp_pass(const QpDev& q, const QpSolveDev& s, const int* noneg, int p, int n, hipStream_t st) {
  hipLaunchKernelGGL(k_qp_pass, dim3(1), dim3(QPS_NT), qp_pass_lds(q.nbmax), st, q, s, noneg, p, n);
}

// ---- w(noneg) = max(w(noneg), 0), then w'w: the block sum over the whole of w (64 lane-strided partials, folded) -------------------
__global__ void __launch_bounds__(256) k_qp_clamp_norm(QpSolveDev s, const int* noneg, int p, int len) {
  qp_clamp(s.w, noneg, p);
  __syncthreads();
  if (threadIdx.x < 64) {
    double v = 0.0;
    for (int e = threadIdx.x; e < len; e += 64) v = __dadd_rn(v, __dmul_rn(s.w[e], s.w[e]));
    v = qp_fold(v);
    if (threadIdx.x == 0) s.stat[QP_STAT_WW] = v;
  }
}

void launch_qp_clamp_norm(const QpSolveDev& s, const int* noneg, int p, int len, hipStream_t st) {
  hipLaunchKernelGGL(k_qp_clamp_norm, dim3(1), dim3(256), 0, st, s, noneg, p, len);
}

// ---- qp_w.m: w ./ wreg + w0 ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_qp_weights(const double* __restrict__ w, const double* __restrict__ wreg,
                                                    const double* __restrict__ w0, int len, double* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < len) out[e] = __dadd_rn(__ddiv_rn(w[e], wreg[e]), w0[e]);
}

void launch_qp_weights(const double* w, const double* wreg, const double* w0, int len, double* out, hipStream_t st) {
  hipLaunchKernelGGL(k_qp_weights, dim3((len + 255) / 256), dim3(256), 0, st, w, wreg, w0, len, out);
}
