// k_qp.hip — the training example cache (include/pbd_c.h "training example cache"): qp_write.m, matlab/mex/score.cc and
// matlab/mex/lincomb.cc on the device.  gfx950 only.
//
// k_qp_write: one workgroup per record.  The gather is k_featvec's (featvec_gather.hpp); a part's blocks are standardised by ONE
//   wavefront and go straight into the example's column — lane-consecutive elements, so the plane reads (a cell is flen contiguous
//   values) and the column stores coalesce; no unscaled window is staged in HBM.  The sums behind d and b follow the order the header
//   states: per block 64 lane-strided partials and a halving fold, then the blocks in block order by one thread.  Nothing of that
//   depends on the grid: a record's bits are the same wherever it lands.
//   The records are the call's uploaded ones (pbd_qp_write) or a mining frame's, read where the back-tracking or the candidate filter
//   left them, through the order k_qp_mine.hip made (QpWriteArgs::perm, ::ids): one text for both.
// k_qp_poswrite: a warped positive (k_warp.hip's window through k_hog) as a two-block column, one wavefront per example.
// k_qp_score: one lane owns one example's serial add chain (score.cc's order); a wavefront stages its 64 columns through LDS in
//   chunks with coalesced loads and each lane walks its own row (pitch 65: no bank conflict).  w is read through L2.
// k_qp_lincomb: one thread per dense element walks inds in order; the per-example block table (written with the column) tells it
//   whether and where the example holds that element — the table reads are uniform over the wavefront.  lincomb.cc's order, no atomics.
// Products and sums are explicit __dmul_rn / __dadd_rn: nothing is fused.
#include "pbd_internal.hpp"
#include "featvec_gather.hpp"
#include "qp_fold.hpp"

#define QW_NT 256
#define QW_WAVES (QW_NT / 64)
#define QS_CH 64          // column elements a score wavefront stages per round
#define QL_NT 256

// one block of the column by one wavefront: header, values, table entry and its two sums.  val(e): element e's value, double, unsigned
template <typename A, typename F>
__device__ __forceinline__ void qp_block(const A& a, float* col, int* tab, double* s_sum, int bi, int o, int start, int n,
                                         bool neg, F val) {
  const int lane = threadIdx.x & 63;
  double sd = 0.0, sb = 0.0;
  for (int e = lane; e < n; e += 64) {
    double v = val(e);
    if (neg) v = -v;
    const double xs = __ddiv_rn(__dmul_rn(a.C, v), a.wreg[start + e]);
    col[o + 2 + e] = (float)xs;
    sd = __dadd_rn(sd, __dmul_rn(xs, xs));
    sb = __dadd_rn(sb, __dmul_rn(a.w0[start + e], v));
  }
  sd = qp_fold(sd); sb = qp_fold(sb);
  if (lane == 0) {
    col[o] = (float)(start + 1); col[o + 1] = (float)(start + n);
    tab[bi * 3] = start; tab[bi * 3 + 1] = n; tab[bi * 3 + 2] = o + 2;
    s_sum[bi * 2] = sd; s_sum[bi * 2 + 1] = sb;
  }
}

// the column's block count, d and b from its blocks' sums, in block order, by one thread
__device__ __forceinline__ void qp_column_sums(const QpDev& q, float* col, int col_i, int nb, const double* s_sum, double C) {
  double d = 0.0, bias = 1.0;
  for (int bi = 0; bi < nb; ++bi) { d = __dadd_rn(d, s_sum[bi * 2]); bias = __dsub_rn(bias, s_sum[bi * 2 + 1]); }
  col[0] = (float)nb;
  q.nblk[col_i] = nb;
  q.d[col_i] = d;
  q.b[col_i] = (float)__dmul_rn(C, bias);
}

template <typename T>
__global__ void __launch_bounds__(QW_NT) k_qp_write(QpWriteArgs a) {
  extern __shared__ double s_sum[];             // [3 mp][2]: a block's sums for d and b
  const FeatVecArgs& fv = a.fv;
  const int mp = fv.in.mp, wave = threadIdx.x >> 6, k = a.q.k;
  int* s_loc = (int*)(s_sum + (size_t)mp * 6);  // [mp][3]
  int* s_off = s_loc + (size_t)mp * 3;          // [mp + 1] first column element of each part's blocks; [np]: the used length
  int* s_bad = s_off + mp + 1;
  const T* feat = (const T*)fv.feat;
  for (int r = blockIdx.x; r < fv.n; r += gridDim.x) {
    const char* rec = fv.in.p + fv.in.stride * (size_t)(a.perm ? a.perm[fv.rec0 + r] : fv.rec0 + r);
    const pbd_candidate_head* hd = (const pbd_candidate_head*)rec;
    const int c = hd->component, lvl = hd->level, np = hd->nparts;
    const bool rec_ok = fv_rec_ok(fv, hd);
    const int* lc = (const int*)(hd + 1) + (size_t)mp * 4;
    if (rec_ok) for (int t = threadIdx.x; t < np * 3; t += QW_NT) s_loc[t] = lc[t];
    if (threadIdx.x == 0) *s_bad = rec_ok ? 0 : 1;
    __syncthreads();
    if (rec_ok) for (int p = threadIdx.x; p < np; p += QW_NT) {
      const FvPart P = fv_part(fv, true, c, lvl, np, s_loc, p);
      s_off[p] = P.ok ? P.kh * P.kw * PBD_FLEN : -1;   // (the window's length for now)
    }
    __syncthreads();
    if (threadIdx.x == 0 && rec_ok) {
      int off = 1;
      for (int p = 0; p < np; ++p) {
        const int wl = s_off[p];
        if (wl < 0) *s_bad = 1;
        s_off[p] = off;
        off += (p == 0 ? 3 : 9) + 2 + (wl < 0 ? 0 : wl);
        if (off > k) { *s_bad = 1; break; }
      }
      s_off[np] = off;
    }
    __syncthreads();
    const bool bad = *s_bad != 0;
    const int col_i = a.q.slot[a.n0 + r];
    float* col = a.q.x + (size_t)k * col_i;
    int* tab = a.q.tab + (size_t)col_i * a.q.nbmax * 3;
    const bool neg = a.label <= 0;
    const int nb = bad ? 0 : 3 * np - 1, used = bad ? 1 : s_off[np];
    if (!bad)
      for (int p = wave; p < np; p += QW_WAVES) {   // (uniform over the wavefront)
        const FvPart P = fv_part(fv, true, c, lvl, np, s_loc, p);
        const int o = s_off[p], bi = p == 0 ? 0 : 3 * p - 1;
        qp_block(a, col, tab, s_sum, bi, o, P.bias_id, 1, neg, [](int) { return 1.0; });
        int ow = o + 3, bw = bi + 1;
        if (p > 0) {
          qp_block(a, col, tab, s_sum, bi + 1, o + 3, fv.nbias + 4 * P.def_id, 4, neg,
                   [&](int e) { return (double)(e == 0 ? P.d0 : e == 1 ? P.d1 : e == 2 ? P.d2 : P.d3); });
          ow = o + 9; bw = bi + 2;
        }
        qp_block(a, col, tab, s_sum, bw, ow, a.foff[P.filter_id], P.kh * P.kw * PBD_FLEN, neg, [&](int e) {
          size_t pc;
          const int ch = e & (PBD_FLEN - 1);
          if (fv_cell(P, e / PBD_FLEN, &pc)) return (double)feat[pc * PBD_FLEN + ch];
          return ch == PBD_FLEN - 1 ? 1.0 : 0.0;   // the bank's border
        });
      }
    for (int t = used + threadIdx.x; t < k; t += QW_NT) col[t] = 0.f;   // qp_write.m:46, the tail
    __syncthreads();
    if (threadIdx.x == 0) qp_column_sums(a.q, col, col_i, nb, s_sum, a.C);
    if (threadIdx.x < 5) {
      const int t = threadIdx.x;
      const int frame = a.nlevels ? lvl / a.nlevels : 0;   // (a mining batch: the frame's id, the frame's own level)
      a.q.ids[(size_t)col_i * 5 + t] = t == 0 ? a.label : t == 1 ? (a.ids ? a.ids[frame] : a.id) : t == 2 ? lvl - frame * a.nlevels : t == 3 ? lc[0] : lc[1];
    }
    __syncthreads();   // the LDS tables are rewritten by the block's next record
  }
}

void launch_qp_write(const QpWriteArgs& a, int ts, hipStream_t s) {
  const int mp = a.fv.in.mp, nb = a.fv.n < 65536 ? (a.fv.n > 0 ? a.fv.n : 1) : 65536;
  const size_t lds = sizeof(double) * 6 * (size_t)mp + sizeof(int) * (4 * (size_t)mp + 2);   // <= 16.4 KB (256 parts)
  if (ts == 8) hipLaunchKernelGGL(k_qp_write<double>, dim3(nb), dim3(QW_NT), lds, s, a);
  else hipLaunchKernelGGL(k_qp_write<float>, dim3(nb), dim3(QW_NT), lds, s, a);
}

// ---- qp_poswrite (train.m:152-161): a warped positive's column — the bias block [1], then its HOG window — from the feature buffer
// the warp left on the device.  One wavefront per example; the blocks, their sums and the column's d and b are k_qp_write's text.
template <typename T>
__global__ void __launch_bounds__(64) k_qp_poswrite(QpPosArgs a) {
  __shared__ double s_sum[4];
  const int r = blockIdx.x, lane = threadIdx.x, k = a.q.k;
  const int col_i = a.q.slot[a.n0 + r];
  float* col = a.q.x + (size_t)k * col_i;
  int* tab = a.q.tab + (size_t)col_i * a.q.nbmax * 3;
  const T* feat = (const T*)a.feat + (size_t)r * a.wlen;
  qp_block(a, col, tab, s_sum, 0, 1, a.bias_start, 1, false, [](int) { return 1.0; });
  qp_block(a, col, tab, s_sum, 1, 4, a.filt_start, a.wlen, false, [&](int e) { return (double)feat[e]; });
  for (int t = 6 + a.wlen + lane; t < k; t += 64) col[t] = 0.f;
  __syncthreads();
  if (lane == 0) qp_column_sums(a.q, col, col_i, 2, s_sum, a.C);
  if (lane < 5) a.q.ids[(size_t)col_i * 5 + lane] = lane == 0 ? 1 : lane == 1 ? a.ids[r] : 0;
}

void launch_qp_poswrite(const QpPosArgs& a, int ts, hipStream_t s) {
  if (a.n <= 0) return;
  if (ts == 8) hipLaunchKernelGGL(k_qp_poswrite<double>, dim3(a.n), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(k_qp_poswrite<float>, dim3(a.n), dim3(64), 0, s, a);
}

// ---- score.cc ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_qp_score(QpDev q, const double* __restrict__ W, const int* __restrict__ inds, int n,
                                                 double* __restrict__ out) {
  __shared__ float s[64][QS_CH + 1];
  const int lane = threadIdx.x, i = blockIdx.x * 64 + lane, k = q.k;
  const bool valid = i < n;
  const int col = valid ? q.slot[inds ? inds[i] : i] : -1;
  bool done = !valid;
  int nbl = 0, phase = 0, rem = 0, wp = 0;
  double y = 0.0;
  for (int c0 = 0; c0 < k; c0 += QS_CH) {
    if (!__any(!done)) break;
    for (int r = 0; r < 64; ++r) {                 // the 64 columns' next chunk, a coalesced row each
      const int cr = __shfl(done ? -1 : col, r, 64);
      if (cr >= 0) s[r][lane] = c0 + lane < k ? q.x[(size_t)k * cr + c0 + lane] : 0.f;
    }
    __syncthreads();
    if (!done) {
      const float* row = s[lane];
      const int lim = k - c0 < QS_CH ? k - c0 : QS_CH;
      int t = 0;
      if (c0 == 0) { nbl = (int)row[0]; t = 1; done = nbl <= 0; }
      while (t < lim && !done) {
        if (phase == 0) { wp = (int)row[t++] - 1; phase = 1; }
        else if (phase == 1) { rem = (int)row[t++] - wp; phase = 2; if (rem <= 0) { phase = 0; done = --nbl == 0; } }
        else {
          const int m = rem < lim - t ? rem : lim - t;
          int u = 0;
          for (; u + 8 <= m; u += 8) {             // eight loads of w in flight; the add chain keeps its order
            double wv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) wv[j] = W[wp + u + j];
#pragma unroll
            for (int j = 0; j < 8; ++j) y = __dadd_rn(y, __dmul_rn(wv[j], (double)row[t + u + j]));
          }
          for (; u < m; ++u) y = __dadd_rn(y, __dmul_rn(W[wp + u], (double)row[t + u]));
          wp += m; t += m; rem -= m;
          if (rem == 0) { phase = 0; done = --nbl == 0; }
        }
      }
    }
    __syncthreads();
  }
  if (valid) out[i] = y;
}

void launch_qp_score(const QpDev& q, const double* w, const int* inds, int n, double* out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_qp_score, dim3((n + 63) / 64), dim3(64), 0, s, q, w, inds, n, out);
}

// ---- lincomb.cc ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(QL_NT) k_qp_lincomb(QpDev q, const double* __restrict__ A, const int* __restrict__ inds, int n,
                                                      double* __restrict__ out) {
  const int e = blockIdx.x * QL_NT + threadIdx.x;
  double w = 0.0;
  for (int i = 0; i < n; ++i) {                    // (everything but the hit test is uniform over the block)
    const int ex = inds ? inds[i] : i, col = q.slot[ex], nb = q.nblk[col];
    const double a = A[ex];
    const int* tab = q.tab + (size_t)col * q.nbmax * 3;
    const float* x = q.x + (size_t)q.k * col;
    for (int j = 0; j < nb; ++j) {
      const int st = tab[j * 3], ln = tab[j * 3 + 1], xo = tab[j * 3 + 2];
      if ((unsigned)(e - st) < (unsigned)ln) w = __dadd_rn(w, __dmul_rn(a, (double)x[xo + (e - st)]));
    }
  }
  if (e < q.len) out[e] = w;
}

void launch_qp_lincomb(const QpDev& q, const double* a, const int* inds, int n, double* w_out, hipStream_t s) {
  hipLaunchKernelGGL(k_qp_lincomb, dim3((q.len + QL_NT - 1) / QL_NT), dim3(QL_NT), 0, s, q, a, inds, n, w_out);
}
