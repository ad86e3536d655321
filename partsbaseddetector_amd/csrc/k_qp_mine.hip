// k_qp_mine.hip — hard-negative mining (include/pbd_c.h "hard-negative mining"): what stands between a frame's final records, left on
// the device by the back-tracking or the candidate filter, and k_qp_write.  gfx950 only.
//
// k_qp_mine_key / k_qp_mine_rank (RAW records only): the back-tracking appends its records in arrival order; the plain entries sort them
//   on the host by (level, component, root row, root column).  Here every record gets that key in 64 bits and its rank — the number
//   of smaller keys, counted against tiles of 256 keys staged in LDS — and perm[rank] = record.  Keys are distinct (one record per
//   root cell of a (level, component)); equal keys would still land in distinct slots, by record position.  Filtered records are in
//   their final order already: the scan writes their perm.
// k_qp_mine_scan: one workgroup per frame, one pass over the frame's `count` small records.  Every thread validates records with the
//   checks pbd_qp_write makes on the host (pbd_i_fv_check's ranges through featvec_gather.hpp, the column length, qp_write.m:34-35's
//   repeated dense start) and the workgroup keeps the smallest bad position; then its first wavefront sums the frame's terms
//   cneg * max(1 + score, 0) in the library's block-sum order (64 lane-strided partials in record order, qp_fold).  The answer — count,
//   first bad record, S — goes straight into a pinned block; no record crosses.
// Products and sums are explicit __dmul_rn / __dadd_rn: nothing is fused; no sum uses an atomic.
#include "pbd_internal.hpp"
#include "featvec_gather.hpp"
#include "qp_record_check.hpp"
#include "qp_fold.hpp"

#define QM_NT 256

__device__ __forceinline__ int mine_n(const RecordSet& in) {   // RAW: the records the back-tracking wrote
  const int c = *in.count;
  return c < in.capacity ? c : in.capacity;
}

__global__ void __launch_bounds__(QM_NT) k_qp_mine_key(MineArgs a) {
  const int n = mine_n(a.in);
  for (int i = blockIdx.x * QM_NT + threadIdx.x; i < n; i += gridDim.x * QM_NT) {
    const char* rec = a.in.p + a.in.stride * (size_t)i;
    const pbd_candidate_head* hd = (const pbd_candidate_head*)rec;
    const int* lc = (const int*)(hd + 1) + (size_t)a.in.mp * 4;
    a.key[i] = ((unsigned long long)(unsigned)(hd->level & 0xffff) << 48) | ((unsigned long long)(unsigned)(hd->component & 0xffff) << 32) |
               ((unsigned long long)(unsigned)(lc[1] & 0xffff) << 16) | (unsigned long long)(unsigned)(lc[0] & 0xffff);
  }
}

__global__ void __launch_bounds__(QM_NT) k_qp_mine_rank(MineArgs a) {
  __shared__ unsigned long long s_key[QM_NT];
  const int n = mine_n(a.in);
  for (int i0 = blockIdx.x * QM_NT; i0 < n; i0 += gridDim.x * QM_NT) {   // (uniform over the block)
    const int i = i0 + threadIdx.x;
    const unsigned long long mine = i < n ? a.key[i] : 0ull;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += QM_NT) {
      __syncthreads();
      s_key[threadIdx.x] = j0 + threadIdx.x < n ? a.key[j0 + threadIdx.x] : ~0ull;
      __syncthreads();
      const int m = n - j0 < QM_NT ? n - j0 : QM_NT;
      for (int t = 0; t < m; ++t) {   // (every lane reads the same word: a broadcast)
        const unsigned long long o = s_key[t];
        rank += o < mine || (o == mine && j0 + t < i);
      }
    }
    if (i < n) a.perm[rank] = i;
  }
}

void launch_qp_mine_order(const MineArgs& a, hipStream_t s) {
  const int cap = a.in.capacity, nb = (cap + QM_NT - 1) / QM_NT;
  hipLaunchKernelGGL(k_qp_mine_key, dim3(nb < 1024 ? nb : 1024), dim3(QM_NT), 0, s, a);
  hipLaunchKernelGGL(k_qp_mine_rank, dim3(nb < 2048 ? nb : 2048), dim3(QM_NT), 0, s, a);
}

// what pbd_qp_write refuses a record for: MINE_OK, or the first reason in its order of checks (qp_record_check.hpp)
__device__ __forceinline__ int mine_check(const MineArgs& a, const pbd_candidate_head* hd, const int* lc) {
  return qp_record_check(a.fv, a.k, a.noshare, hd, lc);
}

__global__ void __launch_bounds__(QM_NT) k_qp_mine_scan(MineArgs a) {
  __shared__ int s_span[2], s_bad;
  const RecordSet& in = a.in;
  const int f = blockIdx.x, B = a.nframes;
  const int raw = in.cf ? in.cf[0] : *in.count;
  MineFrameOut* out = a.out + f;
  if (raw > in.capacity) {   // the back-tracking overflowed: nothing behind it is complete (uniform over the block)
    if (threadIdx.x == 0) { out->count = 0; out->bad = -1; out->code = MINE_OK; out->raw = raw; out->S = 0.0; }
    return;
  }
  if (threadIdx.x == 0) {
    int start = 0, cnt = 0;
    if (in.cf) {   // the filter's final order: frame f's kept records at [cf[2 + B + f], + cf[2 + f])
      for (int g = 0; g < f; ++g) start += in.cf[2 + g];
      cnt = in.cf[2 + f];
    } else if (in.nlevels == 0 || B == 1) {
      cnt = raw;
    } else {       // perm is sorted by key, the (virtual) level first: the frame's records are a run of it
      int lo[2];
      for (int e = 0; e < 2; ++e) {
        const int lim = (f + e) * in.nlevels;
        int l = 0, h = raw;
        while (l < h) {
          const int m = (l + h) >> 1;
          if (((const pbd_candidate_head*)(in.p + in.stride * (size_t)a.perm[m]))->level < lim) l = m + 1; else h = m;
        }
        lo[e] = l;
      }
      start = lo[0]; cnt = lo[1] - lo[0];
    }
    s_span[0] = start; s_span[1] = cnt; s_bad = 0x7fffffff;
  }
  __syncthreads();
  const int start = s_span[0], cnt = s_span[1];
  if (in.cf) {
    const int src = in.cf[2 + B + f];
    for (int j = threadIdx.x; j < cnt; j += QM_NT) a.perm[start + j] = src + j;
    __syncthreads();   // (a thread reads the entries other threads wrote below; block scope: the stores are visible behind the barrier)
  }
  int bad = 0x7fffffff;
  for (int j = threadIdx.x; j < cnt; j += QM_NT) {
    const pbd_candidate_head* hd = (const pbd_candidate_head*)(in.p + in.stride * (size_t)a.perm[start + j]);
    const int code = mine_check(a, hd, (const int*)(hd + 1) + (size_t)in.mp * 4);
    if (code != MINE_OK) { bad = j * 4 + code; break; }   // (a thread's positions ascend: its first bad one is its smallest)
  }
  if (bad != 0x7fffffff) atomicMin(&s_bad, bad);   // an integer minimum, order-free
  if (threadIdx.x < 64) {   // the block sum over the frame's records in record order
    const int lane = threadIdx.x;
    double s = 0.0;
    int j = lane;
    for (; j + 192 < cnt; j += 256) {   // four loads in flight; the add chain keeps its order
      float sc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) sc[u] = ((const pbd_candidate_head*)(in.p + in.stride * (size_t)a.perm[start + j + 64 * u]))->score;
#pragma unroll
      for (int u = 0; u < 4; ++u) s = __dadd_rn(s, __dmul_rn(a.cneg, fmax(__dadd_rn(1.0, (double)sc[u]), 0.0)));
    }
    for (; j < cnt; j += 64) {
      const float sc = ((const pbd_candidate_head*)(in.p + in.stride * (size_t)a.perm[start + j]))->score;
      s = __dadd_rn(s, __dmul_rn(a.cneg, fmax(__dadd_rn(1.0, (double)sc), 0.0)));
    }
    s = qp_fold(s);
    if (lane == 0) out->S = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int b = s_bad;
    out->count = cnt; out->raw = raw;
    out->bad = b == 0x7fffffff ? -1 : b >> 2;
    out->code = b == 0x7fffffff ? MINE_OK : b & 3;
  }
}

void launch_qp_mine_scan(const MineArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_qp_mine_scan, dim3(a.nframes), dim3(QM_NT), 0, s, a);
}
