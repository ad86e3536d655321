// k_eval.hip — the evaluation ledger (include/pbd_c.h "evaluation ledger"): matlab/evaluation/eval_pck.m, eval_apk.m and VOCap.m on
// records that stay on the device.  gfx950 only; the arithmetic is eval_core.hpp's, shared with the host functions.
//
// Adds
//   k_eval_span      whole-path APK frames, one workgroup per frame: where the frame's final records are in mining's order (perm): a
//                    run of the sorted RAW records, or the candidate filter's kept records, whose perm it writes.  {count, start, raw}
//                    goes into a pinned block; the host turns the counts into append positions — no atomics anywhere.
//   k_eval_pck_add   one thread per (person, keypoint): the distance of the person's selected pose, +Inf without one.
//   k_eval_order     per frame, the rank of every detection by (score descending, position ascending), counted against tiles of
//                    PBD_EVAL_ORDER_TILE keys staged in LDS: ord[rank] = position.
//   k_eval_match     one wavefront per (frame, keypoint), lane g holding person g: the frame's detections in ord's order, per detection
//                    a wave minimum of q = d / scale as ordered bits (q >= +0, so the bits order as the values), the first lane of the
//                    minimum by ballot, the taken flags in one 64-bit mask.  Writes the row's tp byte (and, for keypoint 0, its score).
// Results
//   k_eval_pck       one workgroup per keypoint: integer hit count, one division.
//   k_eval_keys, k_eval_sort_local / _global / _merge: a bitonic sort of the 64-bit keys (~score key, sequence) — unique, so the result
//                    is the one permutation —, in LDS tiles of PBD_EVAL_SORT_TILE keys, in device memory for longer distances.
//   k_eval_apk       one workgroup per keypoint: inclusive scan of tp in sorted order, suffix maximum of the precision from the back,
//                    then the first wavefront sums VOCap's terms in the library's block-sum order (64 lane-strided partials, qp_fold).
//   k_eval_curves    prec / rec of every (keypoint, rank), on request.
// Plain C++ and vector stores only; every sum that is not an integer count has one fixed order.
#include "pbd_internal.hpp"
#include "eval_core.hpp"
#include "qp_fold.hpp"

#define EV_NT 256
#define EV_ST (PBD_EVAL_SORT_TILE / 2)   // threads of a sort workgroup: one compare-exchange each per step

// ---- whole-path APK frames: the spans of the frames in mining's order ---------------------------------------------------------------
__global__ void __launch_bounds__(EV_NT) k_eval_span(EvalSpanArgs a) {
  __shared__ int s_span[2];
  const RecordSet& in = a.in;
  const int f = blockIdx.x, B = a.nframes;
  const int raw = in.cf ? in.cf[0] : *in.count;
  EvalFrameOut* out = a.out + f;
  if (raw > in.capacity || raw < 0) {   // the back-tracking overflowed: nothing behind it is complete (uniform over the block)
    if (threadIdx.x == 0) { out->count = 0; out->start = 0; out->raw = raw; out->reserved = 0; }
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
    if (cnt < 0) cnt = 0;
    if (start + cnt > in.capacity) cnt = in.capacity - start > 0 ? in.capacity - start : 0;   // (a filter's counts never exceed it; stay inside perm)
    s_span[0] = start; s_span[1] = cnt;
    out->count = cnt; out->start = start; out->raw = raw; out->reserved = 0;
  }
  __syncthreads();
  if (in.cf) {
    const int start = s_span[0], cnt = s_span[1], src = in.cf[2 + B + f];
    for (int j = threadIdx.x; j < cnt; j += EV_NT) a.perm[start + j] = src + j;
  }
}
void launch_eval_span(const EvalSpanArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_eval_span, dim3(a.nframes), dim3(EV_NT), 0, s, a);
}

// ---- PCK: the instance columns ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(EV_NT) k_eval_pck_add(EvalPckAddArgs a) {
  const EvalFrame fr = a.frames[blockIdx.x];
  const int P = a.L.P;
  for (int t = threadIdx.x; t < fr.ngt * P; t += EV_NT) {
    const int g = t / P, p = t - g * P;
    const size_t slot = (size_t)blockIdx.x * a.slots + g, person = (size_t)fr.goff + g, inst = (size_t)a.n0 + person;
    if (inst >= (size_t)a.L.ncap) continue;   // (the host checked the capacity)
    double d = INFINITY;                      // no pose: the instance misses every keypoint and stays in the denominator
    if (a.found[slot]) {
      const int32_t* b = (const int32_t*)(a.rec + a.stride * slot + sizeof(pbd_candidate_head)) + p * 4;
      double cx, cy;
      eval_keypoint(b, &cx, &cy);
      d = eval_dist(cx, cy, a.points[(person * P + p) * 2], a.points[(person * P + p) * 2 + 1]);
    }
    a.L.dist[inst * P + p] = d;
    if (p == 0) a.L.scale[inst] = a.scale[person];
  }
}
void launch_eval_pck_add(const EvalPckAddArgs& a, int nframes, hipStream_t s) {
  if (nframes > 0) hipLaunchKernelGGL(k_eval_pck_add, dim3(nframes), dim3(EV_NT), 0, s, a);
}

// ---- APK: a frame's order and its matching ---------------------------------------------------------------------------------------
__device__ __forceinline__ const char* ev_record(const EvalApkAddArgs& a, const EvalFrame& fr, int j) {
  const int r = a.perm ? a.perm[fr.start + j] : fr.start + j;
  return a.rec + a.stride * (size_t)r;
}

__global__ void __launch_bounds__(PBD_EVAL_ORDER_TILE) k_eval_order(EvalApkAddArgs a) {
  __shared__ unsigned long long s_key[PBD_EVAL_ORDER_TILE];
  const EvalFrame fr = a.frames[blockIdx.y];
  const int n = fr.count, NT = PBD_EVAL_ORDER_TILE;
  for (int i0 = blockIdx.x * NT; i0 < n; i0 += gridDim.x * NT) {   // (uniform over the block)
    const int i = i0 + threadIdx.x;
    const unsigned long long mine = i < n ? eval_order_key(((const pbd_candidate_head*)ev_record(a, fr, i))->score, (unsigned)i) : 0ull;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += NT) {
      __syncthreads();
      const int j = j0 + threadIdx.x;
      s_key[threadIdx.x] = j < n ? eval_order_key(((const pbd_candidate_head*)ev_record(a, fr, j))->score, (unsigned)j) : ~0ull;
      __syncthreads();
      const int m = n - j0 < NT ? n - j0 : NT;
      for (int t = 0; t < m; ++t) rank += s_key[t] < mine;   // (every lane reads the same word: a broadcast; keys are distinct)
    }
    if (i < n) a.ord[fr.start + rank] = i;
  }
}

__device__ __forceinline__ unsigned long long ev_wave_min(unsigned long long v) {
#pragma unroll
  for (int h = 32; h >= 1; h >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, h, 64), hi = __shfl_xor((unsigned)(v >> 32), h, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o < v ? o : v;
  }
  return v;
}

__global__ void __launch_bounds__(64) k_eval_match(EvalApkAddArgs a) {
  const EvalFrame fr = a.frames[blockIdx.y];
  const int p = blockIdx.x, P = a.L.P, lane = threadIdx.x;
  const bool has = lane < fr.ngt;
  double gx = 0.0, gy = 0.0, sc = 1.0;
  if (has) {
    const size_t person = (size_t)fr.goff + lane;
    gx = a.points[(person * P + p) * 2]; gy = a.points[(person * P + p) * 2 + 1];
    sc = a.scale[person];
  }
  unsigned long long taken = 0ull;
  for (int r = 0; r < fr.count; ++r) {
    const int j = a.ord[fr.start + r];
    const size_t row = (size_t)a.m0 + fr.start + j;
    if (j < 0 || j >= fr.count || row >= (size_t)a.L.mcap) continue;   // (uniform; the host checked the capacity)
    const char* rec = ev_record(a, fr, j);
    int tp = 0;
    if (fr.ngt > 0) {
      double cx, cy;
      eval_keypoint((const int32_t*)(rec + sizeof(pbd_candidate_head)) + p * 4, &cx, &cy);
      const double q = eval_dist(cx, cy, gx, gy) / sc;
      const unsigned long long bits = has ? (unsigned long long)__double_as_longlong(q) : ~0ull;   // q >= +0 or +Inf: ordered as unsigned bits
      const unsigned long long mn = ev_wave_min(bits);
      const unsigned long long at = __ballot(has && bits == mn);
      const int jmin = at ? __ffsll((unsigned long long)at) - 1 : 0;
      tp = eval_match_decide(__longlong_as_double((long long)mn), jmin, a.thresh, &taken);
    }
    if (lane == 0) {
      a.L.tp[row * P + p] = (unsigned char)tp;
      if (p == 0) a.L.score[row] = ((const pbd_candidate_head*)rec)->score;
    }
  }
}

void launch_eval_apk_add(const EvalApkAddArgs& a, int nframes, int maxcount, hipStream_t s) {
  if (nframes <= 0 || maxcount <= 0) return;
  const int nb = (maxcount + PBD_EVAL_ORDER_TILE - 1) / PBD_EVAL_ORDER_TILE;
  hipLaunchKernelGGL(k_eval_order, dim3(nb < 64 ? nb : 64, nframes), dim3(PBD_EVAL_ORDER_TILE), 0, s, a);
  hipLaunchKernelGGL(k_eval_match, dim3(a.L.P, nframes), dim3(64), 0, s, a);
}

// ---- PCK result ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(EV_NT) k_eval_pck(EvalResultArgs a) {
  __shared__ int s_hit[EV_NT];
  const int p = blockIdx.x, P = a.L.P, n = a.n;
  int hits = 0;
  for (int i = threadIdx.x; i < n; i += EV_NT)
    hits += eval_pck_hit(a.L.dist[(size_t)i * P + p], a.thresh, a.L.scale[a.rule == PBD_EVAL_SCALE_LAST ? n - 1 : i]);
  s_hit[threadIdx.x] = hits;
  __syncthreads();
  for (int h = EV_NT / 2; h > 0; h >>= 1) {   // (integers: any order gives the count)
    if ((int)threadIdx.x < h) s_hit[threadIdx.x] += s_hit[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.out[p] = (double)s_hit[0] / (double)n;   // n == 0: 0 / 0 = NaN
}
void launch_eval_pck(const EvalResultArgs& a, hipStream_t s) {
  if (a.L.P > 0) hipLaunchKernelGGL(k_eval_pck, dim3(a.L.P), dim3(EV_NT), 0, s, a);
}

// ---- APK result: the global order -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(EV_NT) k_eval_keys(EvalResultArgs a) {
  for (int i = blockIdx.x * EV_NT + threadIdx.x; i < a.n2; i += gridDim.x * EV_NT)
    a.key[i] = i < a.m ? eval_order_key(a.L.score[i], (unsigned)i) : ~0ull;   // (the padding sorts behind every detection)
}

// pair t of a step with distance j: elements i and i | j, i having bit j clear
__device__ __forceinline__ void ev_cmpx(unsigned long long* k, unsigned base, unsigned t, unsigned j, unsigned kk) {
  const unsigned i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
  const bool up = ((base + i) & kk) == 0;
  const unsigned long long x = k[i], y = k[l];
  if ((x > y) == up) { k[i] = y; k[l] = x; }
}
// every tile ordered in LDS: the stages kk = 2 .. PBD_EVAL_SORT_TILE
__global__ void __launch_bounds__(EV_ST) k_eval_sort_local(EvalResultArgs a) {
  __shared__ unsigned long long s_k[PBD_EVAL_SORT_TILE];
  const unsigned base = blockIdx.x * PBD_EVAL_SORT_TILE, t = threadIdx.x;
  s_k[t] = a.key[base + t]; s_k[t + EV_ST] = a.key[base + t + EV_ST];
  for (unsigned kk = 2; kk <= PBD_EVAL_SORT_TILE; kk <<= 1)
    for (unsigned j = kk >> 1; j > 0; j >>= 1) {
      __syncthreads();
      ev_cmpx(s_k, base, t, j, kk);
    }
  __syncthreads();
  a.key[base + t] = s_k[t]; a.key[base + t + EV_ST] = s_k[t + EV_ST];
}
// one step of stage kk at a distance j >= PBD_EVAL_SORT_TILE, in device memory
__global__ void __launch_bounds__(EV_NT) k_eval_sort_global(EvalResultArgs a, unsigned kk, unsigned j) {
  const unsigned t = blockIdx.x * EV_NT + threadIdx.x;
  if (t < (unsigned)a.n2 / 2) ev_cmpx(a.key, 0u, t, j, kk);
}
// the steps of stage kk at distances below PBD_EVAL_SORT_TILE, in LDS
__global__ void __launch_bounds__(EV_ST) k_eval_sort_merge(EvalResultArgs a, unsigned kk) {
  __shared__ unsigned long long s_k[PBD_EVAL_SORT_TILE];
  const unsigned base = blockIdx.x * PBD_EVAL_SORT_TILE, t = threadIdx.x;
  s_k[t] = a.key[base + t]; s_k[t + EV_ST] = a.key[base + t + EV_ST];
  for (unsigned j = PBD_EVAL_SORT_TILE / 2; j > 0; j >>= 1) {
    __syncthreads();
    ev_cmpx(s_k, base, t, j, kk);
  }
  __syncthreads();
  a.key[base + t] = s_k[t]; a.key[base + t + EV_ST] = s_k[t + EV_ST];
}

// ---- APK result: per keypoint, over the sorted detections --------------------------------------------------------------------------
__global__ void __launch_bounds__(EV_NT) k_eval_apk(EvalResultArgs a) {
  __shared__ int s_i[EV_NT];
  __shared__ double s_d[EV_NT];
  const int p = blockIdx.x, P = a.L.P, m = a.m, t = threadIdx.x;
  int* tpc = a.tpc + (size_t)p * a.L.mcap;
  double* sm = a.sm + (size_t)p * a.L.mcap;
  // tpc = cumsum(tp) in sorted order (eval_apk.m:38-39): chunks of EV_NT, an inclusive scan each, the carry in front
  int carry = 0;
  for (int base = 0; base < m; base += EV_NT) {
    const int i = base + t;
    int v = 0;
    if (i < m) v = a.L.tp[(size_t)(unsigned)(a.key[i] & 0xffffffffu) * P + p] != 0;
    s_i[t] = v;
    __syncthreads();
    for (int h = 1; h < EV_NT; h <<= 1) {
      const int o = t >= h ? s_i[t - h] : 0;
      __syncthreads();
      s_i[t] += o;
      __syncthreads();
    }
    if (i < m) tpc[i] = carry + s_i[t];
    carry += s_i[EV_NT - 1];
    __syncthreads();
  }
  __threadfence_block();
  __syncthreads();
  // mpre's suffix maximum (VOCap.m:4-6), from the last chunk to the first; 0 is mpre's closing element and the identity (prec >= 0)
  double cmax = 0.0;
  for (int base = ((m - 1) / EV_NT) * EV_NT; m > 0 && base >= 0; base -= EV_NT) {
    const int i = base + t;
    s_d[t] = i < m ? eval_prec(tpc[i], i) : 0.0;
    __syncthreads();
    for (int h = 1; h < EV_NT; h <<= 1) {
      const double o = t + h < EV_NT ? s_d[t + h] : 0.0;
      __syncthreads();
      s_d[t] = o > s_d[t] ? o : s_d[t];
      __syncthreads();
    }
    if (i < m) sm[i] = cmax > s_d[t] ? cmax : s_d[t];
    const double top = s_d[0];
    cmax = top > cmax ? top : cmax;
    __syncthreads();
  }
  __threadfence_block();
  __syncthreads();
  // ap = sum_k (mrec(k+1) - mrec(k)) * mpre(k+1), k = 0 .. m, in the block-sum order: lane t takes k = t, t + 64, ...
  if (t < 64) {
    double s = 0.0;
    for (int k = t; k <= m; k += 64) {
      const double prev = k > 0 ? eval_rec(tpc[k - 1], a.npos) : 0.0;
      const double term = k < m ? eval_ap_term(prev, eval_rec(tpc[k], a.npos), sm[k]) : eval_ap_term(prev, 1.0, 0.0);
      s = __dadd_rn(s, term);
    }
    s = qp_fold(s);
    if (t == 0) a.out[p] = s;
  }
}

__global__ void __launch_bounds__(EV_NT) k_eval_curves(EvalResultArgs a) {
  const int p = blockIdx.y;
  const int* tpc = a.tpc + (size_t)p * a.L.mcap;
  for (int i = blockIdx.x * EV_NT + threadIdx.x; i < a.m; i += gridDim.x * EV_NT) {
    if (a.prec) a.prec[(size_t)p * a.m + i] = eval_prec(tpc[i], i);
    if (a.rec) a.rec[(size_t)p * a.m + i] = eval_rec(tpc[i], a.npos);
  }
}

void launch_eval_apk(const EvalResultArgs& a, hipStream_t s) {
  if (a.L.P <= 0) return;
  if (a.m > 0) {
    const unsigned n2 = (unsigned)a.n2, T = PBD_EVAL_SORT_TILE;
    const int kb = (int)((n2 + EV_NT - 1) / EV_NT);
    hipLaunchKernelGGL(k_eval_keys, dim3(kb < 1024 ? kb : 1024), dim3(EV_NT), 0, s, a);
    hipLaunchKernelGGL(k_eval_sort_local, dim3(n2 / T), dim3(EV_ST), 0, s, a);
    for (unsigned kk = 2 * T; kk <= n2 && kk != 0; kk <<= 1) {
      for (unsigned j = kk >> 1; j >= T; j >>= 1)
        hipLaunchKernelGGL(k_eval_sort_global, dim3((n2 / 2 + EV_NT - 1) / EV_NT), dim3(EV_NT), 0, s, a, kk, j);
      hipLaunchKernelGGL(k_eval_sort_merge, dim3(n2 / T), dim3(EV_ST), 0, s, a, kk);
    }
  }
  hipLaunchKernelGGL(k_eval_apk, dim3(a.L.P), dim3(EV_NT), 0, s, a);
  if (a.m > 0 && (a.prec || a.rec)) {
    const int cb = (a.m + EV_NT - 1) / EV_NT;
    hipLaunchKernelGGL(k_eval_curves, dim3(cb < 1024 ? cb : 1024, a.L.P), dim3(EV_NT), 0, s, a);
  }
}
