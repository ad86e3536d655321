// k_cand.hip — Candidate::sort + Candidate::nonMaximaSuppression (include/Candidate.hpp:91-111, 277-304) on the device.
//
// k_cand_filter: one workgroup per frame, after k_backtrack.  The records of frame f (level / nlevels == f) are
//   1. keyed: (score descending, then a tie key ascending) packed into 64 bits.  The tie key is the root's element offset in
//      the handle's root tables (monotone in (virtual level, component, y, x): the order pbd_i_emit gives the host sort) or,
//      for the stand-alone primitive, the input position.  -0.0 and +0.0 get the same key, as `a.score > b.score` has them;
//   2. sorted: bitonic, in LDS when the padded count fits CF_TILE, else tiles in LDS merged in device memory;
//   3. suppressed (mode 2): the host loop keeps candidate n iff (double)painted / (double)area > (double)overlap is false,
//      painted = pixels of n's clipped union box already covered by kept boxes.  Painted only grows, so a candidate that fails
//      against the current mask fails for good; a candidate's painted count only changes when a box that meets it is kept.  A
//      round tests a window of CF_NT undecided candidates against the mask in parallel, rejects the failures, then one
//      wavefront walks the passing ones in order and keeps each whose upper bound min(area, painted + sum of its overlaps with
//      this round's kept boxes) still passes; the first one that may fail ends the round and heads the next window.  The first
//      passing candidate of a window has no round keeps before it, so every round decides at least one candidate exactly;
//   4. written: the kept records in final order at out + start_f * stride (start_f = records of frames < f), and per-frame
//      counts: cnt_out[0] = device count, [1] = frame 0's count (the device count when it overflowed the capacity),
//      [2 + f] = kept in frame f, [2 + nframes + f] = start_f.
// The mask is one bit per pixel, rows of ceil(w / 64) 64-bit words, in LDS when it fits CF_MASK_LDS (640 x 480: 38 400 B),
// else per frame in device memory (1920 x 1080: 259 200 B).
#include "pbd_internal.hpp"

#define CF_NT 1024
#define CF_TILE 4096          // sort entries in LDS: 8 B key + 4 B index
#define CF_MASK_LDS 40960     // bytes
#define CF_KEEPS 512          // kept boxes per round
#define CF_LDS (CF_MASK_LDS + CF_NT * 4 + CF_KEEPS * 16)   // 53 248 B >= CF_TILE * 12

typedef unsigned long long u64;

__device__ __forceinline__ unsigned score_key(float s) {   // ascending key = descending score, -0.0 == +0.0
  unsigned u = __float_as_uint(s);
  if ((u & 0x7fffffffu) == 0) u = 0;
  const unsigned o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~o;
}

__device__ __forceinline__ void cx(u64* K, unsigned* I, int a, int b, bool up) {
  const u64 ka = K[a], kb = K[b];
  if ((ka > kb) == up) { K[a] = kb; K[b] = ka; const unsigned t = I[a]; I[a] = I[b]; I[b] = t; }
}
// one bitonic pass (stage k, distance j) over n entries; `gbase`: index of K[0] in the whole sequence (direction bit)
__device__ __forceinline__ void bpass(u64* K, unsigned* I, int n, int k, int j, int gbase) {
  for (int p = threadIdx.x; p < n / 2; p += CF_NT) {
    const int a = ((p & ~(j - 1)) << 1) | (p & (j - 1));
    cx(K, I, a, a + j, ((gbase + a) & k) == 0);
  }
}

__device__ __forceinline__ long long block_sum(long long v, long long* ws) {   // every thread of the block; returns the total
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  long long t = 0;
  for (int w = 0; w < CF_NT / 64; ++w) t += ws[w];
  return t;
}

struct CfBox { int x0, y0, x1, y1; };

__device__ __forceinline__ int box_count(const u64* M, int wq, CfBox b) {   // set bits of the mask under a non-empty box
  const int w0 = b.x0 >> 6, w1 = (b.x1 - 1) >> 6;
  const u64 m0 = ~0ull << (b.x0 & 63), m1 = ~0ull >> (63 - ((b.x1 - 1) & 63));
  int s = 0;
  for (int y = b.y0; y < b.y1; ++y) {
    const u64* row = M + (size_t)y * wq;
    if (w0 == w1) { s += __popcll(row[w0] & m0 & m1); continue; }
    s += __popcll(row[w0] & m0);
    for (int w = w0 + 1; w < w1; ++w) s += __popcll(row[w]);
    s += __popcll(row[w1] & m1);
  }
  return s;
}
__device__ __forceinline__ long long box_meet(CfBox a, CfBox b) {
  const int w = min(a.x1, b.x1) - max(a.x0, b.x0), h = min(a.y1, b.y1) - max(a.y0, b.y0);
  return (w > 0 && h > 0) ? (long long)w * h : 0;
}
__device__ __forceinline__ bool rejects(long long painted, long long area, double overlap) {   // src :296, 0 / 0 = NaN keeps
  return (double)painted / (double)area > overlap;
}

__global__ __launch_bounds__(CF_NT) void k_cand_filter(CandFilterArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[CF_LDS];
  __shared__ long long s_ws[CF_NT / 64];
  __shared__ int s_ctr, s_next, s_stop, s_nk;
  const int tid = threadIdx.x, lane = tid & 63, f = blockIdx.x, nf = gridDim.x;
  const int raw = *a.in.count;
  if (raw > a.in.capacity) {   // a truncated list cannot be suppressed exactly: the host reports PBD_ERR_CAPACITY with the count
    if (tid == 0) {
      if (f == 0) { a.cnt_out[0] = raw; a.cnt_out[1] = raw; }
      a.cnt_out[2 + f] = 0; a.cnt_out[2 + nf + f] = 0;
    }
    return;
  }
  const int n = raw;
  const size_t stride = a.in.stride;
  const int loc_off = 16 + a.in.mp * 16;   // locs[0] = root (x, y, mixture)
  auto frame_of = [&](int i) -> int {
    return a.in.nlevels ? ((const pbd_candidate_head*)(a.in.p + stride * i))->level / a.in.nlevels : 0;
  };
  // ---- this frame's records: how many, and how many of the frames in front of it
  int before = 0, mine = 0;
  for (int i = tid; i < n; i += CF_NT) { const int fr = frame_of(i); before += fr < f; mine += fr == f; }
  const int start = (int)block_sum(before, s_ws);
  const int m = (int)block_sum(mine, s_ws);
  if (tid == 0) { s_ctr = 0; if (f == 0) a.cnt_out[0] = raw; }
  int n2 = 1;
  while (n2 < m) n2 <<= 1;
  const bool in_lds = n2 <= CF_TILE;
  u64* sK = (u64*)lds;
  unsigned* sI = (unsigned*)(lds + CF_TILE * 8);
  u64* K = in_lds ? sK : a.keys + 2 * (size_t)start;
  unsigned* I = in_lds ? sI : a.idx + 2 * (size_t)start;
  unsigned* ord = a.idx + 2 * (size_t)start;
  __syncthreads();
  // ---- keys
  for (int i = tid; i < n; i += CF_NT) {
    if (frame_of(i) != f) continue;
    const char* r = a.in.p + stride * i;
    const pbd_candidate_head* hd = (const pbd_candidate_head*)r;
    unsigned lo = (unsigned)i;
    if (a.back) {
      const int* lc = (const int*)(r + loc_off);
      const BackLevel B = a.back[hd->level * a.ncomp + hd->component];
      lo = (unsigned)(((const char*)B.rootv - a.rootv_base) / a.ts + (long long)lc[1] * B.W + lc[0]);
    }
    const int p = atomicAdd(&s_ctr, 1);
    K[p] = ((u64)score_key(hd->score) << 32) | lo;
    I[p] = (unsigned)i;
  }
  for (int p = m + tid; p < n2; p += CF_NT) { K[p] = ~0ull; I[p] = 0xffffffffu; }
  __syncthreads();
  // ---- sort
  if (in_lds) {
    for (int k = 2; k <= n2; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) { bpass(K, I, n2, k, j, 0); __syncthreads(); }
    for (int p = tid; p < m; p += CF_NT) ord[p] = I[p];
  } else {
    auto tile_passes = [&](int kmax, bool from_top) {   // every tile: load, stages kmin..kmax below CF_TILE, store
      for (int t = 0; t < n2; t += CF_TILE) {
        for (int p = tid; p < CF_TILE; p += CF_NT) { sK[p] = K[t + p]; sI[p] = I[t + p]; }
        __syncthreads();
        if (!from_top) {
          for (int k = 2; k <= CF_TILE; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) { bpass(sK, sI, CF_TILE, k, j, t); __syncthreads(); }
        } else {
          for (int j = CF_TILE >> 1; j > 0; j >>= 1) { bpass(sK, sI, CF_TILE, kmax, j, t); __syncthreads(); }
        }
        for (int p = tid; p < CF_TILE; p += CF_NT) { K[t + p] = sK[p]; I[t + p] = sI[p]; }
        __syncthreads();
      }
    };
    tile_passes(CF_TILE, false);
    for (int k = 2 * CF_TILE; k <= n2; k <<= 1) {
      for (int j = k >> 1; j >= CF_TILE; j >>= 1) { bpass(K, I, n2, k, j, 0); __syncthreads(); }
      tile_passes(k, true);
    }
  }
  __syncthreads();
  // ---- boxes (Candidate::boundingBox() & image bounds) and the decisions that need no mask
  unsigned char* st = a.st + start;   // 0 undecided, 1 kept, 2 rejected
  CfBox* bx = (CfBox*)a.box + start;
  const bool nms = a.nms != 0;
  const double ov = a.overlap;
  const bool trivial = !(ov >= 0.0 && ov < 1.0);   // >= 1: nothing is rejected (painted <= area); < 0: every non-empty box is
  for (int p = tid; p < m; p += CF_NT) {
    if (!nms) { st[p] = 1; continue; }
    const char* r = a.in.p + stride * ord[p];
    const int* b = (const int*)(r + 16);
    const int np = ((const pbd_candidate_head*)r)->nparts;
    int x = b[0], y = b[1], bw = b[2], bh = b[3];
    for (int q = 0; q < np; ++q) {
      const int* c = b + q * 4;
      const int x1 = min(x, c[0]), y1 = min(y, c[1]);
      bw = max(x + bw, c[0] + c[2]) - x1;
      bh = max(y + bh, c[1] + c[3]) - y1;
      x = x1; y = y1;
    }
    int ix1 = max(x, 0), iy1 = max(y, 0);
    int iw = min(x + bw, a.im_w) - ix1, ih = min(y + bh, a.im_h) - iy1;
    if (iw <= 0 || ih <= 0) ix1 = iy1 = iw = ih = 0;
    bx[p] = CfBox{ix1, iy1, ix1 + iw, iy1 + ih};
    st[p] = (iw == 0 || ov >= 1.0) ? 1 : trivial ? 2 : 0;
  }
  if (nms && !trivial) {
    const int wq = (a.im_w + 63) >> 6;
    const size_t mq = (size_t)wq * a.im_h;
    u64* M = mq * 8 <= CF_MASK_LDS ? (u64*)lds : a.gmask + mq * f;
    int* s_cnt = (int*)(lds + CF_MASK_LDS);
    CfBox* s_keep = (CfBox*)(lds + CF_MASK_LDS + CF_NT * 4);
    __syncthreads();
    for (size_t i = tid; i < mq; i += CF_NT) M[i] = 0;
    if (tid == 0) s_next = 0;
    __syncthreads();
    while (s_next < m) {
      const int next = s_next;
      const int c = next + tid;
      int cnt = -1;
      if (c < m && st[c] == 0) {
        const CfBox b = bx[c];
        const int k = box_count(M, wq, b);
        if (rejects(k, (long long)(b.x1 - b.x0) * (b.y1 - b.y0), ov)) st[c] = 2;
        else cnt = k;
      }
      s_cnt[tid] = cnt;
      __syncthreads();
      if (tid < 64) {   // one wavefront: the passing candidates in order
        int nk = 0, stop = CF_NT;
        for (int base = 0; base < CF_NT && stop == CF_NT; base += 64) {
          u64 pass = __ballot(s_cnt[base + lane] >= 0);
          while (pass) {
            const int q = base + __ffsll((long long)pass) - 1;
            pass &= pass - 1;
            const CfBox b = bx[next + q];
            const long long area = (long long)(b.x1 - b.x0) * (b.y1 - b.y0);
            long long s = 0;
            for (int k = lane; k < nk; k += 64) s += box_meet(s_keep[k], b);
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            const long long ub = min(area, (long long)s_cnt[q] + s);
            if (nk == CF_KEEPS || rejects(ub, area, ov)) { stop = q; break; }
            if (lane == 0) { st[next + q] = 1; s_keep[nk] = b; }
            nk++;
          }
        }
        if (lane == 0) { s_stop = stop; s_nk = nk; }
      }
      __syncthreads();
      const int nk = s_nk;
      for (int k = 0; k < nk; ++k) {   // paint this round's kept boxes
        const CfBox b = s_keep[k];
        const int w0 = b.x0 >> 6, w1 = (b.x1 - 1) >> 6, nw = w1 - w0 + 1;
        const u64 m0 = ~0ull << (b.x0 & 63), m1 = ~0ull >> (63 - ((b.x1 - 1) & 63));
        for (int i = tid; i < nw * (b.y1 - b.y0); i += CF_NT) {
          const int yy = b.y0 + i / nw, w = w0 + i % nw;
          u64 bits = ~0ull;
          if (w == w0) bits &= m0;
          if (w == w1) bits &= m1;
          atomicOr(M + (size_t)yy * wq + w, bits);
        }
      }
      __syncthreads();
      if (tid == 0) s_next = next + s_stop;
      __syncthreads();
    }
  }
  __syncthreads();
  // ---- compaction of the kept order, in place (a kept entry only moves down)
  int kept = 0;
  for (int c0 = 0; c0 < m; c0 += CF_NT) {
    const int i = c0 + tid;
    const bool fl = i < m && st[i] == 1;
    const unsigned v = fl ? ord[i] : 0u;
    const u64 bal = __ballot(fl);
    const int pre = __popcll(bal & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) s_ws[tid >> 6] = __popcll(bal);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < CF_NT / 64; ++w) { if (w < (tid >> 6)) off += (int)s_ws[w]; tot += (int)s_ws[w]; }
    if (fl) ord[kept + off + pre] = v;
    kept += tot;
    __syncthreads();
  }
  // ---- the kept records, in final order
  const int spw = (int)(stride / 4);
  const int* src = (const int*)a.in.p;
  int* dst = (int*)(a.out + stride * start);
  for (long long w = tid; w < (long long)kept * spw; w += CF_NT) {
    const int j = (int)(w / spw), k = (int)(w - (long long)j * spw);
    dst[(size_t)j * spw + k] = src[(size_t)ord[j] * spw + k];
  }
  if (tid == 0) {
    a.cnt_out[2 + f] = kept;
    a.cnt_out[2 + nf + f] = start;
    if (f == 0) a.cnt_out[1] = kept;
  }
}

size_t cand_filter_mask_bytes(int w, int h) {   // device-memory mask per frame (0: the mask lives in LDS)
  const size_t b = (size_t)((w + 63) >> 6) * 8 * h;
  return b <= CF_MASK_LDS ? 0 : b;
}

void launch_cand_filter(const CandFilterArgs& a, int nframes, hipStream_t s) {
  hipLaunchKernelGGL(k_cand_filter, dim3(nframes), dim3(CF_NT), 0, s, a);
}
