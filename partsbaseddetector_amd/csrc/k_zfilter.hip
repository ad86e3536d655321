// k_zfilter.hip — SearchSpacePruning<T>::filterCandidatesByDepth (src/SearchSpacePruning.cpp:73-94) on the device.
//
// A candidate of component c is kept iff nparts(c) >= 2 and, for every part p in 1 .. nparts(c) - 1, NOT
//   (mc > 0 and mp > 0 and (double)|mc - mp|_T > norm(anchor(0)) * zfactor),
// mc = median of the depth image over box p, mp = over the box of parentid[c][p] (thr[c * mp + p] = the right-hand side, on
// the host in double).  The reference's descending loop with `break` only stops early; its `p == 1` push is never reached
// when nparts == 1, so single-part components are always dropped (kept quirk).  Math::median<T> (include/Math.hpp:63-72) is
// the element of rank floor(n / 2) in ascending order (the upper median for even n); here it is an exact radix select.
// Deviation: a box is intersected with the depth image (the reference's depth(child) throws once a box leaves the image); an
// empty intersection is "no data", median 0, so the pair is not tested.  Frames without depth (bit f of `has` clear) keep
// every record, as the reference's detect() does for an empty depth Mat.
//
// Keys: the depth values map on the fly to order-preserving unsigned keys (32-bit for float, 64-bit for double): -0.0 and
// +0.0 share a key, NaN (either sign) is above +inf.  A box's median is found by radix select, most significant digit first:
// each pass histograms, in LDS, only the pixels whose key matches the digits chosen so far, then picks the bin holding the
// remaining rank.  Small boxes use 8-bit digits (float: 4 passes, double: 8), large ones 11-bit digits (float: 11/11/10,
// double: 5 x 11 + 9).
//
// Work split by clipped area: k_zmed_small gives each (record, part) box to one 64-lane workgroup (one wavefront); a box of
// more than ZF_SMALL_MAX pixels is appended to a list that k_zmed_large works through with 256-lane workgroups.  k_zkeep
// then decides each record (one wavefront per record, the parts across the lanes) and writes the kept records at an
// atomically claimed slot (output order: arbitrary; every consumer orders the records itself) or, for the stand-alone
// primitive, a flag per record that the host compacts stably.
#include "pbd_internal.hpp"

#define ZF_DIG_SMALL 8        // 256 bins: a small box's passes are short, the per-pass cost is the histogram's clear and scan
#define ZF_DIG_LARGE 11       // 2048 bins
#define ZF_SMALL_NT 64
#define ZF_LARGE_NT 256
#define ZF_SMALL_MAX 4096      // clipped pixels one wavefront selects in (64 per lane and pass)
#define ZF_SMALL_BLOCKS 8192
#define ZF_LARGE_BLOCKS 512
#define ZF_KEEP_BLOCKS 2048

typedef unsigned long long u64;

template <typename T> struct ZKey;
template <> struct ZKey<float> {
  typedef unsigned K;
  static constexpr int bits = 32;
  __device__ static K key(float v) {
    unsigned u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    if (u == 0x80000000u) u = 0;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  __device__ static float val(K k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
};
template <> struct ZKey<double> {
  typedef u64 K;
  static constexpr int bits = 64;
  __device__ static K key(double v) {
    u64 u = (u64)__double_as_longlong(v);
    if ((u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return ~0ull;
    if (u == 0x8000000000000000ull) u = 0;
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
  }
  __device__ static double val(K k) {
    return __longlong_as_double((long long)((k & 0x8000000000000000ull) ? (k ^ 0x8000000000000000ull) : ~k));
  }
};

template <int NT>
__device__ __forceinline__ unsigned block_incl_scan(unsigned v, unsigned* ws) {
  const int lane = threadIdx.x & 63;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  if (NT == 64) return v;
  const int w = threadIdx.x >> 6;
  if (lane == 63) ws[w] = v;
  __syncthreads();
  unsigned add = 0;
  for (int i = 0; i < w; ++i) add += ws[i];
  return v + add;
}

// The key of rank n / 2 among the n = bw * bh pixels of the (clipped, non-empty) box at (x0, y0), by DIG-bit digits
// (hist: 2^DIG bins).  Every thread of the block.
template <typename T, int NT, int DIG>
__device__ typename ZKey<T>::K zselect(const char* img, size_t pitch, int x0, int y0, unsigned bw, unsigned n, unsigned* hist,
                                       unsigned* ws, unsigned* res) {
  typedef typename ZKey<T>::K K;
  constexpr int BINS = 1 << DIG, C = BINS / NT;
  static_assert(C >= 1, "at least one bin per lane");
  // pixel q = threadIdx.x + k * NT walks the box row-major: (row, column) advanced by (NT / bw, NT % bw), no division per pixel
  const unsigned dy = NT / bw, dx = NT - dy * bw, ty = threadIdx.x / bw, tx = threadIdx.x - ty * bw;
  K prefix = 0;
  unsigned r = n / 2;
  for (int pass = 0;; ++pass) {
    const int hi = ZKey<T>::bits - DIG * pass;   // key bits [hi, bits) are chosen
    const int sh = hi > DIG ? hi - DIG : 0;
    const unsigned dmask = (1u << (hi - sh)) - 1u;
    for (int b = threadIdx.x; b < BINS; b += NT) hist[b] = 0;
    __syncthreads();
    unsigned yy = ty, xx = tx;
    for (unsigned q = threadIdx.x; q < n; q += NT) {
      const K k = ZKey<T>::key(*(const T*)(img + (size_t)(y0 + yy) * pitch + (size_t)(x0 + xx) * sizeof(T)));
      if (pass == 0 || (k >> hi) == (prefix >> hi)) atomicAdd(&hist[(unsigned)(k >> sh) & dmask], 1u);
      yy += dy; xx += dx;
      if (xx >= bw) { xx -= bw; ++yy; }
    }
    __syncthreads();
    unsigned s = 0;
    for (int j = 0; j < C; ++j) s += hist[threadIdx.x * C + j];
    const unsigned incl = block_incl_scan<NT>(s, ws), excl = incl - s;
    if (r >= excl && r < incl) {   // exactly one thread: the counted pixels number > r
      unsigned acc = excl;
      int b = threadIdx.x * C;
      while (b < (int)(threadIdx.x + 1) * C - 1 && acc + hist[b] <= r) acc += hist[b++];
      res[0] = (unsigned)b;
      res[1] = r - acc;
    }
    __syncthreads();
    prefix |= (K)res[0] << sh;
    r = res[1];
    __syncthreads();
    if (sh == 0) return prefix;
  }
}

__device__ __forceinline__ const pbd_candidate_head* zrec(const ZFilterArgs& a, unsigned i) {
  return (const pbd_candidate_head*)(a.in.p + a.in.stride * i);
}
__device__ __forceinline__ int zframe(const ZFilterArgs& a, const pbd_candidate_head* hd) { return a.in.nlevels ? hd->level / a.in.nlevels : 0; }

// box p of record i clipped to the depth image: false when there is nothing to select in
__device__ __forceinline__ bool zbox(const ZFilterArgs& a, const pbd_candidate_head* hd, int p, int* x0, int* y0, unsigned* bw, unsigned* n) {
  const int* b = (const int*)(hd + 1) + p * 4;
  const long long bx = b[0], by = b[1], ex = bx + b[2], ey = by + b[3];
  const long long cx0 = bx > 0 ? bx : 0, cy0 = by > 0 ? by : 0;
  const long long cx1 = ex < a.z.w ? ex : a.z.w, cy1 = ey < a.z.h ? ey : a.z.h;
  if (b[2] <= 0 || b[3] <= 0 || cx1 <= cx0 || cy1 <= cy0) return false;
  *x0 = (int)cx0; *y0 = (int)cy0; *bw = (unsigned)(cx1 - cx0);
  *n = (unsigned)((cx1 - cx0) * (cy1 - cy0));
  return true;
}

template <typename T>
__global__ void __launch_bounds__(ZF_SMALL_NT) k_zmed_small(ZFilterArgs a) {
  typedef typename ZKey<T>::K K;
  __shared__ unsigned hist[1 << ZF_DIG_SMALL];
  __shared__ unsigned res[2];
  const int cnt = *a.in.count;
  if (cnt > a.in.capacity) return;
  const unsigned items = (unsigned)cnt * (unsigned)a.in.mp;
  for (unsigned it = blockIdx.x; it < items; it += gridDim.x) {
    const unsigned i = it / a.in.mp;
    const int p = (int)(it - i * a.in.mp);
    const pbd_candidate_head* hd = zrec(a, i);
    const int np = a.npart[hd->component], f = zframe(a, hd);
    if (np < 2 || p >= np || !((a.z.has >> f) & 1ull)) continue;
    int x0 = 0, y0 = 0;
    unsigned bw = 0, n = 0;
    if (!zbox(a, hd, p, &x0, &y0, &bw, &n)) {
      if (threadIdx.x == 0) a.med[it] = ZKey<T>::key((T)0);   // no data: median 0
      continue;
    }
    if (n > ZF_SMALL_MAX) {
      if (threadIdx.x == 0) a.large[atomicAdd(a.nlarge, 1u)] = it;
      continue;
    }
    const K k = zselect<T, ZF_SMALL_NT, ZF_DIG_SMALL>(a.z.img + a.z.fbytes * f, a.z.pitch, x0, y0, bw, n, hist, nullptr, res);
    if (threadIdx.x == 0) a.med[it] = k;
  }
}

template <typename T>
__global__ void __launch_bounds__(ZF_LARGE_NT) k_zmed_large(ZFilterArgs a) {
  typedef typename ZKey<T>::K K;
  __shared__ unsigned hist[1 << ZF_DIG_LARGE];
  __shared__ unsigned ws[ZF_LARGE_NT / 64];
  __shared__ unsigned res[2];
  const unsigned nl = *a.nlarge;
  for (unsigned j = blockIdx.x; j < nl; j += gridDim.x) {
    const unsigned it = a.large[j];
    const unsigned i = it / a.in.mp;
    const int p = (int)(it - i * a.in.mp);
    const pbd_candidate_head* hd = zrec(a, i);
    int x0 = 0, y0 = 0;
    unsigned bw = 0, n = 0;
    zbox(a, hd, p, &x0, &y0, &bw, &n);   // non-empty: k_zmed_small listed it
    const K k = zselect<T, ZF_LARGE_NT, ZF_DIG_LARGE>(a.z.img + a.z.fbytes * zframe(a, hd), a.z.pitch, x0, y0, bw, n, hist, ws, res);
    if (threadIdx.x == 0) a.med[it] = k;
  }
}

template <typename T>
__global__ void __launch_bounds__(64) k_zkeep(ZFilterArgs a) {
  const int cnt = *a.in.count;
  if (cnt > a.in.capacity) {   // the back-tracking overflowed: pass the count on, the frame fails with PBD_ERR_CAPACITY
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.cnt) *a.cnt = cnt;
    return;
  }
  const int lane = threadIdx.x;
  for (int i = blockIdx.x; i < cnt; i += gridDim.x) {
    const pbd_candidate_head* hd = zrec(a, (unsigned)i);
    const int c = hd->component, np = a.npart[c];
    bool keep = true;
    if ((a.z.has >> zframe(a, hd)) & 1ull) {
      bool bad = false;
      const size_t row = (size_t)i * a.in.mp;
      for (int p = 1 + lane; p < np; p += 64) {
        const T mc = ZKey<T>::val(a.med[row + p]);
        const T mq = ZKey<T>::val(a.med[row + a.par[c * a.in.mp + p]]);
        T d = mc - mq;   // |mc - mp| in T, then promoted (src/SearchSpacePruning.cpp:87)
        d = d < (T)0 ? -d : d;
        if (mc > (T)0 && mq > (T)0 && (double)d > a.thr[c * a.in.mp + p]) bad = true;
      }
      keep = np >= 2 && __ballot(bad) == 0ull;
    }
    if (a.flags) {
      if (lane == 0) a.flags[i] = keep ? 1 : 0;
      continue;
    }
    if (!keep) continue;
    unsigned slot = 0;
    if (lane == 0) slot = (unsigned)atomicAdd(a.cnt, 1);
    slot = __shfl(slot, 0, 64);
    const unsigned* src = (const unsigned*)hd;
    unsigned* dst = (unsigned*)(a.out + a.in.stride * slot);
    for (size_t w = lane; w < a.in.stride / 4; w += 64) dst[w] = src[w];
  }
}

// a.cnt (kept count) and a.nlarge must be zero on the stream in front of the launch (the caller's memset)
void launch_zfilter(const ZFilterArgs& a, int ts, hipStream_t s) {
  const int items = a.in.capacity * a.in.mp;
  const int sb = items < ZF_SMALL_BLOCKS ? (items > 0 ? items : 1) : ZF_SMALL_BLOCKS;
  const int kb = a.in.capacity < ZF_KEEP_BLOCKS ? (a.in.capacity > 0 ? a.in.capacity : 1) : ZF_KEEP_BLOCKS;
  if (ts == 8) {
    hipLaunchKernelGGL(k_zmed_small<double>, dim3(sb), dim3(ZF_SMALL_NT), 0, s, a);
    hipLaunchKernelGGL(k_zmed_large<double>, dim3(ZF_LARGE_BLOCKS), dim3(ZF_LARGE_NT), 0, s, a);
    hipLaunchKernelGGL(k_zkeep<double>, dim3(kb), dim3(64), 0, s, a);
  } else {
    hipLaunchKernelGGL(k_zmed_small<float>, dim3(sb), dim3(ZF_SMALL_NT), 0, s, a);
    hipLaunchKernelGGL(k_zmed_large<float>, dim3(ZF_LARGE_BLOCKS), dim3(ZF_LARGE_NT), 0, s, a);
    hipLaunchKernelGGL(k_zkeep<float>, dim3(kb), dim3(64), 0, s, a);
  }
}
