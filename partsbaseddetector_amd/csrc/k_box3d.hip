// k_box3d.hip — Candidate::boundingBox3D (include/Candidate.hpp:140-215) and the rest of
// PointCloudClusterer::computeBoundingBoxes (include/PointCloudClusterer.hpp:53-150) on the device, one workgroup per record.
//
// Per record:
//   1. boxes: the nparts part rects and bbn (boundingBoxNorm, :117-130), each & the image rect, scaled to the depth image by
//      (dw / im_w, dh / im_h) with x, y, w, h truncated separately (:155-168);
//   2. the valid pixels of those boxes (!= 0 and not NaN), with multiplicity, are the multiset `points` of N values.  The
//      record is invalid when the first box with a non-empty scaled ROI has no valid pixel (the reference's in-loop
//      points.empty() return), or when no box has one (the reference asserts inside cv::resize there);
//   3. cv::resize(points, Size(1, 400)) needs the values at <= 800 ranks of the sorted multiset: rows sy and sy + 1 of each
//      output row.  They are found by an exact multi-rank radix select over order-preserving 32-bit keys, in place (no
//      scratch): pass 0 histograms the top B3_DIG0 key bits of every valid pixel in LDS (its total is N), then the 800
//      target ranks are built and sorted, and every later pass refines all of them at once — the targets sharing a key
//      prefix form a group, each group gets 2^d bins with d = floor(log2(B3_BINS / groups)), and a pixel finds its group
//      by binary search over the groups' prefixes;
//   4. one wavefront: the resample (OpenCV 2.4 resizeGeneric_, a float column), filter2D with the derivative of Gaussian
//      (the kernel's nonzero taps, computed on the host, BORDER_REFLECT_101), and the walk from row 200 (:197-208);
//   5. the cube, its projection through the pinhole camera, and the part centres: a double sum per part over the
//      reference's transposed window (PointCloudClusterer.hpp:97-141), a block reduction.
// A record whose cube contains a NaN (invalid, or zmax - zmin = inf - inf) is skipped like the reference (:80-87): valid 0,
// Rect3d zero, centres zero.
#include "pbd_internal.hpp"

#define B3_NT 256
#define B3_ROWS 400
#define B3_TGT 1024          // target ranks (2 per output row), padded to a power of two for the bitonic sort
#define B3_BINS 16384        // LDS histogram counters shared by the groups of one pass
#define B3_DIG0 14           // pass 0: one group, 2^14 bins
#define B3_BLOCKS 2048

struct B3Box { int x, y, w, h; };

__device__ __forceinline__ unsigned b3_key(float v) {   // order-preserving; v is neither NaN nor +-0 here
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float b3_val(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

template <typename T> __device__ __forceinline__ float b3_px(const char* img, size_t pitch, int x, int y) {
  return (float)*(const T*)(img + (size_t)y * pitch + (size_t)x * sizeof(T));   // Mat_<float> = depth(r): 64F rounds to float
}

// block-wide exclusive scan of one value per thread; *total = the sum.  Every thread.
__device__ __forceinline__ unsigned b3_scan(unsigned v, unsigned* ws, unsigned* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned s = v;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(s, o, 64);
    if (lane >= o) s += u;
  }
  __syncthreads();
  if (lane == 63) ws[w] = s;
  __syncthreads();
  unsigned add = 0, tot = 0;
  for (int i = 0; i < B3_NT / 64; ++i) { if (i < w) add += ws[i]; tot += ws[i]; }
  *total = tot;
  return add + s - v;
}
__device__ __forceinline__ double b3_dsum(double v, double* ws) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < B3_NT / 64; ++i) t += ws[i];
  return t;
}

// Visit every pixel of the (clipped, non-empty) boxes, row-major within a box, boxes in order: f(box, value).
template <typename T, typename F>
__device__ __forceinline__ void b3_pixels(const Box3dArgs& a, const char* img, const B3Box* bx, int nb, F f) {
  for (int b = 0; b < nb; ++b) {
    const B3Box r = bx[b];
    if (r.w <= 0 || r.h <= 0) continue;
    const unsigned bw = (unsigned)r.w, n = (unsigned)r.w * (unsigned)r.h;
    const unsigned dy = B3_NT / bw, dx = B3_NT - dy * bw;
    unsigned yy = threadIdx.x / bw, xx = threadIdx.x - yy * bw;
    for (unsigned q = threadIdx.x; q < n; q += B3_NT) {
      f(b, b3_px<T>(img, a.z.pitch, r.x + (int)xx, r.y + (int)yy));
      yy += dy; xx += dx;
      if (xx >= bw) { xx -= bw; ++yy; }
    }
  }
}

__device__ __forceinline__ double b3_round(double v) { return rint(v); }   // cvRound / saturate_cast<int>(double): half to even

template <typename T>
__global__ void __launch_bounds__(B3_NT) k_box3d(Box3dArgs a) {
  extern __shared__ B3Box s_box[];                  // [mp + 1] scaled, clipped boxes
  __shared__ unsigned hist[B3_BINS];
  __shared__ unsigned tgt[B3_TGT];                 // sorted target ranks
  __shared__ unsigned pk[B3_TGT], rem[B3_TGT];     // key prefix chosen so far, rank left within it
  __shared__ unsigned gpre[B3_TGT];                // a pass's group prefixes (ascending)
  __shared__ unsigned short gid[B3_TGT];           // group of each target
  __shared__ float pts[B3_ROWS], dpt[B3_ROWS];
  __shared__ unsigned ws[B3_NT / 64];
  __shared__ double dws[B3_NT / 64];
  __shared__ int s_first, s_firstcnt, s_g;
  __shared__ int s_bb[4];

  const int tid = threadIdx.x;
  int total = *a.in.count;
  if (total > a.in.capacity) return;                  // overflowed frame: it fails with PBD_ERR_CAPACITY
  for (int i = blockIdx.x; i < total; i += gridDim.x) {
    const pbd_candidate_head* hd = (const pbd_candidate_head*)(a.in.p + a.in.stride * (size_t)i);
    const int f = record_frame(a.in, i);
    if (f < 0 || !((a.z.has >> f) & 1ull)) continue;
    const int np = hd->nparts;
    const int* pb = (const int*)(hd + 1);
    pbd_box3d* out = a.out + i;
    double* cen = a.centres ? a.centres + (size_t)i * a.in.mp * 3 : nullptr;
    if (cen) for (int k = tid; k < a.in.mp * 3; k += B3_NT) cen[k] = 0.0;
    // ---- boxes (thread 0): bb, bbn, scaled ROIs
    if (tid == 0) {
      int x0 = pb[0], y0 = pb[1], x1 = pb[0] + pb[2], y1 = pb[1] + pb[3];
      double sx = 0.0, sy = 0.0, qx = 0.0, qy = 0.0;
      for (int p = 0; p < np; ++p) {
        const int* r = pb + 4 * p;
        x0 = min(x0, r[0]); y0 = min(y0, r[1]); x1 = max(x1, r[0] + r[2]); y1 = max(y1, r[1] + r[3]);
        const double cx = b3_round((double)(r[0] + r[0] + r[2]) * 0.5), cy = b3_round((double)(r[1] + r[1] + r[3]) * 0.5);
        sx += cx; sy += cy; qx += cx * cx; qy += cy * cy;
      }
      s_bb[0] = x0; s_bb[1] = y0; s_bb[2] = x1 - x0; s_bb[3] = y1 - y0;
      const double sc = 1. / np;   // cv::meanStdDev: sums times 1./n
      const double mx = sx * sc, my = sy * sc;
      const double dx = sqrt(fmax(qx * sc - mx * mx, 0.)), dy = sqrt(fmax(qy * sc - my * my, 0.));
      const int nx = (int)(mx - 1.5 * dx), ny = (int)(my - 1.5 * dy), nw = (int)(3 * dx), nh = (int)(3 * dy);
      const double scx = (double)a.z.w / (double)a.im_w, scy = (double)a.z.h / (double)a.im_h;
      s_first = -1;
      for (int p = 0; p <= np; ++p) {
        int rx, ry, rw, rh;
        if (p < np) { rx = pb[4 * p]; ry = pb[4 * p + 1]; rw = pb[4 * p + 2]; rh = pb[4 * p + 3]; }
        else { rx = nx; ry = ny; rw = nw; rh = nh; }
        // & (0, 0, im_w, im_h) (cv::Rect &=: an empty intersection is Rect())
        const int cx0 = max(rx, 0), cy0 = max(ry, 0);
        int cw = min(rx + rw, a.im_w) - cx0, ch = min(ry + rh, a.im_h) - cy0;
        B3Box o{cx0, cy0, cw, ch};
        if (cw <= 0 || ch <= 0) o = B3Box{0, 0, 0, 0};
        o.x = (int)(o.x * scx); o.y = (int)(o.y * scy); o.w = (int)(o.w * scx); o.h = (int)(o.h * scy);
        // (inside the depth image by construction; clipped again so that no rounding can read outside it)
        const int ex = min(o.x + o.w, a.z.w), ey = min(o.y + o.h, a.z.h);
        o.x = min(max(o.x, 0), a.z.w); o.y = min(max(o.y, 0), a.z.h);
        o.w = ex - o.x; o.h = ey - o.y;
        if (o.w <= 0 || o.h <= 0) o = B3Box{0, 0, 0, 0};
        else if (s_first < 0) s_first = p;
        s_box[p] = o;
      }
      s_firstcnt = 0;
    }
    for (int k = tid; k < B3_BINS; k += B3_NT) hist[k] = 0;
    __syncthreads();
    const char* img = a.z.img + a.z.fbytes * (size_t)f;
    // ---- pass 0: the top B3_DIG0 key bits of every valid pixel; the first non-empty box's valid count
    {
      unsigned firstc = 0;
      const int fb = s_first;
      b3_pixels<T>(a, img, s_box, np + 1, [&](int b, float v) {
        if (v != 0.f && !(v != v)) {
          atomicAdd(&hist[b3_key(v) >> (32 - B3_DIG0)], 1u);
          firstc += b == fb;
        }
      });
      if (firstc) atomicAdd((unsigned*)&s_firstcnt, firstc);
    }
    __syncthreads();
    // exclusive cumulative counts, in place (B3_BINS / B3_NT bins per thread)
    constexpr int C0 = B3_BINS / B3_NT;
    unsigned N = 0;
    {
      unsigned s = 0;
      for (int k = 0; k < C0; ++k) s += hist[tid * C0 + k];
      unsigned run = b3_scan(s, ws, &N);
      for (int k = 0; k < C0; ++k) { const unsigned c = hist[tid * C0 + k]; hist[tid * C0 + k] = run; run += c; }
    }
    const bool valid0 = s_first >= 0 && s_firstcnt > 0 && N > 0;
    if (!valid0) {
      if (tid == 0) {
        pbd_box3d o{};
        o.x = s_bb[0]; o.y = s_bb[1]; o.width = s_bb[2]; o.height = s_bb[3];
        o.zmin = o.zmax = __int_as_float(0x7fc00000);
        *out = o;
      }
      __syncthreads();
      continue;
    }
    // ---- targets: rows sy and sy + 1 (clamped) of every output row, sorted (duplicates kept)
    const bool copy = N == B3_ROWS;
    const double scale = 1. / ((double)B3_ROWS / N);   // cv::resize: scale_y = 1. / inv_scale_y
    for (int t = tid; t < B3_TGT; t += B3_NT) {
      unsigned r = 0xffffffffu;
      if (t < 2 * B3_ROWS) {
        const int dyr = t >> 1;
        if (copy) r = (unsigned)dyr;
        else {
          const float fy = (float)((dyr + 0.5) * scale - 0.5);
          const int sy = (int)floorf(fy) + (t & 1);
          r = (unsigned)min(max(sy, 0), (int)N - 1);
        }
      }
      tgt[t] = r;
    }
    __syncthreads();
    for (int k = 2; k <= B3_TGT; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < B3_TGT; t += B3_NT) {
          const int u = t ^ j;
          if (u > t) {
            const unsigned x = tgt[t], y = tgt[u];
            if (((t & k) == 0) == (x > y)) { tgt[t] = y; tgt[u] = x; }
          }
        }
        __syncthreads();
      }
    const int R = 2 * B3_ROWS;   // (the padding sorted to the end)
    // resolve pass 0 for every target: the last bin whose cumulative count <= rank
    for (int t = tid; t < R; t += B3_NT) {
      const unsigned r = tgt[t];
      int lo = 0, hi = (1 << B3_DIG0) - 1;
      while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (hist[mid] <= r) lo = mid; else hi = mid - 1; }
      pk[t] = (unsigned)lo << (32 - B3_DIG0);
      rem[t] = r - hist[lo];
    }
    __syncthreads();
    // ---- refinement passes
    for (int hi = 32 - B3_DIG0; hi > 0;) {
      // groups: runs of equal prefixes (bits >= hi) along the sorted targets
      unsigned flags = 0;
      constexpr int CT = (2 * B3_ROWS + B3_NT - 1) / B3_NT;
      for (int k = 0; k < CT; ++k) {
        const int t = tid * CT + k;
        if (t < R && (t == 0 || pk[t] != pk[t - 1])) flags++;
      }
      unsigned G = 0;
      unsigned g = b3_scan(flags, ws, &G);
      for (int k = 0; k < CT; ++k) {
        const int t = tid * CT + k;
        if (t >= R) break;
        if (t == 0 || pk[t] != pk[t - 1]) { gpre[g] = pk[t] >> hi; gid[t] = (unsigned short)g; ++g; }
        else gid[t] = (unsigned short)(g - 1);
      }
      int d = 0;
      while (d < hi && (G << (d + 1)) <= B3_BINS) ++d;
      const int sh = hi - d;
      const unsigned dmask = (1u << d) - 1u, nbins = G << d;
      for (unsigned k = tid; k < nbins; k += B3_NT) hist[k] = 0;
      __syncthreads();
      b3_pixels<T>(a, img, s_box, np + 1, [&](int, float v) {
        if (v != 0.f && !(v != v)) {
          const unsigned key = b3_key(v), p = key >> hi;
          int lo = 0, up = (int)G - 1;
          while (lo < up) { const int mid = (lo + up + 1) >> 1; if (gpre[mid] <= p) lo = mid; else up = mid - 1; }
          if (gpre[lo] == p) atomicAdd(&hist[((unsigned)lo << d) + ((key >> sh) & dmask)], 1u);
        }
      });
      __syncthreads();
      {
        const unsigned per = (nbins + B3_NT - 1) / B3_NT, b0 = min(nbins, tid * per), b1 = min(nbins, b0 + per);
        unsigned s = 0, tot = 0;
        for (unsigned k = b0; k < b1; ++k) s += hist[k];
        unsigned run = b3_scan(s, ws, &tot);
        for (unsigned k = b0; k < b1; ++k) { const unsigned c = hist[k]; hist[k] = run; run += c; }
      }
      __syncthreads();
      for (int t = tid; t < R; t += B3_NT) {
        const unsigned base = (unsigned)gid[t] << d, r = rem[t] + hist[base];
        int lo = 0, up = (int)dmask;
        while (lo < up) { const int mid = (lo + up + 1) >> 1; if (hist[base + mid] <= r) lo = mid; else up = mid - 1; }
        pk[t] |= (unsigned)lo << sh;
        rem[t] = r - hist[base + lo];
      }
      hi = sh;
      __syncthreads();
    }
    // ---- one wavefront: resample, derivative of Gaussian, walk
    if (tid < 64) {
      auto value = [&](unsigned r) -> float {   // the sorted multiset's element of rank r
        int lo = 0, up = R - 1;
        while (lo < up) { const int mid = (lo + up) >> 1; if (tgt[mid] < r) lo = mid + 1; else up = mid; }
        return b3_val(pk[lo]);
      };
      for (int dyr = tid; dyr < B3_ROWS; dyr += 64) {
        if (copy) { pts[dyr] = value((unsigned)dyr); continue; }
        float fy = (float)((dyr + 0.5) * scale - 0.5);
        const int sy = (int)floorf(fy);
        fy -= (float)sy;
        const float S0 = value((unsigned)min(max(sy, 0), (int)N - 1)), S1 = value((unsigned)min(max(sy + 1, 0), (int)N - 1));
        const float b0 = 1.f - fy;
        const float p0 = S0 * b0, p1 = S1 * fy;
        pts[dyr] = p0 + p1;
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      for (int m = tid; m < B3_ROWS; m += 64) {
        float s = 0.0f;
        for (int k = 0; k < a.ntaps; ++k) {
          int q = m + a.tap_off[k];
          q = q < 0 ? -q : (q >= B3_ROWS ? 2 * (B3_ROWS - 1) - q : q);   // BORDER_REFLECT_101
          const float pr = a.tap[k] * pts[q];
          s = s + pr;
        }
        dpt[m] = s;
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      if (tid == 0) {
        const int midx = B3_ROWS / 2;
        int dmax = midx, dmin = midx;
        for (int m = midx; m < B3_ROWS; ++m) { if ((double)fabsf(dpt[m]) > 0.035) break; dmax = m; }
        for (int m = midx; m >= 0; --m) { if ((double)fabsf(dpt[m]) > 0.035) break; dmin = m; }
        const float zmin = pts[dmin], zmax = pts[dmax];
        pbd_box3d o{};
        o.x = s_bb[0]; o.y = s_bb[1]; o.width = s_bb[2]; o.height = s_bb[3];
        o.zmin = zmin; o.zmax = zmax;
        const double cz = (double)zmin, cd = (double)zmax - (double)zmin;
        o.valid = !(cd != cd);   // PointCloudClusterer.hpp:80-87: a cube with a NaN is skipped
        if (o.valid) {
          const double u0 = o.x, v0 = o.y, u1 = o.x + (double)o.width, v1 = o.y + (double)o.height;
          const double tx = (u0 - a.cam.cx - a.cam.tx) / a.cam.fx * cz, ty = (v0 - a.cam.cy - a.cam.ty) / a.cam.fy * cz, tz = 1.0 * cz;
          const double zb = cz + cd;
          const double bxx = (u1 - a.cam.cx - a.cam.tx) / a.cam.fx * zb, byy = (v1 - a.cam.cy - a.cam.ty) / a.cam.fy * zb, bz = 1.0 * zb;
          o.x3d = tx; o.y3d = ty; o.z3d = tz;
          o.width3d = bxx - tx; o.height3d = byy - ty; o.depth3d = bz - tz;
        }
        *out = o;
        s_g = o.valid;
      }
    }
    __syncthreads();
    // ---- part centres: the reference's transposed window, a double sum per part
    if (s_g && cen) {
      for (int p = 0; p < np; ++p) {
        const int* r = pb + 4 * p;
        const int cx0 = max(r[0], 0), cy0 = max(r[1], 0);
        int w = min(r[0] + r[2], a.im_w) - cx0, h = min(r[1] + r[3], a.im_h) - cy0, x = cx0, y = cy0;
        if (w <= 0 || h <= 0) { x = y = w = h = 0; }
        // rows x .. x + h - 1, columns y .. y + w - 1 of the depth image; outside it: 0
        double s = 0.0;
        const unsigned n = (unsigned)w * (unsigned)h;
        for (unsigned q = tid; q < n; q += B3_NT) {
          const int row = x + (int)(q / (unsigned)w), col = y + (int)(q % (unsigned)w);
          if (row < a.z.h && col < a.z.w) s += (double)b3_px<T>(img, a.z.pitch, col, row);
        }
        s = b3_dsum(s, dws);
        if (tid == 0) {
          double avg = s;
          if (w * h != 0) avg /= w * h;
          const double u = x + w / 2, v = y + h / 2;
          cen[3 * p] = (u - a.cam.cx - a.cam.tx) / a.cam.fx * avg;
          cen[3 * p + 1] = (v - a.cam.cy - a.cam.ty) / a.cam.fy * avg;
          cen[3 * p + 2] = 1.0 * avg;
        }
        __syncthreads();
      }
    }
    __syncthreads();
  }
}

void launch_box3d(const Box3dArgs& a, int ts, hipStream_t s) {
  const int nb = a.in.capacity < B3_BLOCKS ? (a.in.capacity > 0 ? a.in.capacity : 1) : B3_BLOCKS;
  const size_t lds = sizeof(B3Box) * (size_t)(a.in.mp + 1);
  if (ts == 8) hipLaunchKernelGGL(k_box3d<double>, dim3(nb), dim3(B3_NT), lds, s, a);
  else hipLaunchKernelGGL(k_box3d<float>, dim3(nb), dim3(B3_NT), lds, s, a);
}
