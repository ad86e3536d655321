// k_cluster3d.hip — PointCloudClusterer::clusterObjects (include/PointCloudClusterer.hpp:156-290) on the device, one workgroup
// per record: CropBox around the expanded Rect3d, EuclideanClusterExtraction (tolerance tol) as the exact epsilon-graph, the
// largest cluster, its centroid and its point indices.
//
// Per record (workgroup b works in scratch slot b, so records never share scratch and no parent is read across workgroups):
//   1. crop: every point of the organized cloud, in point-index order; the kept ones are compacted with their index and xyz
//      (the slot holds a whole cloud, so no record can run out of scratch);
//   2. grid: cells of edge e >= tol * (1 + 2^-8) + 2^-70 (and >= extent * 2^-20, so that a cell coordinate fits 21 bits) from the
//      kept points' own minimum, in double: two joined points (float d2 <= r2) are never two cells apart.  The 63-bit cell key is
//      hashed into a chained table (head / next); a collision only adds candidates, the float d2 <= r2 test decides;
//   3. union-find over the 27 neighbour cells: a root is hooked under the smaller root (CAS), so every root ends as its
//      component's smallest position = smallest point index, whatever the order of the unions;
//   4. sizes per root, the largest (ties: the smallest root), its indices compacted in order into the pool, its centroid summed in
//      double.  The pool is claimed with one atomic add per record; a record that does not fit writes off = -1 and is run again
//      by the host into a pool of the size then known (pbd_api.cpp).
// r2 = inf (tol_f * tol_f overflows): every pair has d2 <= r2 (inf <= inf), one cluster, no grid.
#include "pbd_internal.hpp"

#pragma clang fp contract(off)

#define CL_NT 256
#define CL_K 4      // consecutive points per thread and crop step

__device__ __forceinline__ int cl_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cl_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x, halving the path on the way (a non-root's parent only moves to one of its ancestors)
__device__ __forceinline__ int cl_find(int* par, int x) {
  int p = cl_load(par + x);
  while (p != x) {
    const int g = cl_load(par + p);
    if (g != p) cl_store(par + x, g);
    x = p; p = g;
  }
  return x;
}
__device__ __forceinline__ void cl_unite(int* par, int a, int b) {
  for (;;) {
    a = cl_find(par, a); b = cl_find(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    int exp = a;   // hook the larger root a under b
    if (__hip_atomic_compare_exchange_strong(par + a, &exp, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  }
}

// block-wide exclusive scan of one value per thread; *total = the sum
__device__ __forceinline__ int cl_scan(int v, int* ws, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int s = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(s, o, 64);
    if (lane >= o) s += u;
  }
  __syncthreads();
  if (lane == 63) ws[w] = s;
  __syncthreads();
  int add = 0, tot = 0;
  for (int i = 0; i < CL_NT / 64; ++i) { if (i < w) add += ws[i]; tot += ws[i]; }
  *total = tot;
  return add + s - v;
}
__device__ __forceinline__ double cl_dsum(double v, double* ws) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < CL_NT / 64; ++i) t += ws[i];
  return t;
}
__device__ __forceinline__ float cl_fmin(float v, float* ws) {
  for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = ws[0];
  for (int i = 1; i < CL_NT / 64; ++i) t = fminf(t, ws[i]);
  return t;
}

// point `q` (row-major over cw x ch) of frame f: the caller's cloud (SRC 0) or the depth image of element type T (SRC 1)
template <int SRC, typename T>
__device__ __forceinline__ void cl_point(const Cluster3dArgs& a, const char* base, int q, float& x, float& y, float& z) {
  const int v = q / a.z.w, u = q - v * a.z.w;
  if (SRC == 0) {
    const float* p = (const float*)(base + (size_t)v * a.z.pitch + (size_t)u * a.pstride);
    x = p[0]; y = p[1]; z = p[2];
  } else {
    const float d = (float)*(const T*)(base + (size_t)v * a.z.pitch + (size_t)u * sizeof(T));   // 64F rounds to float first
    if (d == 0.f || !isfinite(d)) { x = y = z = __int_as_float(0x7fc00000); return; }
    const double dd = (double)d;
    x = (float)(((u - a.cam.cx - a.cam.tx) / a.cam.fx) * dd);
    y = (float)(((v - a.cam.cy - a.cam.ty) / a.cam.fy) * dd);
    z = d;
  }
}

__device__ __forceinline__ unsigned long long cl_key(long long cx, long long cy, long long cz) {
  return (unsigned long long)cx | ((unsigned long long)cy << 21) | ((unsigned long long)cz << 42);
}
__device__ __forceinline__ unsigned cl_hash(unsigned long long k, int tlog) {
  return tlog ? (unsigned)((k * 0x9E3779B97F4A7C15ull) >> (64 - tlog)) : 0u;
}

template <int SRC, typename T>
__global__ void __launch_bounds__(CL_NT) k_cluster3d(Cluster3dArgs a) {
  __shared__ int ws[CL_NT / 64];
  __shared__ float fws[CL_NT / 64];
  __shared__ double dws[CL_NT / 64];
  __shared__ unsigned long long s_best;
  __shared__ int s_ncl;

  const int tid = threadIdx.x;
  const int total = a.list ? a.nlist : *a.in.count;
  if (!a.list && total > a.in.capacity) return;   // overflowed frame: it fails with PBD_ERR_CAPACITY
  char* slot = a.scratch + a.slot_bytes * blockIdx.x;
  int* idx = (int*)slot;                              // [pcap] point index of each kept point, ascending
  float* px = (float*)(idx + a.pcap);                 // [pcap] x, y, z
  float* py = px + a.pcap;
  float* pz = py + a.pcap;
  int* par = (int*)(pz + a.pcap);                     // [pcap] union-find parent
  int* nxt = par + a.pcap;                            // [pcap] chain of the hash table, then the size of each root
  int* head = nxt + a.pcap;                           // [1 << tlog_max]
  const int npts = a.z.w * a.z.h;
  for (int j = blockIdx.x; j < total; j += gridDim.x) {
    int i = j, f;
    if (a.list) { i = a.list[2 * j]; f = a.list[2 * j + 1]; }
    else f = record_frame(a.in, i);
    if (f < 0 || !((a.z.has >> f) & 1ull)) continue;
    const pbd_box3d bx = a.boxes[i];
    Cl3Res res;
    res.r.cropped = 0; res.r.nclusters = 0; res.r.size = 0; res.r.first = -1;
    res.r.cx = res.r.cy = res.r.cz = __longlong_as_double(0x7ff8000000000000ll);
    res.off = 0;
    // ---- crop box (Rect3d in double; CropBox's Eigen::Vector4f)
    const double vol = bx.width3d * bx.height3d * bx.depth3d;
    if (!(vol >= 1e-6) || npts == 0) {
      if (tid == 0) a.out[i] = res;
      continue;
    }
    const double ex = bx.x3d - bx.width3d * 0.1, ey = bx.y3d - bx.height3d * 0.1, ez = bx.z3d - bx.depth3d * 0.1;
    const double ew = bx.width3d * 1.2, eh = bx.height3d * 1.2, ed = bx.depth3d * 1.2;
    const float x0 = (float)ex, y0 = (float)ey, z0 = (float)ez, x1 = (float)(ex + ew), y1 = (float)(ey + eh), z1 = (float)(ez + ed);
    const char* base = a.z.img + a.z.fbytes * (size_t)f;
    // ---- 1. crop, compacted in point order
    int n = 0;
    float mnx = INFINITY, mny = INFINITY, mnz = INFINITY, mxx = -INFINITY, mxy = -INFINITY, mxz = -INFINITY;
    for (int q0 = 0; q0 < npts; q0 += CL_NT * CL_K) {
      float vx[CL_K], vy[CL_K], vz[CL_K];
      unsigned keep = 0;
      int c = 0;
      for (int k = 0; k < CL_K; ++k) {
        const int q = q0 + tid * CL_K + k;
        if (q >= npts) break;
        float x, y, z;
        cl_point<SRC, T>(a, base, q, x, y, z);
        vx[k] = x; vy[k] = y; vz[k] = z;
        if (isfinite(x) && isfinite(y) && isfinite(z) && x >= x0 && x <= x1 && y >= y0 && y <= y1 && z >= z0 && z <= z1) {
          keep |= 1u << k; ++c;
          mnx = fminf(mnx, x); mny = fminf(mny, y); mnz = fminf(mnz, z);
          mxx = fmaxf(mxx, x); mxy = fmaxf(mxy, y); mxz = fmaxf(mxz, z);
        }
      }
      int tot;
      int pos = n + cl_scan(c, ws, &tot);
      for (int k = 0; k < CL_K; ++k)
        if ((keep >> k) & 1u) { idx[pos] = q0 + tid * CL_K + k; px[pos] = vx[k]; py[pos] = vy[k]; pz[pos] = vz[k]; ++pos; }
      n += tot;
    }
    res.r.cropped = n;
    if (n == 0) {
      if (tid == 0) a.out[i] = res;
      __syncthreads();
      continue;
    }
    // ---- 2. grid
    mnx = cl_fmin(mnx, fws); mny = cl_fmin(mny, fws); mnz = cl_fmin(mnz, fws);
    mxx = -cl_fmin(-mxx, fws); mxy = -cl_fmin(-mxy, fws); mxz = -cl_fmin(-mxz, fws);
    const float r2 = a.tol * a.tol;
    const bool all = isinf(r2);
    const double ext = fmax(fmax((double)mxx - (double)mnx, (double)mxy - (double)mny), (double)mxz - (double)mnz);
    const double e = fmax((double)a.tol * (1.0 + 0x1p-8) + 0x1p-70, ext * 0x1p-20);
    const double ie = 1.0 / e;   // (cells only need to be monotone and >= e * (1 - 2^-50) wide)
    int tlog = 0;
    while ((1 << tlog) < n) ++tlog;
    for (int k = tid; k < (1 << tlog); k += CL_NT) head[k] = -1;
    for (int k = tid; k < n; k += CL_NT) par[k] = all ? 0 : k;
    __syncthreads();
    auto cell = [&](int k, long long& cx, long long& cy, long long& cz) {
      cx = (long long)floor(((double)px[k] - (double)mnx) * ie);
      cy = (long long)floor(((double)py[k] - (double)mny) * ie);
      cz = (long long)floor(((double)pz[k] - (double)mnz) * ie);
    };
    if (!all) {
      for (int k = tid; k < n; k += CL_NT) {
        long long cx, cy, cz;
        cell(k, cx, cy, cz);
        nxt[k] = atomicExch(head + cl_hash(cl_key(cx, cy, cz), tlog), k);
      }
      __syncthreads();
      // ---- 3. union-find over the 27 neighbour cells (pairs q < k, each tested once per bucket visit)
      for (int k = tid; k < n; k += CL_NT) {
        long long cx, cy, cz;
        cell(k, cx, cy, cz);
        const float kx = px[k], ky = py[k], kz = pz[k];
        for (int dz = -1; dz <= 1; ++dz)
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              const long long nx = cx + dx, ny = cy + dy, nz = cz + dz;
              if (nx < 0 || ny < 0 || nz < 0) continue;
              for (int q = head[cl_hash(cl_key(nx, ny, nz), tlog)]; q >= 0; q = nxt[q]) {
                if (q >= k) continue;
                const float ddx = __fsub_rn(kx, px[q]), ddy = __fsub_rn(ky, py[q]), ddz = __fsub_rn(kz, pz[q]);
                const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(ddx, ddx), __fmul_rn(ddy, ddy)), __fmul_rn(ddz, ddz));
                if (d2 <= r2) cl_unite(par, k, q);
              }
            }
      }
      __syncthreads();
      // flatten: par[k] = the root (= the component's smallest position).  The walk stores nothing, so no late path-halving
      // store can put a non-root back over a root written here.
      for (int k = tid; k < n; k += CL_NT) {
        int r = k, p = cl_load(par + k);
        while (p != r) { r = p; p = cl_load(par + r); }
        cl_store(par + k, r);
      }
      __syncthreads();
    }
    // ---- 4. sizes, the largest, its indices, its centroid
    for (int k = tid; k < n; k += CL_NT) nxt[k] = 0;
    if (tid == 0) { s_best = 0ull; s_ncl = 0; }
    __syncthreads();
    for (int k = tid; k < n; k += CL_NT) atomicAdd(nxt + cl_load(par + k), 1);
    __syncthreads();
    {
      unsigned long long best = 0ull;   // (size << 32) | ~root: the largest, ties to the smallest root
      int ncl = 0;
      for (int k = tid; k < n; k += CL_NT) {
        const int s = nxt[k];
        if (s > 0) {
          ++ncl;
          const unsigned long long v = ((unsigned long long)(unsigned)s << 32) | (unsigned)~(unsigned)k;
          best = v > best ? v : best;
        }
      }
      if (ncl) atomicAdd(&s_ncl, ncl);
      atomicMax(&s_best, best);
    }
    __syncthreads();
    const int root = (int)~(unsigned)(s_best & 0xffffffffu), S = (int)(s_best >> 32);
    res.r.nclusters = s_ncl;
    res.r.size = S;
    res.r.first = idx[root];
    __shared__ long long s_off;
    if (tid == 0) {
      const unsigned long long o = atomicAdd(a.pool_used, (unsigned long long)S);
      s_off = o + (unsigned long long)S <= a.pool_cap ? (long long)o : -1ll;
    }
    __syncthreads();
    const long long off = s_off;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int w = 0;
    for (int k0 = 0; k0 < n; k0 += CL_NT * CL_K) {
      unsigned keep = 0;
      int c = 0;
      for (int k = 0; k < CL_K; ++k) {
        const int q = k0 + tid * CL_K + k;
        if (q < n && cl_load(par + q) == root) {
          keep |= 1u << k; ++c;
          sx += (double)px[q]; sy += (double)py[q]; sz += (double)pz[q];
        }
      }
      int tot;
      int pos = w + cl_scan(c, ws, &tot);
      if (off >= 0)
        for (int k = 0; k < CL_K; ++k)
          if ((keep >> k) & 1u) a.pool[off + pos++] = idx[k0 + tid * CL_K + k];
      w += tot;
    }
    sx = cl_dsum(sx, dws); sy = cl_dsum(sy, dws); sz = cl_dsum(sz, dws);
    res.r.cx = sx / S; res.r.cy = sy / S; res.r.cz = sz / S;
    res.off = off;
    if (tid == 0) a.out[i] = res;
    __syncthreads();   // (the slot is reused by the next record)
  }
}

size_t cluster3d_slot_bytes(int pcap) {   // idx, x, y, z, parent, next: pcap each; head: the power of two >= pcap
  size_t t = 1;
  while (t < (size_t)pcap) t <<= 1;
  return ((size_t)pcap * 24 + t * 4 + 255) & ~(size_t)255;
}

void launch_cluster3d(const Cluster3dArgs& a, int src, int nblocks, hipStream_t s) {
  if (src == 0) hipLaunchKernelGGL((k_cluster3d<0, float>), dim3(nblocks), dim3(CL_NT), 0, s, a);
  else if (src == 8) hipLaunchKernelGGL((k_cluster3d<1, double>), dim3(nblocks), dim3(CL_NT), 0, s, a);
  else hipLaunchKernelGGL((k_cluster3d<1, float>), dim3(nblocks), dim3(CL_NT), 0, s, a);
}
