// k_pyrstore.hip — the pyramid store's two streaming kernels (include/pbd_c.h "pyramid store"; host side: pbd_pyrstore.cpp).
//
//   k_pyrstore_put    the producer's feature block of a frame -> its slot: a plain copy, 16 bytes per lane and access.
//   k_pyrstore_load   slots -> the consumer's feature buffer, one launch for every frame of a batch (blockIdx.y = the frame's job).
//                     PARTS = 3 / 2 (float handles with a split-product bank): the bank's bfloat16 / binary16 parts of the same
//                     elements go to d_feat_split in the same pass, so a frame's features are read once.  The parts are
//                     pbd_split.hpp's feat_split_bf16 / feat_split_f16 — the text k_hog's epilogue and k_featpad run — applied to
//                     the floats k_hog wrote: the bits k_hog would have left in d_feat_split.
//
// Both are bound by HBM: no LDS, no reuse, a handful of registers.  A job's length is a whole number of cells
// (32 elements = 128 or 256 bytes), so a 16-byte vector — and the 8-channel group of the split variant — never straddles its end;
// the grid's tail is the loop bound.  The job table travels by value in the kernel's arguments (2 KB): no upload, nothing to keep alive.
#include "pbd_internal.hpp"
#include "pbd_split.hpp"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define PYS_NT 256          // lanes of a block
#define PYS_MAX_BLOCKS 2048 // blocks per job: beyond it a lane loops (8 waves x 256 CUs)

__device__ __forceinline__ void pys_copy(const PyrCopyJob& J) {
  const size_t nvec = (size_t)(J.bytes >> 4);
  const u32x4* __restrict__ src = (const u32x4*)J.src;
  u32x4* __restrict__ dst = (u32x4*)J.dst;
  for (size_t v = (size_t)blockIdx.x * PYS_NT + threadIdx.x; v < nvec; v += (size_t)gridDim.x * PYS_NT) dst[v] = src[v];
}

__global__ __launch_bounds__(PYS_NT) void k_pyrstore_put(const PyrCopyTable t) { pys_copy(t.j[blockIdx.y]); }

// PARTS = 0: the copy (double handles: 8-byte elements; float handles without a split bank).  Else one lane = 8 consecutive channels
// of a cell: two 16-byte loads, the same two stores, and one 16-byte store per part ([cell][part][32] 16-bit words).
template <int PARTS>
__global__ __launch_bounds__(PYS_NT) void k_pyrstore_load(const PyrCopyTable t, uint16_t* __restrict__ split) {
  const PyrCopyJob J = t.j[blockIdx.y];
  if constexpr (PARTS == 0) { pys_copy(J); } else {
  const size_t ngroups = (size_t)(J.bytes >> 5);                  // groups of 8 floats
  const f32x4* __restrict__ src = (const f32x4*)J.src;
  f32x4* __restrict__ dst = (f32x4*)J.dst;
  for (size_t i = (size_t)blockIdx.x * PYS_NT + threadIdx.x; i < ngroups; i += (size_t)gridDim.x * PYS_NT) {
    const f32x4 a = src[2 * i], b = src[2 * i + 1];
    dst[2 * i] = a; dst[2 * i + 1] = b;
    const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    uint16_t part[PARTS][8];                                      // part q of channel e at part[q][e]: the splitters' stride is 8
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if constexpr (PARTS == 3) feat_split_bf16(v[e], &part[0][e], 8);
      else feat_split_f16(v[e], (_Float16*)&part[0][e], 8);
    }
    const size_t cell = (size_t)J.dst_cell + (i >> 2), g = i & 3;
#pragma unroll
    for (int q = 0; q < PARTS; ++q) {
      u32x4 w;
#pragma unroll
      for (int d = 0; d < 4; ++d) w[d] = (unsigned)part[q][2 * d] | ((unsigned)part[q][2 * d + 1] << 16);
      *(u32x4*)(split + (cell * PARTS + q) * PBD_FLEN + g * 8) = w;
    }
  }
  }
}

static dim3 pys_grid(const PyrCopyTable& t, int njobs, unsigned unit_bytes) {
  unsigned long long most = 0;
  for (int f = 0; f < njobs; ++f) most = t.j[f].bytes > most ? t.j[f].bytes : most;
  const unsigned long long units = most / unit_bytes;
  unsigned long long bx = (units + PYS_NT - 1) / PYS_NT;
  if (bx > PYS_MAX_BLOCKS) bx = PYS_MAX_BLOCKS;
  return dim3((unsigned)(bx ? bx : 1), (unsigned)njobs);
}

void launch_pyrstore_put(const PyrCopyTable& t, int njobs, hipStream_t s) {
  if (njobs < 1) return;
  hipLaunchKernelGGL(k_pyrstore_put, pys_grid(t, njobs, 16), dim3(PYS_NT), 0, s, t);
}

void launch_pyrstore_load(const PyrCopyTable& t, int njobs, uint16_t* split, int split_parts, hipStream_t s) {
  if (njobs < 1) return;
  if (split && split_parts == 3) hipLaunchKernelGGL(k_pyrstore_load<3>, pys_grid(t, njobs, 32), dim3(PYS_NT), 0, s, t, split);
  else if (split && split_parts == 2) hipLaunchKernelGGL(k_pyrstore_load<2>, pys_grid(t, njobs, 32), dim3(PYS_NT), 0, s, t, split);
  else hipLaunchKernelGGL(k_pyrstore_load<0>, pys_grid(t, njobs, 16), dim3(PYS_NT), 0, s, t, split);
}
