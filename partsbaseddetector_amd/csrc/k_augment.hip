// k_augment.hip — virtual positives (include/pbd_c.h "virtual positives"): the mirrored and rotated copies of one frame, all ops in one
// launch.  gfx950 only; a pixel is augment_core.hpp's text, shared with pbd_augment_host_u8.
//   k_augment  grid (tiles across the widest canvas, tiles down the tallest, ops); a workgroup is one 64 x 4 output tile of op
//              blockIdx.z, one wavefront per output row.  The op's descriptor is read through blockIdx.z alone: wave-uniform.  A lane
//              computes one pixel with all its channels and stores its cn bytes; a wavefront's stores cover 64 * cn consecutive bytes
//              of one row.  The gathers go through L2: under rotation a tile's source footprint is a compact parallelogram, so LDS
//              would stage what the cache already holds.  Tiles and lanes outside their op's canvas leave; nothing beyond a canvas
//              row's cols * cn bytes is written.
// No loop but the channels', no workgroup waits on another.  Plain C++ and vector stores only.
#include "pbd_internal.hpp"
#include "augment_core.hpp"

__global__ void __launch_bounds__(AUG_TILE_W * AUG_TILE_H) k_augment(AugArgs a) {
  const AugDesc d = a.desc[blockIdx.z];
  const int q = (int)blockIdx.x * AUG_TILE_W + (int)threadIdx.x, r = (int)blockIdx.y * AUG_TILE_H + (int)threadIdx.y;
  if (q >= d.cols || r >= d.rows) return;
  uint8_t* o = d.out + (size_t)r * (size_t)d.out_stride + (size_t)q * (size_t)a.cn;
  if (a.cn == 3) {
    uint8_t px[3];
    aug_pixel_n<3>(a.im, a.w, a.h, (size_t)a.stride, d, r, q, px);
    o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
  } else {
    uint8_t px[1];
    aug_pixel_n<1>(a.im, a.w, a.h, (size_t)a.stride, d, r, q, px);
    o[0] = px[0];
  }
}

void launch_augment(const AugArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)((a.max_cols + AUG_TILE_W - 1) / AUG_TILE_W), (unsigned)((a.max_rows + AUG_TILE_H - 1) / AUG_TILE_H), (unsigned)a.nops);
  hipLaunchKernelGGL(k_augment, grid, dim3(AUG_TILE_W, AUG_TILE_H), 0, s, a);
}
