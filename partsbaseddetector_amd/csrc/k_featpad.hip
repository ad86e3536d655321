// k_featpad.hip — the border ring of the boundary padding (pbd_set_boundary_pad), every level of every frame in one launch.
// Reference: copyMakeBorder(feature, padded, 3, 3, 3 * flen_, 3 * flen_, BORDER_CONSTANT, 0) + boundaryOcclusionFeature(padded, flen_, 3),
// src/HOGFeatures.cpp:147-148 (commented out at the call site) and :57-79: a cell outside the image holds 0 in channels 0 .. flen - 2
// and 1 in channel flen - 1 — the value matlab/detection/featpyramid.m:37-44 trains the models' last channel on.
//
// The ring of a level is listed by the host (PadJob, pbd_plan.cpp); a block takes PBD_FEATPAD_CPB consecutive ring cells of one level
// (ReduceBlock{job, first ring cell}), a lane one 16-byte piece of a cell: consecutive lanes write consecutive addresses — the pad top /
// bottom rows of a level are one contiguous run, the right border of row y and the left border of row y + 1 another.  The interior is
// k_hog's; the two kernels write disjoint cells.  No LDS.  On split banks the same lanes then write the cells' split operands, produced
// from the values 0 and 1 by the routine k_hog's epilogue uses (pbd_split.hpp): bfloat16 parts (1, 0, 0), binary16 parts (4096, 0).
#include "pbd_internal.hpp"
#include "pbd_split.hpp"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ring cell r of the job's cw x ch plane -> its cell y * cw + x, ring cells in row-major order (r < nring)
__device__ __forceinline__ unsigned featpad_ring_cell(const PadJob& J, unsigned r) {
  const unsigned cw = (unsigned)J.cw, pad = (unsigned)J.pad, ih = (unsigned)J.ch - 2 * pad, side = 2 * pad;
  if (r < pad * cw) return r;                              // rows 0 .. pad - 1, whole
  r -= pad * cw;
  if (r < ih * side) {                                     // interior rows: columns 0 .. pad - 1 and cw - pad .. cw - 1
    const unsigned y = r / side, k = r - y * side;
    return (pad + y) * cw + (k < pad ? k : cw - side + k);
  }
  return (pad + ih) * cw + (r - ih * side);                // rows ch - pad .. ch - 1, whole
}

template <typename T>
__global__ __launch_bounds__(256) void k_featpad(const PadJob* __restrict__ jobs, const ReduceBlock* __restrict__ blocks, T* __restrict__ feat,
                                                 uint16_t* __restrict__ split, int split_parts) {
  const ReduceBlock b = blocks[blockIdx.x];
  const PadJob J = jobs[b.job];
  const unsigned r0 = b.cell0, n = min((unsigned)PBD_FEATPAD_CPB, (unsigned)J.nring - r0), tid = threadIdx.x;
  constexpr unsigned FC = PBD_FLEN * sizeof(T) / 16, EPC = 16 / sizeof(T);   // 16-byte pieces of a cell, elements of a piece
  for (unsigned i = tid; i < n * FC; i += 256) {
    const unsigned cell = i / FC, c = i - cell * FC;
    const size_t gc = (size_t)J.cell_off + featpad_ring_cell(J, r0 + cell);
    T e[EPC];
#pragma unroll
    for (unsigned k = 0; k < EPC; ++k) e[k] = (T)0;
    if (c == FC - 1) e[EPC - 1] = (T)1;                    // channel flen - 1 (:68-76)
    u32x4 v;
    __builtin_memcpy(&v, e, 16);
    *(u32x4*)(feat + gc * PBD_FLEN + c * EPC) = v;
  }
  if constexpr (sizeof(T) == 4) {
    if (!split) return;
    // the operands of a 0 and of a 1, by the banks' own splitting; part q of the cell's 32 channels = 4 pieces of 8
    uint16_t z[3] = {0, 0, 0}, o[3] = {0, 0, 0};
    if (split_parts == 3) { feat_split_bf16(0.f, z, 1); feat_split_bf16(1.f, o, 1); }
    else { feat_split_f16(0.f, (_Float16*)z, 1); feat_split_f16(1.f, (_Float16*)o, 1); }
    const unsigned SP = (unsigned)split_parts, SC = SP * 4;
    for (unsigned i = tid; i < n * SC; i += 256) {
      const unsigned cell = i / SC, c = i - cell * SC, q = c >> 2, g = c & 3;
      const size_t gc = (size_t)J.cell_off + featpad_ring_cell(J, r0 + cell);
      const unsigned zq = q == 0 ? z[0] : q == 1 ? z[1] : z[2], oq = q == 0 ? o[0] : q == 1 ? o[1] : o[2];
      const unsigned zz = zq | (zq << 16);
      const u32x4 w = {zz, zz, zz, g == 3 ? (zq | (oq << 16)) : zz};
      *(u32x4*)(split + (gc * SP + q) * PBD_FLEN + g * 8) = w;
    }
  }
}

// feat: the handle's features (T = float: ts 4, double: ts 8); split != nullptr: the split bank's copy too (split_parts 3: bfloat16, 2: binary16)
void launch_featpad(const PadJob* jobs, const ReduceBlock* blocks, int nblocks, void* feat, int ts, uint16_t* split, int split_parts, hipStream_t s) {
  if (nblocks <= 0) return;
  if (ts == 8) hipLaunchKernelGGL(k_featpad<double>, dim3(nblocks), dim3(256), 0, s, jobs, blocks, (double*)feat, nullptr, 0);
  else hipLaunchKernelGGL(k_featpad<float>, dim3(nblocks), dim3(256), 0, s, jobs, blocks, (float*)feat, split, split_parts);
}
