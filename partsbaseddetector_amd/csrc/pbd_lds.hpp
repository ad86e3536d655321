// pbd_lds.hpp — LDS footprints of the DT and HOG workgroups: one definition for the kernels (k_dp.hip, k_hog.hip) and the
// host-only frame planner (pbd_plan.cpp), which sizes tiles and lines per block by them.  Compiles with hipcc and plain g++.
#pragma once
#include <stddef.h>
#include "pbd_plan.hpp"

#ifdef __HIPCC__
#define PBD_HD __host__ __device__ inline
#else
#define PBD_HD inline
#endif

// LDS per block: a header (per-line and per-lane descriptors, segment table), ONE table of exact reciprocals
// 1/dx, dx < len (double[S], shared by all lines whatever their map: dt_core.hpp), and per line
// {(y, z) : T2[S]; B : u8[S] (S <= 256) or u16[S]}.
// 9 bytes per line element for float: the lines resident on a CU are bounded by these bytes.
#define DT_SEGS 72                                   // SEG entries: P + 1 <= 65 starts, then {0, len} for a line redone as one segment
PBD_HD size_t dt_hdr_bytes(int nt, int ts, int its, int lpb) {   // per line 16 B, per lane T + 4 IT
  return ((size_t)lpb * 16 + DT_SEGS * 4 + (size_t)nt * (ts + 4 * its) + 15) & ~(size_t)15;
}
inline size_t dt_lds_bytes(int stride, int lpb, int ts, int nt) {   // ts = sizeof(T): (y, z) is a float or a double pair
  const int its = stride <= 256 ? 1 : 2;
  return (size_t)lpb * stride * (2 * ts + its) + dt_hdr_bytes(nt, ts, its, lpb) + (((size_t)stride + 1) & ~(size_t)1) * 8 + 16;
}

struct HogLds {
  int PT;        // pixel window side
  int NB;        // blocks per side (TC+2)
  int P0;        // window rows / columns kept before the first pixel that contributes to the tile's first block
  int MG;        // raw-tile margin before the window (source clamping can reach back sbin/2 pixels)
  int RT;        // raw tile side (pixels)
  int RP;        // raw tile row pitch in bytes (multiple of 4: rows are staged with 4-byte loads)
  int QS;        // (|g|, bin) planes: a row holds its pixels de-interleaved by the cell size — pixel wx at (wx % sbin) * QS + wx / sbin — so
                 // that the histogram walk's lanes (one block each: sbin pixels apart) read CONSECUTIVE words instead of words sbin apart
                 // (4-way bank conflicts on every read with 4-pixel cells; round 6)
  int MP;        // (|g|, bin) plane row pitch in elements = sbin * QS >= PT
  size_t mag_off, bin_off, hist_off, norm_off, ninv_off, tab_off, raw_off, out_off, total;
};

// need_ip: the kernel reads the per-row / per-column block indices (ipy, ipx) — the generic walk of odd or run-time cell sizes; the compile-time even-cell instantiations do not,
// and without the two tables the benched tile (4-pixel cells, 16 x 16 cells, 8-bit BGR) asks for 53 424 B instead of 54 032: THREE workgroups fit a CU's 160 KB instead of two
// (round 6: the hardware allocates LDS in 1 280-byte granules — 43 of them x 3 = 165 120 B did not fit; SQ counters had shown ~11 resident wavefronts per CU, not 18)
PBD_HD HogLds hog_lds_layout(int sbin, int tc, int bpp, int ts, bool need_ip = true) {   // ts = sizeof(T); bpp = bytes per pixel (channels x element size)
  HogLds L;
  L.NB = tc + 2;
  // A pixel y feeds the blocks floor((y + 0.5) / sbin - 0.5) and the next one (:252-255): block b receives exactly the
  // 2*sbin pixels from b*sbin - sbin/2 on when sbin is even, so NB blocks need (NB + 1) * sbin window rows.  Odd cell
  // sizes keep one spare row on either side.
  L.P0 = (sbin & 1) ? 1 : 0;
  L.PT = L.NB * sbin + sbin + 2 * L.P0;
  L.MG = sbin / 2 + 2;
  L.RT = L.PT + L.MG + 1;
  L.RP = (bpp & 7) ? (L.RT * bpp + 3) & ~3 : (L.RT * bpp + 7) & ~7;   // (8-byte pixels elements: rows stay 8-byte aligned)
  L.QS = (L.PT + sbin - 1) / sbin;
  L.MP = L.QS * sbin;
  size_t o = 0;
  // (|g|, bin) per window pixel are dead once the histograms are complete: the block energies, the normalisers and the
  // staging area of the finished features (half a tile of cells at a time) are written over them (barriers separate the phases)
  const size_t nn = (size_t)ts * (L.NB * L.NB + (tc + 1) * (tc + 1));
  L.mag_off = o; L.norm_off = o; L.ninv_off = o + (size_t)ts * L.NB * L.NB;
  L.out_off = (o + nn + 15) & ~(size_t)15;
  {
    const size_t a = (size_t)ts * L.PT * L.MP, b = L.out_off + (size_t)ts * ((tc * tc + 1) / 2) * (PBD_FLEN + 1);
    o += ((a > b ? a : b) + 15) & ~(size_t)15;
  }
  // the staged source pixels (raw) are dead once (|g|, bin) are computed and the histograms are not live
  // before: they share one region (one barrier more)
  const size_t hist_bytes = (size_t)ts * L.NB * L.NB * PBD_NORIENT, raw_bytes = (size_t)L.RT * L.RP;
  L.hist_off = o; L.raw_off = o;
  o += ((hist_bytes > raw_bytes ? hist_bytes : raw_bytes) + 15) & ~(size_t)15;
  L.tab_off = o; o += ((size_t)ts * 2 + (need_ip ? sizeof(int) : 0)) * 2 * L.PT;  // w0, w1 (, ip) for y and x
  L.bin_off = (o + 3) & ~(size_t)3; o = L.bin_off + (size_t)L.PT * L.MP;
  L.total = (o + 15) & ~(size_t)15;
  return L;
}
inline size_t hog_lds_bytes(int sbin, int tc, int ts, int bpp = 3) { return hog_lds_layout(sbin, tc, bpp, ts).total; }   // (the planner's bound: with the index tables)
