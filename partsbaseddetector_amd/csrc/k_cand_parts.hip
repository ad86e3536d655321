// k_cand_parts.hip — the part-wise overlap NMS of matlab/detection/nms.m (include/pbd_c.h: pbd_candidates_nms_parts) on the device.
//
// k_cand_parts: one workgroup per frame, behind k_cand_filter in SORT mode.  That kernel left frame f's records, sorted, at
// in + start_f * stride, and (count block) their number m_f and start_f.  Of these the first n = min(m_f, top) take part (top = 0: all).
//   1. restaged: the rectangles of a record sit a whole record (~744 B in the person model) apart, so they are copied once into
//      planes [rectangle][record slot] of 16-byte units — plane r < mp: part r as (x, y, w, h); planes mp, mp + 1: the covering box
//      of the non-empty parts as (x0, x1) and (y0, y1) in 64 bits (junk int32 coordinates do not fit 32) — and the part counts
//      beside them.  A round's loads are then one coalesced dwordx4 per lane and rectangle;
//   2. decided in rounds, one per kept record: an undecided bit per record (LDS up to CP_LDS_WORDS * 64 records, else device
//      memory).  One wavefront finds the lowest set bit — that record is kept — and puts its rectangles and areas into LDS; then
//      every lane tests its undecided records behind it, rectangle by rectangle in fp64, leaving at the first one that rejects, and
//      a wavefront clears the bits of its 64 records with one ballot.  For overlap >= 0 a record whose covering box misses the
//      kept one's is skipped: its parts lie inside it.  overlap >= 1 rejects nothing (inter <= area), so every record is kept
//      without rounds;
//   3. written: the kept records in order at out + start_f * stride and the count block, as k_cand_filter writes them.
#include "pbd_internal.hpp"

#define CP_NT 1024
#define CP_LDS_WORDS 2048

typedef unsigned long long u64;

struct CpRect { long long x0, y0, x1, y1; };   // empty: all zero

__device__ __forceinline__ CpRect cp_part(int4 b) {   // a part box (x, y, w, h)
  if (b.z <= 0 || b.w <= 0) return CpRect{0, 0, 0, 0};
  return CpRect{b.x, b.y, (long long)b.x + b.z, (long long)b.y + b.w};
}
__device__ __forceinline__ double cp_area(CpRect r) { return (double)(r.x1 - r.x0) * (double)(r.y1 - r.y0); }
__device__ __forceinline__ double cp_inter(CpRect a, CpRect b) {
  const long long w = min(a.x1, b.x1) - max(a.x0, b.x0), h = min(a.y1, b.y1) - max(a.y0, b.y0);
  return (w > 0 && h > 0) ? (double)w * (double)h : 0.0;
}
__device__ __forceinline__ CpRect cp_cover(const int4* rect, size_t cap, int mp, size_t slot) {
  const int4 cx = rect[(size_t)mp * cap + slot], cy = rect[(size_t)(mp + 1) * cap + slot];
  CpRect c;
  c.x0 = (long long)(((u64)(unsigned)cx.y << 32) | (unsigned)cx.x); c.x1 = (long long)(((u64)(unsigned)cx.w << 32) | (unsigned)cx.z);
  c.y0 = (long long)(((u64)(unsigned)cy.y << 32) | (unsigned)cy.x); c.y1 = (long long)(((u64)(unsigned)cy.w << 32) | (unsigned)cy.z);
  return c;
}
__device__ __forceinline__ int4 cp_pack(long long a, long long b) {
  return make_int4((int)(unsigned)(u64)a, (int)(unsigned)((u64)a >> 32), (int)(unsigned)(u64)b, (int)(unsigned)((u64)b >> 32));
}

__global__ __launch_bounds__(CP_NT) void k_cand_parts(CandPartsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char dyn[];   // the kept record's rectangles [mp + 1] and their areas
  __shared__ u64 s_bits[CP_LDS_WORDS];
  __shared__ int s_cur, s_np;
  const int tid = threadIdx.x, lane = tid & 63, f = blockIdx.x, nf = gridDim.x;
  const int raw = a.cnt_in[0];
  if (raw > a.capacity) {   // the sort kept nothing: the same count block, and the host reports PBD_ERR_CAPACITY
    if (tid == 0) {
      if (f == 0) { a.cnt_out[0] = raw; a.cnt_out[1] = raw; }
      a.cnt_out[2 + f] = 0; a.cnt_out[2 + nf + f] = 0;
    }
    return;
  }
  const int mp = a.mp, m = a.cnt_in[2 + f], start = a.cnt_in[2 + nf + f];
  const int n = a.top > 0 && m > a.top ? a.top : m;
  const size_t stride = a.stride, cap = (size_t)a.capacity;
  const double ov = a.overlap;
  CpRect* s_rect = (CpRect*)dyn;
  double* s_area = (double*)(dyn + sizeof(CpRect) * (mp + 1));
  const int W = (n + 63) >> 6;
  u64* U = W <= CP_LDS_WORDS ? s_bits : a.gbits + (start >> 6) + f;
  unsigned* kl = a.kept + start;
  int* npj = a.np + start;
  int kept = 0;
  if (ov >= 1.0) {
    for (int j = tid; j < n; j += CP_NT) kl[j] = (unsigned)j;
    kept = n;
  } else {
    // ---- restage
    for (int j = tid; j < n; j += CP_NT) {
      const char* r = a.in + stride * (size_t)(start + j);
      const int* b = (const int*)(r + 16);
      const int P = min(max(((const pbd_candidate_head*)r)->nparts, 0), mp);
      long long x0 = 0, y0 = 0, x1 = 0, y1 = 0;
      bool any = false;
      for (int q = 0; q < P; ++q) {
        const int4 bx = make_int4(b[q * 4], b[q * 4 + 1], b[q * 4 + 2], b[q * 4 + 3]);
        a.rect[(size_t)q * cap + start + j] = bx;
        const CpRect c = cp_part(bx);
        if (c.x1 == c.x0) continue;
        x0 = any ? min(x0, c.x0) : c.x0; y0 = any ? min(y0, c.y0) : c.y0;
        x1 = any ? max(x1, c.x1) : c.x1; y1 = any ? max(y1, c.y1) : c.y1;
        any = true;
      }
      a.rect[(size_t)mp * cap + start + j] = cp_pack(x0, x1);
      a.rect[(size_t)(mp + 1) * cap + start + j] = cp_pack(y0, y1);
      npj[j] = P;
    }
    for (int w = tid; w < W; w += CP_NT) U[w] = n - w * 64 >= 64 ? ~0ull : (1ull << (n - w * 64)) - 1ull;
    __syncthreads();
    // ---- rounds
    int cur = 0;   // (the first wavefront's: every record in front of it is decided)
    for (;;) {
      if (tid < 64) {
        int found = -1;
        for (int wb = cur >> 6; wb < W && found < 0; wb += 64) {
          const u64 bits = wb + lane < W ? U[wb + lane] : 0ull;
          const u64 bal = __ballot(bits != 0ull);
          if (bal) {
            const int l = __ffsll((long long)bal) - 1;
            const u64 b = __shfl(bits, l);
            found = ((wb + l) << 6) + __ffsll((long long)b) - 1;
          }
        }
        if (found >= 0) {
          const int P = npj[found];
          for (int r = lane; r < P; r += 64) {
            const CpRect c = cp_part(a.rect[(size_t)r * cap + start + found]);
            s_rect[r] = c; s_area[r] = cp_area(c);
          }
          if (lane == 0) {
            const CpRect c = cp_cover(a.rect, cap, mp, (size_t)start + found);
            s_rect[mp] = c; s_area[mp] = cp_area(c);
            s_np = P;
            U[found >> 6] &= ~(1ull << (found & 63));
          }
          cur = found + 1;
        }
        if (lane == 0) s_cur = found;
      }
      __syncthreads();
      const int i = s_cur;
      if (i < 0) break;
      if (tid == 0) kl[kept] = (unsigned)i;
      kept++;
      const int Pi = s_np;
      const CpRect ci = s_rect[mp];
      const double ai = s_area[mp];
      for (int jb = ((i + 1) & ~(CP_NT - 1)) + (tid & ~63); jb < n; jb += CP_NT) {   // (a wavefront's 64 records share a word)
        const u64 word = U[jb >> 6];
        if (!word) continue;
        const int j = jb + lane;
        bool rej = false;
        if (j > i && ((word >> lane) & 1ull)) {
          const double ic = cp_inter(ci, cp_cover(a.rect, cap, mp, (size_t)start + j));
          if (ic > 0.0 || ov < 0.0) {
            rej = ic / ai > ov;
            const int P = min(Pi, npj[j]);
            for (int r = 0; r < P && !rej; ++r)
              rej = cp_inter(s_rect[r], cp_part(a.rect[(size_t)r * cap + start + j])) / s_area[r] > ov;
          }
        }
        const u64 bal = __ballot(rej);
        if (lane == 0 && bal) U[jb >> 6] = word & ~bal;
      }
      __syncthreads();
    }
  }
  __syncthreads();
  // ---- the kept records, in order
  const int spw = (int)(stride / 4);
  const int* src = (const int*)(a.in + stride * (size_t)start);
  int* dst = (int*)(a.out + stride * (size_t)start);
  for (long long w = tid; w < (long long)kept * spw; w += CP_NT) {
    const int j = (int)(w / spw), k = (int)(w - (long long)j * spw);
    dst[(size_t)j * spw + k] = src[(size_t)kl[j] * spw + k];
  }
  if (tid == 0) {
    if (f == 0) { a.cnt_out[0] = raw; a.cnt_out[1] = kept; }
    a.cnt_out[2 + f] = kept;
    a.cnt_out[2 + nf + f] = start;
  }
}

size_t cand_parts_bits_words(int capacity, int nframes) { return ((size_t)capacity >> 6) + (size_t)nframes + 2; }

void launch_cand_parts(const CandPartsArgs& a, int nframes, hipStream_t s) {
  hipLaunchKernelGGL(k_cand_parts, dim3(nframes), dim3(CP_NT), (sizeof(CpRect) + sizeof(double)) * (size_t)(a.mp + 1), s, a);
}
