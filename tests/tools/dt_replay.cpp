// dt_replay.cpp — host replay of pbd_dt2d exactly as k_dt_pass (partsbaseddetector_amd/csrc/k_dp.hip) processes it, with the
// kernel's path counters (pbd_debug_dt_counters).  The block geometry comes from the planner itself (pbd_plan.cpp: dt_group,
// dt_add_tasks, dt_mark_fused) with the lane count and LDS budget pbd_dt2d uses; every block then runs dt_core.hpp's local
// scans, speculative stitches, validation rounds (lowest stale boundary of a line first), stitch redos and sequential redos
// in the kernel's order, and reads out like the kernel.  Built as a shared library beside pbd_plan.cpp by
// tests/test_dt_paths_cpu.py:
//   g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared -I partsbaseddetector_amd/csrc tests/tools/dt_replay.cpp
//       partsbaseddetector_amd/csrc/pbd_plan.cpp -o dt_replay.so
//
// Speculation: the speculative stitches of one line read its segments while the other stitches of the line may be patching
// theirs.  The replay lets every stitch read its left neighbour UNPATCHED (what happens when both lanes sit in one wavefront:
// the loop's reads all precede the patch behind it).  What a stitch reads above its neighbour's F is never patched, so whether
// a line has a stale boundary in the first judgement, which one is the lowest, and the local-scan flags do not depend on
// timing; flags raised by a stale speculative stitch and the rounds behind the first may.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "pbd_lds.hpp"
#include "pbd_plan.hpp"

static int g_lost = 0, g_suspect = 0;   // why the last dt_stitch1 call flagged its line
#define DT_NOTE_STITCH_FLAG(lost, suspect) (g_lost = (lost), g_suspect = (suspect))
#include "dt_core.hpp"

// counters [0..7]: those of pbd_debug_dt_counters; host only: [8] lines flagged in a REDONE stitch, [9] stitch flags for a lost
// invariant, [10] stitch flags for a suspect quotient, [11] blocks, [12] lines, [13] groups with the fused arithmetic (of 2)
enum { NCOUNT = 14 };

template <typename T, typename IT, bool FZ>
static void replay_block(const T* src, const DtTask& t, const DtMap& mp, T* dst, int16_t* ptr, long long* c) {
  const DtGroup& g = t.g;
  const int len = g.len, S = g.stride, lpb = g.lpb, nl = t.nl, P = g.P, nsub = g.nsub;
  constexpr bool EX = sizeof(T) == 8;
  std::vector<DtPair<T>> YZ((size_t)lpb * S + 1);
  std::vector<IT> B((size_t)lpb * S + 1);
  std::vector<double> RDX(S + 1, 0.0);
  if (!EX) for (int dx = 1; dx < S; ++dx) RDX[dx] = 1.0 / (double)dx;
  std::vector<int> seg(P + 1);
  for (int p = 0; p <= P; ++p) seg[p] = dt_seg_start(p, P, len);
  const int INF = 0x7fffffff;
  std::vector<int> FLAG(lpb, 0), FIX(lpb, INF), FT((size_t)P * lpb, 0), DMIN((size_t)P * lpb, 0), BS((size_t)P * lpb, 0), FSPEC((size_t)P * lpb, 0);
  std::vector<T> ZS((size_t)P * lpb, (T)0);
  auto L = [&](int p, int l) { return (size_t)p * lpb + l; };
  const double a = mp.a, b = mp.b, i2a = mp.r2a;
  for (int l = 0; l < nl; ++l) {
    const T* s = src + (size_t)(t.g0 + l) * len;
    for (int e = 0; e < len; ++e) YZ[(size_t)l * S + e].x = s[e];
  }
  // local scans
  for (int l = 0; l < nl; ++l)
    for (int p = 0; p < P; ++p)
      if (dt_seg_scan<EX, FZ, T, IT>(&YZ[(size_t)l * S], &B[(size_t)l * S], RDX.data(), i2a, seg[p], seg[p + 1], a, b)) FLAG[l] = 1;
  std::vector<int> scanflag(FLAG);
  for (int l = 0; l < nl; ++l) c[5] += scanflag[l];
  // speculative stitches: right to left, so that every stitch reads its left neighbour unpatched
  for (int l = 0; l < nl; ++l) {
    if (FLAG[l]) continue;
    bool bad = false;
    for (int p = P - 1; p >= 1; --p) {
      int f, dmin, bs;
      T zs;
      const bool fl = dt_stitch1<EX, FZ, T, IT>(&YZ[(size_t)l * S], &B[(size_t)l * S], RDX.data(), i2a, seg[p], seg[p + 1], a, b, f, dmin, zs, bs);
      if (fl) { c[9] += g_lost; c[10] += g_suspect && !g_lost; }
      bad |= fl;
      FT[L(p, l)] = f; DMIN[L(p, l)] = dmin; ZS[L(p, l)] = zs; BS[L(p, l)] = bs;
    }
    if (bad) FLAG[l] = 1;
  }
  // first judgement, then rounds: the lowest stale boundary of each line is redone, the others judged again against the new F
  bool any = false;
  for (int l = 0; l < nl; ++l) {
    if (FLAG[l]) continue;
    for (int p = 2; p < P; ++p) {
      FSPEC[L(p, l)] = FT[L(p - 1, l)];
      if (dt_stitch_stale(DMIN[L(p, l)], FSPEC[L(p, l)], FSPEC[L(p, l)])) { FIX[l] = std::min(FIX[l], p); any = true; }
    }
  }
  if (any) {
    c[0]++;
    for (int round = 0;; ++round) {
      for (int l = 0; l < nl; ++l) {
        if (FIX[l] == INF) continue;
        const int ps = FIX[l];
        int f, bs = BS[L(ps, l)];
        T zs = ZS[L(ps, l)];
        const bool fl = dt_stitch_redo<EX, FZ, T, IT>(&YZ[(size_t)l * S], &B[(size_t)l * S], RDX.data(), i2a, seg[ps], seg[ps + 1], a, b,
                                                      FT[L(ps, l)], f, zs, bs);
        FT[L(ps, l)] = f; BS[L(ps, l)] = bs;
        DMIN[L(ps, l)] = seg[ps];
        c[3]++;
        if (fl) { FLAG[l] = 1; c[8]++; c[9] += g_lost; c[10] += g_suspect && !g_lost; }
      }
      bool anyn = false;
      for (int l = 0; l < nl; ++l) {
        FIX[l] = INF;
        if (FLAG[l]) continue;
        for (int p = 2; p < P; ++p) {
          const int dm = DMIN[L(p, l)], fs = FSPEC[L(p, l)], fn = FT[L(p - 1, l)];
          if (dt_stitch_stale(dm, fs, fn)) { FIX[l] = std::min(FIX[l], p); anyn = true; }
          if (dm > fs && dm <= fn) c[4]++;
        }
      }
      if (!anyn) { c[1] += round + 1; c[2] = std::max<long long>(c[2], round + 1); break; }
    }
  }
  for (int l = 0; l < nl; ++l) {
    if (!FLAG[l]) continue;
    c[6] += !scanflag[l];
    c[7]++;
    dt_seg_scan<true, false, T, IT>(&YZ[(size_t)l * S], &B[(size_t)l * S], RDX.data(), i2a, 0, len, a, b);
  }
  c[11]++;
  c[12] += nl;
  // read-out (:172-178), as the kernel: descending q per sub-range, the entry found by dt_cover
  const int whole_seg[2] = {0, len};
  for (int l = 0; l < nl; ++l) {
    DtPair<T>* YZl = &YZ[(size_t)l * S];
    IT* Bl = &B[(size_t)l * S];
    const bool whole = FLAG[l] != 0;
    const int Pl = whole ? 1 : P;
    std::vector<IT> BELOW(Pl);
    std::vector<T> ZLO(Pl);
    for (int p = 0; p < Pl; ++p) { const int f = p ? FT[L(p, l)] : 0; BELOW[p] = Bl[f]; ZLO[p] = YZl[f].y; }
    const int li = t.g0 + l, chunk = g.chunk;
    for (int sub = 0; sub < nsub; ++sub) {
      const int q0 = sub * chunk, q1 = std::min(len, q0 + chunk);
      if (q0 >= q1) continue;
      int os = mp.os + q1 - 1;
      int e = dt_cover<T, IT>(YZl, Bl, whole ? whole_seg : seg.data(), Pl, BELOW.data(), ZLO.data(), 1, os);
      for (int q = q1 - 1; q >= q0; --q, --os) {
        const T fos = (T)os;
        while (!(YZl[e].y < fos)) e = (int)Bl[e];
        const double d = (double)(os - e), ad2 = a * (d * d);
        dst[(size_t)q * g.nlines + li] = (T)((FZ ? fma(b, d, ad2) : (ad2 + b * d)) + (double)YZl[e].x);
        ptr[mp.ptr_natural ? (size_t)li * len + q : (size_t)q * g.nlines + li] = (int16_t)e;
      }
    }
  }
}

template <typename T>
static void replay_pass(const T* src, const DtTask* tasks, int ntasks, const DtMap& mp, T* dst, int16_t* ptr, long long* c) {
  for (int i = 0; i < ntasks; ++i) {
    const DtTask& t = tasks[i];
    const bool fz = sizeof(T) == 4 && (t.g.fused & DT_G_FUSED) != 0;
    if (i == 0 && fz) c[13]++;
    if (t.g.stride <= 256) {
      if (fz) replay_block<T, uint8_t, true>(src, t, mp, dst, ptr, c);
      else replay_block<T, uint8_t, false>(src, t, mp, dst, ptr, c);
    } else {
      if (fz) replay_block<T, uint16_t, true>(src, t, mp, dst, ptr, c);
      else replay_block<T, uint16_t, false>(src, t, mp, dst, ptr, c);
    }
  }
}

// pbd_dt2d's two passes (pbd_api.cpp: dt2d_): out = the y pass's scores [rows][cols], ix / iy composed like pbd_dt2d's
// (dt_correct_ptr = 0), counts[NCOUNT] accumulated over both passes.  Returns 0; -1 for arguments pbd_dt2d refuses; 1 where the x pass's or the
// y pass's scores left the finite range although the arguments were finite (pbd_dt2d: PBD_ERR_ARG after the run — outside the domain, where only
// termination is promised).  CHECKED = false (dt_replay_core_*, host only): dt_core.hpp on ANY bit pattern, for the termination tests — the stitch
// loop ends whatever the line holds; the product never runs such a map (pbd_dt2d refuses it).
template <typename T, bool CHECKED = true>
static int replay_dt2d(const T* in, int rows, int cols, double ax, double bx, double ay, double by, int osx, int osy, T* out, int32_t* ix,
                       int32_t* iy, long long* counts) {
  const int tsz = (int)sizeof(T);
  if (rows <= 0 || cols <= 0 || rows > 32767 || cols > 32767 || ax == 0 || ay == 0) return -1;
  // pbd_dt2d's domain: finite quadratics, finite scores (pbd_plan.hpp: pbd_first_nonfinite) — a map outside it never reaches dt_core.hpp
  if (!std::isfinite(ax) || !std::isfinite(bx) || !std::isfinite(ay) || !std::isfinite(by)) return -1;
  if (CHECKED && pbd_first_nonfinite(in, (size_t)rows * cols) != (size_t)rows * cols) return -1;
  const int nt = tsz == 8 ? 64 : PBD_DT_NT_DEFAULT;
  const size_t budget = std::max<size_t>(40 * 1024, dt_lds_bytes(dt_stride_for(std::max(rows, cols)), 4, tsz, nt));
  if (budget > 160 * 1024) return -1;
  const size_t HW = (size_t)rows * cols;
  std::vector<T> tmp(HW);
  std::vector<int16_t> hx(HW), hy(HW);
  DtMap maps[2] = {dt_map(in, tmp.data(), hx.data(), 0.f, 0.f, osx, 1), dt_map(tmp.data(), out, hy.data(), 0.f, 0.f, osy, 0)};
  maps[0].a = ax; maps[0].b = bx; maps[0].r2a = 1.0 / (2.0 * ax);
  maps[1].a = ay; maps[1].b = by; maps[1].r2a = 1.0 / (2.0 * ay);
  const DtGroup groups[2] = {dt_group(0, 1, rows, cols, budget, tsz, nt, 0, true), dt_group(1, 1, cols, rows, budget, tsz, nt, 0, false)};
  std::vector<DtTask> tasks;
  dt_add_tasks(groups[0], tasks);
  const int nx = (int)tasks.size();
  dt_add_tasks(groups[1], tasks);
  dt_mark_fused(tasks, maps, tsz);
  replay_pass<T>(in, tasks.data(), nx, maps[0], tmp.data(), hx.data(), counts);
  replay_pass<T>(tmp.data(), tasks.data() + nx, (int)tasks.size() - nx, maps[1], out, hy.data(), counts);
  for (size_t i = 0; i < HW; ++i) {
    const int m = (int)(i / cols), x = hx[i];
    ix[i] = x;
    iy[i] = hy[(size_t)m * cols + x];
  }
  return pbd_first_nonfinite(tmp.data(), HW) != HW || pbd_first_nonfinite(out, HW) != HW ? 1 : 0;
}

extern "C" int dt_replay_ncounts() { return NCOUNT; }
extern "C" int dt_replay_dt2d(const float* in, int rows, int cols, double ax, double bx, double ay, double by, int osx, int osy, float* out,
                              int32_t* ix, int32_t* iy, long long* counts) {
  return replay_dt2d<float>(in, rows, cols, ax, bx, ay, by, osx, osy, out, ix, iy, counts);
}
extern "C" int dt_replay_dt2d_f64(const double* in, int rows, int cols, double ax, double bx, double ay, double by, int osx, int osy,
                                  double* out, int32_t* ix, int32_t* iy, long long* counts) {
  return replay_dt2d<double>(in, rows, cols, ax, bx, ay, by, osx, osy, out, ix, iy, counts);
}
// host only: no domain check in front (see replay_dt2d)
extern "C" int dt_replay_core_dt2d(const float* in, int rows, int cols, double ax, double bx, double ay, double by, int osx, int osy, float* out,
                                   int32_t* ix, int32_t* iy, long long* counts) {
  return replay_dt2d<float, false>(in, rows, cols, ax, bx, ay, by, osx, osy, out, ix, iy, counts);
}
extern "C" int dt_replay_core_dt2d_f64(const double* in, int rows, int cols, double ax, double bx, double ay, double by, int osx, int osy,
                                       double* out, int32_t* ix, int32_t* iy, long long* counts) {
  return replay_dt2d<double, false>(in, rows, cols, ax, bx, ay, by, osx, osy, out, ix, iy, counts);
}
