// pbd_qp.hpp — the training example cache's host object, shared by pbd_qp.cpp (the cache) and pbd_qp_solve.cpp (the solver).
#pragma once
#include <algorithm>
#include <string>
#include <vector>
#include "pbd_internal.hpp"

// the solver's state (include/pbd_c.h "QP solver"): allocated by the first solver call, so a cache that never solves holds none of it
struct QpSolveState {
  bool have = false;
  QpSolveDev dev{};                 // a, sv, w, stat, the pass's scratch
  int* d_noneg = nullptr; int p = 0;
  int nfix = 0;
  double l = 0, lb = 0, lb_old = 0, ub = 0, ww = 0;   // host mirror of dev.stat, current after every solver call
};

struct pbd_qp {
  pbd_handle* h = nullptr;
  QpDev dev{};
  int n = 0;
  double cpos = 0, cneg = 0;
  double* d_wreg = nullptr; double* d_w0 = nullptr; int* d_foff = nullptr;
  std::vector<int> slot;            // host copy of dev.slot
  std::vector<int> foff;            // [nfilters] dense start of each filter, the caller's order
  DevBufs bufs;                     // everything the cache holds on the device (pbd_qp_footprint: its bytes)
  template <typename T> int alloc(T** p, size_t n) {
    const hipError_t e = bufs.alloc(p, n);
    return e == hipSuccess ? PBD_OK : fail(h, PBD_ERR_HIP, pbd_alloc_error("example cache: ", e));
  }
  // solver side
  QpSolveState sol;
  std::vector<char> overlap;        // [capacity] by column: a column put with blocks that overlap each other (never one of pbd_qp_write's)
  std::vector<int> m_ids;           // [capacity][5] host mirror of dev.ids, by column; current while !meta_dirty
  std::vector<float> m_b;           // [capacity]    host mirror of dev.b
  bool meta_dirty = true;
};

namespace pbd_qp_detail {
inline int finish(pbd_handle* h, const char* what) {
  hipError_t e = hipStreamSynchronize(h->stream);
  return e == hipSuccess ? PBD_OK : fail(h, PBD_ERR_HIP, std::string(what) + hipGetErrorString(e));
}
}  // namespace pbd_qp_detail

// pbd_qp_solve.cpp: examples n0 .. n0 + n - 1 were appended — with solver state they start at a = 0, sv = 1 (qp_write.m:74)
int pbd_i_qp_appended(pbd_qp* q, int n0, int n);
// pbd_qp_solve.cpp: the solver's state as any solver entry allocates it (pbd_qp_mine_* keeps ub there)
int pbd_i_qp_ensure(pbd_qp* q);
