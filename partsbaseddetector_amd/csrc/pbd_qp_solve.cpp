// pbd_qp_solve.cpp — the QP solver over the device-resident example cache (include/pbd_c.h "QP solver"; kernels: k_qp_solve.hip and
// k_qp.hip's score and lincomb): the solver's state, sumAlpha of matlab/mex/qp_one_sparse.cc:90-124 (host, before the pass's launch),
// qp_one.m, qp_refresh.m, qp_opt.m with its loss, qp_prune.m and qp_w.m.  What crosses PCIe in a solver call is per example (a, sv,
// ids, b, a score) or per dense element (w, on request) — never a column.
#include <cmath>
#include <cstring>
#include "pbd_qp.hpp"

using namespace pbd_qp_detail;

namespace {
const char* const kNoState = "QP solver: the cache holds no example";

// the solver's buffers, at the first solver call: a = 0, sv = 1 for the examples held (qp_write.m:74), w = 0, l = lb = lb_old = ub = 0
int ensure(pbd_qp* q) {
  QpSolveState& S = q->sol;
  if (S.have) return PBD_OK;
  pbd_handle* h = q->h;
  const size_t cap = (size_t)q->dev.capacity, len = (size_t)q->dev.len;
  QpSolveDev& D = S.dev;
  int rc;
  if ((rc = q->alloc(&D.a, cap)) || (rc = q->alloc(&D.sv, cap)) || (rc = q->alloc(&D.w, len)) || (rc = q->alloc(&D.stat, QP_STAT_N)) ||
      (rc = q->alloc(&D.idC, cap)) || (rc = q->alloc(&D.idP, cap)) || (rc = q->alloc(&D.idI, cap)) || (rc = q->alloc(&D.err, cap)) ||
      (rc = q->alloc(&D.order, cap)) || (rc = q->alloc(&D.scores, cap)))
    return rc;   // (what was allocated stays with the cache and is freed with it)
  HIPCHK(h, hipMemsetAsync(D.a, 0, sizeof(double) * cap, h->stream));
  HIPCHK(h, hipMemsetAsync(D.sv, 0, cap, h->stream));
  if (q->n > 0) HIPCHK(h, hipMemsetAsync(D.sv, 1, (size_t)q->n, h->stream));
  HIPCHK(h, hipMemsetAsync(D.w, 0, sizeof(double) * len, h->stream));
  HIPCHK(h, hipMemsetAsync(D.stat, 0, sizeof(double) * QP_STAT_N, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  S.have = true;
  return PBD_OK;
}

// ids and b of every column, once per change of the columns
int mirror(pbd_qp* q) {
  if (!q->meta_dirty) return PBD_OK;
  pbd_handle* h = q->h;
  const size_t cap = (size_t)q->dev.capacity;
  q->m_ids.resize(cap * 5); q->m_b.resize(cap);
  HIPCHK(h, hipMemcpyAsync(q->m_ids.data(), q->dev.ids, sizeof(int) * cap * 5, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(q->m_b.data(), q->dev.b, sizeof(float) * cap, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  q->meta_dirty = false;
  return PBD_OK;
}

int get_a(pbd_qp* q, std::vector<double>& a, int n) {
  a.resize((size_t)n);
  if (n > 0) HIPCHK(q->h, hipMemcpyAsync(a.data(), q->sol.dev.a, sizeof(double) * n, hipMemcpyDeviceToHost, q->h->stream));
  return finish(q->h, "QP solver: ");
}
int get_sv(pbd_qp* q, std::vector<unsigned char>& sv, int n) {
  sv.resize((size_t)n);
  if (n > 0) HIPCHK(q->h, hipMemcpyAsync(sv.data(), q->sol.dev.sv, (size_t)n, hipMemcpyDeviceToHost, q->h->stream));
  return finish(q->h, "QP solver: ");
}

// the noneg clamp, w'w, and lb = l - w'w / 2 with l as given
int clamp_norm_lb(pbd_qp* q, double l) {
  pbd_handle* h = q->h;
  QpSolveState& S = q->sol;
  launch_qp_clamp_norm(S.dev, S.d_noneg, S.p, q->dev.len, h->stream);
  LAUNCHCHK(h, "QP solver clamp");
  HIPCHK(h, hipMemcpyAsync(S.dev.stat + QP_STAT_L, &l, sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(&S.ww, S.dev.stat + QP_STAT_WW, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  int rc = finish(h, "QP solver clamp: ");
  if (rc) return rc;
  S.l = l;
  S.lb = l - S.ww * .5;
  return PBD_OK;
}

// qp_refresh.m
int refresh(pbd_qp* q) {
  pbd_handle* h = q->h;
  QpSolveState& S = q->sol;
  const int cap = q->dev.capacity;
  std::vector<double> a;
  int rc;
  if ((rc = mirror(q)) || (rc = get_a(q, a, cap))) return rc;
  std::vector<int> I;
  for (int i = 0; i < cap; ++i) if (a[i] > 0) I.push_back(i);        // find(qp.a > 0)
  if (I.empty()) I.push_back(0);
  std::stable_sort(I.begin(), I.end(), [&](int u, int v) { return a[u] < a[v]; });
  double l = 0.0;
  for (int i : I) l = l + (double)q->m_b[q->slot[i]] * a[i];
  HIPCHK(h, hipMemcpyAsync(S.dev.order, I.data(), sizeof(int) * I.size(), hipMemcpyHostToDevice, h->stream));
  launch_qp_lincomb(q->dev, S.dev.a, S.dev.order, (int)I.size(), S.dev.w, h->stream);
  LAUNCHCHK(h, "QP solver refresh");
  S.lb_old = S.lb;
  return clamp_norm_lb(q, l);   // (synchronises: `I` is pageable)
}

// sumAlpha (qp_one_sparse.cc:90-124) and the pass
int pass(pbd_qp* q, const int32_t* order, int n, double* loss) {
  pbd_handle* h = q->h;
  QpSolveState& S = q->sol;
  if (q->n == 0) return fail(h, PBD_ERR_STATE, kNoState);
  if (n < 0 || n > q->n || (n > 0 && !order)) return fail(h, PBD_ERR_ARG, "QP solver pass: order / n");
  std::vector<char> seen((size_t)q->n, 0);
  for (int t = 0; t < n; ++t) {
    if (order[t] < 0 || order[t] >= q->n) return fail(h, PBD_ERR_ARG, "QP solver pass: an index outside [0, n)");
    if (seen[order[t]]) return fail(h, PBD_ERR_ARG, "QP solver pass: an index occurs twice");
    seen[order[t]] = 1;
  }
  for (int t = 0; t < n; ++t)
    if (q->overlap[q->slot[order[t]]])
      return fail(h, PBD_ERR_UNSUPPORTED, "QP solver pass: a column handed in by pbd_qp_put has blocks that overlap each other");
  if (n == 0) { if (loss) *loss = 0.0; return PBD_OK; }
  int rc;
  std::vector<double> a;
  if ((rc = mirror(q)) || (rc = get_a(q, a, q->n))) return rc;
  auto id = [&](int t) { return (const void*)&q->m_ids[(size_t)q->slot[order[t]] * 5]; };
  std::vector<int> srt((size_t)n);
  for (int t = 0; t < n; ++t) srt[t] = t;
  std::stable_sort(srt.begin(), srt.end(), [&](int u, int v) { return memcmp(id(u), id(v), 20) < 0; });
  std::vector<double> idC((size_t)n, 0.0);
  std::vector<int> idP((size_t)n, 0), idI((size_t)n, 0);
  int num = 0, t0 = srt[0];
  for (int t = 0; t < n; ++t) {
    const int j = srt[t], i1 = order[j];
    if (memcmp(id(j), id(t0), 20) != 0) num++;
    idP[j] = num + 1;
    idC[num] += a[i1];
    t0 = j;
    if (a[i1] > 0) idI[num] = i1 + 1;
  }
  QpSolveDev& D = S.dev;
  HIPCHK(h, hipMemcpyAsync(D.idC, idC.data(), sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(D.idP, idP.data(), sizeof(int) * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(D.idI, idI.data(), sizeof(int) * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(D.order, order, sizeof(int) * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemsetAsync(D.err, 0, sizeof(double) * n, h->stream));
  launch_qp_pass(q->dev, D, S.d_noneg, S.p, n, h->stream);
  LAUNCHCHK(h, "QP solver pass");
  double st[QP_STAT_N];
  HIPCHK(h, hipMemcpyAsync(st, D.stat, sizeof st, hipMemcpyDeviceToHost, h->stream));
  if ((rc = finish(h, "QP solver pass: "))) return rc;
  S.l = st[QP_STAT_L];
  if (loss) *loss = st[QP_STAT_LOSS];
  return PBD_OK;
}

int fix_sv(pbd_qp* q) {
  if (q->sol.nfix > 0) HIPCHK(q->h, hipMemsetAsync(q->sol.dev.sv, 1, (size_t)q->sol.nfix, q->h->stream));
  return PBD_OK;
}

// qp_one.m:15-139
int one(pbd_qp* q, const int32_t* order, int n) {
  QpSolveState& S = q->sol;
  double loss = 0.0;
  int rc;
  if ((rc = pass(q, order, n, &loss)) || (rc = refresh(q)) || (rc = fix_sv(q))) return rc;
  S.lb_old = S.lb;                      // (:137, after the refresh has moved lb)
  S.lb = S.l - S.ww * .5;
  S.ub = S.ww * .5 + loss;
  return finish(q->h, "QP solver: ");
}

// computeloss of qp_opt.m:56-86 over examples 0 .. n - 1
int loss_all(pbd_qp* q, double* out) {
  pbd_handle* h = q->h;
  QpSolveState& S = q->sol;
  const int n = q->n;
  if (n == 0) return fail(h, PBD_ERR_STATE, kNoState);
  int rc;
  if ((rc = mirror(q))) return rc;
  launch_qp_score(q->dev, S.dev.w, nullptr, n, S.dev.scores, h->stream);
  LAUNCHCHK(h, "QP solver loss");
  std::vector<double> sc((size_t)n);
  HIPCHK(h, hipMemcpyAsync(sc.data(), S.dev.scores, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  if ((rc = finish(h, "QP solver loss: "))) return rc;
  auto id = [&](int i) { return &q->m_ids[(size_t)q->slot[i] * 5]; };
  std::vector<int> J((size_t)n);
  for (int i = 0; i < n; ++i) J[i] = i;
  std::stable_sort(J.begin(), J.end(), [&](int u, int v) { return std::lexicographical_compare(id(u), id(u) + 5, id(v), id(v) + 5); });
  double loss = 0.0, v = 0.0;
  bool open = false;                     // a positive best of the current id is pending
  for (int t = 0; t < n; ++t) {
    const int i = J[t];
    const double slack = (double)q->m_b[q->slot[i]] - sc[i];
    if (t == 0 || !std::equal(id(i), id(i) + 5, id(J[t - 1]))) {
      if (open) loss = loss + v;
      v = slack;
      open = v > 0;
      if (!open) v = 0;
    } else if (slack > v) {
      v = slack; open = true;
    }
  }
  if (open) loss = loss + v;
  *out = loss;
  return PBD_OK;
}

struct SplitMix64 {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};
}  // namespace

int pbd_i_qp_appended(pbd_qp* q, int n0, int n) {
  if (!q->sol.have || n <= 0) return PBD_OK;
  HIPCHK(q->h, hipMemsetAsync(q->sol.dev.a + n0, 0, sizeof(double) * n, q->h->stream));
  HIPCHK(q->h, hipMemsetAsync(q->sol.dev.sv + n0, 1, (size_t)n, q->h->stream));
  return PBD_OK;
}

int pbd_i_qp_ensure(pbd_qp* q) { return ensure(q); }

#define SOLVER_ENTRY(q)                   \
  if (!(q)) return PBD_ERR_ARG;           \
  pbd_handle* h = (q)->h;                 \
  ON_DEVICE(h);                           \
  { int rc_ = ensure(q); if (rc_) return rc_; }

#pragma GCC visibility push(default)
extern "C" {

int pbd_qp_noneg(pbd_qp* q, const int32_t* idx, int p) {
  if (!q) return PBD_ERR_ARG;
  pbd_handle* h = q->h;
  if (p < 0 || (p > 0 && !idx)) return fail(h, PBD_ERR_ARG, "QP solver noneg: idx / p");
  for (int d = 0; d < p; ++d)
    if (idx[d] < 0 || idx[d] >= q->dev.len) return fail(h, PBD_ERR_ARG, "QP solver noneg: an index outside [0, len)");
  ON_DEVICE(h);
  int rc = ensure(q);
  if (rc) return rc;
  QpSolveState& S = q->sol;
  int* d_new = nullptr;
  if (p > 0) {
    if ((rc = q->alloc(&d_new, (size_t)p))) return rc;
    HIPCHK(h, hipMemcpyAsync(d_new, idx, sizeof(int) * p, hipMemcpyHostToDevice, h->stream));
    if ((rc = finish(h, "QP solver noneg: "))) return rc;
  }
  if (S.d_noneg) q->bufs.release(S.d_noneg);   // the list this one replaces (every solver call is synchronous: nothing in flight reads it)
  S.d_noneg = d_new; S.p = p;
  return PBD_OK;
}

int pbd_qp_fix(pbd_qp* q, int nfix) {
  if (!q) return PBD_ERR_ARG;
  pbd_handle* h = q->h;
  if (nfix < 0 || nfix > q->n) return fail(h, PBD_ERR_ARG, "QP solver fix: nfix outside [0, n]");
  ON_DEVICE(h);
  int rc = ensure(q);
  if (rc) return rc;
  q->sol.nfix = nfix;
  return PBD_OK;
}

int pbd_qp_state_put(pbd_qp* q, const double* a, const unsigned char* sv, int n) {
  if (!q) return PBD_ERR_ARG;
  pbd_handle* h = q->h;
  if (n < 0 || n > q->dev.capacity) return fail(h, PBD_ERR_ARG, "QP solver state: n outside [0, capacity]");
  ON_DEVICE(h);
  int rc = ensure(q);
  if (rc) return rc;
  if (n > 0 && a) HIPCHK(h, hipMemcpyAsync(q->sol.dev.a, a, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
  if (n > 0 && sv) HIPCHK(h, hipMemcpyAsync(q->sol.dev.sv, sv, (size_t)n, hipMemcpyHostToDevice, h->stream));
  return finish(h, "QP solver state: ");
}

int pbd_qp_state_get(pbd_qp* q, double* a, unsigned char* sv, double* w, double* stats) {
  SOLVER_ENTRY(q);
  QpSolveState& S = q->sol;
  const size_t cap = (size_t)q->dev.capacity;
  if (a) HIPCHK(h, hipMemcpyAsync(a, S.dev.a, sizeof(double) * cap, hipMemcpyDeviceToHost, h->stream));
  if (sv) HIPCHK(h, hipMemcpyAsync(sv, S.dev.sv, cap, hipMemcpyDeviceToHost, h->stream));
  if (w) HIPCHK(h, hipMemcpyAsync(w, S.dev.w, sizeof(double) * (size_t)q->dev.len, hipMemcpyDeviceToHost, h->stream));
  if (stats) { stats[0] = S.l; stats[1] = S.lb; stats[2] = S.lb_old; stats[3] = S.ub; }
  return finish(h, "QP solver state: ");
}

int pbd_qp_pass(pbd_qp* q, const int32_t* order, int n, double* loss) {
  SOLVER_ENTRY(q);
  return pass(q, order, n, loss);
}

int pbd_qp_one(pbd_qp* q, const int32_t* order, int n) {
  SOLVER_ENTRY(q);
  return one(q, order, n);
}

int pbd_qp_refresh(pbd_qp* q) {
  SOLVER_ENTRY(q);
  if (q->n == 0) return fail(h, PBD_ERR_STATE, kNoState);
  return refresh(q);
}

int pbd_qp_loss(pbd_qp* q, double* loss) {
  SOLVER_ENTRY(q);
  if (!loss) return fail(h, PBD_ERR_ARG, "QP solver loss: loss is NULL");
  return loss_all(q, loss);
}

int pbd_qp_opt(pbd_qp* q, double tol, int max_iter, uint64_t seed, double* lb_out, double* ub_out, int* passes) {
  SOLVER_ENTRY(q);
  QpSolveState& S = q->sol;
  if (q->n == 0) return fail(h, PBD_ERR_STATE, kNoState);
  if (!(tol == tol) || max_iter < 0) return fail(h, PBD_ERR_ARG, "QP solver opt: tol / max_iter");
  const int n = q->n;
  int rc;
  double loss = 0.0;
  if ((rc = refresh(q)) || (rc = loss_all(q, &loss))) return rc;
  double ub = S.ww * .5 + loss, lb = S.lb;
  HIPCHK(h, hipMemsetAsync(S.dev.sv, 1, (size_t)n, h->stream));            // qp.sv(I) = 1
  SplitMix64 g{seed};
  std::vector<unsigned char> sv;
  std::vector<int32_t> I;
  int t = 0;
  while (t < max_iter) {
    if ((rc = get_sv(q, sv, n))) return rc;
    I.clear();
    for (int i = 0; i < n; ++i) if (sv[i]) I.push_back(i);
    if (I.empty()) return fail(h, PBD_ERR_STATE, "QP solver opt: no support vector left (qp_one.m:11)");
    for (size_t u = I.size() - 1; u >= 1; --u) std::swap(I[u], I[(size_t)(g.next() % (uint64_t)(u + 1))]);
    if ((rc = one(q, I.data(), (int)I.size()))) return rc;
    ++t;
    lb = S.lb;
    const double ub_est = std::fmin(S.ub, ub);
    if (lb > 0 && 1 - lb / ub_est < tol) {
      if ((rc = loss_all(q, &loss))) return rc;
      ub = std::fmin(ub, S.ww * .5 + loss);
      if (1 - lb / ub < tol) break;
      HIPCHK(h, hipMemsetAsync(S.dev.sv, 1, (size_t)n, h->stream));
    }
  }
  S.ub = ub;
  if (lb_out) *lb_out = lb;
  if (ub_out) *ub_out = ub;
  if (passes) *passes = t;
  return finish(h, "QP solver opt: ");
}

int pbd_qp_prune(pbd_qp* q, int* n_out) {
  SOLVER_ENTRY(q);
  QpSolveState& S = q->sol;
  if (q->n == 0) return fail(h, PBD_ERR_STATE, kNoState);
  const int cap = q->dev.capacity;
  std::vector<double> a;
  std::vector<unsigned char> sv;
  int rc;
  if ((rc = mirror(q)) || (rc = get_a(q, a, cap)) || (rc = get_sv(q, sv, cap))) return rc;
  if (std::all_of(sv.begin(), sv.end(), [](unsigned char c) { return c != 0; })) {   // the cache is full of support vectors
    for (int i = 0; i < cap; ++i) sv[i] = a[i] > 0;
    for (int i = 0; i < S.nfix; ++i) sv[i] = 1;
  }
  std::vector<int32_t> I;
  for (int i = 0; i < q->n; ++i) if (sv[i]) I.push_back(i);
  const int n = (int)I.size();
  if (n == 0) return fail(h, PBD_ERR_STATE, "QP solver prune: no support vector (qp_prune.m:13)");
  if ((rc = pbd_qp_keep(q, I.data(), n))) return rc;
  std::vector<double> a2((size_t)cap, 0.0);
  std::vector<unsigned char> sv2((size_t)cap, 0);
  double l = 0.0;
  for (int j = 0; j < n; ++j) {
    a2[j] = a[I[j]]; sv2[j] = 1;
    l = l + (double)q->m_b[q->slot[j]] * a2[j];
  }
  HIPCHK(h, hipMemcpyAsync(S.dev.a, a2.data(), sizeof(double) * cap, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(S.dev.sv, sv2.data(), (size_t)cap, hipMemcpyHostToDevice, h->stream));
  launch_qp_lincomb(q->dev, S.dev.a, nullptr, n, S.dev.w, h->stream);
  LAUNCHCHK(h, "QP solver prune");
  if ((rc = clamp_norm_lb(q, l))) return rc;   // (lb_old is left alone)
  if (n_out) *n_out = n;
  return PBD_OK;
}

int pbd_qp_weights(pbd_qp* q, double* w_out) {
  SOLVER_ENTRY(q);
  if (!w_out) return fail(h, PBD_ERR_ARG, "QP solver weights: w_out is NULL");
  const size_t len = (size_t)q->dev.len;
  CallScratch t(h);
  double* d_wq;
  int rc;
  if ((rc = t.get(&d_wq, len, "QP solver: "))) return rc;
  launch_qp_weights(q->sol.dev.w, q->d_wreg, q->d_w0, (int)len, d_wq, h->stream);
  LAUNCHCHK(h, "QP solver weights");
  HIPCHK(h, hipMemcpyAsync(w_out, d_wq, sizeof(double) * len, hipMemcpyDeviceToHost, h->stream));
  return finish(h, "QP solver weights: ");
}

// train.m:94,112 model = vec2model(qp_w, model): the same w ./ wreg + w0 into a device temporary, then pbd_set_weights_dev on the cache's
// handle.  The cache's columns are features, not weights: they stay valid.
int pbd_qp_apply_weights(pbd_qp* q) {
  SOLVER_ENTRY(q);
  const size_t len = (size_t)q->dev.len;
  CallScratch t(h);
  double* d_wq;
  int rc;
  if ((rc = t.get(&d_wq, len, "QP solver: "))) return rc;
  launch_qp_weights(q->sol.dev.w, q->d_wreg, q->d_w0, (int)len, d_wq, h->stream);
  LAUNCHCHK(h, "QP solver weights");
  return pbd_i_set_weights_dev(h, d_wq, (int)len);
}

// train.m:75 qp.n = 0.  The cache goes back to what pbd_qp_create left — columns, tables and the example -> column map included, so
// that what pbd_qp_get reads behind n is a new cache's too — and the solver's state, where it exists, to a cache's that never solved.
// Capacity, footprint, wreg, w0, cpos / cneg, noneg and the binding stay.
int pbd_qp_clear(pbd_qp* q) {
  if (!q) return PBD_ERR_ARG;
  pbd_handle* h = q->h;
  ON_DEVICE(h);
  QpDev& D = q->dev;
  const size_t cap = (size_t)D.capacity;
  for (size_t i = 0; i < cap; ++i) q->slot[i] = (int)i;
  HIPCHK(h, hipMemsetAsync(D.x, 0, sizeof(float) * cap * (size_t)D.k, h->stream));
  HIPCHK(h, hipMemsetAsync(D.ids, 0, sizeof(int) * cap * 5, h->stream));
  HIPCHK(h, hipMemsetAsync(D.b, 0, sizeof(float) * cap, h->stream));
  HIPCHK(h, hipMemsetAsync(D.d, 0, sizeof(double) * cap, h->stream));
  HIPCHK(h, hipMemsetAsync(D.tab, 0, sizeof(int) * cap * D.nbmax * 3, h->stream));
  HIPCHK(h, hipMemsetAsync(D.nblk, 0, sizeof(int) * cap, h->stream));
  HIPCHK(h, hipMemcpyAsync(D.slot, q->slot.data(), sizeof(int) * cap, hipMemcpyHostToDevice, h->stream));
  QpSolveState& S = q->sol;
  if (S.have) {
    HIPCHK(h, hipMemsetAsync(S.dev.a, 0, sizeof(double) * cap, h->stream));
    HIPCHK(h, hipMemsetAsync(S.dev.sv, 0, cap, h->stream));
    HIPCHK(h, hipMemsetAsync(S.dev.w, 0, sizeof(double) * (size_t)D.len, h->stream));
    HIPCHK(h, hipMemsetAsync(S.dev.stat, 0, sizeof(double) * QP_STAT_N, h->stream));
  }
  int rc = finish(h, "example cache clear: ");
  if (rc) return rc;
  S.l = S.lb = S.lb_old = S.ub = S.ww = 0;
  S.nfix = 0;
  q->overlap.assign(cap, 0);
  q->meta_dirty = true;
  q->n = 0;
  return PBD_OK;
}

// train.m:116-118 with qp_scorepos (:198-204): the selection, w + w0 .* wreg, the scores, / Cpos and the order statistic all on the
// device (k_qp_thresh.hip).  The selection and the scores borrow the pass's scratch (order, scores): nothing a getter answers moves.
int pbd_qp_positive_threshold(pbd_qp* q, double frac, double* thresh, int* npos) {
  SOLVER_ENTRY(q);
  if (!thresh || !npos) return fail(h, PBD_ERR_ARG, "positive threshold: thresh / npos is NULL");
  if (!(frac > 0.0) || !(frac <= 1.0)) return fail(h, PBD_ERR_ARG, "positive threshold: q must lie in (0, 1]");
  if (q->n == 0) return fail(h, PBD_ERR_STATE, "positive threshold: the cache holds no positive example");
  QpSolveDev& D = q->sol.dev;
  const size_t len = (size_t)q->dev.len;
  CallScratch t(h);
  char* tp;
  int rc;
  if ((rc = t.get(&tp, sizeof(double) * len + sizeof(QpThreshOut), "positive threshold: "))) return rc;
  double* d_weff = (double*)tp;
  QpThreshOut* d_out = (QpThreshOut*)(d_weff + len);
  QpThreshOut out{0.0, -1, 0};
  HIPCHK(h, hipMemsetAsync(d_out, 0, sizeof(QpThreshOut), h->stream));
  launch_qp_thresh_select(q->dev, q->n, D.order, d_out, h->stream);
  launch_qp_thresh_weff(D.w, q->d_w0, q->d_wreg, (int)len, d_weff, h->stream);
  LAUNCHCHK(h, "positive threshold");
  HIPCHK(h, hipMemcpyAsync(&out.m, &d_out->m, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if ((rc = finish(h, "positive threshold: "))) return rc;
  const int m = out.m;
  if (m < 0 || m > q->n) return fail(h, PBD_ERR_HIP, "positive threshold: the selection's count is out of range");
  if (m == 0) return fail(h, PBD_ERR_STATE, "positive threshold: the cache holds no positive example");
  const int rank = std::min(std::max((int)std::ceil((double)m * frac), 1), m) - 1;   // Model.positive_threshold's rule
  launch_qp_score(q->dev, d_weff, D.order, m, D.scores, h->stream);
  launch_qp_thresh_scale(D.scores, D.order, m, q->cpos, d_out, h->stream);
  launch_qp_thresh_rank(D.scores, m, rank, d_out, h->stream);
  LAUNCHCHK(h, "positive threshold");
  HIPCHK(h, hipMemcpyAsync(&out, d_out, sizeof(QpThreshOut), hipMemcpyDeviceToHost, h->stream));
  if ((rc = finish(h, "positive threshold: "))) return rc;
  if (out.bad >= 0)
    return fail(h, PBD_ERR_ARG, "positive threshold: the score of example " + std::to_string(out.bad) + " is not finite");
  *thresh = out.thresh;
  *npos = m;
  return PBD_OK;
}

}  // extern "C"
#pragma GCC visibility pop
