// pbd_qp.cpp — the training example cache's host side (include/pbd_c.h "training example cache"; kernels: k_qp.hip): the cache's
// buffers, the dense layout and its defaults (model2vec.m), the repeated-block check of qp_write.m:34-35, the validation of columns
// handed in, and the pbd_qp_* entry points.  The cache borrows its handle's model, stream and device; errors go through the handle.
#include <algorithm>
#include <cmath>
#include <utility>
#include "pbd_qp.hpp"

namespace {
using namespace pbd_qp_detail;
// size of the caller's filter n
void filter_size(const pbd_handle* h, int n, int* kh, int* kw) {
  const int f = h->mixed && !h->fperm.empty() ? h->fperm[n] : n;
  *kh = h->mixed ? h->fkh[f] : h->md.kh; *kw = h->mixed ? h->fkw[f] : h->md.kw;
}
int check_inds(pbd_qp* q, const int32_t* inds, int n) {
  if (n < 0) return fail(q->h, PBD_ERR_ARG, "example cache: n < 0");
  if (!inds && n > q->n) return fail(q->h, PBD_ERR_ARG, "example cache: more examples asked for than the cache holds");
  if (inds) for (int i = 0; i < n; ++i)
    if (inds[i] < 0 || inds[i] >= q->n) return fail(q->h, PBD_ERR_ARG, "example cache: an index outside [0, n)");
  return PBD_OK;
}
// one column handed in: block bounds against len and k, the tail left alone; nb: its blocks
int check_column(const pbd_qp* q, const float* x, std::vector<int>& tab) {
  const int k = q->dev.k, len = q->dev.len;
  const float fb = x[0];
  if (!(fb >= 0.f) || fb != std::floor(fb) || fb > (float)k) return -1;
  const int nb = (int)fb;
  if (nb > q->dev.nbmax) return -2;
  int xp = 1;
  tab.clear();
  for (int b = 0; b < nb; ++b) {
    if (xp + 2 > k) return -1;
    const float f1 = x[xp], f2 = x[xp + 1];
    if (!(f1 >= 1.f) || !(f2 >= f1) || f1 != std::floor(f1) || f2 != std::floor(f2) || f2 > (float)len) return -1;
    const int i1 = (int)f1, i2 = (int)f2, ln = i2 - i1 + 1;
    if (xp + 2 + ln > k) return -1;
    tab.push_back(i1 - 1); tab.push_back(ln); tab.push_back(xp + 2);
    xp += 2 + ln;
  }
  return nb;
}
// do two blocks of one column share a dense element?  (the solver's pass adds a column into w with one writer per element)
char blocks_overlap(const std::vector<int>& tab) {
  std::vector<std::pair<int, int>> se;
  for (size_t b = 0; b + 2 < tab.size(); b += 3) se.emplace_back(tab[b], tab[b] + tab[b + 1]);
  std::sort(se.begin(), se.end());
  for (size_t b = 1; b < se.size(); ++b) if (se[b].first < se[b - 1].second) return 1;
  return 0;
}
}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int pbd_qp_create(pbd_handle* h, int capacity, double cpos, double cneg, const double* wreg, const double* w0, pbd_qp** out) {
  if (!h || !out) return PBD_ERR_ARG;
  *out = nullptr;
  if (capacity < 1 || !std::isfinite(cpos) || !std::isfinite(cneg)) return fail(h, PBD_ERR_ARG, "example cache: capacity >= 1, finite cpos / cneg");
  if (h->in_group) return fail(h, PBD_ERR_UNSUPPORTED, "example cache: pbd_group members are not supported");
  const int nbias = (int)h->biasw.size(), ndefs = h->md.ndefs, nf = h->md.nfilters, mp = h->max_parts;
  std::vector<int> foff((size_t)nf), fsz((size_t)nf);
  long long len = (long long)nbias + 4LL * ndefs;
  for (int n = 0; n < nf; ++n) {
    int kh, kw;
    filter_size(h, n, &kh, &kw);
    fsz[n] = kh * kw * PBD_FLEN;
    if (len >= (1LL << 24)) break;
    foff[n] = (int)len; len += fsz[n];
  }
  if (len >= (1LL << 24)) return fail(h, PBD_ERR_UNSUPPORTED, "example cache: the dense feature vector has 2^24 elements or more (block bounds are stored as floats)");
  if (wreg) for (long long j = 0; j < len; ++j)
    if (!std::isfinite(wreg[j]) || wreg[j] == 0.0) return fail(h, PBD_ERR_ARG, "example cache: wreg must be finite and non-zero");
  if (w0) for (long long j = 0; j < len; ++j)
    if (!std::isfinite(w0[j])) return fail(h, PBD_ERR_ARG, "example cache: w0 must be finite");
  // sparselen (train.m:207-239): 1 + 2 * blocks + values, the largest component; a part at its largest mixture's filter
  std::vector<int> caller((size_t)nf);
  for (int n = 0; n < nf; ++n) caller[h->mixed && !h->fperm.empty() ? h->fperm[n] : n] = n;
  long long k = 1;
  for (int c = 0; c < h->md.ncomponents; ++c) {
    const int f0 = h->part_offset[c], np = h->part_offset[c + 1] - f0;
    long long kc = 1 + 2LL * (3 * np - 1);
    for (int p = 0; p < np; ++p) {
      int wl = 0;
      for (int fm = h->mix_offset[f0 + p]; fm < h->mix_offset[f0 + p + 1]; ++fm) wl = std::max(wl, fsz[caller[h->filterid[fm]]]);
      kc += 1 + (p > 0 ? 4 : 0) + wl;
    }
    k = std::max(k, kc);
  }
  if (k * (long long)capacity >= (1LL << 40)) return fail(h, PBD_ERR_ARG, "example cache: capacity too large");
  ON_DEVICE(h);
  pbd_qp* q = new pbd_qp;
  q->h = h; q->cpos = cpos; q->cneg = cneg; q->foff = foff;
  QpDev& D = q->dev;
  D.k = (int)k; D.len = (int)len; D.capacity = capacity; D.nbmax = 3 * mp;
  const size_t cap = (size_t)capacity;
  int rc;
  if ((rc = q->alloc(&D.x, cap * (size_t)k)) || (rc = q->alloc(&D.ids, cap * 5)) || (rc = q->alloc(&D.b, cap)) ||
      (rc = q->alloc(&D.d, cap)) || (rc = q->alloc(&D.tab, cap * D.nbmax * 3)) || (rc = q->alloc(&D.nblk, cap)) ||
      (rc = q->alloc(&D.slot, cap)) || (rc = q->alloc(&q->d_wreg, (size_t)len)) || (rc = q->alloc(&q->d_w0, (size_t)len)) ||
      (rc = q->alloc(&q->d_foff, (size_t)nf))) {
    pbd_qp_destroy(q);
    return rc;
  }
  // model2vec.m: wreg = .01 at the root bias of every component, 1 elsewhere; w0 = .01 at elements 0 and 2 of every deformation
  std::vector<double> vr((size_t)len, 1.0), v0((size_t)len, 0.0);
  if (wreg) std::copy(wreg, wreg + len, vr.begin());
  else for (int c = 0; c < h->md.ncomponents; ++c) vr[h->biasid[h->mix_offset[h->part_offset[c]]]] = .01;
  if (w0) std::copy(w0, w0 + len, v0.begin());
  else for (int dd = 0; dd < ndefs; ++dd) v0[(size_t)nbias + 4 * dd] = v0[(size_t)nbias + 4 * dd + 2] = .01;
  q->slot.resize(cap);
  q->overlap.assign(cap, 0);
  for (size_t i = 0; i < cap; ++i) q->slot[i] = (int)i;
  hipError_t e = hipSuccess;
  auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; };
  chk(hipMemsetAsync(D.x, 0, sizeof(float) * cap * (size_t)k, h->stream));
  chk(hipMemsetAsync(D.ids, 0, sizeof(int) * cap * 5, h->stream));
  chk(hipMemsetAsync(D.b, 0, sizeof(float) * cap, h->stream));
  chk(hipMemsetAsync(D.d, 0, sizeof(double) * cap, h->stream));
  chk(hipMemsetAsync(D.tab, 0, sizeof(int) * cap * D.nbmax * 3, h->stream));
  chk(hipMemsetAsync(D.nblk, 0, sizeof(int) * cap, h->stream));
  chk(hipMemcpyAsync(D.slot, q->slot.data(), sizeof(int) * cap, hipMemcpyHostToDevice, h->stream));
  chk(hipMemcpyAsync(q->d_wreg, vr.data(), sizeof(double) * (size_t)len, hipMemcpyHostToDevice, h->stream));
  chk(hipMemcpyAsync(q->d_w0, v0.data(), sizeof(double) * (size_t)len, hipMemcpyHostToDevice, h->stream));
  chk(hipMemcpyAsync(q->d_foff, foff.data(), sizeof(int) * (size_t)nf, hipMemcpyHostToDevice, h->stream));
  chk(hipStreamSynchronize(h->stream));
  if (e != hipSuccess) {
    pbd_qp_destroy(q);
    return fail(h, PBD_ERR_HIP, std::string("example cache: ") + hipGetErrorString(e));
  }
  *out = q;
  return PBD_OK;
}

void pbd_qp_destroy(pbd_qp* q) {
  if (!q) return;
  hipStreamSynchronize(q->h->stream);   // (like pbd_destroy: the caller's current device is left alone)
  delete q;
}

int pbd_qp_dims(const pbd_qp* q, int* len, int* k, int* capacity, int* n) {
  if (!q) return PBD_ERR_ARG;
  if (len) *len = q->dev.len;
  if (k) *k = q->dev.k;
  if (capacity) *capacity = q->dev.capacity;
  if (n) *n = q->n;
  return PBD_OK;
}

int pbd_qp_footprint(const pbd_qp* q, size_t* bytes) {
  if (!q || !bytes) return PBD_ERR_ARG;
  *bytes = q->bufs.bytes();
  return PBD_OK;
}

// qp_write.m:34-35 for one record: its blocks' dense starts are distinct iff no bias, def or filter id repeats among its parts
static bool repeats_block(const pbd_handle* h, const pbd_candidate_head& hd, const int32_t* lc) {
  const int f0 = h->part_offset[hd.component], np = hd.nparts;
  std::vector<int> fi, di, bi;
  for (int p = 0; p < np; ++p) {
    const int fm = h->mix_offset[f0 + p] + lc[p * 3 + 2];
    fi.push_back(h->filterid[fm]);
    if (p == 0) bi.push_back(h->biasid[h->mix_offset[f0]]);
    else {
      const int q = h->parentid[f0 + p];
      di.push_back(h->defid[fm]);
      bi.push_back(h->biasid[fm] + (q >= 0 && q < np ? lc[q * 3 + 2] : 0));
    }
  }
  for (std::vector<int>* v : {&fi, &di, &bi}) {
    std::sort(v->begin(), v->end());
    if (std::adjacent_find(v->begin(), v->end()) != v->end()) return true;
  }
  return false;
}

int pbd_qp_write(pbd_qp* q, const pbd_candidate_head* heads, const int32_t* locs, int count, int label, int id, int* written) {
  if (!q) return PBD_ERR_ARG;
  pbd_handle* h = q->h;
  if (!written) return fail(h, PBD_ERR_ARG, "example cache: written is NULL");
  int rc = pbd_i_fv_check(h, heads, locs, count);   // every refusal of pbd_candidates_features_dev
  if (rc) return rc;
  for (int i = 0; i < count; ++i)
    if (repeats_block(h, heads[i], locs + (size_t)i * h->max_parts * 3))
      return fail(h, PBD_ERR_ARG, "example cache: a record's blocks repeat a dense start index (two of its parts share a filter, def or bias "
                                  "id): qp_write's assertion (matlab/learning/qp_write.m:34-35)");
  *written = 0;
  if (count == 0) return PBD_OK;
  const int n = std::min(count, q->dev.capacity - q->n);   // a full cache is no error (qp_write.m:21-23)
  if (n > 0) {   // (a full cache returns here: nothing is uploaded, nothing synchronised)
    QpWriteArgs a{};
    if ((rc = pbd_i_fv_upload(h, heads, locs, n, &a.fv))) return rc;
    a.fv.rec0 = 0; a.fv.n = n;
    a.q = q->dev; a.n0 = q->n;
    a.wreg = q->d_wreg; a.w0 = q->d_w0; a.foff = q->d_foff;
    a.C = label > 0 ? q->cpos : q->cneg; a.label = label; a.id = id;
    launch_qp_write(a, h->ts, h->stream);
    LAUNCHCHK(h, "example cache write");
    for (int i = 0; i < n; ++i) q->overlap[q->slot[q->n + i]] = 0;   // (a record's blocks never overlap: the check above)
    q->meta_dirty = true;
    if ((rc = pbd_i_qp_appended(q, q->n, n))) return rc;
    q->n += n;
  }
  *written = n;
  return PBD_OK;
}

int pbd_qp_score_dev(pbd_qp* q, const double* d_w, const int32_t* d_inds, int n, double* d_out) {
  if (!q) return PBD_ERR_ARG;
  pbd_handle* h = q->h;
  if (n < 0 || !d_w || (n > 0 && !d_out) || (!d_inds && n > q->n)) return fail(h, PBD_ERR_ARG, "example cache score: w / out / n");
  if (n == 0) return PBD_OK;
  ON_DEVICE(h);
  launch_qp_score(q->dev, d_w, d_inds, n, d_out, h->stream);
  LAUNCHCHK(h, "example cache score");
  return PBD_OK;
}

int pbd_qp_score(pbd_qp* q, const double* w, const int32_t* inds, int n, double* out) {
  if (!q) return PBD_ERR_ARG;
  pbd_handle* h = q->h;
  if (!w || (n > 0 && !out)) return fail(h, PBD_ERR_ARG, "example cache score: w / out");
  int rc = check_inds(q, inds, n);
  if (rc || n == 0) return rc;
  ON_DEVICE(h);
  const size_t len = (size_t)q->dev.len;
  CallScratch t(h);
  char* tp;
  if ((rc = t.get(&tp, sizeof(double) * (len + n) + sizeof(int) * n, "example cache: "))) return rc;
  double* d_w = (double*)tp; double* d_out = d_w + len; int* d_inds = (int*)(d_out + n);
  HIPCHK(h, hipMemcpyAsync(d_w, w, sizeof(double) * len, hipMemcpyHostToDevice, h->stream));
  if (inds) HIPCHK(h, hipMemcpyAsync(d_inds, inds, sizeof(int) * n, hipMemcpyHostToDevice, h->stream));
  launch_qp_score(q->dev, d_w, inds ? d_inds : nullptr, n, d_out, h->stream);
  LAUNCHCHK(h, "example cache score");
  HIPCHK(h, hipMemcpyAsync(out, d_out, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  return finish(h, "example cache score: ");
}

int pbd_qp_lincomb_dev(pbd_qp* q, const double* d_a, const int32_t* d_inds, int n, double* d_w_out) {
  if (!q) return PBD_ERR_ARG;
  pbd_handle* h = q->h;
  if (n < 0 || !d_w_out || (n > 0 && !d_a) || (!d_inds && n > q->n)) return fail(h, PBD_ERR_ARG, "example cache lincomb: a / w_out / n");
  ON_DEVICE(h);
  launch_qp_lincomb(q->dev, d_a, d_inds, n, d_w_out, h->stream);
  LAUNCHCHK(h, "example cache lincomb");
  return PBD_OK;
}

int pbd_qp_lincomb(pbd_qp* q, const double* a, const int32_t* inds, int n, double* w_out) {
  if (!q) return PBD_ERR_ARG;
  pbd_handle* h = q->h;
  if (!w_out || (n > 0 && !a)) return fail(h, PBD_ERR_ARG, "example cache lincomb: a / w_out");
  int rc = check_inds(q, inds, n);
  if (rc) return rc;
  ON_DEVICE(h);
  const size_t len = (size_t)q->dev.len, cap = (size_t)q->dev.capacity;
  CallScratch t(h);
  char* tp;
  if ((rc = t.get(&tp, sizeof(double) * (len + cap) + sizeof(int) * std::max(n, 1), "example cache: "))) return rc;
  double* d_w = (double*)tp; double* d_a = d_w + len; int* d_inds = (int*)(d_a + cap);
  if (n > 0) HIPCHK(h, hipMemcpyAsync(d_a, a, sizeof(double) * cap, hipMemcpyHostToDevice, h->stream));
  if (inds && n > 0) HIPCHK(h, hipMemcpyAsync(d_inds, inds, sizeof(int) * n, hipMemcpyHostToDevice, h->stream));
  launch_qp_lincomb(q->dev, d_a, inds ? d_inds : nullptr, n, d_w, h->stream);
  LAUNCHCHK(h, "example cache lincomb");
  HIPCHK(h, hipMemcpyAsync(w_out, d_w, sizeof(double) * len, hipMemcpyDeviceToHost, h->stream));
  return finish(h, "example cache lincomb: ");
}

int pbd_qp_keep(pbd_qp* q, const int32_t* inds, int n) {
  if (!q) return PBD_ERR_ARG;
  pbd_handle* h = q->h;
  if (n < 0 || n > q->n || (n > 0 && !inds)) return fail(h, PBD_ERR_ARG, "example cache keep: inds / n");
  for (int i = 0; i < n; ++i)
    if (inds[i] < 0 || inds[i] >= q->n || (i > 0 && inds[i] <= inds[i - 1]))
      return fail(h, PBD_ERR_ARG, "example cache keep: indices must be strictly ascending and inside [0, n)");
  // the kept examples' columns first, in order; the freed columns behind them, then the ones never used
  std::vector<int> ns;
  std::vector<char> kept((size_t)q->n, 0);
  for (int i = 0; i < n; ++i) { ns.push_back(q->slot[inds[i]]); kept[inds[i]] = 1; }
  for (int i = 0; i < q->n; ++i) if (!kept[i]) ns.push_back(q->slot[i]);
  for (int i = q->n; i < q->dev.capacity; ++i) ns.push_back(q->slot[i]);
  ON_DEVICE(h);
  HIPCHK(h, hipMemcpyAsync(q->dev.slot, ns.data(), sizeof(int) * ns.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // (`ns` is pageable: the copy is done when it goes)
  q->slot.swap(ns);
  q->n = n;
  return PBD_OK;
}

int pbd_qp_get(pbd_qp* q, int i0, int n, float* x, int32_t* ids, float* b, double* d) {
  if (!q) return PBD_ERR_ARG;
  pbd_handle* h = q->h;
  if (i0 < 0 || n < 0 || (long long)i0 + n > q->dev.capacity) return fail(h, PBD_ERR_ARG, "example cache get: i0 + n exceeds the capacity");
  if (n == 0) return PBD_OK;
  ON_DEVICE(h);
  const size_t k = (size_t)q->dev.k;
  for (int i = 0; i < n; ++i) {   // by column: consecutive examples need not be consecutive columns (pbd_qp_keep)
    const size_t c = (size_t)q->slot[i0 + i];
    if (x) HIPCHK(h, hipMemcpyAsync(x + k * i, q->dev.x + k * c, sizeof(float) * k, hipMemcpyDeviceToHost, h->stream));
    if (ids) HIPCHK(h, hipMemcpyAsync(ids + 5 * (size_t)i, q->dev.ids + 5 * c, sizeof(int) * 5, hipMemcpyDeviceToHost, h->stream));
    if (b) HIPCHK(h, hipMemcpyAsync(b + i, q->dev.b + c, sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (d) HIPCHK(h, hipMemcpyAsync(d + i, q->dev.d + c, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  return finish(h, "example cache get: ");
}

int pbd_qp_put(pbd_qp* q, int n, const float* x, const int32_t* ids, const float* b, const double* d) {
  if (!q) return PBD_ERR_ARG;
  pbd_handle* h = q->h;
  if (n < 0 || (n > 0 && (!x || !ids || !b || !d))) return fail(h, PBD_ERR_ARG, "example cache put: x / ids / b / d / n");
  if (n > q->dev.capacity - q->n) return fail(h, PBD_ERR_CAPACITY, "example cache put: more columns than the cache has room for");
  const size_t k = (size_t)q->dev.k, nbm = (size_t)q->dev.nbmax;
  std::vector<std::vector<int>> tabs((size_t)n);
  for (int i = 0; i < n; ++i) {
    const int nb = check_column(q, x + k * i, tabs[i]);
    if (nb == -2) return fail(h, PBD_ERR_UNSUPPORTED, "example cache put: a column has more than 3 * max_parts blocks");
    if (nb < 0) return fail(h, PBD_ERR_ARG, "example cache put: a column's block bounds do not fit the dense length or the column length");
  }
  if (n == 0) return PBD_OK;
  ON_DEVICE(h);
  std::vector<int> nbv((size_t)n);
  for (int i = 0; i < n; ++i) {
    const size_t c = (size_t)q->slot[q->n + i];
    nbv[i] = (int)tabs[i].size() / 3;
    HIPCHK(h, hipMemcpyAsync(q->dev.x + k * c, x + k * i, sizeof(float) * k, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(q->dev.ids + 5 * c, ids + 5 * (size_t)i, sizeof(int) * 5, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(q->dev.b + c, b + i, sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(q->dev.d + c, d + i, sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (nbv[i]) HIPCHK(h, hipMemcpyAsync(q->dev.tab + c * nbm * 3, tabs[i].data(), sizeof(int) * 3 * nbv[i], hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(q->dev.nblk + c, &nbv[i], sizeof(int), hipMemcpyHostToDevice, h->stream));
  }
  q->meta_dirty = true;
  int rc = pbd_i_qp_appended(q, q->n, n);
  if (!rc) rc = finish(h, "example cache put: ");   // (the tables are pageable: the copies are done when they go)
  if (rc) return rc;
  for (int i = 0; i < n; ++i) q->overlap[q->slot[q->n + i]] = blocks_overlap(tabs[i]);
  q->n += n;
  return PBD_OK;
}

}  // extern "C"
#pragma GCC visibility pop
