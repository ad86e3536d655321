// pbd_weights.cpp — a live handle's weights and threshold replaced (include/pbd_c.h "weight and threshold updates"; kernels:
// k_weights.hip): train.m:94,112's model = vec2model(qp_w, model) without a new handle, so that the example cache tied to the handle
// (pbd_qp_create) goes on reading its feature planes.
//
// One rule: whatever is derived from weights is rebuilt by what builds it at create.  The filter banks' buffers (upload_bank's d_wT,
// d_wS, d_oscale) and d_biasw are written again in place, from the same float32 values, by kernels that reproduce the host packing bit
// for bit; the frame plan's tables (fold biases, the distance transform's coefficients, the root biases) and the captured graph are
// dropped whole — free_frame — and planned again by the next frame from the host mirrors; k_partscore's mixture table is rewritten in
// place if it exists.  Nothing is patched field by field.
#include <cmath>
#include "pbd_internal.hpp"

namespace {
// Model.feature_layout(): [biasw | defw (ndefs x 4) | the filters back to back in the CALLER's order]
struct WeightLayout {
  size_t nbias, ndef4, len;
  std::vector<int> start;      // [internal filter] its first element in the vector
  std::vector<size_t> mirror;  // [internal filter] its first element in pbd_handle::filters (the internal order)
  std::vector<int> size;       // [internal filter] kh * kw * flen
};
WeightLayout layout_of(const pbd_handle* h) {
  WeightLayout L;
  const int nf = h->md.nfilters;
  L.nbias = h->biasw.size(); L.ndef4 = h->defw.size();
  L.start.assign(nf, 0); L.mirror.assign(nf, 0); L.size.assign(nf, 0);
  size_t at = L.nbias + L.ndef4;
  for (int n = 0; n < nf; ++n) {   // the caller's filter n
    const int f = h->mixed ? h->fperm[n] : n;
    L.size[f] = (h->mixed ? h->fkh[f] * h->fkw[f] : h->md.kh * h->md.kw) * h->md.flen;
    L.start[f] = (int)at;
    at += L.size[f];
  }
  L.len = at;
  size_t m = 0;
  for (int f = 0; f < nf; ++f) { L.mirror[f] = m; m += L.size[f]; }
  return L;
}
// the refusals every update shares, in front of anything that touches the device
int check_update(pbd_handle* h, const char* what) {
  if (h->in_group) return fail(h, PBD_ERR_UNSUPPORTED, std::string(what) + ": pbd_group members are not supported");
  if (h->pf.active) return fail(h, PBD_ERR_STATE, "a frame is in flight: collect it first");
  return PBD_OK;
}
// w: len doubles on the host, or on the handle's device
int set_weights(pbd_handle* h, const double* w, int len, bool on_host) {
  if (!w) return fail(h, PBD_ERR_ARG, "weights: null vector");
  const WeightLayout L = layout_of(h);
  if (len < 0 || (size_t)len != L.len)
    return fail(h, PBD_ERR_ARG, "weights: len must be the model's " + std::to_string(L.len) + " elements (Model.feature_layout())");
  int rc = check_update(h, "weights");
  if (rc) return rc;
  ON_DEVICE(h);
  CallScratch tmp(h);
  double* d_up = nullptr;
  if (on_host) {
    if ((rc = tmp.get(&d_up, L.len, "weights: "))) return rc;
    HIPCHK(h, hipMemcpyAsync(d_up, w, sizeof(double) * L.len, hipMemcpyHostToDevice, h->stream));
  }
  const double* d_w = on_host ? d_up : w;
  // the float32 values and the validation word, in one buffer and one copy back: the host mirror and what the checks below read
  float* d_stage; int* d_src;
  if ((rc = tmp.get(&d_stage, L.len + 1, "weights: ")) || (rc = tmp.get(&d_src, L.start.size(), "weights: "))) return rc;
  launch_weights_round(d_w, len, d_stage, (int*)(d_stage + L.len), h->stream);
  LAUNCHCHK(h, "weights");
  std::vector<float> st(L.len + 1);
  HIPCHK(h, hipMemcpyAsync(st.data(), d_stage, sizeof(float) * st.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_src, L.start.data(), sizeof(int) * L.start.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int bad;
  memcpy(&bad, &st[L.len], sizeof(int));
  if (bad >= 0)
    return fail(h, PBD_ERR_ARG, std::string("weights: non-finite ") + ((size_t)bad < L.nbias ? "bias" : (size_t)bad < L.nbias + L.ndef4 ?
                "deformation weight" : "filter weight") + " (element " + std::to_string(bad) + " as a float32)");
  const float* defw = st.data() + L.nbias;
  for (const PartInfo& P : h->parts)   // ingest_model's check, of the deformations it checks
    for (int k = 0; P.p > 0 && k < P.K; ++k)
      if (defw[P.defid[k] * 4] == 0.f || defw[P.defid[k] * 4 + 2] == 0.f)
        return fail(h, PBD_ERR_ARG, "model: quadratic deformation weights must be non-zero "
                                    "(include/DistanceTransform.hpp:99 divides by 2a)");
  if (h->split_parts)
    for (size_t i = L.nbias + L.ndef4; i < L.len; ++i)
      if (!(std::fabs(st[i]) < 3.0e38f)) return fail(h, PBD_ERR_UNSUPPORTED, "PBD_CONV_SPLIT: a filter weight outside bfloat16's finite range");

  // ---- nothing refuses from here on ----
  std::copy(st.begin(), st.begin() + L.nbias, h->biasw.begin());
  std::copy(defw, defw + L.ndef4, h->defw.begin());
  for (size_t f = 0; f < L.start.size(); ++f) std::copy(st.begin() + L.start[f], st.begin() + L.start[f] + L.size[f], h->filters.begin() + L.mirror[f]);
  auto pack = [&](int n0, int nf, int kh, int kw, int nfpad, void* wT, uint16_t* wS, float* oscale) {
    launch_bank_pack(d_stage, d_src + n0, nf, kh, kw, nfpad, wT, h->ts, h->stream);
    if (h->split_parts == 3) launch_bank_split(d_stage, d_src + n0, nf, kh, kw, wS, h->stream);
    if (h->split_parts == 2) launch_bank_split16(d_stage, d_src + n0, nf, kh, kw, wS, oscale, h->stream);
  };
  if (h->mixed) for (const SizeGroup& g : h->groups) pack(g.n0, g.nf, g.kh, g.kw, g.nfpad, g.d_wT, g.d_wS, g.d_oscale);
  else pack(0, h->md.nfilters, h->md.kh, h->md.kw, h->nfpad, h->d_wT, h->d_wS, h->d_split_oscale);
  LAUNCHCHK(h, "weights: filter banks");
  HIPCHK(h, hipMemcpyAsync(h->d_biasw, d_stage, sizeof(float) * L.nbias, hipMemcpyDeviceToDevice, h->stream));   // (its trailing 0 stays)
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if ((rc = pbd_i_ps_reweigh(h))) return rc;
  free_frame(h);   // the plan's tables and the captured graph bake weights in, the resident responses and DP tables are the old model's
  return PBD_OK;
}
}  // namespace

int pbd_i_set_weights_dev(pbd_handle* h, const double* d_w, int len) { return set_weights(h, d_w, len, false); }

#pragma GCC visibility push(default)
extern "C" {

int pbd_set_weights_dev(pbd_handle* h, const double* d_w, int len) { return h ? set_weights(h, d_w, len, false) : PBD_ERR_ARG; }
int pbd_set_weights(pbd_handle* h, const double* w, int len) { return h ? set_weights(h, w, len, true) : PBD_ERR_ARG; }

int pbd_get_weights(const pbd_handle* h, double* w, int len) {
  if (!h || !w) return PBD_ERR_ARG;
  const WeightLayout L = layout_of(h);
  if (len < 0 || (size_t)len != L.len) return PBD_ERR_ARG;
  std::copy(h->biasw.begin(), h->biasw.end(), w);
  std::copy(h->defw.begin(), h->defw.end(), w + L.nbias);
  for (size_t f = 0; f < L.start.size(); ++f) std::copy(h->filters.begin() + L.mirror[f], h->filters.begin() + L.mirror[f] + L.size[f], w + L.start[f]);
  return PBD_OK;
}

int pbd_set_threshold(pbd_handle* h, float thresh) {
  if (!h) return PBD_ERR_ARG;
  if (thresh != thresh) return fail(h, PBD_ERR_ARG, "threshold: NaN");
  int rc = check_update(h, "threshold");
  if (rc) return rc;
  ON_DEVICE(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->md.thresh = thresh;
  drop_graph(h);                          // the threshold is a launch argument of the captured k_root
  if (h->have_dp) h->root_dirty = true;   // a resident min()'s hit list is the old threshold's: argmin thresholds the root tables again
  return PBD_OK;
}

int pbd_get_threshold(const pbd_handle* h, float* thresh) {
  if (!h || !thresh) return PBD_ERR_ARG;
  *thresh = h->md.thresh;
  return PBD_OK;
}

}  // extern "C"
#pragma GCC visibility pop
