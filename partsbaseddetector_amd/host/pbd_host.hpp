// pbd_host.hpp — C++ host side above the C ABI (include/pbd_c.h), mirroring the reference's
// interfaces so code written against wg-perception/PartsBasedDetector reads the same:
//
//   reference                                              here (namespace pbd)
//   IFeatures            include/IFeatures.hpp:49-73       pbd::IFeatures, pbd::HipHOGFeatures
//   IConvolutionEngine   include/IConvolutionEngine.hpp:44-68  pbd::IConvolutionEngine, pbd::HipConvolutionEngine
//   DynamicProgram<T>    include/DynamicProgram.hpp:61-77  pbd::DynamicProgram<T>
//   PartsBasedDetector<T> include/PartsBasedDetector.hpp:152-175  pbd::PartsBasedDetector<T>
//   Candidate            include/Candidate.hpp:56-111,277-304  pbd::Candidate
//   Model                include/Model.hpp:49-122          pbd::Model (+ pbd::BinaryModel reader)
//
// The reference passes cv::Mat; OpenCV is not a dependency of this library, so a minimal dense
// matrix (pbd::Mat: rows, cols, channels, 8U/32S/32F) carries the same data.  The OpenCV-typed
// adaptors for dropping the engines into the reference tree itself are in INTEGRATION.md.
// All numerics run in libpbd_hip.so; this header only marshals.  T = float or double, the two
// instantiations the reference declares (src/PartsBasedDetector.cpp:132-133).
#ifndef PBD_HOST_HPP_
#define PBD_HOST_HPP_

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/pbd_c.h"

namespace pbd {

enum { PBD_8U = 0, PBD_16U = 2, PBD_32S = 4, PBD_32F = 5, PBD_64F = 6 };  // depth codes (numerically OpenCV's CV_8U/16U/32S/32F/64F = pbd_c.h's PBD_DEPTH_*)
template <typename T> struct DataType;               // cv::DataType<T>::type
template <> struct DataType<float> { enum { type = PBD_32F, scalar = PBD_SCALAR_F32 }; };
template <> struct DataType<double> { enum { type = PBD_64F, scalar = PBD_SCALAR_F64 }; };

class Exception : public std::runtime_error {   // plays the role of cv::Exception
 public:
  int code;
  Exception(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

class Mat {
 public:
  int rows = 0, cols = 0;
  Mat() {}
  Mat(int r, int c, int depth, int cn = 1) { create(r, c, depth, cn); }
  void create(int r, int c, int depth, int cn = 1) {
    rows = r; cols = c; depth_ = depth; cn_ = cn;
    buf_.assign((size_t)r * c * cn * elem1(), 0);
  }
  bool empty() const { return buf_.empty(); }
  int depth() const { return depth_; }
  int channels() const { return cn_; }
  size_t elem1() const { return depth_ == PBD_8U ? 1 : depth_ == PBD_16U ? 2 : depth_ == PBD_64F ? 8 : 4; }
  size_t step() const { return (size_t)cols * cn_ * elem1(); }
  size_t bytes() const { return buf_.size(); }
  template <typename T> T* ptr(int r = 0) { return (T*)(buf_.data() + (size_t)r * step()); }
  template <typename T> const T* ptr(int r = 0) const { return (const T*)(buf_.data() + (size_t)r * step()); }
  template <typename T> T& at(int r, int c) { return ptr<T>(r)[c]; }
  template <typename T> const T& at(int r, int c) const { return ptr<T>(r)[c]; }
 private:
  int depth_ = PBD_8U, cn_ = 1;
  std::vector<uint8_t> buf_;
};

struct Rect { int x, y, width, height; };
struct Point { int x, y; };
typedef std::vector<int> vectori;
typedef std::vector<float> vectorf;
typedef std::vector<Mat> vectorMat;
typedef std::vector<vectorMat> vector2DMat;
typedef std::vector<vector2DMat> vector3DMat;
typedef std::vector<vector3DMat> vector4DMat;
typedef std::vector<vectori> vector2Di;
typedef std::vector<vector2Di> vector3Di;
typedef std::vector<vectorf> vector2Df;

// a ground-truth box of testmodel_gtbox.m: inclusive corners (x1, y1, x2, y2), as doubles (include/pbd_c.h "best pose per ground-truth box")
struct GtBox { double x1, y1, x2, y2; };

// an 8-bit frame in device memory (include/pbd_c.h "virtual positives"): rows of `cols` pixels of `channels` bytes, `step` bytes apart,
// from the device pointer `data` on; the caller keeps the allocation alive
struct DeviceFrame { const void* data; int rows, cols, channels; size_t step; };

// ---- include/Candidate.hpp:56-111 ---------------------------------------------------------
class Candidate {
  std::vector<Rect> parts_;
  vectorf confidence_;
  int component_ = 0;
  std::vector<pbd_part_score> part_scores_;
 public:
  // PartsBasedDetector::setPartScores: the three terms (app, def, bias) of every part's score; empty with the step off
  const std::vector<pbd_part_score>& partScores() const { return part_scores_; }
  void setPartScores(const pbd_part_score* ps, int nparts) {   // confidence()[p], p >= 1, = (float)score_p; [0] stays the root score
    part_scores_.assign(ps, ps + nparts);
    for (int p = 1; p < nparts && p < (int)confidence_.size(); ++p) confidence_[p] = (float)((ps[p].app + ps[p].def) + ps[p].bias);
  }
  int level = -1;                        // extra: pyramid level of the root
  std::vector<int> locs;                 // extra: (x, y, mixture) per part, in cells
  const std::vector<Rect>& parts() const { return parts_; }
  const vectorf& confidence() const { return confidence_; }
  void addPart(Rect r, float c) { parts_.push_back(r); confidence_.push_back(c); }
  float score() const { return confidence_.empty() ? -std::numeric_limits<float>::infinity() : confidence_[0]; }
  void setScore(float c) { if (confidence_.empty()) confidence_.resize(1); confidence_[0] = c; }   // :76
  void setComponent(int c) { component_ = c; }
  int component() const { return component_; }
  void resize(const float factor) {      // :82-89: `int *= float` — converted to float, multiplied, truncated back
    for (Rect& r : parts_) {
      r.height = (int)((float)r.height * factor); r.width = (int)((float)r.width * factor);
      r.y = (int)((float)r.y * factor); r.x = (int)((float)r.x * factor);
    }
  }
  Rect boundingBox() const {             // union of the part rects (:103-109)
    Rect h = parts_[0];
    for (const Rect& q : parts_) {
      const int x1 = std::min(h.x, q.x), y1 = std::min(h.y, q.y);
      h.width = std::max(h.x + h.width, q.x + q.width) - x1;
      h.height = std::max(h.y + h.height, q.y + q.height) - y1;
      h.x = x1; h.y = y1;
    }
    return h;
  }
  static void sort(std::vector<Candidate>& c);                                         // :97-99
  static void nonMaximaSuppression(int im_w, int im_h, std::vector<Candidate>& c, float overlap = 0.0f);  // :277-304
  // matlab/detection/nms.m on sorted candidates (pbd_candidates_nms_parts): part by part and by the covering box, over the kept
  // detection's area, after a cut to the `top` best (1000: nms.m's; 0: none)
  static void nonMaximaSuppressionParts(std::vector<Candidate>& c, float overlap = 0.3f, int top = 1000);
  // matlab/detection/bestoverlap.m (pbd_candidates_best_overlap): per gt box the index in `c` of the highest-scoring candidate whose
  // box of part centres covers more than `overlap` of it, or -1; the first of equal scores.  o (may be null): the winners' overlaps
  static std::vector<int> bestOverlap(const std::vector<Candidate>& c, const std::vector<GtBox>& gt, double overlap = 0.3,
                                      std::vector<double>* o = nullptr);
};
typedef std::vector<Candidate> vectorCandidate;

// ---- include/Model.hpp:49-122 ---------------------------------------------------------------
class Model {
 protected:
  vectorMat filtersw_; vector2Df defw_; vectorf biasw_; std::vector<Point> anchors_;
  vector3Di biasid_, filterid_, defid_; vector2Di parentid_;
  std::string name_; int nscales_ = 0; float thresh_ = 0; int binsize_ = 0, flen_ = 0, norient_ = 0;
 public:
  virtual ~Model() {}
  vectorMat& filters() { return filtersw_; }
  vector2Df& def() { return defw_; }
  vectorf& bias() { return biasw_; }
  std::vector<Point>& anchors() { return anchors_; }
  vector3Di& filterid() { return filterid_; }
  vector3Di& biasid() { return biasid_; }
  vector3Di& defid() { return defid_; }
  vector2Di& parentid() { return parentid_; }
  std::string name() { return name_; }
  float thresh() const { return thresh_; }
  void setThresh(float t) { thresh_ = t; }
  int binsize() const { return binsize_; }
  int nscales() const { return nscales_; }
  int flen() const { return flen_; }
  int norient() const { return norient_; }
  int ncomponents() const { return (int)filterid_.size(); }
  virtual bool deserialize(const std::string& filename) = 0;
};

// Flat little-endian dump of the fields above (written by partsbaseddetector_amd.model.Model.save);
// the reference's own formats (cv::FileStorage XML/YAML, .mat) are SURVEY §8(f) "next".
class BinaryModel : public Model {
  static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }
 public:
  bool deserialize(const std::string& filename) override {
    FILE* f = fopen(filename.c_str(), "rb");
    if (!f) return false;
    int32_t hd[12];
    char magic[8];
    bool ok = rd(f, magic, 8) && !memcmp(magic, "PBDMODL1", 8) && rd(f, hd, sizeof(hd));
    if (!ok) { fclose(f); return false; }
    const int nf = hd[0], kh = hd[1], kw = hd[2];
    flen_ = hd[3]; norient_ = hd[4]; binsize_ = hd[5]; nscales_ = hd[6];
    const int ndefs = hd[7], nbias = hd[8], ncomp = hd[9];
    // the header counts size every allocation below: bound them by what the file can actually hold
    fseek(f, 0, SEEK_END);
    const long long fsize = ftell(f);
    fseek(f, 8 + (long)sizeof(hd), SEEK_SET);
    const long long per_filter = (long long)kh * kw * flen_ * 4;
    if (nf <= 0 || kh <= 0 || kw <= 0 || kh > 64 || kw > 64 || flen_ <= 0 || flen_ > 1024 || ndefs < 0 || nbias <= 0 || ncomp <= 0 ||
        (long long)nf * per_filter > fsize || (long long)ndefs * 24 > fsize || (long long)nbias * 4 > fsize || (long long)ncomp * 4 > fsize) {
      fclose(f);
      return false;
    }
    ok = rd(f, &thresh_, 4);
    filtersw_.resize(nf);
    for (int n = 0; n < nf && ok; ++n) { filtersw_[n].create(kh, kw * flen_, PBD_32F); ok = rd(f, filtersw_[n].ptr<float>(), (size_t)kh * kw * flen_ * 4); }
    defw_.assign(ndefs, vectorf(4)); anchors_.resize(ndefs);
    for (int d = 0; d < ndefs && ok; ++d) ok = rd(f, defw_[d].data(), 16);
    for (int d = 0; d < ndefs && ok; ++d) { int32_t a[2]; ok = rd(f, a, 8); anchors_[d] = Point{a[0], a[1]}; }
    biasw_.resize(nbias);
    ok = ok && rd(f, biasw_.data(), (size_t)nbias * 4);
    filterid_.resize(ncomp); biasid_.resize(ncomp); defid_.resize(ncomp); parentid_.resize(ncomp);
    for (int c = 0; c < ncomp && ok; ++c) {
      int32_t np; ok = rd(f, &np, 4);
      if (!ok || np <= 0 || (long long)np * 8 > fsize) { ok = false; break; }
      filterid_[c].resize(np); biasid_[c].resize(np); defid_[c].resize(np); parentid_[c].resize(np);
      for (int p = 0; p < np && ok; ++p) {
        int32_t pk[2]; ok = rd(f, pk, 8);
        if (!ok || pk[1] <= 0 || (long long)pk[1] * 12 > fsize) { ok = false; break; }
        parentid_[c][p] = pk[0];
        filterid_[c][p].resize(pk[1]); biasid_[c][p].resize(pk[1]); defid_[c][p].resize(pk[1]);
        ok = ok && rd(f, filterid_[c][p].data(), 4 * pk[1]) && rd(f, defid_[c][p].data(), 4 * pk[1]) && rd(f, biasid_[c][p].data(), 4 * pk[1]);
      }
    }
    name_ = filename;
    fclose(f);
    return ok;
  }
  // The dump carries ONE kh, kw (header): a bank of mixed sizes is refused (false, no file written) — writing kh_0 * kw_0 * flen floats
  // of every filter would read past the end of any filter smaller than the first
  bool serialize(const std::string& filename) const {
    if (filtersw_.empty()) return false;
    const int kh = filtersw_[0].rows, kw = filtersw_[0].cols / flen_;
    for (const Mat& m : filtersw_)
      if (m.rows != kh || m.cols != filtersw_[0].cols) return false;
    FILE* f = fopen(filename.c_str(), "wb");
    if (!f) return false;
    int32_t hd[12] = {(int32_t)filtersw_.size(), kh, kw, flen_, norient_, binsize_, nscales_, (int32_t)defw_.size(),
                      (int32_t)biasw_.size(), (int32_t)filterid_.size(), 0, 0};
    fwrite("PBDMODL1", 1, 8, f); fwrite(hd, 4, 12, f); fwrite(&thresh_, 4, 1, f);
    for (const Mat& m : filtersw_) fwrite(m.ptr<float>(), 4, (size_t)kh * kw * flen_, f);
    for (const vectorf& d : defw_) fwrite(d.data(), 4, 4, f);
    for (const Point& a : anchors_) { int32_t v[2] = {a.x, a.y}; fwrite(v, 4, 2, f); }
    fwrite(biasw_.data(), 4, biasw_.size(), f);
    for (size_t c = 0; c < filterid_.size(); ++c) {
      int32_t np = (int32_t)filterid_[c].size(); fwrite(&np, 4, 1, f);
      for (int p = 0; p < np; ++p) {
        const int32_t k = (int32_t)filterid_[c][p].size();
        int32_t pk[2] = {p ? parentid_[c][p] : -1, k}; fwrite(pk, 4, 2, f);
        std::vector<int32_t> d(k, 0), b(k, biasid_[c][p].empty() ? 0 : biasid_[c][p][0]);
        for (int q = 0; q < k && p > 0 && q < (int)defid_[c][p].size(); ++q) d[q] = defid_[c][p][q];
        for (int q = 0; q < k && q < (int)biasid_[c][p].size(); ++q) b[q] = biasid_[c][p][q];
        fwrite(filterid_[c][p].data(), 4, k, f); fwrite(d.data(), 4, k, f); fwrite(b.data(), 4, k, f);
      }
    }
    fclose(f);
    return true;
  }
  void assign(Model& o) {
    filtersw_ = o.filters(); defw_ = o.def(); biasw_ = o.bias(); anchors_ = o.anchors(); biasid_ = o.biasid();
    filterid_ = o.filterid(); defid_ = o.defid(); parentid_ = o.parentid(); name_ = o.name(); nscales_ = o.nscales();
    thresh_ = o.thresh(); binsize_ = o.binsize(); flen_ = o.flen(); norient_ = o.norient();
  }
};

// Content fingerprint of a host buffer (four independent multiply-add lanes over its 64-bit words).  The stage
// adaptors below take their inputs as ARGUMENTS, like the reference's interfaces do (IConvolutionEngine::pdf(features,
// ...), DynamicProgram::min(parts, scores, ...), argmin(..., rootv, rooti, ..., Ix, Iy, Ik, ...)): what the caller
// passes is what is processed.  The device keeps the fingerprint of everything it handed out; an argument whose
// bytes still match is already resident and is not uploaded again, anything else — another engine's output, a
// buffer edited in place — is uploaded first.  Nothing is ever answered from stale resident buffers.
static inline uint64_t fingerprint(const void* p, size_t bytes) {
  const uint8_t* b = (const uint8_t*)p;
  uint64_t a0 = 0x9E3779B97F4A7C15ull, a1 = 0xC2B2AE3D27D4EB4Full, a2 = 0x165667B19E3779F9ull, a3 = 0x27D4EB2F165667C5ull;
  size_t i = 0;
  for (; i + 32 <= bytes; i += 32) {
    uint64_t w[4];
    memcpy(w, b + i, 32);
    a0 = (a0 ^ w[0]) * 0x100000001B3ull + 1; a1 = (a1 ^ w[1]) * 0x100000001B3ull + 3;
    a2 = (a2 ^ w[2]) * 0x100000001B3ull + 5; a3 = (a3 ^ w[3]) * 0x100000001B3ull + 7;
  }
  for (; i < bytes; ++i) a0 = (a0 ^ b[i]) * 0x100000001B3ull + 11;
  return (a0 ^ (a1 << 1) ^ (a2 << 2) ^ (a3 << 3)) + bytes;
}

// ---- shared device handle -------------------------------------------------------------------
class Device {
 public:
  pbd_handle* h = nullptr;
  int scalar = PBD_SCALAR_F32;   // T of the detector that owns this device (cv::DataType<T>::type)
  int max_candidates = 4096;     // pbd_options.max_candidates: device-side capacity, also the host arrays' size
  // what the device holds, as fingerprints of the host copies handed out (0 = nothing resident / unknown)
  std::vector<uint64_t> fp_feat;                 // [level]
  std::vector<std::vector<uint64_t>> fp_resp;    // [level][filter]
  std::vector<std::vector<uint64_t>> fp_root;    // [level][component]: rootv ^ rooti
  std::vector<uint64_t> fp_tab;                  // per (level, component, part, parent mixture) in walk order: Ix ^ Iy ^ Ik
  bool tables_resident = false;                  // min() of THIS device produced the tables on the device
  std::vector<int32_t> cell_w, cell_h;           // level sizes of the current frame geometry
  vectorf scales;
  void geometry(int w, int hgt) {                // after pbd_pyramid_u8 / pbd_begin_frame
    int n = 0;
    check(pbd_pyramid_geometry(h, w, hgt, &n, 0, 0, 0, 0, 0));
    cell_w.resize(n); cell_h.resize(n); scales.resize(n);
    check(pbd_pyramid_geometry(h, w, hgt, &n, 0, 0, cell_w.data(), cell_h.data(), scales.data()));
    fp_feat.assign(n, 0); fp_resp.clear(); fp_root.clear(); fp_tab.clear(); tables_resident = false;
  }
  // What the fingerprints claim to be resident must still BE resident: on a handle with the compact memory plan min()
  // overwrites the features and the responses (pbd_get_stage_state), so an argument that matches a fingerprint taken
  // before that min() would be skipped and the DP would run on the overwritten planes.
  void dropStale() {
    int32_t st[4] = {1, 1, 1, 1};
    check(pbd_get_stage_state(h, st));
    if (!st[1]) std::fill(fp_feat.begin(), fp_feat.end(), 0);
    if (!st[2]) for (auto& v : fp_resp) std::fill(v.begin(), v.end(), 0);
    if (!st[3]) { tables_resident = false; fp_tab.clear(); for (auto& v : fp_root) std::fill(v.begin(), v.end(), 0); }
  }
  // a caller that brings features from another IFeatures declares the frame first (the level sizes follow from it)
  void beginFrame(int w, int hgt, int cn) { check(pbd_begin_frame(h, w, hgt, cn)); geometry(w, hgt); }
  void checkLevels(const vectorMat& v, int per_cell, const char* what) const {
    if (v.size() != cell_w.size()) throw Exception(PBD_ERR_STATE, std::string(what) + ": level count differs from the frame geometry of the device "
                                                                  "(run HipHOGFeatures::pyramid or Device::beginFrame for this image first)");
    for (size_t l = 0; l < v.size(); ++l)
      if (v[l].rows != cell_h[l] || v[l].cols != cell_w[l] * per_cell)
        throw Exception(PBD_ERR_ARG, std::string(what) + ": level " + std::to_string(l) + " has the wrong size for the frame geometry of the device");
  }
  std::vector<float> filters, defw, biasw;
  std::vector<int32_t> anchors, part_offset, parentid, mix_offset, filterid, defid, biasid;
  std::vector<int32_t> fsize;   // mixed banks: {kh, kw} per filter (pbd_create_sized); empty for a uniform bank
  Device(Model& m, int device, int conv_mode, int scalar_type = PBD_SCALAR_F32, int max_cand = 4096) {
    pbd_model_desc d{};
    // The reference's engine takes a size per filter (src/SpatialConvolutionEngine.cpp:133-159, include/Parts.hpp:185-187): a uniform
    // bank goes through pbd_create (desc kh x kw), a mixed one (e.g. matlab/modelTransfer.m's VOC path) through pbd_create_sized
    const int kh = m.filters()[0].rows, kw = m.filters()[0].cols / m.flen();
    bool uniform = true;
    for (Mat& f : m.filters()) {
      uniform = uniform && f.rows == kh && f.cols == kw * m.flen();
      fsize.push_back(f.rows); fsize.push_back(f.cols / m.flen());
      filters.insert(filters.end(), f.ptr<float>(), f.ptr<float>() + (size_t)f.rows * f.cols);
    }
    if (uniform) fsize.clear();
    for (vectorf& w : m.def()) defw.insert(defw.end(), w.begin(), w.begin() + 4);
    for (Point& a : m.anchors()) { anchors.push_back(a.x); anchors.push_back(a.y); }
    biasw = m.bias();
    part_offset.push_back(0); mix_offset.push_back(0);
    for (size_t c = 0; c < m.filterid().size(); ++c) {
      for (size_t p = 0; p < m.filterid()[c].size(); ++p) {
        parentid.push_back(p ? m.parentid()[c][p] : -1);
        for (size_t k = 0; k < m.filterid()[c][p].size(); ++k) {
          filterid.push_back(m.filterid()[c][p][k]);
          const vectori& dv = m.defid()[c][p]; const vectori& bv = m.biasid()[c][p];
          defid.push_back(p && k < dv.size() ? dv[k] : 0);
          biasid.push_back(bv.empty() ? 0 : bv[std::min(k, bv.size() - 1)]);
        }
        mix_offset.push_back((int32_t)filterid.size());
      }
      part_offset.push_back((int32_t)parentid.size());
    }
    d.nfilters = (int)m.filters().size(); d.kh = uniform ? kh : 0; d.kw = uniform ? kw : 0; d.flen = m.flen(); d.norient = m.norient();
    d.sbin = m.binsize(); d.interval = m.nscales(); d.thresh = m.thresh();
    d.filters = filters.data(); d.ndefs = (int)m.def().size(); d.defw = defw.data(); d.anchors = anchors.data();
    d.nbias = (int)biasw.size(); d.biasw = biasw.data(); d.ncomponents = (int)m.filterid().size();
    d.part_offset = part_offset.data(); d.parentid = parentid.data(); d.mix_offset = mix_offset.data();
    d.filterid = filterid.data(); d.defid = defid.data(); d.biasid = biasid.data();
    pbd_options opt{};
    opt.device = device; opt.conv_mode = conv_mode; opt.scalar_type = scalar_type; opt.max_candidates = max_cand;
    scalar = scalar_type; max_candidates = max_cand > 0 ? max_cand : 4096;
    if (pbd_abi_version() != PBD_ABI_VERSION) throw Exception(PBD_ERR_UNSUPPORTED, "libpbd_hip.so was built for another pbd_c.h (pbd_abi_version)");
    const int rc = uniform ? pbd_create(&d, &opt, &h) : pbd_create_sized(&d, fsize.data(), &opt, &h);
    if (rc != PBD_OK) { std::string msg = h ? pbd_last_error(h) : "pbd_create failed"; if (h) pbd_destroy(h); h = nullptr; throw Exception(rc, msg); }
  }
  ~Device() { if (h) pbd_destroy(h); }
  void check(int rc) const { if (rc != PBD_OK) throw Exception(rc, pbd_last_error(h)); }
  // Candidate::sort (+ nonMaximaSuppression(overlap)) of every detect() on the GPU: PBD_CAND_RAW / _SORT / _SORT_NMS
  void setCandidateFilter(int mode, float overlap = 0.f) { check(pbd_set_candidate_filter(h, mode, overlap)); }
  // what the NMS of PBD_CAND_SORT_NMS is: PBD_NMS_PAINTED, or PBD_NMS_PARTS = nms.m's part-wise rule after a cut to the `top` best
  void setCandidateNms(int kind, int top = 0) { check(pbd_set_candidate_nms(h, kind, top)); }
  // SearchSpacePruning::filterCandidatesByDepth inside every detect(im, depth) with a non-empty depth image, on the GPU
  void setDepthFilter(bool on, float zfactor) { check(pbd_set_depth_filter(h, on ? 1 : 0, zfactor)); }
  // per-part scores of every record detect() returns, on the GPU
  void setPartScores(bool on) { check(pbd_set_part_scores(h, on ? 1 : 0)); }
  // padded feature pyramid with the boundary-occlusion feature (src/HOGFeatures.cpp:147-148): pad cells around every level, 0 = off
  void setBoundaryPad(int pad) { check(pbd_set_boundary_pad(h, pad)); }
  // the image pyramid under the features: PBD_PYRAMID_OPENCV (src/HOGFeatures.cpp:95-127) or PBD_PYRAMID_MATLAB (matlab/detection/featpyramid.m:13-34)
  void setPyramidKind(int kind) { check(pbd_set_pyramid_kind(h, kind)); }
  // train.m:95-96,121 model.interval = 2 on the live handle: the levels per octave from the next frame on (1..16).  The plan is dropped,
  // so nothing handed out earlier is resident any more.
  void setInterval(int interval) {
    check(pbd_set_interval(h, interval));
    cell_w.clear(); cell_h.clear(); scales.clear();
    fp_feat.clear(); fp_resp.clear(); fp_root.clear(); fp_tab.clear(); tables_resident = false;
  }
  int interval() const { return pbd_get_interval(h); }
};

// ---- include/IFeatures.hpp:49-73 --------------------------------------------------------------
class IFeatures {
 public:
  virtual ~IFeatures() {}
  virtual size_t binsize() const = 0;
  virtual size_t nscales() const = 0;
  virtual vectorf scales() const = 0;
  virtual void pyramid(const Mat& im, vectorMat& pyrafeatures) = 0;
};

class HipHOGFeatures : public IFeatures {          // include/HOGFeatures.hpp:52-88
  std::shared_ptr<Device> dev_; size_t binsize_, nscales_; vectorf scales_;
 public:
  HipHOGFeatures(std::shared_ptr<Device> d, size_t binsize, size_t nscales) : dev_(d), binsize_(binsize), nscales_(nscales) {}
  size_t binsize() const override { return binsize_; }
  size_t nscales() const override { return nscales_; }
  vectorf scales() const override { return scales_; }
  // The lines src/HOGFeatures.cpp:147-148 leave commented out — copyMakeBorder(feature, padded, 3, 3, ...) + boundaryOcclusionFeature(padded,
  // flen_, 3) — for every level, on the GPU: pyramid() then hands out the padded features (0 = off, the default; 3 = the reference's literal)
  void setBoundaryPad(int pad) { dev_->setBoundaryPad(pad); }
  // featpyramid.m:13-34 instead of :95-127 below: the frame in double, matlab/mex/resize.cc for the first octave, matlab/mex/reduce.cc for the
  // rest, with its own level count, sizes and scales (PBD_PYRAMID_MATLAB; 8-bit frames only).  PBD_PYRAMID_OPENCV: the default
  void setPyramidKind(int kind) { dev_->setPyramidKind(kind); }
  void pyramid(const Mat& im, vectorMat& pyrafeatures) override {   // src/HOGFeatures.cpp:95-151
    // :136-146 dispatches features<uint8_t | uint16_t | float | double> on im.depth(); any other depth: StsUnsupportedFormat (the library refuses it)
    dev_->check(pbd_pyramid_image(dev_->h, im.ptr<uint8_t>(), im.depth(), im.cols, im.rows, im.channels(), (int)im.step()));
    dev_->geometry(im.cols, im.rows);
    const int n = (int)dev_->cell_w.size();
    const std::vector<int32_t>&cw = dev_->cell_w, &ch = dev_->cell_h;
    scales_ = dev_->scales; nscales_ = n;
    pyrafeatures.clear(); pyrafeatures.resize(n);
    for (int l = 0; l < n; ++l) {
      const bool f64 = dev_->scalar == PBD_SCALAR_F64;   // HOGFeatures<T>: Mat of DataType<T>::type
      pyrafeatures[l].create(ch[l], cw[l] * 32, f64 ? PBD_64F : PBD_32F);
      if (ch[l] > 0 && cw[l] > 0)
        dev_->check(f64 ? pbd_get_level_features_f64(dev_->h, l, pyrafeatures[l].ptr<double>())
                        : pbd_get_level_features(dev_->h, l, pyrafeatures[l].ptr<float>()));
      dev_->fp_feat[l] = fingerprint(pyrafeatures[l].ptr<uint8_t>(), pyrafeatures[l].bytes());
    }
  }
};

// ---- include/IConvolutionEngine.hpp:44-68 -------------------------------------------------------
class IConvolutionEngine {
 public:
  virtual ~IConvolutionEngine() {}
  virtual void pdf(const vectorMat& features, vector2DMat& responses) = 0;
  virtual void setFilters(const vectorMat& filters) = 0;
};

class HipConvolutionEngine : public IConvolutionEngine {   // include/SpatialConvolutionEngine.hpp:44-58
  std::shared_ptr<Device> dev_; size_t nfilters_ = 0;
 public:
  explicit HipConvolutionEngine(std::shared_ptr<Device> d) : dev_(d) {}
  void setFilters(const vectorMat& filters) override { nfilters_ = filters.size(); }  // uploaded by pbd_create
  void pdf(const vectorMat& features, vector2DMat& responses) override {  // src/SpatialConvolutionEngine.cpp:106-124
    const bool f64 = dev_->scalar == PBD_SCALAR_F64;   // SpatialConvolutionEngine(type_)
    dev_->checkLevels(features, 32, "pdf(features)");
    // the features that are processed are the ones passed in: levels whose bytes the device does not already hold
    // (another IFeatures' pyramid, a pyramid edited after pyramid()) are uploaded first
    for (size_t l = 0; l < features.size(); ++l) {
      if (features[l].empty()) continue;
      if (features[l].depth() != (f64 ? PBD_64F : PBD_32F)) throw Exception(PBD_ERR_ARG, "pdf(features): element type differs from the detector's T");
      const uint64_t fp = fingerprint(features[l].ptr<uint8_t>(), features[l].bytes());
      if (fp == dev_->fp_feat[l]) continue;
      dev_->check(f64 ? pbd_set_level_features_f64(dev_->h, (int)l, features[l].ptr<double>())
                      : pbd_set_level_features(dev_->h, (int)l, features[l].ptr<float>()));
      dev_->fp_feat[l] = fp;
    }
    dev_->check(pbd_pdf(dev_->h));
    responses.assign(features.size(), vectorMat(nfilters_));
    dev_->fp_resp.assign(features.size(), std::vector<uint64_t>(nfilters_, 0));
    dev_->tables_resident = false;
    for (size_t l = 0; l < features.size(); ++l)
      for (size_t n = 0; n < nfilters_; ++n) {
        responses[l][n].create(features[l].rows, features[l].cols / 32, f64 ? PBD_64F : PBD_32F);
        if (!responses[l][n].empty())
          dev_->check(f64 ? pbd_get_level_response_f64(dev_->h, (int)l, (int)n, responses[l][n].ptr<double>())
                          : pbd_get_level_response(dev_->h, (int)l, (int)n, responses[l][n].ptr<float>()));
        dev_->fp_resp[l][n] = fingerprint(responses[l][n].ptr<uint8_t>(), responses[l][n].bytes());
      }
  }
};

// ---- include/DynamicProgram.hpp:61-77 ----------------------------------------------------------
static inline void append_candidates(std::vector<Candidate>& out, const std::vector<pbd_candidate_head>& heads,
                                     const std::vector<int32_t>& boxes, const std::vector<int32_t>& locs, int n, int mp) {
  for (int i = 0; i < n; ++i) {                    // src/DynamicProgram.cpp:216-251 (appends)
    Candidate c;
    c.setComponent(heads[i].component);
    c.level = heads[i].level;
    for (int p = 0; p < heads[i].nparts; ++p) {
      const int32_t* b = &boxes[((size_t)i * mp + p) * 4];
      c.addPart(Rect{b[0], b[1], b[2], b[3]}, p == 0 ? heads[i].score : 0.0f);
      for (int k = 0; k < 3; ++k) c.locs.push_back(locs[((size_t)i * mp + p) * 3 + k]);
    }
    out.push_back(c);
  }
}

// ---- include/Parts.hpp:51-261 (index tables only: all numerics run on the device) -------------------------
class Parts {
  vector3Di filterid_; vector2Di parentid_;
 public:
  Parts() {}
  explicit Parts(Model& m) : filterid_(m.filterid()), parentid_(m.parentid()) {}
  int ncomponents() const { return (int)filterid_.size(); }                  // :236
  int nparts(int c) const { return (int)filterid_[c].size(); }               // :238
  int nmixtures(int c, int p) const { return (int)filterid_[c][p].size(); }  // ComponentPart::nmixtures, :131
  int parent(int c, int p) const { return p ? parentid_[c][p] : -1; }        // ComponentPart::parent, :143
};

// DynamicProgram<T> with the reference's signatures (include/DynamicProgram.hpp:74-75).  min() transforms the SCORES
// IT IS GIVEN (planes the device does not already hold are uploaded), leaves the tables on the device and materialises
// them in the reference's shapes — rootv / rooti[level][component] and, unless fetchPointerTables(false), Ix / Iy /
// Ik[level][component][part][parent mixture] as CV_32S-like maps (src/DynamicProgram.cpp:72-76,147-151; 250 MB for the
// person model at 640x480, which is why a caller that only goes on to argmin() may switch them off).  argmin()
// back-tracks on the device from THE TABLES IT IS GIVEN: tables whose bytes are the ones min() handed out are
// already there, anything else (another engine's min(), tables edited in between) is uploaded first
// (pbd_set_root / pbd_set_dp_pointers).  Empty pointer tables (fetchPointerTables(false)) stand for "the tables of
// this object's last min()"; if there was none, argmin() throws instead of answering from whatever is resident.
template <typename T>
class DynamicProgram {
  std::shared_ptr<Device> dev_;
  bool fetch_ptr_ = true;
  static int set_resp(pbd_handle* h, int l, int n, const float* p) { return pbd_set_level_response(h, l, n, p); }
  static int set_resp(pbd_handle* h, int l, int n, const double* p) { return pbd_set_level_response_f64(h, l, n, p); }
  static int set_root(pbd_handle* h, int l, int c, const float* v, const int32_t* i) { return pbd_set_root(h, l, c, v, i); }
  static int set_root(pbd_handle* h, int l, int c, const double* v, const int32_t* i) { return pbd_set_root_f64(h, l, c, v, i); }
  static uint64_t fp3(const Mat& a, const Mat& b, const Mat& c) {
    return fingerprint(a.ptr<uint8_t>(), a.bytes()) ^ (fingerprint(b.ptr<uint8_t>(), b.bytes()) * 3) ^ (fingerprint(c.ptr<uint8_t>(), c.bytes()) * 5);
  }
 public:
  DynamicProgram() {}
  explicit DynamicProgram(std::shared_ptr<Device> d) : dev_(d) {}
  void fetchPointerTables(bool on) { fetch_ptr_ = on; }
  void min(Parts& parts, vector2DMat& scores, vector4DMat& Ix, vector4DMat& Iy, vector4DMat& Ik, vector2DMat& rootv,
           vector2DMat& rooti) {
    const size_t nscales = scores.size();
    const int ncomponents = parts.ncomponents();
    if (nscales != dev_->cell_w.size())
      throw Exception(PBD_ERR_STATE, "min(scores): level count differs from the frame geometry of the device (run HipHOGFeatures::pyramid or Device::beginFrame first)");
    if (dev_->fp_resp.size() != nscales) dev_->fp_resp.assign(nscales, std::vector<uint64_t>());
    for (size_t n = 0; n < nscales; ++n) {                        // the scores that are transformed are the ones passed in
      dev_->fp_resp[n].resize(scores[n].size(), 0);
      for (size_t f = 0; f < scores[n].size(); ++f) {
        const Mat& sc = scores[n][f];
        if (sc.rows != dev_->cell_h[n] || sc.cols != dev_->cell_w[n]) throw Exception(PBD_ERR_ARG, "min(scores): a score map has the wrong size for the frame geometry of the device");
        if (sc.empty()) continue;
        if (sc.depth() != (int)DataType<T>::type) throw Exception(PBD_ERR_ARG, "min(scores): element type differs from the detector's T");
        const uint64_t fp = fingerprint(sc.ptr<uint8_t>(), sc.bytes());
        if (fp == dev_->fp_resp[n][f]) continue;
        dev_->check(set_resp(dev_->h, (int)n, (int)f, sc.template ptr<T>()));
        dev_->fp_resp[n][f] = fp;
      }
    }
    dev_->check(pbd_dp_min(dev_->h));
    dev_->dropStale();   // compact memory plan: min() reused the feature memory and transformed the responses in place
    Ix.assign(nscales, vector3DMat(ncomponents)); Iy.assign(nscales, vector3DMat(ncomponents)); Ik.assign(nscales, vector3DMat(ncomponents));
    rootv.assign(nscales, vectorMat(ncomponents));
    rooti.assign(nscales, vectorMat(ncomponents));
    dev_->fp_root.assign(nscales, std::vector<uint64_t>(ncomponents, 0));
    dev_->fp_tab.clear();
    dev_->tables_resident = true;
    for (size_t n = 0; n < nscales; ++n)
      for (int c = 0; c < ncomponents; ++c) {
        const int rows = dev_->cell_h[n], cols = dev_->cell_w[n];
        rootv[n][c].create(rows, cols, DataType<T>::type);
        rooti[n][c].create(rows, cols, PBD_32S);
        if (!rootv[n][c].empty()) dev_->check(get_root(dev_->h, (int)n, c, rootv[n][c].template ptr<T>(), rooti[n][c].ptr<int32_t>()));
        dev_->fp_root[n][c] = fingerprint(rootv[n][c].template ptr<uint8_t>(), rootv[n][c].bytes()) ^ (fingerprint(rooti[n][c].ptr<uint8_t>(), rooti[n][c].bytes()) * 3);
        Ix[n][c].resize(parts.nparts(c)); Iy[n][c].resize(parts.nparts(c)); Ik[n][c].resize(parts.nparts(c));   // :89-91
        for (int p = 1; p < parts.nparts(c) && fetch_ptr_; ++p) {
          const int L = parts.nmixtures(c, parts.parent(c, p));
          Ix[n][c][p].resize(L); Iy[n][c][p].resize(L); Ik[n][c][p].resize(L);
          for (int m = 0; m < L; ++m) {
            Ix[n][c][p][m].create(rows, cols, PBD_32S); Iy[n][c][p][m].create(rows, cols, PBD_32S); Ik[n][c][p][m].create(rows, cols, PBD_32S);
            if (rows > 0 && cols > 0)
              dev_->check(pbd_get_dp_pointers(dev_->h, (int)n, c, p, m, Ix[n][c][p][m].ptr<int32_t>(), Iy[n][c][p][m].ptr<int32_t>(),
                                              Ik[n][c][p][m].ptr<int32_t>()));
            dev_->fp_tab.push_back(fp3(Ix[n][c][p][m], Iy[n][c][p][m], Ik[n][c][p][m]));
          }
        }
      }
  }
  static int get_root(pbd_handle* h, int l, int c, float* v, int32_t* i) { return pbd_get_root(h, l, c, v, i); }
  static int get_root(pbd_handle* h, int l, int c, double* v, int32_t* i) { return pbd_get_root_f64(h, l, c, v, i); }
  void argmin(Parts& parts, const vector2DMat& rootv, const vector2DMat& rooti, const vectorf scales,
              const vector4DMat& Ix, const vector4DMat& Iy, const vector4DMat& Ik, vectorCandidate& candidates) {
    const size_t nscales = dev_->cell_w.size();
    if (rootv.size() != nscales || rooti.size() != nscales || Ix.size() != nscales || Iy.size() != nscales || Ik.size() != nscales)
      throw Exception(PBD_ERR_ARG, "argmin(): table level count differs from the frame geometry of the device");
    // boxes are scaled by scales[n] (src/DynamicProgram.cpp:198,238): the device scales them by its pyramid's
    if (scales.size() != nscales || memcmp(scales.data(), dev_->scales.data(), nscales * sizeof(float)))
      throw Exception(PBD_ERR_UNSUPPORTED, "argmin(): `scales` differ from the scales of the device's pyramid geometry");
    if (dev_->fp_root.size() != nscales) dev_->fp_root.assign(nscales, std::vector<uint64_t>(parts.ncomponents(), 0));
    size_t t = 0;
    for (size_t n = 0; n < nscales; ++n)
      for (int c = 0; c < parts.ncomponents(); ++c) {
        const Mat &rv = rootv[n][c], &ri = rooti[n][c];
        if (rv.rows != dev_->cell_h[n] || rv.cols != dev_->cell_w[n] || ri.rows != rv.rows || ri.cols != rv.cols)
          throw Exception(PBD_ERR_ARG, "argmin(): a root table has the wrong size for the frame geometry of the device");
        if (!rv.empty()) {
          if (rv.depth() != (int)DataType<T>::type || ri.depth() != PBD_32S) throw Exception(PBD_ERR_ARG, "argmin(): root table element types");
          const uint64_t fp = fingerprint(rv.template ptr<uint8_t>(), rv.bytes()) ^ (fingerprint(ri.ptr<uint8_t>(), ri.bytes()) * 3);
          if (fp != dev_->fp_root[n][c]) {
            dev_->check(set_root(dev_->h, (int)n, c, rv.template ptr<T>(), ri.ptr<int32_t>()));
            dev_->fp_root[n][c] = fp;
          }
        }
        for (int p = 1; p < parts.nparts(c); ++p) {
          const int L = parts.nmixtures(c, parts.parent(c, p));
          const bool given = (int)Ix[n][c].size() > p && (int)Ix[n][c][p].size() == L && (int)Iy[n][c][p].size() == L && (int)Ik[n][c][p].size() == L;
          if (!given) {   // no table passed for this part: only legitimate for the tables this object's min() left on the device
            if (!dev_->tables_resident) throw Exception(PBD_ERR_STATE, "argmin(): empty pointer tables and no min() of this engine to take them from");
            continue;
          }
          for (int m = 0; m < L; ++m, ++t) {
            const Mat &x = Ix[n][c][p][m], &y = Iy[n][c][p][m], &k = Ik[n][c][p][m];
            if (x.rows != dev_->cell_h[n] || x.cols != dev_->cell_w[n] || y.rows != x.rows || y.cols != x.cols || k.rows != x.rows || k.cols != x.cols)
              throw Exception(PBD_ERR_ARG, "argmin(): a pointer table has the wrong size for the frame geometry of the device");
            if (x.empty()) continue;
            const uint64_t fp = fp3(x, y, k);
            if (t < dev_->fp_tab.size() && dev_->fp_tab[t] == fp) continue;
            dev_->check(pbd_set_dp_pointers(dev_->h, (int)n, c, p, m, x.ptr<int32_t>(), y.ptr<int32_t>(), k.ptr<int32_t>()));
            if (dev_->fp_tab.size() <= t) dev_->fp_tab.resize(t + 1, 0);
            dev_->fp_tab[t] = fp;
          }
        }
      }
    const int capacity = dev_->max_candidates, mp = pbd_max_parts(dev_->h);
    std::vector<pbd_candidate_head> heads(capacity);
    std::vector<int32_t> boxes((size_t)capacity * mp * 4), locs((size_t)capacity * mp * 3);
    int n = 0;
    dev_->check(pbd_dp_argmin(dev_->h, heads.data(), boxes.data(), locs.data(), capacity, &n));
    append_candidates(candidates, heads, boxes, locs, n, mp);      // appends, like :246-251
  }
};

// ---- include/PartsBasedDetector.hpp:152-175 ----------------------------------------------------
// ---- include/SearchSpacePruning.hpp: filterCandidatesByDepth (src/SearchSpacePruning.cpp:73-94) on the device -----------------
// The depth Mat's element type is T (Math::median<T> reads it as T); boxes are clipped to it (pbd_c.h: the one deviation).
// filterResponseByDepth is a no-op in the reference (it computes Z and discards it) and is not provided.
template <typename T>
class SearchSpacePruning {
  std::shared_ptr<Device> dev_;
 public:
  explicit SearchSpacePruning(std::shared_ptr<Device> dev) : dev_(std::move(dev)) {}
  void filterCandidatesByDepth(Parts& parts, vectorCandidate& candidates, const Mat& depth, const float zfactor) {
    const int n = (int)candidates.size(), mp = pbd_max_parts(dev_->h);
    if (n == 0) return;
    std::vector<pbd_candidate_head> heads((size_t)n);
    std::vector<int32_t> boxes((size_t)n * mp * 4, 0);
    for (int i = 0; i < n; ++i) {
      const Candidate& c = candidates[i];
      const int np = parts.nparts(c.component());
      if ((int)c.parts().size() != np) throw Exception(PBD_ERR_ARG, "filterCandidatesByDepth: a candidate's part count differs from its component's");
      heads[i] = pbd_candidate_head{c.score(), c.component(), i, np};   // level: the input position, to map the kept ones back
      for (int p = 0; p < np; ++p) {
        const Rect& r = c.parts()[p];
        int32_t* b = &boxes[((size_t)i * mp + p) * 4];
        b[0] = r.x; b[1] = r.y; b[2] = r.width; b[3] = r.height;
      }
    }
    int kept = 0;
    dev_->check(pbd_candidates_depth_filter(dev_->h, zfactor, depth.empty() ? nullptr : depth.ptr<uint8_t>(), depth.depth(),
                                            depth.empty() ? 0 : depth.cols, depth.empty() ? 0 : depth.rows, (int)depth.step(),
                                            heads.data(), boxes.data(), nullptr, n, &kept));
    vectorCandidate out;
    out.reserve((size_t)kept);
    for (int k = 0; k < kept; ++k) out.push_back(candidates[heads[k].level]);
    candidates.swap(out);
  }
};

template <typename T>
class PartsBasedDetector {
  std::string name_;
  std::shared_ptr<Device> dev_;
  std::unique_ptr<IFeatures> features_;
  std::unique_ptr<IConvolutionEngine> convolution_engine_;
  DynamicProgram<T> dp_;
  Parts parts_;
  int device_, conv_mode_, ncomponents_ = 0;
  int cand_mode_ = PBD_CAND_RAW; float cand_overlap_ = 0.f;
  int cand_nms_ = PBD_NMS_PAINTED, cand_top_ = 0;
  bool depth_on_ = false; float zfactor_ = 0.03f;
  bool part_scores_on_ = false;
  int boundary_pad_ = 0;
  int pyramid_kind_ = PBD_PYRAMID_OPENCV;
  // the last detect's per-part scores -> the `n` candidates it appended: fills Candidate::confidence_ of the non-root parts
  void attach_part_scores(vectorCandidate& candidates, int n, int mp) {
    if (!part_scores_on_ || n == 0) return;
    std::vector<pbd_part_score> ps((size_t)n * mp);
    int got = 0;
    dev_->check(pbd_get_part_scores(dev_->h, 0, ps.data(), n, &got));
    Candidate* c = candidates.data() + (candidates.size() - (size_t)n);
    for (int i = 0; i < got; ++i) c[i].setPartScores(ps.data() + (size_t)i * mp, (int)c[i].parts().size());
  }
 public:
  int max_candidates_ = 4096;
  explicit PartsBasedDetector(int device = 0, int conv_mode = PBD_CONV_AUTO, int max_candidates = 4096)
      : device_(device), conv_mode_(conv_mode), max_candidates_(max_candidates) {}
  Device& device() { return *dev_; }
  const std::string& name() const { return name_; }
  IFeatures& features() { return *features_; }
  IConvolutionEngine& convolutionEngine() { return *convolution_engine_; }
  DynamicProgram<T>& dp() { return dp_; }
  Parts& parts() { return parts_; }
  int ncomponents() const { return ncomponents_; }
  void distributeModel(Model& model) {             // src/PartsBasedDetector.cpp:102-127
    name_ = model.name();
    ncomponents_ = model.ncomponents();
    min_area_ = 0;   // prod(maxsize * sbin), train.m:170: the largest filter rows and columns of the model
    {
      int mh = 0, mw = 0;
      for (const Mat& f : model.filters()) { mh = std::max(mh, f.rows); mw = std::max(mw, f.cols / std::max(model.flen(), 1)); }
      min_area_ = (double)(mh * model.binsize()) * (double)(mw * model.binsize());
    }
    nbias_ = (int)model.bias().size(); ndefs_ = (int)model.def().size();
    root_filter_ = model.filterid()[0][0][0]; root_bias_ = model.biasid()[0][0][0];
    // DataType<T>::type selects the instantiation (:110,113-117)
    dev_ = std::make_shared<Device>(model, device_, conv_mode_, (int)DataType<T>::scalar, max_candidates_);
    features_.reset(new HipHOGFeatures(dev_, model.binsize(), model.nscales()));
    convolution_engine_.reset(new HipConvolutionEngine(dev_));
    convolution_engine_->setFilters(model.filters());
    parts_ = Parts(model);                         // :121-122
    dp_ = DynamicProgram<T>(dev_);
    if (cand_mode_ != PBD_CAND_RAW) dev_->setCandidateFilter(cand_mode_, cand_overlap_);
    if (cand_nms_ != PBD_NMS_PAINTED) dev_->setCandidateNms(cand_nms_, cand_top_);
    if (depth_on_) dev_->setDepthFilter(true, zfactor_);
    if (part_scores_on_) dev_->setPartScores(true);
    if (boundary_pad_) dev_->setBoundaryPad(boundary_pad_);
    if (pyramid_kind_ != PBD_PYRAMID_OPENCV) dev_->setPyramidKind(pyramid_kind_);
  }
  // matlab/learning/vec2model.m on the live detector (include/pbd_c.h "weight and threshold updates"): biases, deformations and filters
  // become w's elements (Model.feature_layout()'s order: [biasw | defw | the filters back to back], rounded to float32); every setter's
  // state is kept, and so is an ExampleCache bound to this detector.  The Model object handed to distributeModel is not touched.
  void setWeights(const std::vector<double>& w) { dev_->check(pbd_set_weights(dev_->h, w.data(), (int)w.size())); }
  void weights(std::vector<double>& w, int len) { w.assign((size_t)len, 0.0); dev_->check(pbd_get_weights(dev_->h, w.data(), len)); }
  // the model's threshold for every detect from now on (train.m: 0 for latent positives, -1 for mining, then the positives' 5th percentile)
  void setThresh(float t) { dev_->check(pbd_set_threshold(dev_->h, t)); }
  float thresh() const { float t = 0; dev_->check(pbd_get_threshold(dev_->h, &t)); return t; }
  // train.m:95-96,121 model.interval = 2 while mining: the pyramid's levels per octave from the next frame on (1..16).  The detector then
  // behaves like one given the same model with that interval; an ExampleCache or Evaluation bound to it stays valid.
  void setInterval(int interval) { dev_->setInterval(interval); }
  int interval() const { return dev_->interval(); }
  // The image pyramid detect() builds its features on.  PBD_PYRAMID_OPENCV (the default): HOGFeatures<T>::pyramid, cv::resize and
  // cv::pyrDown in the pixel type (src/HOGFeatures.cpp:95-127).  PBD_PYRAMID_MATLAB: matlab/detection/featpyramid.m:13-34 — the frame
  // goes to double once, matlab/mex/resize.cc makes the first octave, matlab/mex/reduce.cc every further one — with its level count,
  // level sizes and box scales: the levels the MATLAB pipeline trains and evaluates its models on.  8-bit frames only.  With
  // setBoundaryPad the two together are featpyramid.m.  Kept across distributeModel().
  void setPyramidKind(int kind) {
    if (kind != PBD_PYRAMID_OPENCV && kind != PBD_PYRAMID_MATLAB) throw Exception(PBD_ERR_ARG, "setPyramidKind: PBD_PYRAMID_OPENCV or PBD_PYRAMID_MATLAB");
    if (dev_) dev_->setPyramidKind(kind);
    pyramid_kind_ = kind;
  }
  // The third step detect()'s author left commented out (src/HOGFeatures.cpp:147-148): every pyramid level surrounded by `pad` cells
  // that hold 0 and, in the last channel, 1 — the "outside the image" value the models are trained with (matlab/detection/
  // featpyramid.m:37-44) — so that detections may reach over the frame border; boxes are shifted back by the padding
  // (matlab/detection/detect.m:266-267).  0 (the default): off; 3: the reference's literal.  Kept across distributeModel().
  void setBoundaryPad(int pad) {
    if (pad < 0 || pad > 8) throw Exception(PBD_ERR_ARG, "setBoundaryPad: 0 (off) .. 8 cells");
    if (dev_) dev_->setBoundaryPad(pad);
    boundary_pad_ = pad;
  }
  // The record promises a confidence per part (include/Candidate.hpp:54-72); the reference stores 0.0 for every part but the
  // root (src/DynamicProgram.cpp:241-244).  On: Candidate::confidence()[p], p >= 1, is the part's own score — appearance +
  // deformation + bias of the returned configuration, computed by the GPU inside detect() — and Candidate::partScores() gives
  // the three terms; confidence()[0] stays the root score.  Off (the default): zeros.  Kept across distributeModel().
  void setPartScores(bool on) {
    if (dev_) dev_->setPartScores(on);
    part_scores_on_ = on;
  }
  // SearchSpacePruning<T>::filterCandidatesByDepth(parts, candidates, depth, zfactor), the call the reference leaves commented out
  // in detect() (src/PartsBasedDetector.cpp:91-93, zfactor 0.03), done by the GPU inside detect(im, depth, candidates) for a
  // non-empty depth of element type T; off (the default): depth is ignored.  Kept across distributeModel().
  void setDepthFilter(bool on, float zfactor = 0.03f) {
    if (dev_) dev_->setDepthFilter(on, zfactor);
    depth_on_ = on; zfactor_ = zfactor;
  }
  // What the reference's callers do after detect() — Candidate::sort, then Candidate::nonMaximaSuppression(im, candidates,
  // overlap) (ros/Node.cpp:192-196, cells/detect.cpp:237-238) — done by the GPU inside detect(): PBD_CAND_SORT or
  // PBD_CAND_SORT_NMS (PBD_CAND_RAW: off, the default).  Kept across distributeModel().
  void setCandidateFilter(int mode, float overlap = 0.f) {
    if (dev_) dev_->setCandidateFilter(mode, overlap);
    cand_mode_ = mode; cand_overlap_ = overlap;
  }
  // The NMS of PBD_CAND_SORT_NMS: PBD_NMS_PAINTED (default, Candidate::nonMaximaSuppression) or PBD_NMS_PARTS
  // (Candidate::nonMaximaSuppressionParts(overlap, top): matlab/detection/nms.m, what testmodel.m runs).  Kept across distributeModel().
  void setCandidateNms(int kind, int top = 0) {
    if (dev_) dev_->setCandidateNms(kind, top);
    else if ((kind != PBD_NMS_PAINTED && kind != PBD_NMS_PARTS) || top < 0) throw Exception(PBD_ERR_ARG, "candidate NMS: kind PBD_NMS_PAINTED / _PARTS, top >= 0");
    cand_nms_ = kind; cand_top_ = top;
  }
  void detect(const Mat& im, vectorCandidate& candidates) { detect(im, Mat(), candidates); }
  // src/PartsBasedDetector.cpp:69-95: fused path, everything stays in HBM; `depth` ignored (:91-93) unless setDepthFilter is on
  void detect(const Mat& im, const Mat& depth, vectorCandidate& candidates) {
    if (!dev_) throw Exception(PBD_ERR_STATE, "detect() before distributeModel()");
    const int cap = dev_->max_candidates, mp = pbd_max_parts(dev_->h);
    std::vector<pbd_candidate_head> heads(cap);
    std::vector<int32_t> boxes((size_t)cap * mp * 4), locs((size_t)cap * mp * 3);
    int n = 0;
    if (depth_on_ && !depth.empty()) {   // depth-carrying frames: 8-bit colour only
      if (im.depth() != PBD_8U) throw Exception(PBD_ERR_UNSUPPORTED, "depth pruning: 8-bit colour frames only");
      if (depth.rows != im.rows || depth.cols != im.cols) throw Exception(PBD_ERR_ARG, "depth image: the frame's size");
      dev_->check(pbd_detect_rgbd_u8(dev_->h, im.ptr<uint8_t>(), im.cols, im.rows, im.channels(), (int)im.step(), depth.ptr<uint8_t>(),
                                     depth.depth(), (int)depth.step(), heads.data(), boxes.data(), locs.data(), cap, &n));
      append_candidates(candidates, heads, boxes, locs, n, mp);
      attach_part_scores(candidates, n, mp);
      return;
    }
    // (CV_8U forwards to pbd_detect_u8; CV_16U / CV_32F / CV_64F: src/HOGFeatures.cpp:136-146; anything else: PBD_ERR_UNSUPPORTED = StsUnsupportedFormat)
    dev_->check(pbd_detect_image(dev_->h, im.ptr<uint8_t>(), im.depth(), im.cols, im.rows, im.channels(), (int)im.step(),
                                 heads.data(), boxes.data(), locs.data(), cap, &n));
    append_candidates(candidates, heads, boxes, locs, n, mp);
    attach_part_scores(candidates, n, mp);
  }
  // ---- pyramid store (include/pbd_c.h "pyramid store") ----
  // `slots` device-resident feature pyramids of frames up to max_w x max_h, each computed once by this detector (the producer) in put().
  // Any detector on the same device whose sbin, interval, pyramid kind, boundary pad and T equal the producer's detects
  // (detectStored) and mines (ExampleCache::mineStored) from a slot with the image entries' results, in bits, whatever its model.
  // Holds the producer's device alive; destroyed before it.
  class PyramidStore {
    std::shared_ptr<Device> dev_;
    pbd_pyrstore* s_ = nullptr;
    friend class PartsBasedDetector;
   public:
    PyramidStore(std::shared_ptr<Device> dev, int slots, int max_w, int max_h) : dev_(std::move(dev)) {
      dev_->check(pbd_pyrstore_create(dev_->h, slots, max_w, max_h, &s_));
    }
    ~PyramidStore() { pbd_pyrstore_destroy(s_); }
    PyramidStore(const PyramidStore&) = delete;
    PyramidStore& operator=(const PyramidStore&) = delete;
    pbd_pyrstore* get() const { return s_; }
    struct Dims { int slots, sbin, interval, kind, pad, scalar_bytes; size_t slot_bytes; };
    Dims dims() const { Dims d{}; dev_->check(pbd_pyrstore_dims(s_, &d.slots, &d.sbin, &d.interval, &d.kind, &d.pad, &d.scalar_bytes, &d.slot_bytes)); return d; }
    struct Slot { int w, hgt, cn, nlevels; };   // w == 0: empty
    Slot slot(int i) const { Slot v{}; dev_->check(pbd_pyrstore_slot(s_, i, &v.w, &v.hgt, &v.cn, &v.nlevels)); return v; }
    void put(int slot, const Mat& im) {
      if (im.depth() != PBD_8U) throw Exception(PBD_ERR_UNSUPPORTED, "pyramid store: 8-bit frames only");
      dev_->check(pbd_pyrstore_put_u8(s_, slot, im.ptr<uint8_t>(), im.cols, im.rows, im.channels(), (int)im.step()));
    }
    void putDev(int slot, const void* d_im, int w, int hgt, int cn, int stride) { dev_->check(pbd_pyrstore_put_dev_u8(s_, slot, d_im, w, hgt, cn, stride)); }
    void putBatch(const std::vector<int32_t>& slots, const std::vector<Mat>& ims) {   // same-sized 8-bit frames with one row step
      if (ims.empty() || slots.size() != ims.size()) throw Exception(PBD_ERR_ARG, "PyramidStore::putBatch: one slot per frame");
      std::vector<const uint8_t*> p;
      for (const Mat& m : ims) {
        if (m.depth() != PBD_8U || m.cols != ims[0].cols || m.rows != ims[0].rows || m.channels() != ims[0].channels() || m.step() != ims[0].step())
          throw Exception(PBD_ERR_ARG, "PyramidStore::putBatch: 8-bit frames of one size and row step");
        p.push_back(m.ptr<uint8_t>());
      }
      dev_->check(pbd_pyrstore_put_batch_u8(s_, slots.data(), p.data(), (int)ims.size(), ims[0].cols, ims[0].rows, ims[0].channels(), (int)ims[0].step()));
    }
    // level `level` of the slot's pyramid: cw * ch * 32 elements of the producer's T; `elements` = the room in out
    void level(int slot, int level, T* out, size_t elements) { dev_->check(pbd_pyrstore_get_level(s_, slot, level, out, elements * sizeof(T))); }
  };
  std::unique_ptr<PyramidStore> pyramidStore(int slots, int max_w, int max_h) {
    if (!dev_) throw Exception(PBD_ERR_STATE, "pyramidStore() before distributeModel()");
    return std::unique_ptr<PyramidStore>(new PyramidStore(dev_, slots, max_w, max_h));
  }
  // detect() on the frame that was put into `slot`: the image entry's candidates in bits, without the image pyramid and HOG
  void detectStored(const PyramidStore& store, int slot, vectorCandidate& candidates) {
    if (!dev_) throw Exception(PBD_ERR_STATE, "detectStored() before distributeModel()");
    const int cap = dev_->max_candidates, mp = pbd_max_parts(dev_->h);
    std::vector<pbd_candidate_head> heads(cap);
    std::vector<int32_t> boxes((size_t)cap * mp * 4), locs((size_t)cap * mp * 3);
    int n = 0;
    dev_->check(pbd_detect_stored(dev_->h, store.get(), slot, heads.data(), boxes.data(), locs.data(), cap, &n));
    append_candidates(candidates, heads, boxes, locs, n, mp);
    attach_part_scores(candidates, n, mp);
  }
  // detect(im, model, thresh, bbox, overlap) of matlab/detection/detect.m:18-23: the single highest-scoring pose whose every part
  // overlaps its box in `truth` (one cv::Rect per part, in the convention detect() returns: x .. x + width) by more than `overlap`
  // (in [0, 1)), appended to `candidates`; nothing is appended when no pose qualifies.  mix: empty = every mixture free, else per part
  // -1 = free or the mixture the part must take; component -1: all.  The model's threshold plays no part.  8-bit frames.
  void detectLatent(const Mat& im, const std::vector<Rect>& truth, double overlap, vectorCandidate& candidates,
                    const std::vector<int>& mix = std::vector<int>(), int component = -1) {
    if (!dev_) throw Exception(PBD_ERR_STATE, "detectLatent() before distributeModel()");
    if (im.depth() != PBD_8U) throw Exception(PBD_ERR_UNSUPPORTED, "latent detection: 8-bit colour frames only");
    const int mp = pbd_max_parts(dev_->h);
    std::vector<int32_t> tr((size_t)mp * 4, 0), mx((size_t)mp, -1);
    for (size_t p = 0; p < truth.size() && p < (size_t)mp; ++p) {
      tr[p * 4] = truth[p].x; tr[p * 4 + 1] = truth[p].y; tr[p * 4 + 2] = truth[p].width; tr[p * 4 + 3] = truth[p].height;
    }
    for (size_t p = 0; p < mix.size() && p < (size_t)mp; ++p) mx[p] = mix[p];
    std::vector<pbd_candidate_head> heads(1);
    std::vector<int32_t> boxes((size_t)mp * 4), locs((size_t)mp * 3);
    int n = 0;
    dev_->check(pbd_detect_latent_u8(dev_->h, im.ptr<uint8_t>(), im.cols, im.rows, im.channels(), (int)im.step(), tr.data(),
                                     mix.empty() ? nullptr : mx.data(), component, overlap, heads.data(), boxes.data(), locs.data(), &n));
    append_candidates(candidates, heads, boxes, locs, n, mp);
    attach_part_scores(candidates, n, mp);
  }
  // testmodel_gtbox.m:17-21: detect at the model's threshold, then per gt box bestoverlap(box, gtbox, overlap) — on the GPU, where only
  // the winners come home.  The chosen pose of every gt box that has one is appended to `candidates`; which[g] (may be null) = its index
  // in `candidates` or -1, o[g] (may be null) its overlap.  RAW candidate mode, no depth stages, no per-part scores; 8-bit frames.
  void detectGtBox(const Mat& im, const std::vector<GtBox>& gt, double overlap, vectorCandidate& candidates,
                   std::vector<int>* which = nullptr, std::vector<double>* o = nullptr) {
    if (!dev_) throw Exception(PBD_ERR_STATE, "detectGtBox() before distributeModel()");
    if (im.depth() != PBD_8U) throw Exception(PBD_ERR_UNSUPPORTED, "gt boxes: 8-bit colour frames only");
    const int mp = pbd_max_parts(dev_->h), ng = (int)gt.size();
    std::vector<pbd_candidate_head> heads((size_t)std::max(ng, 1)), one(1);
    std::vector<int32_t> boxes((size_t)std::max(ng, 1) * mp * 4), locs((size_t)std::max(ng, 1) * mp * 3);
    std::vector<int> found((size_t)std::max(ng, 1), 0);
    std::vector<double> ov((size_t)std::max(ng, 1), 0.0);
    static_assert(sizeof(GtBox) == 4 * sizeof(double), "GtBox layout");
    dev_->check(pbd_detect_gtbox_u8(dev_->h, im.ptr<uint8_t>(), im.cols, im.rows, im.channels(), (int)im.step(),
                                    ng ? &gt[0].x1 : nullptr, ng, overlap, heads.data(), boxes.data(), locs.data(), found.data(), ov.data(), nullptr));
    if (which) which->assign((size_t)ng, -1);
    if (o) o->assign(ov.begin(), ov.begin() + ng);
    for (int g = 0; g < ng; ++g) {
      if (!found[g]) continue;
      if (which) (*which)[g] = (int)candidates.size();
      one[0] = heads[g];
      append_candidates(candidates, one, std::vector<int32_t>(boxes.begin() + (size_t)g * mp * 4, boxes.begin() + (size_t)(g + 1) * mp * 4),
                        std::vector<int32_t>(locs.begin() + (size_t)g * mp * 3, locs.begin() + (size_t)(g + 1) * mp * 3), 1, mp);
    }
  }
  // The feature vectors of `candidates` — records of the LAST frame's detect() / detectLatent(), or a selection of them — gathered by
  // the GPU from the frame's resident feature planes: what matlab/detection/detect.m:272-308 collects as ex.blocks.  blocks[i *
  // max_parts + p] (ids -1 beyond the record's parts), windows[(i * max_parts + p) * wmax ...]: part p's HOG window, [kh][kw * flen] at
  // the front of its slot of wmax = pbd_feature_window_max() elements.  include/pbd_c.h, pbd_feature_block.
  typedef pbd_feature_block FeatureBlock;
  void features(const vectorCandidate& candidates, std::vector<FeatureBlock>& blocks, std::vector<T>& windows) {
    if (!dev_) throw Exception(PBD_ERR_STATE, "features() before distributeModel()");
    const size_t n = candidates.size(), mp = (size_t)pbd_max_parts(dev_->h), wmax = (size_t)pbd_feature_window_max(dev_->h);
    std::vector<pbd_candidate_head> heads(n);
    std::vector<int32_t> locs(n * mp * 3, 0);
    for (size_t i = 0; i < n; ++i) {
      const Candidate& c = candidates[i];
      heads[i].score = c.score(); heads[i].component = c.component(); heads[i].level = c.level; heads[i].nparts = (int32_t)c.parts().size();
      std::copy(c.locs.begin(), c.locs.begin() + std::min(c.locs.size(), mp * 3), locs.begin() + i * mp * 3);
    }
    blocks.assign(n * mp, FeatureBlock());
    windows.assign(n * mp * wmax, (T)0);
    dev_->check(features_entry(heads.data(), locs.data(), (int)n, blocks.data(), windows.data()));
  }
  // The QP's cache of block-sparse training examples on the device (include/pbd_c.h "training example cache"): qp_write.m's columns,
  // matlab/mex/score.cc and lincomb.cc.  Holds the detector's device alive; the coordinate-descent pass is not part of it (a host
  // solver reads the columns with get()).
  class ExampleCache {
    std::shared_ptr<Device> dev_;
    pbd_qp* q_ = nullptr;
    friend class PartsBasedDetector;
   public:
    ExampleCache(std::shared_ptr<Device> dev, int capacity, double cpos, double cneg, const double* wreg = nullptr, const double* w0 = nullptr)
        : dev_(std::move(dev)) { dev_->check(pbd_qp_create(dev_->h, capacity, cpos, cneg, wreg, w0, &q_)); }
    ~ExampleCache() { pbd_qp_destroy(q_); }
    ExampleCache(const ExampleCache&) = delete;
    ExampleCache& operator=(const ExampleCache&) = delete;
    void dims(int* len, int* k, int* capacity, int* n) const { dev_->check(pbd_qp_dims(q_, len, k, capacity, n)); }
    int size() const { int n = 0; dims(nullptr, nullptr, nullptr, &n); return n; }
    int capacity() const { int c = 0; dims(nullptr, nullptr, &c, nullptr); return c; }
    // score.cc: w (len values) on the examples `inds`; without inds: on all size() examples
    void score(const std::vector<double>& w, const std::vector<int32_t>& inds, std::vector<double>& out) { score_(w, inds.data(), (int)inds.size(), out); }
    void score(const std::vector<double>& w, std::vector<double>& out) { score_(w, nullptr, size(), out); }
    // lincomb.cc: a[i] multiplies example i (shorter than the capacity: the rest counts as zero; longer: refused), summed in the
    // order of `inds`; without inds: all size() examples in order
    void lincomb(const std::vector<double>& a, const std::vector<int32_t>& inds, std::vector<double>& w) { lincomb_(a, inds.data(), (int)inds.size(), w); }
    void lincomb(const std::vector<double>& a, std::vector<double>& w) { lincomb_(a, nullptr, size(), w); }
    void keep(const std::vector<int32_t>& inds) { dev_->check(pbd_qp_keep(q_, inds.data(), (int)inds.size())); }
    void get(int i0, int n, float* x, int32_t* ids, float* b, double* d) { dev_->check(pbd_qp_get(q_, i0, n, x, ids, b, d)); }
    void put(int n, const float* x, const int32_t* ids, const float* b, const double* d) { dev_->check(pbd_qp_put(q_, n, x, ids, b, d)); }
    // ---- the QP solver over the cache (include/pbd_c.h "QP solver"): the columns stay on the device ----
    void noneg(const std::vector<int32_t>& idx) { dev_->check(pbd_qp_noneg(q_, idx.data(), (int)idx.size())); }
    void fix(int nfix) { dev_->check(pbd_qp_fix(q_, nfix)); }
    struct SolverStats { double l, lb, lb_old, ub; };
    // a and sv by example over the capacity, w over len; any may be nullptr
    SolverStats state(std::vector<double>* a, std::vector<unsigned char>* sv, std::vector<double>* w) {
      int len = 0, cap = 0; dims(&len, nullptr, &cap, nullptr);
      if (a) a->assign((size_t)cap, 0.0);
      if (sv) sv->assign((size_t)cap, 0);
      if (w) w->assign((size_t)len, 0.0);
      double st[4];
      dev_->check(pbd_qp_state_get(q_, a ? a->data() : nullptr, sv ? sv->data() : nullptr, w ? w->data() : nullptr, st));
      return SolverStats{st[0], st[1], st[2], st[3]};
    }
    void set_state(const double* a, const unsigned char* sv, int n) { dev_->check(pbd_qp_state_put(q_, a, sv, n)); }
    // qp_one_sparse.cc over the examples `order` (distinct); returns its loss
    double solve_pass(const std::vector<int32_t>& order) { double loss = 0; dev_->check(pbd_qp_pass(q_, order.data(), (int)order.size(), &loss)); return loss; }
    void one(const std::vector<int32_t>& order) { dev_->check(pbd_qp_one(q_, order.data(), (int)order.size())); }
    void refresh() { dev_->check(pbd_qp_refresh(q_)); }
    double loss() { double v = 0; dev_->check(pbd_qp_loss(q_, &v)); return v; }
    // qp_opt.m: returns the number of passes; the shuffle is the header's stated generator, seeded with `seed`
    int opt(double tol, int max_iter, uint64_t seed, double* lb = nullptr, double* ub = nullptr) {
      int passes = 0; dev_->check(pbd_qp_opt(q_, tol, max_iter, seed, lb, ub, &passes)); return passes;
    }
    int prune() { int n = 0; dev_->check(pbd_qp_prune(q_, &n)); return n; }
    // qp_w.m: the next model's weights, w ./ wreg + w0 (Model.feature_layout() maps them back)
    void weights(std::vector<double>& w) { int len = 0; dims(&len, nullptr, nullptr, nullptr); w.assign((size_t)len, 0.0); dev_->check(pbd_qp_weights(q_, w.data())); }
    // train.m:94,112 model = vec2model(qp_w, model): weights() into the detector this cache is bound to, without leaving the device
    // (include/pbd_c.h "weight and threshold updates"); the cache's columns stay valid
    void applyWeights() { dev_->check(pbd_qp_apply_weights(q_)); }
    // ---- one training round (include/pbd_c.h "one training round") ----
    // train.m:75 qp.n = 0: capacity, wreg, w0, noneg and binding stay; the rest, the solver's a, sv, w, bounds and nfix included, is a new cache's
    void clear() { dev_->check(pbd_qp_clear(q_)); }
    // train.m:116-118 on the device: the element of rank max(ceil(m * q), 1) - 1 of the m positives' sorted scores (w + w0 .* wreg) . x / cpos
    double positiveThreshold(double q = .05, int* npos = nullptr) {
      double t = 0; int m = 0;
      dev_->check(pbd_qp_positive_threshold(q_, q, &t, &m));
      if (npos) *npos = m;
      return t;
    }
    int supportCount() {
      std::vector<unsigned char> sv;
      state(nullptr, &sv, nullptr);
      int nsv = 0;
      for (int e = 0, n = size(); e < n; ++e) nsv += sv[e] != 0;
      return nsv;
    }
    // poswarp of matlab/learning/train.m:131-161 (include/pbd_c.h "warped positives"): the boxes (1-based inclusive) of the 8-bit frame
    // warped to filter `filter`'s size (warppos.m), HOGed and appended as [bias | window] positives, all on the GPU.  Boxes below
    // min_area (prod(maxsize * sbin), train.m:135) are skipped; status (optional): PBD_WARP_WRITTEN / _SKIPPED / _FULL per box; ids
    // (optional): one id per box, else the box's index.  Returns how many were written.
    int writeWarped(const Mat& im, const std::vector<GtBox>& boxes, int filter, int bias, double min_area, std::vector<int32_t>* status = nullptr,
                    const std::vector<int32_t>* ids = nullptr) {
      if (im.depth() != PBD_8U) throw Exception(PBD_ERR_UNSUPPORTED, "warped positives: 8-bit frames only");
      if (ids && ids->size() != boxes.size()) throw Exception(PBD_ERR_ARG, "ExampleCache::writeWarped: one id per box");
      if (status) status->assign(boxes.size(), -1);
      int written = 0;
      dev_->check(pbd_qp_write_warped_u8(q_, im.ptr<uint8_t>(), im.cols, im.rows, im.channels(), (int)im.step(), boxes.empty() ? nullptr : &boxes[0].x1,
                                         ids ? ids->data() : nullptr, (int)boxes.size(), filter, bias, min_area, status ? status->data() : nullptr, &written));
      return written;
    }
    // the same from a frame in device memory (pbd_qp_write_warped_dev_u8): a virtual positive that pbd::augmentDevice left there.
    // The frame is read on the detector's stream, which waits for no other: whatever produced it on the caller's streams must be
    // complete before the call (pbd::augmentDevice is synchronous: its canvases are).
    int writeWarped(const DeviceFrame& im, const std::vector<GtBox>& boxes, int filter, int bias, double min_area, std::vector<int32_t>* status = nullptr,
                    const std::vector<int32_t>* ids = nullptr) {
      if (ids && ids->size() != boxes.size()) throw Exception(PBD_ERR_ARG, "ExampleCache::writeWarped: one id per box");
      if (status) status->assign(boxes.size(), -1);
      int written = 0;
      dev_->check(pbd_qp_write_warped_dev_u8(q_, im.data, im.cols, im.rows, im.channels, (int)im.step, boxes.empty() ? nullptr : &boxes[0].x1,
                                             ids ? ids->data() : nullptr, (int)boxes.size(), filter, bias, min_area, status ? status->data() : nullptr, &written));
      return written;
    }
    // ---- hard-negative mining (include/pbd_c.h "hard-negative mining") ----
    // train.m:102's detect(im, model, -1, [], 0, id, -1) on the detector this cache is bound to: the frame is detected as detect() would
    // detect it (threshold — train.m uses -1, setThresh —, candidate filter, pad, pyramid kind), its records stay on the device and become
    // negatives, ub grows by every record's slack.  action: PBD_MINE_NONE / _ONE / _OPT, what detect.m would now run.
    struct Mined { int records, written, action; };
    Mined mine(const Mat& im, int id) {
      if (im.depth() != PBD_8U) throw Exception(PBD_ERR_UNSUPPORTED, "mining: 8-bit frames only");
      Mined m{-1, -1, -1};
      dev_->check(pbd_qp_mine_u8(q_, im.ptr<uint8_t>(), im.cols, im.rows, im.channels(), (int)im.step(), id, &m.records, &m.written, &m.action));
      return m;
    }
    // the same on the frame that was put into `slot` of a pyramid store whose signature is this cache's detector's: mine(image, id)'s
    // records, examples, ub and action in bits (include/pbd_c.h "pyramid store")
    Mined mineStored(const PyramidStore& store, int slot, int id) {
      Mined m{-1, -1, -1};
      dev_->check(pbd_qp_mine_stored(q_, store.get(), slot, id, &m.records, &m.written, &m.action));
      return m;
    }
    // ---- latent positives (include/pbd_c.h "latent positives") ----
    // train.m:187's detect(im, model, 0, bbox, overlap, id, 1) on the detector this cache is bound to: the best pose whose every part
    // overlaps its box in `truth` (as detectLatent takes them) stays on the device and becomes one example of label +1.  roi (optional;
    // x, y, width, height as pbd_croppos gives it): the frame is that view of `im`, read in place; `truth` is then relative to it.
    // found = 0: no pose, nothing written; found = 1, written = 0: the cache was full.
    pbd_latent_example writeLatent(const Mat& im, const std::vector<Rect>& truth, double overlap, int id,
                                   const std::vector<int>& mix = std::vector<int>(), int component = -1, const int32_t* roi = nullptr) {
      if (im.depth() != PBD_8U) throw Exception(PBD_ERR_UNSUPPORTED, "latent positives: 8-bit frames only");
      const int mp = pbd_max_parts(dev_->h), cn = im.channels();
      std::vector<int32_t> tr((size_t)mp * 4, 0), mx((size_t)mp, -1);
      for (size_t p = 0; p < truth.size() && p < (size_t)mp; ++p) {
        tr[p * 4] = truth[p].x; tr[p * 4 + 1] = truth[p].y; tr[p * 4 + 2] = truth[p].width; tr[p * 4 + 3] = truth[p].height;
      }
      for (size_t p = 0; p < mix.size() && p < (size_t)mp; ++p) mx[p] = mix[p];
      int x = 0, y = 0, w = im.cols, h = im.rows;
      if (roi) {
        x = roi[0]; y = roi[1]; w = roi[2]; h = roi[3];
        if (x < 0 || y < 0 || w < 1 || h < 1 || x + w > im.cols || y + h > im.rows) throw Exception(PBD_ERR_ARG, "ExampleCache::writeLatent: roi outside the frame");
      }
      pbd_latent_example out{};
      dev_->check(pbd_qp_write_latent_u8(q_, im.ptr<uint8_t>(y) + (size_t)x * cn, w, h, cn, (int)im.step(), tr.data(), mix.empty() ? nullptr : mx.data(),
                                         component, overlap, id, &out));
      return out;
    }
    // find(qp.sv) shuffled as pbd_qp_opt shuffles its first pass: Fisher-Yates from the back, SplitMix64(seed) modulo the positions left
    std::vector<int32_t> shuffledSupport(uint64_t seed) {
      std::vector<unsigned char> sv;
      state(nullptr, &sv, nullptr);
      std::vector<int32_t> I;
      for (int i = 0, n = size(); i < n; ++i) if (sv[i]) I.push_back(i);
      uint64_t s = seed;
      for (size_t u = I.size(); u-- > 1;) {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        std::swap(I[u], I[(size_t)(z % (uint64_t)(u + 1))]);
      }
      return I;
    }
    // train.m:99-108 with detect.m's optimize at frame granularity: per image mine(); on PBD_MINE_OPT opt then prune, on PBD_MINE_ONE one()
    // over shuffledSupport(seed); after either applyWeights(); stops behind the image after which sum(sv) == capacity (train.m:105).
    // Not done here: mid-frame model updates and detect.m's random visiting order.  train.m:96's model.interval = 2 is the detector's
    // setInterval(2) around this call (PartsBasedDetector::train does it).
    std::vector<Mined> mineNegatives(const std::vector<Mat>& images, int first_id = 0, double tol = .05, int max_iter = 1000, uint64_t seed = 0) {
      std::vector<Mined> out;
      for (size_t i = 0; i < images.size(); ++i) {
        out.push_back(mine(images[i], first_id + (int)i));
        const int act = out.back().action;
        if (act == PBD_MINE_OPT) { opt(tol, max_iter, seed); prune(); }
        else if (act == PBD_MINE_ONE) one(shuffledSupport(seed));
        if (act != PBD_MINE_NONE) applyWeights();
        std::vector<unsigned char> sv;
        state(nullptr, &sv, nullptr);
        int nsv = 0;
        for (int e = 0, n = size(); e < n; ++e) nsv += sv[e] != 0;
        if (nsv == capacity()) break;
      }
      return out;
    }
   private:
    void score_(const std::vector<double>& w, const int32_t* inds, int n, std::vector<double>& out) {
      int len = 0; dims(&len, nullptr, nullptr, nullptr);
      if (w.size() != (size_t)len) throw Exception(PBD_ERR_ARG, "ExampleCache::score: w must have len elements");
      out.assign((size_t)n, 0.0);
      dev_->check(pbd_qp_score(q_, w.data(), inds, n, out.data()));
    }
    void lincomb_(const std::vector<double>& a, const int32_t* inds, int n, std::vector<double>& w) {
      int len = 0, cap = 0; dims(&len, nullptr, &cap, nullptr);
      if (a.size() > (size_t)cap) throw Exception(PBD_ERR_ARG, "ExampleCache::lincomb: a has more elements than the cache's capacity");
      std::vector<double> av((size_t)cap, 0.0);   // pbd_qp_lincomb reads capacity doubles
      std::copy(a.begin(), a.end(), av.begin());
      w.assign((size_t)len, 0.0);
      dev_->check(pbd_qp_lincomb(q_, av.data(), inds, n, w.data()));
    }
  };
  std::unique_ptr<ExampleCache> exampleCache(int capacity, double cpos, double cneg, const double* wreg = nullptr, const double* w0 = nullptr) {
    if (!dev_) throw Exception(PBD_ERR_STATE, "exampleCache() before distributeModel()");
    return std::unique_ptr<ExampleCache>(new ExampleCache(dev_, capacity, cpos, cneg, wreg, w0));
  }
  // ---- evaluation ledger (include/pbd_c.h "evaluation ledger"): matlab/evaluation/eval_pck.m, eval_apk.m and VOCap.m on the GPU ----
  // Test frames go in with their annotated persons — points[ngt][P][2] and scale[ngt], P = the model's parts per component —; per frame
  // only counts and found flags come back; pck() and apk() return P doubles each.  addPck is testmodel_gtbox.m's protocol (the best pose
  // on every person's keypoint box), addApk testmodel.m's (this detector's threshold, candidate filter and NMS).  A call that would
  // overflow the ledger throws PBD_ERR_CAPACITY and adds nothing.
  class Evaluation {
    std::shared_ptr<Device> dev_;
    pbd_eval* e_ = nullptr;
   public:
    Evaluation(std::shared_ptr<Device> dev, int nparts, int max_instances, int max_detections, double apk_thresh) : dev_(std::move(dev)) {
      dev_->check(pbd_eval_create(dev_->h, nparts, max_instances, max_detections, apk_thresh, &e_));
    }
    ~Evaluation() { pbd_eval_destroy(e_); }
    Evaluation(const Evaluation&) = delete;
    Evaluation& operator=(const Evaluation&) = delete;
    struct Dims { int nparts, instances, detections, frames; long long npos; };
    Dims dims() const { Dims d{}; dev_->check(pbd_eval_dims(e_, &d.nparts, &d.instances, &d.detections, &d.npos, &d.frames)); return d; }
    void reset() { dev_->check(pbd_eval_reset(e_)); }
    // -> found[ngt]: which persons have a pose
    std::vector<int> addPck(const Mat& im, const std::vector<double>& points, const std::vector<double>& scale, double overlap = 0.3) {
      if (im.depth() != PBD_8U) throw Exception(PBD_ERR_UNSUPPORTED, "evaluation: 8-bit frames only");
      persons(points, scale);
      std::vector<int> found(scale.size(), 0);
      dev_->check(pbd_eval_pck_frame_u8(e_, im.ptr<uint8_t>(), im.cols, im.rows, im.channels(), (int)im.step(), points.data(), scale.data(),
                                        (int)scale.size(), overlap, found.data(), nullptr, nullptr));
      return found;
    }
    // -> the frame's final records
    int addApk(const Mat& im, const std::vector<double>& points, const std::vector<double>& scale) {
      if (im.depth() != PBD_8U) throw Exception(PBD_ERR_UNSUPPORTED, "evaluation: 8-bit frames only");
      persons(points, scale);
      int records = 0;
      dev_->check(pbd_eval_apk_frame_u8(e_, im.ptr<uint8_t>(), im.cols, im.rows, im.channels(), (int)im.step(), points.data(), scale.data(),
                                        (int)scale.size(), &records, nullptr));
      return records;
    }
    // same-sized frames; points[f] / scale[f]: frame f's persons (at most PBD_GT_MAX).  -> found per frame / records per frame
    std::vector<std::vector<int>> addPckBatch(const std::vector<Mat>& ims, const std::vector<std::vector<double>>& points,
                                              const std::vector<std::vector<double>>& scale, double overlap = 0.3) {
      Batch b(*this, ims, points, scale);
      std::vector<int> found(ims.size() * PBD_GT_MAX, 0);
      dev_->check(pbd_eval_pck_frame_batch_u8(e_, b.ptrs.data(), (int)ims.size(), ims[0].cols, ims[0].rows, ims[0].channels(), (int)ims[0].step(),
                                              b.pts.data(), b.sc.data(), b.ngt.data(), overlap, found.data(), nullptr, nullptr));
      std::vector<std::vector<int>> out(ims.size());
      for (size_t f = 0; f < ims.size(); ++f) out[f].assign(found.begin() + f * PBD_GT_MAX, found.begin() + f * PBD_GT_MAX + b.ngt[f]);
      return out;
    }
    std::vector<int32_t> addApkBatch(const std::vector<Mat>& ims, const std::vector<std::vector<double>>& points,
                                     const std::vector<std::vector<double>>& scale) {
      Batch b(*this, ims, points, scale);
      std::vector<int32_t> records(ims.size(), 0);
      dev_->check(pbd_eval_apk_frame_batch_u8(e_, b.ptrs.data(), (int)ims.size(), ims[0].cols, ims[0].rows, ims[0].channels(), (int)ims[0].step(),
                                              b.pts.data(), b.sc.data(), b.ngt.data(), records.data(), nullptr));
      return records;
    }
    // rule: PBD_EVAL_SCALE_LAST is eval_pck.m:13 as written (the last instance's scale for all), PBD_EVAL_SCALE_OWN each instance's own
    std::vector<double> pck(double thresh = .5, int rule = PBD_EVAL_SCALE_LAST) {
      std::vector<double> out((size_t)dims().nparts, 0.0);
      dev_->check(pbd_eval_pck(e_, thresh, rule, out.data()));
      return out;
    }
    // prec / rec (optional): [P][M] in sorted order
    std::vector<double> apk(std::vector<double>* prec = nullptr, std::vector<double>* rec = nullptr) {
      const Dims d = dims();
      std::vector<double> out((size_t)d.nparts, 0.0);
      if (prec) prec->assign((size_t)d.nparts * d.detections, 0.0);
      if (rec) rec->assign((size_t)d.nparts * d.detections, 0.0);
      dev_->check(pbd_eval_apk(e_, out.data(), prec ? prec->data() : nullptr, rec ? rec->data() : nullptr));
      return out;
    }
    pbd_eval* ledger() { return e_; }
   private:
    void persons(const std::vector<double>& points, const std::vector<double>& scale) const {
      if (points.size() != scale.size() * (size_t)dims().nparts * 2) throw Exception(PBD_ERR_ARG, "Evaluation: points[ngt][P][2] and scale[ngt]");
    }
    struct Batch {
      std::vector<const uint8_t*> ptrs; std::vector<double> pts, sc; std::vector<int> ngt;
      Batch(const Evaluation& e, const std::vector<Mat>& ims, const std::vector<std::vector<double>>& points, const std::vector<std::vector<double>>& scale) {
        const size_t B = ims.size(), P = (size_t)e.dims().nparts;
        if (!B || points.size() != B || scale.size() != B) throw Exception(PBD_ERR_ARG, "Evaluation: one points / scale vector per frame");
        pts.assign(B * PBD_GT_MAX * P * 2, 0.0); sc.assign(B * PBD_GT_MAX, 0.0); ngt.assign(B, 0);
        for (size_t f = 0; f < B; ++f) {
          if (ims[f].depth() != PBD_8U || ims[f].cols != ims[0].cols || ims[f].rows != ims[0].rows || ims[f].channels() != ims[0].channels() ||
              ims[f].step() != ims[0].step())
            throw Exception(PBD_ERR_ARG, "Evaluation: a batch is 8-bit frames of one size and stride");
          e.persons(points[f], scale[f]);
          if (scale[f].size() > PBD_GT_MAX) throw Exception(PBD_ERR_ARG, "Evaluation: at most PBD_GT_MAX persons per frame");
          ptrs.push_back(ims[f].ptr<uint8_t>());
          ngt[f] = (int)scale[f].size();
          std::copy(points[f].begin(), points[f].end(), pts.begin() + f * PBD_GT_MAX * P * 2);
          std::copy(scale[f].begin(), scale[f].end(), sc.begin() + f * PBD_GT_MAX);
        }
      }
    };
  };
  std::unique_ptr<Evaluation> evaluation(int nparts, int max_instances, int max_detections, double apk_thresh = .5) {
    if (!dev_) throw Exception(PBD_ERR_STATE, "evaluation() before distributeModel()");
    return std::unique_ptr<Evaluation>(new Evaluation(dev_, nparts, max_instances, max_detections, apk_thresh));
  }
  // detect(im, model, thresh, [], 0, id, label)'s qp_write of every detection (matlab/learning/train.m:102): `candidates` (of the LAST
  // frame, or a selection) appended to `cache` as standardised examples, on the GPU.  Returns how many were written (a full cache
  // takes no more and is no error).
  int writeExamples(const vectorCandidate& candidates, ExampleCache& cache, int label, int id) {
    if (!dev_) throw Exception(PBD_ERR_STATE, "writeExamples() before distributeModel()");
    const size_t n = candidates.size(), mp = (size_t)pbd_max_parts(dev_->h);
    std::vector<pbd_candidate_head> heads(n);
    std::vector<int32_t> locs(n * mp * 3, 0);
    for (size_t i = 0; i < n; ++i) {
      const Candidate& c = candidates[i];
      heads[i].score = c.score(); heads[i].component = c.component(); heads[i].level = c.level; heads[i].nparts = (int32_t)c.parts().size();
      std::copy(c.locs.begin(), c.locs.begin() + std::min(c.locs.size(), mp * 3), locs.begin() + i * mp * 3);
    }
    int written = 0;
    dev_->check(pbd_qp_write(cache.q_, heads.data(), locs.data(), (int)n, label, id, &written));
    return written;
  }
  // poslatent of matlab/learning/train.m:166-193: every item whose parts all have a box area (width + 1) * (height + 1) of at least
  // prod(maxsize * sbin) is cropped around its boxes (croppos.m: a view, nothing is copied) and its best overlapping pose becomes one
  // positive of `cache` on the GPU (ExampleCache::writeLatent).  The image id is first_id + the item's index (MATLAB: 1-based), skipped
  // items included.  numpositives[c]: the found poses of component c; blocks (optional): per item its block, found = -1 where skipped.
  struct Positive { const Mat* im; std::vector<Rect> truth; std::vector<int> mix; };
  std::vector<int> latentPositives(const std::vector<Positive>& positives, ExampleCache& cache, double overlap = 0.6, int first_id = 1,
                                   std::vector<pbd_latent_example>* blocks = nullptr) {
    if (!dev_) throw Exception(PBD_ERR_STATE, "latentPositives() before distributeModel()");
    std::vector<int> numpositives((size_t)ncomponents_, 0);
    if (blocks) blocks->clear();
    for (size_t i = 0; i < positives.size(); ++i) {
      const Positive& P = positives[i];
      pbd_latent_example blk{};
      blk.found = -1;
      bool small = P.truth.empty();
      for (const Rect& r : P.truth) small = small || ((double)r.width + 1) * ((double)r.height + 1) < min_area_;
      if (!small) {
        std::vector<int32_t> tr(P.truth.size() * 4), out(P.truth.size() * 4);
        for (size_t p = 0; p < P.truth.size(); ++p) { tr[p * 4] = P.truth[p].x; tr[p * 4 + 1] = P.truth[p].y; tr[p * 4 + 2] = P.truth[p].width; tr[p * 4 + 3] = P.truth[p].height; }
        int32_t roi[4];
        const int rc = pbd_croppos(tr.data(), (int)P.truth.size(), P.im->cols, P.im->rows, roi, out.data());
        if (rc != PBD_OK) throw Exception(rc, "latentPositives: the truth boxes lie outside the frame, or have a negative size");
        std::vector<Rect> rel(P.truth.size());
        for (size_t p = 0; p < rel.size(); ++p) rel[p] = Rect{out[p * 4], out[p * 4 + 1], out[p * 4 + 2], out[p * 4 + 3]};
        blk = cache.writeLatent(*P.im, rel, overlap, first_id + (int)i, P.mix, -1, roi);
        if (blk.found && blk.component >= 0 && blk.component < ncomponents_) numpositives[(size_t)blk.component]++;
      }
      if (blocks) blocks->push_back(blk);
    }
    return numpositives;
  }
  // ---- matlab/learning/train.m on the live detector (include/pbd_c.h "one training round") ----
  // One call for train.m:73-121: per round cache.clear(); the positives — latent (warp == 0: latentPositives(overlap), ids 1, 2, ...) or
  // warped (warp > 0: writeWarped of every box at component 0's root filter and bias, id i + 1, boxes below prod(maxsize * sbin)
  // skipped) —; fix(n), prune, opt, applyWeights; interval0 = interval(), setInterval(2), setThresh(-1); mineNegatives with ids 1, 2, ...
  // (it stops behind the image after which sum(sv) == capacity); opt, applyWeights; setThresh((float)positiveThreshold(.05));
  // setInterval(interval0).  An exception from the interval change on restores the interval and the threshold before it goes on.
  // The cache has cpos = C * wpos, cneg = C, model2vec.m's wreg and w0 (pbd_qp_create's defaults) and its noneg; capacity <= 0: the
  // default 10 * (wpos + 1) * positives (train.m:30-31,46 without its 6 GB floor).  The trained weights and threshold are the detector's
  // (weights(), thresh()); the Model object handed to distributeModel is not touched.
  // Deviations from train.m, as the binding's train(): no 6 GB floor; clear() also resets the solver's a, sv and bounds (train.m:75 leaves
  // stale ones for rounds after the first); and mineNegatives' — the model is constant over a frame, the level order is fixed, the
  // shuffles are seeded.
  struct WarpedPositive { const Mat* im; GtBox box; };   // box: (x1, y1, x2, y2), 1-based inclusive
  struct TrainOptions { int iter = 1; double C = 0.002, wpos = 2, overlap = 0.6; int capacity = 0; double tol = .05; int max_iter = 1000; uint64_t seed = 0; };
  struct TrainReport {
    std::vector<int> numpositives;   // per component (warped: one entry, the examples written)
    int n[3] = {0, 0, 0}, sv[3] = {0, 0, 0};   // examples and support vectors after the positives, after mining, after the last solve
    double lb = 0, ub = 0;           // the last solve's bounds
    float thresh = 0;                // as set
    std::vector<typename ExampleCache::Mined> mined;   // per frame mined
    int passes[2] = {0, 0};          // pbd_qp_one calls of the first and the last solve
  };
  std::vector<TrainReport> train(const std::vector<Positive>& positives, const std::vector<Mat>& negatives) { TrainOptions o; return train(positives, negatives, o); }
  std::vector<TrainReport> train(const std::vector<Positive>& positives, const std::vector<Mat>& negatives, const TrainOptions& o) {
    return train_(positives.size(), negatives, o, [&](ExampleCache& cache, TrainReport& r) {
      r.numpositives = latentPositives(positives, cache, o.overlap);
    });
  }
  std::vector<TrainReport> train(const std::vector<WarpedPositive>& positives, const std::vector<Mat>& negatives) { TrainOptions o; return train(positives, negatives, o); }
  std::vector<TrainReport> train(const std::vector<WarpedPositive>& positives, const std::vector<Mat>& negatives, const TrainOptions& o) {
    return train_(positives.size(), negatives, o, [&](ExampleCache& cache, TrainReport& r) {
      for (size_t i = 0; i < positives.size(); ++i) {
        const std::vector<int32_t> id(1, (int32_t)i + 1);
        cache.writeWarped(*positives[i].im, std::vector<GtBox>(1, positives[i].box), root_filter_, root_bias_, min_area_, nullptr, &id);
      }
      r.numpositives.assign(1, cache.size());
    });
  }
 private:
  template <typename F>
  std::vector<TrainReport> train_(size_t npos, const std::vector<Mat>& negatives, const TrainOptions& o, F write_positives) {
    if (!dev_) throw Exception(PBD_ERR_STATE, "train() before distributeModel()");
    const int cap = o.capacity > 0 ? o.capacity : (int)(10 * (o.wpos + 1) * (double)npos);
    auto cache = exampleCache(cap, o.C * o.wpos, o.C);
    std::vector<int32_t> noneg;   // model2vec.m: elements 0 and 2 of every deformation
    for (int d = 0; d < ndefs_; ++d) { noneg.push_back(nbias_ + 4 * d); noneg.push_back(nbias_ + 4 * d + 2); }
    cache->noneg(noneg);
    std::vector<TrainReport> report;
    for (int t = 0; t < o.iter; ++t) {
      TrainReport r;
      auto count = [&](int at) { r.n[at] = cache->size(); r.sv[at] = cache->supportCount(); };
      cache->clear();
      write_positives(*cache, r);
      count(0);
      cache->fix(r.n[0]);
      cache->prune();
      r.passes[0] = cache->opt(o.tol, o.max_iter, o.seed);
      cache->applyWeights();
      const int interval0 = interval();
      const float thresh0 = thresh();
      try {
        setInterval(2);
        setThresh(-1.f);
        r.mined = cache->mineNegatives(negatives, 1, o.tol, o.max_iter, o.seed);
        count(1);
        r.passes[1] = cache->opt(o.tol, o.max_iter, o.seed, &r.lb, &r.ub);
        cache->applyWeights();
        count(2);
        r.thresh = (float)cache->positiveThreshold(.05);
        setThresh(r.thresh);
      } catch (...) {
        setThresh(thresh0);
        setInterval(interval0);
        throw;
      }
      setInterval(interval0);
      report.push_back(r);
    }
    return report;
  }
  int nbias_ = 0, ndefs_ = 0, root_filter_ = 0, root_bias_ = 0;   // of the distributed model: noneg's indices, writeWarped's defaults
  double min_area_ = 0;   // prod(maxsize * sbin) of the distributed model: latentPositives' minimum part area (train.m:170)
  int features_entry(const pbd_candidate_head* hd, const int32_t* lc, int n, FeatureBlock* b, float* w) { return pbd_candidates_features(dev_->h, hd, lc, n, b, w); }
  int features_entry(const pbd_candidate_head* hd, const int32_t* lc, int n, FeatureBlock* b, double* w) { return pbd_candidates_features_f64(dev_->h, hd, lc, n, b, w); }
};

inline void Candidate::sort(std::vector<Candidate>& c) {
  std::stable_sort(c.begin(), c.end(), [](const Candidate& a, const Candidate& b) { return a.score() > b.score(); });
}
inline void Candidate::nonMaximaSuppression(int im_w, int im_h, std::vector<Candidate>& c, float overlap) {
  std::vector<uint8_t> scratch((size_t)im_w * im_h, 0);
  size_t keep = 0;
  for (size_t n = 0; n < c.size(); ++n) {
    Rect b = c[n].boundingBox();
    int x1 = std::max(b.x, 0), y1 = std::max(b.y, 0);
    int w = std::min(b.x + b.width, im_w) - x1, h = std::min(b.y + b.height, im_h) - y1;
    if (w <= 0 || h <= 0) x1 = y1 = w = h = 0;
    double sum = 0;
    for (int y = y1; y < y1 + h; ++y) for (int x = x1; x < x1 + w; ++x) sum += scratch[(size_t)y * im_w + x];
    if (sum / (double)(w * h) > (double)overlap) continue;
    for (int y = y1; y < y1 + h; ++y) memset(&scratch[(size_t)y * im_w + x1], 1, w);
    if (keep != n) c[keep] = c[n];
    keep++;
  }
  c.resize(keep);
}
inline void Candidate::nonMaximaSuppressionParts(std::vector<Candidate>& c, float overlap, int top) {
  size_t mp = 1;
  for (const Candidate& k : c) mp = std::max(mp, k.parts().size());
  std::vector<pbd_candidate_head> heads(c.size());
  std::vector<int32_t> boxes(c.size() * mp * 4, 0);
  for (size_t n = 0; n < c.size(); ++n) {
    heads[n] = pbd_candidate_head{c[n].score(), c[n].component(), (int)n, (int)c[n].parts().size()};   // (level: the index, to find the kept ones)
    for (size_t p = 0; p < c[n].parts().size(); ++p) {
      const Rect& r = c[n].parts()[p];
      int32_t* b = &boxes[(n * mp + p) * 4];
      b[0] = r.x; b[1] = r.y; b[2] = r.width; b[3] = r.height;
    }
  }
  int kept = 0;
  const int rc = pbd_candidates_nms_parts(heads.data(), boxes.data(), nullptr, (int)c.size(), (int)mp, overlap, top, &kept);
  if (rc != PBD_OK) throw Exception(rc, "Candidate::nonMaximaSuppressionParts: a finite overlap and top >= 0");
  for (int k = 0; k < kept; ++k)
    if (heads[k].level != k) c[k] = c[heads[k].level];
  c.resize((size_t)kept);
}

inline std::vector<int> Candidate::bestOverlap(const std::vector<Candidate>& c, const std::vector<GtBox>& gt, double overlap, std::vector<double>* o) {
  size_t mp = 1;
  for (const Candidate& k : c) mp = std::max(mp, k.parts().size());
  std::vector<pbd_candidate_head> heads(c.size());
  std::vector<int32_t> boxes(c.size() * mp * 4, 0);
  for (size_t n = 0; n < c.size(); ++n) {
    heads[n] = pbd_candidate_head{c[n].score(), c[n].component(), c[n].level, (int)c[n].parts().size()};
    for (size_t p = 0; p < c[n].parts().size(); ++p) {
      const Rect& r = c[n].parts()[p];
      int32_t* b = &boxes[(n * mp + p) * 4];
      b[0] = r.x; b[1] = r.y; b[2] = r.width; b[3] = r.height;
    }
  }
  std::vector<int> best(gt.size(), -1);
  std::vector<double> ov(gt.size(), 0.0);
  const int rc = pbd_candidates_best_overlap(heads.data(), boxes.data(), (int)c.size(), (int)mp, gt.empty() ? nullptr : &gt[0].x1, (int)gt.size(),
                                             overlap, best.data(), ov.data());
  if (rc != PBD_OK) throw Exception(rc, "Candidate::bestOverlap: finite gt boxes, overlap and scores, at most PBD_GT_MAX boxes");
  if (o) *o = ov;
  return best;
}

// matlab/learning/clusterparts.m on the GPU (pbd_cluster_parts; needs no detector): def[P][n][2] the parts' positions (data_def.m),
// parent 0-based with -1 at the root, K[p] clusters for part p, R k-means trials per part -> the positives' 0-based mixture labels
// [P][n], what Positive::mix and buildmodel.m take.  Throws on the header's refusals.
inline std::vector<int32_t> clusterParts(const std::vector<double>& def, int n, const std::vector<int32_t>& parent, const std::vector<int32_t>& K,
                                         int R = 100, uint64_t seed = 0, int max_iter = 1000, int device = 0, int* capped = nullptr) {
  const size_t P = parent.size();
  if (n < 1 || K.size() != P || def.size() != P * (size_t)n * 2) throw Exception(PBD_ERR_ARG, "clusterParts: def[P][n][2], one parent and one K per part");
  std::vector<int32_t> idx(P * (size_t)n);
  int32_t cap = 0;
  const int rc = pbd_cluster_parts(device, def.data(), n, (int)P, parent.data(), K.data(), R, seed, max_iter, idx.data(), nullptr, nullptr, nullptr,
                                   nullptr, nullptr, &cap);
  if (rc != PBD_OK) throw Exception(rc, "clusterParts: refused (include/pbd_c.h \"part mixtures\"), or a HIP failure");
  if (capped) *capped = cap;
  return idx;
}

// ---- virtual positives (include/pbd_c.h "virtual positives"; need no detector) ----
// matlab/learning/map_rotate_points.m: (x, y) rows in the 0-based frame of a w x hgt image into its canvas at `deg` degrees
// (PBD_ROT_ORI2NEW) or back (PBD_ROT_NEW2ORI); pts = x0, y0, x1, y1, ...
inline std::vector<double> mapRotatePoints(const std::vector<double>& pts, int w, int hgt, double deg, int dir = PBD_ROT_ORI2NEW) {
  std::vector<double> out(pts.size());
  const int rc = pts.size() % 2 ? PBD_ERR_ARG : pbd_map_rotate_points(pts.data(), (int)(pts.size() / 2), w, hgt, deg, dir, out.data());
  if (rc != PBD_OK) throw Exception(rc, pts.size() % 2 ? "mapRotatePoints: (x, y) pairs" : pbd_augment_last_error());
  return out;
}
// the keypoints of the mirrored frame: out[p] = (w - 1 - x[mirror[p]], y[mirror[p]]); an empty mirror is the identity
inline std::vector<double> flipPoints(const std::vector<double>& pts, int w, const std::vector<int32_t>& mirror = std::vector<int32_t>()) {
  std::vector<double> out(pts.size());
  const bool bad = pts.size() % 2 || (!mirror.empty() && mirror.size() != pts.size() / 2);
  const int rc = bad ? PBD_ERR_ARG : pbd_flip_points(pts.data(), (int)(pts.size() / 2), w, mirror.empty() ? nullptr : mirror.data(), out.data());
  if (rc != PBD_OK) throw Exception(rc, bad ? "flipPoints: (x, y) pairs, one mirror entry per point" : pbd_augment_last_error());
  return out;
}
// the virtual copies of an 8-bit frame, one per op (the mirror first, then the rotation), on HIP device `device` in one launch
// (host = true: pbd_augment_host_u8, the same definition without a GPU, identical bytes)
inline std::vector<Mat> augment(const Mat& im, const std::vector<pbd_augment_op>& ops, int device = 0, bool host = false) {
  if (im.depth() != PBD_8U) throw Exception(PBD_ERR_UNSUPPORTED, "augment: 8-bit frames only");
  std::vector<Mat> out(ops.size());
  std::vector<uint8_t*> ptrs(ops.size());
  std::vector<int> steps(ops.size());
  for (size_t i = 0; i < ops.size(); ++i) {
    int ow = im.cols, oh = im.rows;
    if (ops[i].rotate && pbd_rotate_geometry(im.cols, im.rows, ops[i].deg, &ow, &oh, nullptr) != PBD_OK) throw Exception(PBD_ERR_ARG, pbd_augment_last_error());
    out[i].create(oh, ow, PBD_8U, im.channels());
    ptrs[i] = out[i].ptr<uint8_t>(); steps[i] = (int)out[i].step();
  }
  const int rc = host ? pbd_augment_host_u8(im.ptr<uint8_t>(), im.cols, im.rows, im.channels(), (int)im.step(), ops.data(), (int)ops.size(), ptrs.data(), steps.data())
                      : pbd_augment_u8(device, im.ptr<uint8_t>(), im.cols, im.rows, im.channels(), (int)im.step(), ops.data(), (int)ops.size(), ptrs.data(), steps.data());
  if (rc != PBD_OK) throw Exception(rc, pbd_augment_last_error());
  return out;
}
// the same from device memory into device memory the caller allocated: outs[i] takes op i's canvas (pbd_rotate_geometry).  The library
// works on a stream of its own, which waits for no other: whatever produced `im`, or still uses the outputs, on the caller's streams
// must be complete before the call; on return the canvases are complete.
inline void augmentDevice(const DeviceFrame& im, const std::vector<pbd_augment_op>& ops, const std::vector<DeviceFrame>& outs, int device = 0) {
  if (outs.size() != ops.size()) throw Exception(PBD_ERR_ARG, "augmentDevice: one output per op");
  std::vector<void*> ptrs(ops.size());
  std::vector<int> steps(ops.size());
  for (size_t i = 0; i < ops.size(); ++i) { ptrs[i] = const_cast<void*>(outs[i].data); steps[i] = (int)outs[i].step; }
  const int rc = pbd_augment_dev_u8(device, im.data, im.cols, im.rows, im.channels, (int)im.step, ops.data(), (int)ops.size(), ptrs.data(), steps.data());
  if (rc != PBD_OK) throw Exception(rc, pbd_augment_last_error());
}

}  // namespace pbd
#endif  // PBD_HOST_HPP_
