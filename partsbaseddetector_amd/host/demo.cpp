// demo.cpp — the reference's canonical caller (src/demo.cpp:55-118) against the MI355X path:
//   pbd_demo model.bin image.raw width height channels [stagewise|double|stagewise-double] [--part-scores] [--pad N] [--features FILE] [--examples FILE] [--matlab-pyramid]
//            [--gtbox x1,y1,x2,y2[,overlap]]... [--mine FILE]... [--poslatent FILE x,y,w,h[;x,y,w,h...]]... [--train]
//   pbd_demo model.bin image.raw width height channels perturb-features <responses-out.bin>
//   pbd_demo model.bin image.raw width height channels oracle-responses <responses-in.bin>
// deserialize -> distributeModel -> detect -> Candidate::sort, then prints the candidates (the
// reference shows them in a window; here they go to stdout so tests can compare them).
// `stagewise` walks pyramid -> pdf -> min -> argmin through the interface classes instead of the
// fused detect() (src/PartsBasedDetector.cpp:73-89); `double` runs PartsBasedDetector<double> like the
// ROS node and the ecto cell (ros/Node.hpp:121, cells/detect.cpp:93) instead of <float> (src/demo.cpp:85).
#include <cstdio>
#include <cstdlib>
#include <memory>
#include "pbd_filestorage.hpp"
using namespace pbd;

// --gtbox x1,y1,x2,y2[,overlap] (anywhere, repeatable): testmodel_gtbox.m's protocol — per box the highest-scoring pose whose part centres'
// box covers more than `overlap` of it (default 0.3; the last one given holds for every box), printed instead of the candidate list
static std::vector<GtBox> g_gtbox;
static const char* g_examples_file = nullptr;   // --examples FILE (anywhere): the detections as QP examples, written to FILE
static double g_gt_overlap = 0.3;
static std::vector<GtBox> g_warp;               // --warp x1,y1,x2,y2 (anywhere, repeatable): the boxes as warped positives, dumped and nothing else
// --mine FILE (anywhere, repeatable): raw frames of the image's size mined as negatives (train.m:99-108) into a cache of 256 examples,
// Cpos = Cneg = 1, ids 0, 1, ..., at the model's threshold; per frame the records, how many were written, and the action
static std::vector<const char*> g_mine;
// --poslatent FILE x,y,w,h[;...] (anywhere, repeatable): raw frames of the image's size as latent positives (train.m:166-193) — one truth
// box per part, as detect() returns boxes — into a cache of 256 examples, Cpos = Cneg = 1, ids 1, 2, ..., overlap 0.6; per frame its block
struct PosLatent { const char* file; std::vector<Rect> truth; };
static std::vector<PosLatent> g_poslatent;
// --train (anywhere; with --poslatent and --mine): one latent round of train.m (PartsBasedDetector<T>::train, defaults: C .002, wpos 2,
// overlap .6, capacity 30 per positive) over the --poslatent frames as positives and the --mine frames as negatives; one line per report field
static bool g_train = false;
static Mat read_frame(const char* what, const char* name, const Mat& im) {
  Mat fr(im.rows, im.cols, PBD_8U, im.channels());
  const size_t bytes = (size_t)im.rows * im.cols * im.channels();
  FILE* f = fopen(name, "rb");
  if (!f || fread(fr.ptr<uint8_t>(), 1, bytes, f) != bytes) { printf("%s %s: not found or not a frame of the image's size\n", what, name); exit(-4); }
  fclose(f);
  return fr;
}
static void print_pose(const Candidate& c) {
  printf("%.9g %d %d", c.score(), c.component(), c.level);
  for (const Rect& r : c.parts()) printf(" %d,%d,%d,%d", r.x, r.y, r.width, r.height);
  printf("\n");
}

// The stage interfaces process THEIR ARGUMENTS (include/IConvolutionEngine.hpp:56, include/DynamicProgram.hpp:74-75):
//   perturb:  the feature pyramid is halved in place between pyramid() and pdf(); the responses of the first and the
//             last level go to `io_file` (the test compares them with the oracle's filter bank on the halved features);
//   oracle:   the scores min() transforms are read from `io_file` (random planes written by the test) instead of coming
//             from pdf(), and the tables min() returns are edited before argmin() (a root score raised, part 1's x
//             pointer at that cell redirected): the candidates must be those of the edited tables.
template <typename T>
static void run(Model& model, const Mat& im, bool stagewise, int special = 0, const char* io_file = nullptr, bool part_scores = false, int pad = 0,
                const char* features_file = nullptr, const float* nms_parts = nullptr, bool matlab_pyramid = false) {
  PartsBasedDetector<T> pbd(0, PBD_CONV_EXACT);
  if (nms_parts && !stagewise) {   // the fused detect() sorts and suppresses on the GPU
    pbd.setCandidateFilter(PBD_CAND_SORT_NMS, *nms_parts);
    pbd.setCandidateNms(PBD_NMS_PARTS, 1000);
  }
  pbd.setPartScores(part_scores);
  pbd.setBoundaryPad(pad);
  if (matlab_pyramid) pbd.setPyramidKind(PBD_PYRAMID_MATLAB);
  pbd.distributeModel(model);
  vectorCandidate candidates;
  if (!g_warp.empty()) {   // --warp: train.m's poswarp of the boxes at component 0's root filter and bias (Cpos 1), the columns dumped
    const int filter = model.filterid()[0][0][0], bias = model.biasid()[0][0][0];
    int mh = 0, mw = 0;
    for (const Mat& f : model.filters()) { mh = std::max(mh, f.rows); mw = std::max(mw, f.cols / model.flen()); }
    const double min_area = (double)(mh * model.binsize()) * (double)(mw * model.binsize());   // train.m:135
    auto cache = pbd.exampleCache((int)g_warp.size(), 1.0, 1.0);
    std::vector<int32_t> status;
    const int n = cache->writeWarped(im, g_warp, filter, bias, min_area, &status);
    int len = 0, k = 0;
    cache->dims(&len, &k, nullptr, nullptr);
    std::vector<float> x((size_t)n * k), b((size_t)n);
    std::vector<int32_t> ids((size_t)n * 5);
    std::vector<double> d((size_t)n);
    cache->get(0, n, x.data(), ids.data(), b.data(), d.data());
    printf("Warped positives: %d of %zu written, k %d, len %d, min area %g\n", n, g_warp.size(), k, len, min_area);
    for (size_t i = 0, e = 0; i < g_warp.size(); ++i) {
      printf("Box %zu (%g,%g,%g,%g): %s", i, g_warp[i].x1, g_warp[i].y1, g_warp[i].x2, g_warp[i].y2,
             status[i] == PBD_WARP_WRITTEN ? "written" : status[i] == PBD_WARP_SKIPPED ? "skipped" : "full");
      if (status[i] == PBD_WARP_WRITTEN) {
        double sum = 0;   // position-weighted checksum of the column, for a comparison with another run
        for (int t = 0; t < k; ++t) sum += (double)(t + 1) * (double)x[e * k + t];
        printf(" id %d blocks %d b %.9g d %.17g checksum %.17g", ids[e * 5 + 1], (int)x[e * k], b[e], d[e], sum);
        ++e;
      }
      printf("\n");
    }
    return;
  }
  if (g_train) {
    std::vector<Mat> pos, neg;
    for (const PosLatent& pl : g_poslatent) pos.push_back(read_frame("--poslatent", pl.file, im));
    for (const char* name : g_mine) neg.push_back(read_frame("--mine", name, im));
    std::vector<typename PartsBasedDetector<T>::Positive> items;
    for (size_t i = 0; i < pos.size(); ++i) items.push_back({&pos[i], g_poslatent[i].truth, {}});
    const auto report = pbd.train(items, neg);
    for (size_t t = 0; t < report.size(); ++t) {
      const auto& r = report[t];
      printf("Train %zu numpositives:", t);
      for (int c : r.numpositives) printf(" %d", c);
      printf("\nTrain %zu n: %d %d %d\nTrain %zu sv: %d %d %d\n", t, r.n[0], r.n[1], r.n[2], t, r.sv[0], r.sv[1], r.sv[2]);
      printf("Train %zu lb: %.17g\nTrain %zu ub: %.17g\nTrain %zu thresh: %.17g\n", t, r.lb, t, r.ub, t, (double)r.thresh);
      printf("Train %zu mined:", t);
      for (const auto& m : r.mined) printf(" %d,%d,%d", m.records, m.written, m.action);
      printf("\nTrain %zu passes: %d %d\n", t, r.passes[0], r.passes[1]);
    }
    printf("Interval: %d\nThreshold: %.17g\n", pbd.interval(), (double)pbd.thresh());
    return;
  }
  if (!g_mine.empty()) {
    std::vector<Mat> frames;
    for (const char* name : g_mine) {
      Mat fr(im.rows, im.cols, PBD_8U, im.channels());
      const size_t bytes = (size_t)im.rows * im.cols * im.channels();
      FILE* f = fopen(name, "rb");
      if (!f || fread(fr.ptr<uint8_t>(), 1, bytes, f) != bytes) { printf("--mine %s: not found or not a frame of the image's size\n", name); exit(-4); }
      fclose(f);
      frames.push_back(fr);
    }
    auto cache = pbd.exampleCache(256, 1.0, 1.0);
    const auto mined = cache->mineNegatives(frames);
    for (size_t i = 0; i < mined.size(); ++i)
      printf("Mine %zu: records %d written %d action %d\n", i, mined[i].records, mined[i].written, mined[i].action);
    printf("Cache: %d of %d examples, ub %.17g\n", cache->size(), cache->capacity(), cache->state(nullptr, nullptr, nullptr).ub);
    return;
  }
  if (!g_poslatent.empty()) {
    std::vector<Mat> frames;
    std::vector<typename PartsBasedDetector<T>::Positive> items;
    for (const PosLatent& pl : g_poslatent) {
      Mat fr(im.rows, im.cols, PBD_8U, im.channels());
      const size_t bytes = (size_t)im.rows * im.cols * im.channels();
      FILE* f = fopen(pl.file, "rb");
      if (!f || fread(fr.ptr<uint8_t>(), 1, bytes, f) != bytes) { printf("--poslatent %s: not found or not a frame of the image's size\n", pl.file); exit(-4); }
      fclose(f);
      frames.push_back(fr);
    }
    for (size_t i = 0; i < frames.size(); ++i) items.push_back({&frames[i], g_poslatent[i].truth, {}});
    auto cache = pbd.exampleCache(256, 1.0, 1.0);
    std::vector<pbd_latent_example> blocks;
    const std::vector<int> numpositives = pbd.latentPositives(items, *cache, 0.6, 1, &blocks);
    for (size_t i = 0; i < blocks.size(); ++i) {
      const pbd_latent_example& b = blocks[i];
      if (b.found < 0) printf("Poslatent %zu: skipped (a box below the minimum area)\n", i);
      else printf("Poslatent %zu: found %d written %d component %d level %d x %d y %d score %.17g\n", i, b.found, b.written, b.component, b.level, b.x, b.y, b.score);
    }
    printf("Positives per component:");
    for (int c : numpositives) printf(" %d", c);
    printf("\nCache: %d of %d examples\n", cache->size(), cache->capacity());
    return;
  }
  if (stagewise) {
    vectorMat pyramid;
    pbd.features().pyramid(im, pyramid);
    vector2DMat pdf, rootv, rooti;
    vector4DMat Ix, Iy, Ik;
    if (special == 1)
      for (Mat& f : pyramid)
        for (int i = 0; i < f.rows * f.cols; ++i) f.ptr<T>()[i] *= (T)0.5;
    if (special == 2) {
      FILE* f = fopen(io_file, "rb");
      if (!f) { fprintf(stderr, "cannot open %s\n", io_file); exit(6); }
      pdf.assign(pyramid.size(), vectorMat(model.filters().size()));
      for (size_t l = 0; l < pyramid.size(); ++l)
        for (Mat& r : pdf[l]) {
          r.create(pyramid[l].rows, pyramid[l].cols / 32, DataType<T>::type);
          if (!r.empty() && fread(r.ptr<T>(), sizeof(T), (size_t)r.rows * r.cols, f) != (size_t)r.rows * r.cols) { fprintf(stderr, "short read\n"); exit(6); }
        }
      fclose(f);
    } else {
      pbd.convolutionEngine().pdf(pyramid, pdf);                                // src/PartsBasedDetector.cpp:78
    }
    if (special == 1) {
      FILE* f = fopen(io_file, "wb");
      for (size_t l : {(size_t)0, pyramid.size() - 1})
        for (const Mat& r : pdf[l]) fwrite(r.ptr<T>(), sizeof(T), (size_t)r.rows * r.cols, f);
      fclose(f);
    }
    pbd.dp().min(pbd.parts(), pdf, Ix, Iy, Ik, rootv, rooti);                   // :83, the reference's signature
    if (special == 2) {
      rootv[0][0].template at<T>(0, 0) = (T)1e6;
      for (Mat& x : Ix[0][0][1]) x.at<int32_t>(0, 0) = x.cols - 1;
    }
    // the tables came back in the reference's shapes: [level][component][part][parent mixture]
    if (Ix.size() != pyramid.size() || Ix[0][0].size() != (size_t)pbd.parts().nparts(0) || !Ix[0][0][0].empty() ||
        Ix[0][0][1].empty() || Ix[0][0][1][0].rows != pdf[0][0].rows || rootv[0][0].cols != pdf[0][0].cols) {
      fprintf(stderr, "min(): unexpected table shapes\n");
      exit(5);
    }
    // position-weighted checksum of every pointer table, in [level][component][part][parent mixture] order (Ix, Iy, Ik
    // interleaved per table): the test compares it with the oracle's tables
    unsigned long long sum = 0, idx = 0;
    for (size_t n = 0; n < Ix.size(); ++n)
      for (size_t c = 0; c < Ix[n].size(); ++c)
        for (size_t p = 1; p < Ix[n][c].size(); ++p)
          for (size_t m = 0; m < Ix[n][c][p].size(); ++m)
            for (const Mat* t : {&Ix[n][c][p][m], &Iy[n][c][p][m], &Ik[n][c][p][m]})
              for (int i = 0; i < t->rows * t->cols; ++i) sum += (++idx) * (unsigned long long)(unsigned)t->ptr<int32_t>()[i];
    printf("Tables: %llu\n", sum);
    pbd.dp().argmin(pbd.parts(), rootv, rooti, pbd.features().scales(), Ix, Iy, Ik, candidates);   // :89
  } else if (!g_gtbox.empty()) {   // the selection runs on the GPU behind the detect: only the winners come back
    std::vector<int> which;
    std::vector<double> o;
    pbd.detectGtBox(im, g_gtbox, g_gt_overlap, candidates, &which, &o);
    for (size_t g = 0; g < g_gtbox.size(); ++g) {
      printf("GtBox %zu (%g,%g,%g,%g) overlap > %g: ", g, g_gtbox[g].x1, g_gtbox[g].y1, g_gtbox[g].x2, g_gtbox[g].y2, g_gt_overlap);
      if (which[g] < 0) { printf("none\n"); continue; }
      printf("o %.17g: ", o[g]);
      print_pose(candidates[which[g]]);
    }
    return;
  } else {
    Mat depth;
    pbd.detect(im, depth, candidates);
  }
  printf("Number of candidates: %ld\n", (long)candidates.size());
  if (!g_gtbox.empty()) {          // stagewise: the host function on the candidates argmin() returned, in their order
    std::vector<double> o;
    const std::vector<int> which = Candidate::bestOverlap(candidates, g_gtbox, g_gt_overlap, &o);
    for (size_t g = 0; g < g_gtbox.size(); ++g) {
      printf("GtBox %zu (%g,%g,%g,%g) overlap > %g: ", g, g_gtbox[g].x1, g_gtbox[g].y1, g_gtbox[g].x2, g_gtbox[g].y2, g_gt_overlap);
      if (which[g] < 0) { printf("none\n"); continue; }
      printf("o %.17g: ", o[g]);
      print_pose(candidates[which[g]]);
    }
    return;
  }
  Candidate::sort(candidates);
  if (nms_parts) {
    if (stagewise) Candidate::nonMaximaSuppressionParts(candidates, *nms_parts, 1000);
    printf("Kept by the parts NMS: %ld\n", (long)candidates.size());
  }
  if (features_file) {   // --features FILE: the sorted records' dense feature vectors, one row of doubles each, in the order
                         // [biasw | defw (ndefs x 4) | the filters back to back] (w . row = the record's score); header: rows, columns (int64)
    std::vector<pbd_feature_block> blocks;
    std::vector<T> windows;
    pbd.features(candidates, blocks, windows);
    const size_t mp = candidates.empty() ? 0 : blocks.size() / candidates.size(), wmax = blocks.empty() ? 0 : windows.size() / blocks.size();
    const size_t nb = model.bias().size(), nd = model.def().size();
    std::vector<size_t> foff;
    size_t dim = nb + 4 * nd;
    for (const Mat& f : model.filters()) { foff.push_back(dim); dim += (size_t)f.rows * f.cols; }
    FILE* f = fopen(features_file, "wb");
    if (!f) { fprintf(stderr, "cannot open %s\n", features_file); exit(6); }
    const long long hdr[2] = {(long long)candidates.size(), (long long)dim};
    fwrite(hdr, sizeof(long long), 2, f);
    std::vector<double> row(dim);
    for (size_t i = 0; i < candidates.size(); ++i) {
      std::fill(row.begin(), row.end(), 0.0);
      for (size_t p = 0; p < mp; ++p) {
        const pbd_feature_block& b = blocks[i * mp + p];
        if (b.bias_id < 0) continue;
        row[b.bias_id] += 1.0;
        if (b.def_id >= 0) for (int k = 0; k < 4; ++k) row[nb + 4 * (size_t)b.def_id + k] += b.def[k];
        const T* win = windows.data() + (i * mp + p) * wmax;
        for (size_t k = 0; k < (size_t)b.kh * b.kw * model.flen(); ++k) row[foff[b.filter_id] + k] += (double)win[k];
      }
      fwrite(row.data(), sizeof(double), dim, f);
    }
    fclose(f);
    printf("Features: %ld x %ld\n", (long)candidates.size(), (long)dim);
  }
  if (g_examples_file) {   // --examples FILE: the sorted records as the QP's negative examples (label -1, id 0, Cneg 1): header n, k, len
                           // (int64), then the n columns (k float32 each, qp.x verbatim), ids (5 int32 each), b (float32), d (float64)
    auto cache = pbd.exampleCache(std::max<int>(1, (int)candidates.size()), 1.0, 1.0);
    const int n = pbd.writeExamples(candidates, *cache, -1, 0);
    int len = 0, k = 0;
    cache->dims(&len, &k, nullptr, nullptr);
    std::vector<float> x((size_t)n * k), b((size_t)n);
    std::vector<int32_t> ids((size_t)n * 5);
    std::vector<double> d((size_t)n);
    cache->get(0, n, x.data(), ids.data(), b.data(), d.data());
    FILE* f = fopen(g_examples_file, "wb");
    if (!f) { fprintf(stderr, "cannot open %s\n", g_examples_file); exit(6); }
    const long long hdr[3] = {n, k, len};
    fwrite(hdr, sizeof(long long), 3, f);
    fwrite(x.data(), sizeof(float), x.size(), f);
    fwrite(ids.data(), sizeof(int32_t), ids.size(), f);
    fwrite(b.data(), sizeof(float), b.size(), f);
    fwrite(d.data(), sizeof(double), d.size(), f);
    fclose(f);
    printf("Examples: %d x %d\n", n, k);
  }
  for (const Candidate& c : candidates) {
    printf("%.9g %d %d", c.score(), c.component(), c.level);
    for (const Rect& r : c.parts()) printf(" %d,%d,%d,%d", r.x, r.y, r.width, r.height);
    printf("\n");
    if (!c.partScores().empty()) {   // --part-scores: the re-scored total beside the root score, and the weakest part
      double total = 0;
      size_t weak = 0;
      std::vector<double> sc;
      for (const pbd_part_score& s : c.partScores()) { sc.push_back((s.app + s.def) + s.bias); total += sc.back(); }
      for (size_t p = 1; p < sc.size(); ++p) if (sc[p] < sc[weak]) weak = p;
      printf("  part scores: total %.9g root %.9g weakest part %zu (%.9g = app %.9g + def %.9g + bias %.9g)\n", total, c.score(), weak,
             sc[weak], c.partScores()[weak].app, c.partScores()[weak].def, c.partScores()[weak].bias);
    }
  }
}

int main(int argc, char** argv) {
  bool part_scores = false;   // --part-scores (anywhere): per detection, the re-scored total, the root score and the weakest part
  const char* features_file = nullptr;   // --features FILE (anywhere): the detections' dense feature vectors, written to FILE
  float nms_overlap = 0.f; const float* nms_parts = nullptr;   // --nms-parts OVERLAP (anywhere): sort + nms.m's part-wise NMS, the 1000 best
  bool matlab_pyramid = false;   // --matlab-pyramid (anywhere): the image pyramid of matlab/detection/featpyramid.m (area resize + reduce, in double)
  int pad = 0;                // --pad N (anywhere): N cells of boundary padding around every pyramid level (0: off)
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--pad") {
      char* end = nullptr;
      const long v = i + 1 < argc ? strtol(argv[i + 1], &end, 10) : -1;
      if (i + 1 >= argc || !*argv[i + 1] || *end || v < 0 || v > 8) { printf("--pad N: 0 (off) .. 8 cells\n"); exit(-1); }
      pad = (int)v;
      for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
      argc -= 2; --i;
    } else
    if (std::string(argv[i]) == "--nms-parts") {
      char* end = nullptr;
      const float v = i + 1 < argc ? strtof(argv[i + 1], &end) : 0.f;
      if (i + 1 >= argc || !*argv[i + 1] || *end || !(v - v == 0.f)) { printf("--nms-parts OVERLAP: a finite number\n"); exit(-1); }
      nms_overlap = v; nms_parts = &nms_overlap;
      for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
      argc -= 2; --i;
    } else
    if (std::string(argv[i]) == "--gtbox") {
      double v[5] = {0, 0, 0, 0, g_gt_overlap};
      int n = 0;
      const char* p = i + 1 < argc ? argv[i + 1] : "";
      while (*p && n < 5) {
        char* end = nullptr;
        v[n] = strtod(p, &end);
        if (end == p || !(v[n] - v[n] == 0.0)) { n = -1; break; }
        ++n;
        p = *end == ',' ? end + 1 : end;
        if (*end && *end != ',') { n = -1; break; }
      }
      if (n < 4 || *p || g_gtbox.size() >= PBD_GT_MAX) { printf("--gtbox x1,y1,x2,y2[,overlap]: finite numbers, at most %d boxes\n", PBD_GT_MAX); exit(-1); }
      g_gtbox.push_back(GtBox{v[0], v[1], v[2], v[3]});
      g_gt_overlap = v[4];
      for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
      argc -= 2; --i;
    } else
    if (std::string(argv[i]) == "--warp") {
      double v[4] = {0, 0, 0, 0};
      int n = 0;
      const char* p = i + 1 < argc ? argv[i + 1] : "";
      while (*p && n < 4) {
        char* end = nullptr;
        v[n] = strtod(p, &end);
        if (end == p || !(v[n] - v[n] == 0.0)) { n = -1; break; }
        ++n;
        p = *end == ',' ? end + 1 : end;
        if (*end && *end != ',') { n = -1; break; }
      }
      if (n < 4 || *p) { printf("--warp x1,y1,x2,y2: finite numbers, 1-based inclusive pixel coordinates\n"); exit(-1); }
      g_warp.push_back(GtBox{v[0], v[1], v[2], v[3]});
      for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
      argc -= 2; --i;
    } else
    if (std::string(argv[i]) == "--mine") {
      if (i + 1 >= argc || !*argv[i + 1]) { printf("--mine FILE\n"); exit(-1); }
      g_mine.push_back(argv[i + 1]);
      for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
      argc -= 2; --i;
    } else
    if (std::string(argv[i]) == "--poslatent") {
      if (i + 2 >= argc || !*argv[i + 1] || !*argv[i + 2]) { printf("--poslatent FILE x,y,w,h[;x,y,w,h...]\n"); exit(-1); }
      PosLatent pl{argv[i + 1], {}};
      const char* p = argv[i + 2];
      bool ok = true;
      while (ok && *p) {
        long v[4] = {0, 0, 0, 0};
        for (int n = 0; n < 4 && ok; ++n) {
          char* end = nullptr;
          v[n] = strtol(p, &end, 10);
          ok = end != p && (n < 3 ? *end == ',' : (*end == ';' || !*end));
          p = *end ? end + 1 : end;
        }
        if (ok) pl.truth.push_back(Rect{(int)v[0], (int)v[1], (int)v[2], (int)v[3]});
      }
      if (!ok || pl.truth.empty()) { printf("--poslatent FILE x,y,w,h[;x,y,w,h...]: one box of integers per part, as detect() returns boxes\n"); exit(-1); }
      g_poslatent.push_back(pl);
      for (int k = i; k + 3 < argc; ++k) argv[k] = argv[k + 3];
      argc -= 3; --i;
    } else
    if (std::string(argv[i]) == "--examples") {
      if (i + 1 >= argc || !*argv[i + 1]) { printf("--examples FILE\n"); exit(-1); }
      g_examples_file = argv[i + 1];
      for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
      argc -= 2; --i;
    } else
    if (std::string(argv[i]) == "--features") {
      if (i + 1 >= argc || !*argv[i + 1]) { printf("--features FILE\n"); exit(-1); }
      features_file = argv[i + 1];
      for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
      argc -= 2; --i;
    } else
    if (std::string(argv[i]) == "--matlab-pyramid") {
      matlab_pyramid = true;
      for (int k = i; k + 1 < argc; ++k) argv[k] = argv[k + 1];
      --argc; --i;
    } else
    if (std::string(argv[i]) == "--train") {
      g_train = true;
      for (int k = i; k + 1 < argc; ++k) argv[k] = argv[k + 1];
      --argc; --i;
    } else
    if (std::string(argv[i]) == "--part-scores") {
      part_scores = true;
      for (int k = i; k + 1 < argc; ++k) argv[k] = argv[k + 1];
      --argc; --i;
    }
  if (argc < 6 || argc > 8) {
    printf("Usage: pbd_demo model_file image.raw width height channels [stagewise|double|stagewise-double] [--part-scores] [--pad N] [--features FILE] [--examples FILE] [--nms-parts OVERLAP] [--matlab-pyramid] [--gtbox x1,y1,x2,y2[,overlap]]... [--warp x1,y1,x2,y2]... [--mine FILE]... [--poslatent FILE x,y,w,h[;x,y,w,h...]]... [--train]\n");
    exit(-1);
  }
  // determine the type of model to read (src/demo.cpp:63-82)
  std::unique_ptr<Model> modelp;
  const std::string mf = argv[1];
  const std::string ext = mf.find('.') == std::string::npos ? "" : mf.substr(mf.rfind('.'));
  if (ext == ".xml" || ext == ".yaml" || ext == ".yml") modelp.reset(new FileStorageModel);
  else if (ext == ".bin") modelp.reset(new BinaryModel);
  else { printf("Unsupported model format: %s\n", ext.c_str()); exit(-2); }
  if (!modelp->deserialize(argv[1])) { printf("Error deserializing file\n"); exit(-3); }
  Model& model = *modelp;
  const int w = atoi(argv[3]), h = atoi(argv[4]), cn = atoi(argv[5]);
  Mat im(h, w, PBD_8U, cn);
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(im.ptr<uint8_t>(), 1, (size_t)w * h * cn, f) != (size_t)w * h * cn) {
    printf("Image not found or invalid image format\n");
    exit(-4);
  }
  fclose(f);
  const std::string mode = argc >= 7 ? argv[6] : "";
  const int special = mode == "perturb-features" ? 1 : mode == "oracle-responses" ? 2 : 0;
  if (special && argc != 8) { printf("%s needs a file argument\n", mode.c_str()); exit(-1); }
  const bool stagewise = special || mode.find("stagewise") != std::string::npos;
  try {
    if (part_scores && stagewise) { printf("--part-scores: the fused detect() only\n"); exit(-1); }
    if (features_file && special) { printf("--features: not with %s\n", mode.c_str()); exit(-1); }
    if (g_examples_file && (special || !g_gtbox.empty())) { printf("--examples: not with %s\n", special ? mode.c_str() : "--gtbox"); exit(-1); }
    if (!g_warp.empty() && (special || stagewise || !g_gtbox.empty() || g_examples_file || features_file || part_scores || nms_parts)) { printf("--warp: on its own (or with double)\n"); exit(-1); }
    if (g_train && (g_poslatent.empty() || special || stagewise || !g_gtbox.empty() || !g_warp.empty() || g_examples_file || features_file || part_scores)) { printf("--train: with --poslatent (the positives) and --mine (the negatives), or with double, --pad, --nms-parts, --matlab-pyramid\n"); exit(-1); }
    if (!g_train && !g_mine.empty() && (special || stagewise || !g_gtbox.empty() || !g_warp.empty() || g_examples_file || features_file || part_scores)) { printf("--mine: on its own (or with double, --pad, --nms-parts, --matlab-pyramid)\n"); exit(-1); }
    if (!g_train && !g_poslatent.empty() && (special || stagewise || !g_gtbox.empty() || !g_warp.empty() || !g_mine.empty() || g_examples_file || features_file || part_scores)) { printf("--poslatent: on its own (or with double, --pad, --nms-parts, --matlab-pyramid)\n"); exit(-1); }
    if (!g_gtbox.empty() && (part_scores || nms_parts || features_file)) { printf("--gtbox: not with --part-scores, --nms-parts or --features\n"); exit(-1); }
    if (mode.find("double") != std::string::npos) run<double>(model, im, stagewise, 0, nullptr, part_scores, pad, features_file, nms_parts, matlab_pyramid);
    else run<float>(model, im, stagewise, special, special ? argv[7] : nullptr, part_scores, pad, features_file, nms_parts, matlab_pyramid);
  } catch (const Exception& e) {
    printf("error %d: %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
