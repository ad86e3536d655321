// eval_host_check.cpp — pbd::PartsBasedDetector<float>::Evaluation (partsbaseddetector_amd/host/pbd_host.hpp) on one frame, for
// tests/test_gpu_eval.py: model.bin image.raw width height channels persons.bin, where persons.bin holds int32 ngt, int32 P, then
// points[ngt][P][2] and scale[ngt] as doubles.  The frame is added through addPck and addApk (RAW records); prints the found flags, the
// record count, the ledger's dims and pck / apk as hexadecimal floats: one value per token, nothing rounds on the way out.
#include <cstdio>
#include <cstdlib>
#include "../../partsbaseddetector_amd/host/pbd_host.hpp"

using namespace pbd;

int main(int argc, char** argv) {
  if (argc != 7) { printf("usage: eval_host_check model.bin image.raw width height channels persons.bin\n"); return 2; }
  BinaryModel model;
  if (!model.deserialize(argv[1])) { printf("model?\n"); return 3; }
  const int w = atoi(argv[3]), h = atoi(argv[4]), cn = atoi(argv[5]);
  Mat im(h, w, PBD_8U, cn);
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(im.ptr<uint8_t>(), 1, (size_t)w * h * cn, f) != (size_t)w * h * cn) { printf("image?\n"); return 4; }
  fclose(f);
  int32_t hd[2] = {0, 0};
  f = fopen(argv[6], "rb");
  if (!f || fread(hd, sizeof(int32_t), 2, f) != 2) { printf("persons?\n"); return 5; }
  std::vector<double> points((size_t)hd[0] * hd[1] * 2), scale((size_t)hd[0]);
  if (fread(points.data(), sizeof(double), points.size(), f) != points.size() || fread(scale.data(), sizeof(double), scale.size(), f) != scale.size()) {
    printf("persons?\n");
    return 5;
  }
  fclose(f);
  try {
    PartsBasedDetector<float> det(0, PBD_CONV_EXACT, 8192);
    det.distributeModel(model);
    auto ev = det.evaluation(hd[1], 64, 8192);
    const std::vector<int> found = ev->addPck(im, points, scale, 0.3);
    const int records = ev->addApk(im, points, scale);
    const auto d = ev->dims();
    printf("found");
    for (int v : found) printf(" %d", v);
    printf("\nrecords %d\ndims %d %d %d %lld %d\n", records, d.nparts, d.instances, d.detections, d.npos, d.frames);
    for (int rule : {PBD_EVAL_SCALE_LAST, PBD_EVAL_SCALE_OWN}) {
      printf("pck%d", rule);
      for (double v : ev->pck(.5, rule)) printf(" %a", v);
      printf("\n");
    }
    std::vector<double> prec, rec;
    printf("apk");
    for (double v : ev->apk(&prec, &rec)) printf(" %a", v);
    printf("\nprec0 %a rec_last %a\n", prec.empty() ? 0.0 : prec[0], rec.empty() ? 0.0 : rec.back());
  } catch (const Exception& e) {
    printf("error %d: %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
