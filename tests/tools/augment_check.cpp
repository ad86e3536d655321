// augment_check.cpp — pbd::augment, pbd::mapRotatePoints and pbd::flipPoints (partsbaseddetector_amd/host/pbd_host.hpp) for
// tests/test_augment_cpu.py ("host": pbd_augment_host_u8, no GPU) and tests/test_gpu_augment.py ("device": pbd_augment_u8): a
// frame [hgt][w][cn] of bytes from a file -> per op its canvas and an FNV-1a hash of its bytes; the points mapped, mapped back and
// mirrored; then a refusal.  ExampleCache::writeWarped from a pbd::DeviceFrame is instantiated, so that it compiles against the header.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../partsbaseddetector_amd/host/pbd_host.hpp"

typedef pbd::PartsBasedDetector<float>::ExampleCache Cache;

int main(int argc, char** argv) {
  if (argc != 6) { printf("usage: augment_check frame.bin w hgt cn host|device\n"); return 2; }
  const int w = atoi(argv[2]), hgt = atoi(argv[3]), cn = atoi(argv[4]);
  const bool host = argv[5][0] == 'h';
  pbd::Mat im(hgt, w, pbd::PBD_8U, cn);
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(im.ptr<uint8_t>(), 1, im.bytes(), f) != im.bytes()) { printf("frame?\n"); return 3; }
  fclose(f);
  std::vector<pbd_augment_op> ops(4);
  ops[0] = pbd_augment_op{1, PBD_ROT_NEAREST, 0.0, 0, 0};
  ops[1] = pbd_augment_op{0, PBD_ROT_BILINEAR, 15.0, 1, 0};
  ops[2] = pbd_augment_op{1, PBD_ROT_NEAREST, -7.5, 1, 0};
  ops[3] = pbd_augment_op{0, PBD_ROT_BILINEAR, 90.0, 1, 0};
  try {
    const std::vector<pbd::Mat> out = pbd::augment(im, ops, 0, host);
    for (size_t i = 0; i < out.size(); ++i) {
      unsigned long long hsh = 1469598103934665603ull;
      for (size_t b = 0; b < out[i].bytes(); ++b) hsh = (hsh ^ out[i].ptr<uint8_t>()[b]) * 1099511628211ull;
      printf("op%zu %d %d %llu\n", i, out[i].rows, out[i].cols, hsh);
    }
    const std::vector<double> pts = {3.0, 4.0, 20.5, 11.25};
    const std::vector<double> fwd = pbd::mapRotatePoints(pts, w, hgt, 15.0), back = pbd::mapRotatePoints(fwd, w, hgt, 15.0, PBD_ROT_NEW2ORI);
    const std::vector<double> mir = pbd::flipPoints(pts, w, std::vector<int32_t>{1, 0});
    printf("fwd %a %a %a %a\nback %a %a %a %a\nmir %a %a %a %a\n", fwd[0], fwd[1], fwd[2], fwd[3], back[0], back[1], back[2], back[3], mir[0], mir[1], mir[2], mir[3]);
  } catch (const pbd::Exception& e) { printf("error %d %s\n", e.code, e.what()); return 1; }
  try {
    ops[1].method = 7;
    pbd::augment(im, ops, 0, host);
    printf("refused 0\n");
  } catch (const pbd::Exception& e) { printf("refused %d %s\n", e.code, e.what()); }
  int (Cache::*from_device)(const pbd::DeviceFrame&, const std::vector<pbd::GtBox>&, int, int, double, std::vector<int32_t>*, const std::vector<int32_t>*) =
      &Cache::writeWarped;
  printf("writeWarped_dev %d\n", from_device != nullptr);
  return 0;
}
