// pyrstore_check.cpp — the pyramid store's host-only layout (pbd_pyrstore_layout, pbd_plan.cpp) in a program of its own, built with
// AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_pyrstore_cpu.py: every combination of the grid below is laid out into a
// heap level_off array of exactly the documented size (a write past either end is the sanitizer's to report), refused frames leave the
// outputs alone, and the offsets are the prefix sums of the levels' cells.  Prints one line per case: "w h sbin interval kind pad rc nlevels total".
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pbd_plan.hpp"

int main() {
  const int sizes[][2] = {{64, 48}, {97, 75}, {640, 480}, {30, 30}, {3, 3}, {2, 2}, {4096, 16}};
  int failures = 0;
  for (const auto& wh : sizes)
    for (int sbin : {4, 8})
      for (int interval : {2, 10})
        for (int kind : {PBD_PYRAMID_OPENCV, PBD_PYRAMID_MATLAB})
          for (int pad : {0, 2}) {
            // exactly PBD_PYRSTORE_MAX_LEVELS entries on the heap: a write past either end is the sanitizer's to report
            std::vector<long long> off((size_t)PBD_PYRSTORE_MAX_LEVELS, -7);
            int n = -7;
            long long total = -7;
            const int rc = pbd_pyrstore_layout(wh[0], wh[1], sbin, interval, kind, pad, &n, off.data(), &total);
            std::printf("%d %d %d %d %d %d %d %d %lld\n", wh[0], wh[1], sbin, interval, kind, pad, rc, n, total);
            if (rc != PBD_OK) {
              if (rc != PBD_ERR_ARG || n != -7 || total != -7 || off[0] != -7) { std::printf("FAIL: a refusal wrote its outputs\n"); ++failures; }
              continue;
            }
            if (n < interval || n > PBD_PYRSTORE_MAX_LEVELS || off[0] != 0) { std::printf("FAIL: level count / first offset\n"); ++failures; continue; }
            std::vector<Level> lv((size_t)PBD_MAX_LEVELS, Level{});
            int n2 = 0;
            const int g = kind == PBD_PYRAMID_MATLAB ? compute_geometry_matlab(wh[0], wh[1], sbin, interval, &n2, lv.data())
                                                     : compute_geometry(wh[0], wh[1], sbin, interval, &n2, lv.data());
            pad_geometry(pad, n2, lv.data());
            long long sum = 0;
            bool ok = g == 0 && n2 == n;
            for (int l = 0; ok && l < n; ++l) {
              ok = off[l] == sum;
              sum += (long long)lv[l].cw * lv[l].ch * PBD_FLEN;
            }
            if (!ok || sum != total) { std::printf("FAIL: offsets are not the prefix sums of cw * ch * 32\n"); ++failures; }
            for (int l = n; l < PBD_PYRSTORE_MAX_LEVELS; ++l)
              if (off[l] != -7) { std::printf("FAIL: an entry beyond the levels was written\n"); ++failures; break; }
          }
  // NULL outputs and arguments outside the setters' ranges are refused, level_off may be NULL
  int n = 0;
  long long total = 0;
  if (pbd_pyrstore_layout(64, 48, 4, 2, 0, 0, nullptr, nullptr, &total) != PBD_ERR_ARG || pbd_pyrstore_layout(64, 48, 4, 2, 0, 0, &n, nullptr, nullptr) != PBD_ERR_ARG ||
      pbd_pyrstore_layout(64, 48, 0, 2, 0, 0, &n, nullptr, &total) != PBD_ERR_ARG || pbd_pyrstore_layout(64, 48, 4, 17, 0, 0, &n, nullptr, &total) != PBD_ERR_ARG ||
      pbd_pyrstore_layout(64, 48, 4, 2, 2, 0, &n, nullptr, &total) != PBD_ERR_ARG || pbd_pyrstore_layout(64, 48, 4, 2, 0, 9, &n, nullptr, &total) != PBD_ERR_ARG ||
      pbd_pyrstore_layout(64, 48, 4, 2, 0, 0, &n, nullptr, &total) != PBD_OK || n < 2 || total <= 0) {
    std::printf("FAIL: argument checks\n");
    ++failures;
  }
  std::printf("%s\n", failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
