/* ref_dt_driver.cpp — two extern "C" entry points that run the reference's DistanceTransform<T>::compute
 * (include/DistanceTransform.hpp, compiled in place from the checkout) with Quadratic penalties, on storage from our
 * opencv2/core/core.hpp.  Like that header this file moves memory and nothing else: no arithmetic on scores. */
#include <stdint.h>
#include <string.h>
#include "DistanceTransform.hpp"

/* in: M x N row-major.  out / ix / iy: M x N row-major, exactly as compute() left score_out / Ix / Iy. */
template <typename T>
static void run(const T* in, int M, int N, double ax, double bx, double ay, double by, int osx, int osy, T* out, int32_t* ix, int32_t* iy) {
  cv::Mat_<T> score_in(cv::Size(N, M)), score_out;
  cv::Mat_<int> Ix, Iy;
  for (int m = 0; m < M; ++m) memcpy(score_in[m], in + (size_t)m * N, sizeof(T) * (size_t)N);
  const Quadratic fx(ax, bx), fy(ay, by);
  DistanceTransform<T>().compute(score_in, fx, fy, cv::Point(osx, osy), score_out, Ix, Iy);
  for (int m = 0; m < M; ++m) {
    memcpy(out + (size_t)m * N, score_out[m], sizeof(T) * (size_t)N);
    for (int n = 0; n < N; ++n) { ix[(size_t)m * N + n] = Ix[m][n]; iy[(size_t)m * N + n] = Iy[m][n]; }
  }
}

extern "C" __attribute__((visibility("default")))
void ref_dt2d(const float* in, int M, int N, double ax, double bx, double ay, double by, int osx, int osy, float* out, int32_t* ix, int32_t* iy) {
  run<float>(in, M, N, ax, bx, ay, by, osx, osy, out, ix, iy);
}
extern "C" __attribute__((visibility("default")))
void ref_dt2d_f64(const double* in, int M, int N, double ax, double bx, double ay, double by, int osx, int osy, double* out, int32_t* ix, int32_t* iy) {
  run<double>(in, M, N, ax, bx, ay, by, osx, osy, out, ix, iy);
}
