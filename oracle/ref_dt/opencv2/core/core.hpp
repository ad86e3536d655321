/* opencv2/core/core.hpp — OUR stand-in for the part of OpenCV that the reference's include/DistanceTransform.hpp touches:
 * cv::Size, cv::Point, cv::Mat_<T> as row-major storage (rows, cols, create, operator[]) and cv::transpose.
 * STORAGE ONLY: elements are allocated, indexed and moved, never computed with — not one arithmetic operation on T.
 * Every floating-point operation of the distance transform is executed from the reference's own text (Quadratic, computeRow).
 * See README.md beside this directory for why this stand-in is admissible. */
#ifndef PBD_REF_DT_OPENCV_CORE_STANDIN_HPP_
#define PBD_REF_DT_OPENCV_CORE_STANDIN_HPP_
#include <cstddef>
#include <vector>

namespace cv {

struct Size {
  int width, height;
  Size() : width(0), height(0) {}
  Size(int w, int h) : width(w), height(h) {}          /* cv::Size(cols, rows) */
};

struct Point {
  int x, y;
  Point() : x(0), y(0) {}
  Point(int x_, int y_) : x(x_), y(y_) {}
};

template <typename T>
class Mat_ {
 public:
  int rows, cols;
  Mat_() : rows(0), cols(0) {}
  explicit Mat_(Size s) : rows(0), cols(0) { create(s); }
  void create(Size s) {
    rows = s.height;
    cols = s.width;
    data_.assign((size_t)rows * (size_t)cols, T());
  }
  T* operator[](int r) { return data_.data() + (size_t)r * (size_t)cols; }
  const T* operator[](int r) const { return data_.data() + (size_t)r * (size_t)cols; }

 private:
  std::vector<T> data_;
};

/* dst = src^T; dst may be src itself (the header calls transpose(x, x)) */
template <typename T>
void transpose(const Mat_<T>& src, Mat_<T>& dst) {
  Mat_<T> t(Size(src.rows, src.cols));
  for (int r = 0; r < src.rows; ++r)
    for (int c = 0; c < src.cols; ++c) t[c][r] = src[r][c];
  dst = t;
}

}  // namespace cv
#endif
