/* ref_features_driver.cpp — the storage behind mex.h and one extern "C" entry point that calls process() of the
 * reference's matlab/mex/features.cc (compiled as its own translation unit, in place from the checkout).
 * Like mex.h this file moves memory and nothing else: no arithmetic on pixels or features. */
#include <stdexcept>
#include <stdlib.h>
#include <string.h>
#include "mex.h"

void* mxGetPr(const mxArray* a) { return a->data; }
const int* mxGetDimensions(const mxArray* a) { return a->dims; }
int mxGetNumberOfDimensions(const mxArray* a) { return a->ndims; }
mxClassID mxGetClassID(const mxArray* a) { return a->cls; }
double mxGetScalar(const mxArray* a) { return a->data[0]; }
void* mxCalloc(size_t n, size_t size) { return calloc(n ? n : 1, size ? size : 1); }
void mxFree(void* p) { free(p); }
void mexErrMsgTxt(const char* msg) { throw std::runtime_error(msg); }

mxArray* mxCreateNumericArray(int ndims, const int* dims, mxClassID cls, mxComplexity) {
  mxArray* a = (mxArray*)calloc(1, sizeof(mxArray));
  size_t n = 1;
  a->ndims = ndims;
  for (int i = 0; i < ndims && i < 4; ++i) { a->dims[i] = dims[i]; n *= (size_t)dims[i]; }
  a->cls = cls;
  a->data = (double*)calloc(n ? n : 1, sizeof(double));
  return a;
}

void mxDestroyArray(mxArray* a) {
  if (!a) return;
  if (!a->borrowed) free(a->data);
  free(a);
}

mxArray* process(const mxArray* mximage, const mxArray* mxsbin);   /* matlab/mex/features.cc */

/* planar_colmajor: rows x cols x 3 doubles, MATLAB layout (element (y, x, c) at y + rows * (x + cols * c)).
 * out: orows x ocols x 32 doubles in the same layout, exactly as process() left them; out == NULL only reports the size.
 * returns 0, or -1 where features.cc refused its input. */
extern "C" __attribute__((visibility("default")))
int ref_features(const double* planar_colmajor, int rows, int cols, int sbin, double* out, int* orows, int* ocols) {
  mxArray image, bin;
  double sb = sbin;
  memset(&image, 0, sizeof image);
  memset(&bin, 0, sizeof bin);
  image.data = (double*)planar_colmajor; image.ndims = 3; image.cls = mxDOUBLE_CLASS; image.borrowed = 1;
  image.dims[0] = rows; image.dims[1] = cols; image.dims[2] = 3;
  bin.data = &sb; bin.ndims = 2; bin.dims[0] = 1; bin.dims[1] = 1; bin.cls = mxDOUBLE_CLASS; bin.borrowed = 1;
  mxArray* feat = NULL;
  try {
    feat = process(&image, &bin);
  } catch (const std::exception&) {
    return -1;
  }
  const int* d = mxGetDimensions(feat);
  *orows = d[0];
  *ocols = d[1];
  if (out) memcpy(out, feat->data, sizeof(double) * (size_t)d[0] * (size_t)d[1] * (size_t)d[2]);
  mxDestroyArray(feat);
  return 0;
}
