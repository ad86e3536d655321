/* ref_matpyr_driver.cpp — the storage behind oracle/ref_features/mex.h and one extern "C" entry point that calls resize() of the
 * reference's matlab/mex/resize.cc (-DREF_RESIZE) or reduce() of matlab/mex/reduce.cc (-DREF_REDUCE), each compiled as its own
 * translation unit, in place from the checkout (tests/golden/make_ref_matpyr.py).  This file moves memory and nothing else: no
 * arithmetic on pixels. */
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

#ifdef REF_RESIZE
mxArray* resize(const mxArray* mxsrc, const mxArray* mxscale);   /* matlab/mex/resize.cc */
#else
mxArray* reduce(const mxArray* mxsrc);                           /* matlab/mex/reduce.cc */
#endif

/* planar_colmajor: rows x cols x chan doubles, MATLAB layout (element (y, x, c) at y + rows * (x + cols * c)); scale: resize only.
 * out: orows x ocols x chan doubles in the same layout, exactly as the reference left them; out == NULL only reports the size.
 * returns 0, or -1 where the reference refused its input. */
extern "C" __attribute__((visibility("default")))
int ref_matpyr(const double* planar_colmajor, int rows, int cols, int chan, double scale, double* out, int* orows, int* ocols) {
  mxArray image, sc;
  memset(&image, 0, sizeof image);
  memset(&sc, 0, sizeof sc);
  image.data = (double*)planar_colmajor; image.ndims = 3; image.cls = mxDOUBLE_CLASS; image.borrowed = 1;
  image.dims[0] = rows; image.dims[1] = cols; image.dims[2] = chan;
  sc.data = &scale; sc.ndims = 2; sc.dims[0] = 1; sc.dims[1] = 1; sc.cls = mxDOUBLE_CLASS; sc.borrowed = 1;
  mxArray* res = NULL;
  try {
#ifdef REF_RESIZE
    res = resize(&image, &sc);
#else
    res = reduce(&image);
#endif
  } catch (const std::exception&) {
    return -1;
  }
  const int* d = mxGetDimensions(res);
  *orows = d[0];
  *ocols = d[1];
  if (out) memcpy(out, res->data, sizeof(double) * (size_t)d[0] * (size_t)d[1] * (size_t)d[2]);
  mxDestroyArray(res);
  return 0;
}
