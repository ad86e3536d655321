/* ref_qp_driver.cpp — the storage behind tests/golden/ref_qp_shim/mex.h and one extern "C" entry point that calls mexFunction of the
 * reference's matlab/mex/score.cc (-DREF_SCORE) or matlab/mex/lincomb.cc (-DREF_LINCOMB), each compiled as its own translation unit,
 * in place from the checkout (tests/golden/make_ref_qp.py).  This file moves memory and nothing else: no arithmetic on examples,
 * weights or multipliers. */
#include <stdexcept>
#include <stdlib.h>
#include <string.h>
#include "mex.h"

void* mxGetPr(const mxArray* a) { return a->data; }
size_t mxGetM(const mxArray* a) { return a->m; }
size_t mxGetN(const mxArray* a) { return a->n; }
size_t mxGetNumberOfElements(const mxArray* a) { return a->m * a->n; }
bool mxIsDouble(const mxArray* a) { return a->cls == mxDOUBLE_CLASS; }
bool mxIsSingle(const mxArray* a) { return a->cls == mxSINGLE_CLASS; }
void mexErrMsgTxt(const char* msg) { throw std::runtime_error(msg); }

mxArray* mxCreateDoubleMatrix(size_t m, size_t n, mxComplexity) {
  mxArray* a = (mxArray*)calloc(1, sizeof(mxArray));
  a->m = m; a->n = n; a->cls = mxDOUBLE_CLASS;
  a->data = calloc(m * n ? m * n : 1, sizeof(double));
  return a;
}

void mxDestroyArray(mxArray* a) {
  if (!a) return;
  if (!a->borrowed) free(a->data);
  free(a);
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]);   /* score.cc / lincomb.cc */

static mxArray borrow(const void* p, size_t m, size_t n, mxClassID cls) {
  mxArray a;
  memset(&a, 0, sizeof a);
  a.data = (void*)p; a.m = m; a.n = n; a.cls = cls; a.borrowed = 1;
  return a;
}

/* x: k x ncols float32 columns (qp.x); inds: n 1-based column indices as doubles, as MATLAB passes them.
 * REF_SCORE:   score(w, qp.x, inds)       v = w [vlen], out [n]
 * REF_LINCOMB: lincomb(qp.x, a, inds, m)  v = a [ncols], out [vlen], m = vlen
 * returns 0, or -1 where the reference refused its input. */
extern "C" __attribute__((visibility("default")))
int ref_qp(const float* x, int k, int ncols, const double* v, int vlen, const double* inds, int n, double* out) {
  mxArray X = borrow(x, (size_t)k, (size_t)ncols, mxSINGLE_CLASS);
  mxArray I = borrow(inds, (size_t)n, 1, mxDOUBLE_CLASS);
  mxArray* res[1] = {NULL};
  try {
#ifdef REF_SCORE
    mxArray W = borrow(v, (size_t)vlen, 1, mxDOUBLE_CLASS);
    const mxArray* in[3] = {&W, &X, &I};
    mexFunction(1, res, 3, in);
    memcpy(out, res[0]->data, sizeof(double) * (size_t)n);
#else
    double m = (double)vlen;
    mxArray A = borrow(v, (size_t)ncols, 1, mxDOUBLE_CLASS);
    mxArray M = borrow(&m, 1, 1, mxDOUBLE_CLASS);
    const mxArray* in[4] = {&X, &A, &I, &M};
    mexFunction(1, res, 4, in);
    memcpy(out, res[0]->data, sizeof(double) * (size_t)vlen);
#endif
  } catch (const std::exception&) {
    return -1;
  }
  mxDestroyArray(res[0]);
  return 0;
}
