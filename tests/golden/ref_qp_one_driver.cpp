/* ref_qp_one_driver.cpp — the storage behind tests/golden/ref_qp_one_shim/mex.h and one extern "C" entry point that calls mexFunction
 * of the reference's matlab/mex/qp_one_sparse.cc, compiled as its own translation unit in place from the checkout
 * (tests/golden/make_ref_qp_one.py).  This file moves memory and nothing else: no arithmetic on examples, weights or multipliers. */
#include <stdexcept>
#include <stdlib.h>
#include <string.h>
#include "mex.h"

void* mxGetPr(const mxArray* a) { return a->data; }
double mxGetScalar(const mxArray* a) { return *(const double*)a->data; }
size_t mxGetM(const mxArray* a) { return a->m; }
size_t mxGetN(const mxArray* a) { return a->n; }
bool mxIsDouble(const mxArray* a) { return a->cls == mxDOUBLE_CLASS; }
bool mxIsSingle(const mxArray* a) { return a->cls == mxSINGLE_CLASS; }
bool mxIsInt32(const mxArray* a) { return a->cls == mxINT32_CLASS; }
bool mxIsUint32(const mxArray* a) { return a->cls == mxUINT32_CLASS; }
bool mxIsLogical(const mxArray* a) { return a->cls == mxLOGICAL_CLASS; }
void* mxCalloc(size_t n, size_t size) { return calloc(n ? n : 1, size ? size : 1); }
void mxFree(void* p) { free(p); }
void mexErrMsgTxt(const char* msg) { throw std::runtime_error(msg); }

mxArray* mxCreateDoubleScalar(double v) {
  mxArray* a = (mxArray*)calloc(1, sizeof(mxArray));
  a->m = a->n = 1; a->cls = mxDOUBLE_CLASS;
  a->data = calloc(1, sizeof(double));
  memcpy(a->data, &v, sizeof v);
  return a;
}

void mxDestroyArray(mxArray* a) {
  if (!a) return;
  if (!a->borrowed) free(a->data);
  free(a);
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]);   /* qp_one_sparse.cc */

static mxArray borrow(const void* p, size_t m, size_t n, mxClassID cls) {
  mxArray a;
  memset(&a, 0, sizeof a);
  a.data = (void*)p; a.m = m; a.n = n; a.cls = cls; a.borrowed = 1;
  return a;
}

/* loss = qp_one_sparse(qp.x, qp.i, qp.b, qp.d, qp.a, qp.w, qp.noneg, qp.sv, qp.l, C, I): x k x ncols float32 columns, ids 5 x ncols
 * int32, b / d / a [ncols], w [len], noneg p 1-based uint32, sv [ncols] bool, l [1], order n 1-based doubles; a, w, sv and l are
 * updated in place, as the file does.  Returns 0, or -1 where the reference refused its input. */
extern "C" __attribute__((visibility("default")))
int ref_qp_one(const float* x, int k, int ncols, const int* ids, const float* b, const double* d, double* a, double* w, int len,
               const unsigned* noneg, int p, bool* sv, double* l, double C, const double* order, int n, double* loss) {
  mxArray X = borrow(x, (size_t)k, (size_t)ncols, mxSINGLE_CLASS), ID = borrow(ids, 5, (size_t)ncols, mxINT32_CLASS);
  mxArray B = borrow(b, (size_t)ncols, 1, mxSINGLE_CLASS), D = borrow(d, (size_t)ncols, 1, mxDOUBLE_CLASS);
  mxArray A = borrow(a, (size_t)ncols, 1, mxDOUBLE_CLASS), W = borrow(w, (size_t)len, 1, mxDOUBLE_CLASS);
  mxArray NN = borrow(noneg, (size_t)p, 1, mxUINT32_CLASS), SV = borrow(sv, (size_t)ncols, 1, mxLOGICAL_CLASS);
  mxArray L = borrow(l, 1, 1, mxDOUBLE_CLASS), CC = borrow(&C, 1, 1, mxDOUBLE_CLASS), I = borrow(order, (size_t)n, 1, mxDOUBLE_CLASS);
  mxArray* res[1] = {NULL};
  const mxArray* in[11] = {&X, &ID, &B, &D, &A, &W, &NN, &SV, &L, &CC, &I};
  try {
    mexFunction(1, res, 11, in);
    memcpy(loss, res[0]->data, sizeof(double));
  } catch (const std::exception&) {
    return -1;
  }
  mxDestroyArray(res[0]);
  return 0;
}
