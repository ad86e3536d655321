/* mex.h — a stand-in for the MATLAB MEX accessor API, written for tests/golden/ref_qp_one_driver.cpp: what
 * matlab/mex/qp_one_sparse.cc of the reference uses.  STORAGE AND ACCESSORS ONLY: an mxArray is a borrowed or owned block of memory
 * with its two dimensions and its class.  No arithmetic on examples, weights or multipliers happens here or in the driver: every
 * number the compiled reference file produces is computed by its own text, read in place from the reference checkout. */
#ifndef PBD_REF_QP_ONE_MEX_H
#define PBD_REF_QP_ONE_MEX_H

#include <stddef.h>

typedef enum { mxLOGICAL_CLASS = 3, mxDOUBLE_CLASS = 6, mxSINGLE_CLASS = 7, mxINT32_CLASS = 12, mxUINT32_CLASS = 13 } mxClassID;

typedef struct mxArray_tag {
  void* data;        /* column-major */
  size_t m, n;
  mxClassID cls;
  int borrowed;
} mxArray;

void* mxGetPr(const mxArray* a);
double mxGetScalar(const mxArray* a);   /* the first element of a double array */
size_t mxGetM(const mxArray* a);
size_t mxGetN(const mxArray* a);
bool mxIsDouble(const mxArray* a);
bool mxIsSingle(const mxArray* a);
bool mxIsInt32(const mxArray* a);
bool mxIsUint32(const mxArray* a);
bool mxIsLogical(const mxArray* a);
void* mxCalloc(size_t n, size_t size);  /* zero-filled, as MATLAB's */
void mxFree(void* p);
mxArray* mxCreateDoubleScalar(double v);
void mxDestroyArray(mxArray* a);
void mexErrMsgTxt(const char* msg);     /* does not return: throws, the driver turns it into an error code */

#endif
