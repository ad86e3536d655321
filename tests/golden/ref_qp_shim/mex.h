/* mex.h — a stand-in for the MATLAB MEX accessor API, written for tests/golden/ref_qp_driver.cpp: what matlab/mex/score.cc and
 * matlab/mex/lincomb.cc of the reference use.  STORAGE AND ACCESSORS ONLY: an mxArray is a borrowed or owned block of memory with its
 * two dimensions and its class.  No arithmetic on example or weight data happens here or in the driver: every number the compiled
 * reference files produce is computed by their own text, read in place from the reference checkout. */
#ifndef PBD_REF_QP_MEX_H
#define PBD_REF_QP_MEX_H

#include <stddef.h>

typedef enum { mxDOUBLE_CLASS = 6, mxSINGLE_CLASS = 7 } mxClassID;
typedef enum { mxREAL = 0, mxCOMPLEX = 1 } mxComplexity;

typedef struct mxArray_tag {
  void* data;        /* column-major */
  size_t m, n;
  mxClassID cls;
  int borrowed;
} mxArray;

void* mxGetPr(const mxArray* a);
size_t mxGetM(const mxArray* a);
size_t mxGetN(const mxArray* a);
size_t mxGetNumberOfElements(const mxArray* a);
bool mxIsDouble(const mxArray* a);
bool mxIsSingle(const mxArray* a);
mxArray* mxCreateDoubleMatrix(size_t m, size_t n, mxComplexity cplx);   /* zero-filled, as MATLAB's */
void mxDestroyArray(mxArray* a);
void mexErrMsgTxt(const char* msg);   /* does not return: throws, the driver turns it into an error code */

#endif
