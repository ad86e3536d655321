/* mex.h — OUR OWN stand-in for the MATLAB MEX accessor API, written for this repository.
 *
 * STORAGE AND ACCESSORS ONLY.  An mxArray here is a block of doubles plus its dimensions; the functions below hand
 * out that block, its dimensions and its class, allocate and free.  There is not one arithmetic operation on image
 * or feature data in this file or in ref_features_driver.cpp, and none may be added: every number the compiled
 * reference produces is computed by the reference's own matlab/mex/features.cc, read in place from its checkout.
 * (That is what separates this header from an OpenCV stand-in, where the header IS the arithmetic: DESIGN.md §3.)
 */
#ifndef PBD_REF_FEATURES_MEX_H
#define PBD_REF_FEATURES_MEX_H

#include <stddef.h>

typedef enum { mxUNKNOWN_CLASS = 0, mxDOUBLE_CLASS = 6 } mxClassID;
typedef enum { mxREAL = 0, mxCOMPLEX = 1 } mxComplexity;

typedef struct mxArray_tag {
  double* data;      /* column-major, owned by the array unless `borrowed` */
  int ndims;
  int dims[4];
  mxClassID cls;
  int borrowed;
} mxArray;

void* mxGetPr(const mxArray* a);
const int* mxGetDimensions(const mxArray* a);
int mxGetNumberOfDimensions(const mxArray* a);
mxClassID mxGetClassID(const mxArray* a);
double mxGetScalar(const mxArray* a);
void* mxCalloc(size_t n, size_t size);
void mxFree(void* p);
mxArray* mxCreateNumericArray(int ndims, const int* dims, mxClassID cls, mxComplexity cplx);
void mxDestroyArray(mxArray* a);
void mexErrMsgTxt(const char* msg);   /* does not return: throws, the driver turns it into an error code */

#endif
