// qp_fold.hpp — the example cache's block sum (include/pbd_c.h "training example cache"), shared by k_qp.hip and k_qp_solve.hip.
#pragma once
#include <hip/hip_runtime.h>

// the header's block sum: lane t holds partial t; folded s[t] += s[t + h], h = 32 .. 1; lane 0 has the sum
__device__ __forceinline__ double qp_fold(double v) {
#pragma unroll
  for (int h = 32; h >= 1; h >>= 1) v = __dadd_rn(v, __shfl_down(v, h, 64));
  return v;
}
