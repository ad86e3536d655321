// pbd_augment.cpp — pbd_augment_u8 and pbd_augment_dev_u8 (include/pbd_c.h "virtual positives"): the mirrored and rotated copies of one
// frame on the device.  No handle: the call uploads the ops' descriptors (and, for the host entry, the frame), launches k_augment.hip
// once on a stream of its own, waits, and frees what it allocated; the calling thread's device is restored on every path.
#include <vector>
#include "pbd_internal.hpp"
#include "augment_core.hpp"

namespace {
// rows of row_bytes between two pitches: one flat copy where both are dense (copy_rows' rule)
hipError_t copy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t row_bytes, size_t rows, hipMemcpyKind kind, hipStream_t st) {
  if (dpitch == row_bytes && spitch == row_bytes) return hipMemcpyAsync(dst, src, row_bytes * rows, kind, st);
  return hipMemcpy2DAsync(dst, dpitch, src, spitch, row_bytes, rows, kind, st);
}

#define AUGHIP(x) do { if ((x) != hipSuccess) return aug_fail(PBD_ERR_HIP, "virtual positives: a HIP call failed"); } while (0)

// dev: im and outs[] are device memory, read and written in place; else host memory, staged dense on the device
int augment_run(int device, const uint8_t* im, int w, int hgt, int cn, int stride, const pbd_augment_op* ops, int nops, uint8_t* const* outs,
                const int* out_strides, bool dev) {
  AugDesc desc[AUG_MAX_OPS];
  const int rc = aug_check(im, w, hgt, cn, stride, ops, nops, (const void* const*)outs, out_strides, desc);
  if (rc != PBD_OK) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    (void)hipGetLastError();
    return aug_fail(PBD_ERR_HIP, "virtual positives: no such HIP device");
  }
  DeviceRun run;
  AUGHIP(hipSetDevice(device));
  CLEAR_STICKY();
  AUGHIP(run.open());

  AugArgs a{};
  a.w = w; a.h = hgt; a.cn = cn; a.nops = nops;
  const size_t rowb = (size_t)w * cn;
  if (dev) {
    a.im = im; a.stride = (unsigned long long)stride;
  } else {
    uint8_t* d_im;
    AUGHIP(run.alloc(&d_im, rowb * hgt));
    AUGHIP(copy2d(d_im, rowb, im, (size_t)stride, rowb, (size_t)hgt, hipMemcpyHostToDevice, run.stream));
    a.im = d_im; a.stride = rowb;
  }
  for (int i = 0; i < nops; ++i) {
    AugDesc& d = desc[i];
    a.max_rows = d.rows > a.max_rows ? d.rows : a.max_rows;
    a.max_cols = d.cols > a.max_cols ? d.cols : a.max_cols;
    if (dev) {
      d.out = outs[i]; d.out_stride = (unsigned long long)out_strides[i];
    } else {
      AUGHIP(run.alloc(&d.out, (size_t)d.rows * d.cols * cn));
      d.out_stride = (unsigned long long)d.cols * cn;
    }
  }
  AugDesc* d_desc;
  AUGHIP(run.alloc(&d_desc, (size_t)nops));
  AUGHIP(hipMemcpyAsync(d_desc, desc, sizeof(AugDesc) * (size_t)nops, hipMemcpyHostToDevice, run.stream));
  a.desc = d_desc;
  launch_augment(a, run.stream);
  AUGHIP(hipGetLastError());
  if (!dev)
    for (int i = 0; i < nops; ++i) {
      const AugDesc& d = desc[i];   // (only the canvas row's bytes of an output row are written)
      AUGHIP(copy2d(outs[i], (size_t)out_strides[i], d.out, (size_t)d.out_stride, (size_t)d.cols * cn, (size_t)d.rows, hipMemcpyDeviceToHost, run.stream));
    }
  AUGHIP(hipStreamSynchronize(run.stream));
  return PBD_OK;
}
}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int pbd_augment_u8(int device, const uint8_t* im, int w, int hgt, int cn, int stride, const pbd_augment_op* ops, int nops, uint8_t* const* outs,
                   const int* out_strides) {
  return augment_run(device, im, w, hgt, cn, stride, ops, nops, outs, out_strides, false);
}
int pbd_augment_dev_u8(int device, const void* d_im, int w, int hgt, int cn, int stride, const pbd_augment_op* ops, int nops, void* const* d_outs,
                       const int* out_strides) {
  return augment_run(device, (const uint8_t*)d_im, w, hgt, cn, stride, ops, nops, (uint8_t* const*)d_outs, out_strides, true);
}

}  // extern "C"
#pragma GCC visibility pop
