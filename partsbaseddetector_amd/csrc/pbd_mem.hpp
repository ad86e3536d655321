// pbd_mem.hpp — who owns device memory (DESIGN.md "who owns device memory").  The only file of the library that allocates or frees
// device or pinned host memory:
//   DevBufs      a list of allocations, freed together: a member holds an object's buffers, a local a call's temporaries
//   CallScratch  the temporaries of one call on a handle's stream, with the first HIP error latched
//   DeviceRun    the temporaries of a handle-less call: its own device switch and stream
// Every allocation and free moves two process-wide counters (pbd_debug_live_allocs): a call gives back what it took.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <string>
#include <vector>
#include "../../include/pbd_c.h"

inline std::atomic<long long> pbd_live_buffers{0}, pbd_live_bytes{0};   // everything a DevBufs holds, counted or not
// the text of a failed allocation: "<what>hipMalloc: <hip string>"
inline std::string pbd_alloc_error(const char* what, hipError_t e, bool pinned = false) {
  return std::string(what) + (pinned ? "hipHostMalloc: " : "hipMalloc: ") + hipGetErrorString(e);
}

class DevBufs {
  struct Buf { void* p; size_t bytes; bool pinned, counted; };
  std::vector<Buf> bufs_;
  size_t counted_ = 0;
  static void free_buf(const Buf& b) {
    if (b.pinned) hipHostFree(b.p); else hipFree(b.p);
    --pbd_live_buffers; pbd_live_bytes -= (long long)b.bytes;
  }
 public:
  DevBufs() = default;
  DevBufs(const DevBufs&) = delete;
  DevBufs& operator=(const DevBufs&) = delete;
  ~DevBufs() { clear(); }
  // max(n, 1) elements of T, device or pinned host; counted = false: held and freed like the others, left out of bytes()
  template <class T> hipError_t alloc(T** p, size_t n, bool pinned = false, bool counted = true) {
    const size_t bytes = sizeof(T) * (n > 1 ? n : 1);
    void* q = nullptr;
    const hipError_t e = pinned ? hipHostMalloc(&q, bytes) : hipMalloc(&q, bytes);
    if (e != hipSuccess) return e;
    bufs_.push_back({q, bytes, pinned, counted});
    if (counted) counted_ += bytes;
    ++pbd_live_buffers; pbd_live_bytes += (long long)bytes;
    *p = (T*)q;
    return hipSuccess;
  }
  void release(void* p) {   // one buffer, early (not one of this list's: nothing happens)
    for (auto b = bufs_.begin(); b != bufs_.end(); ++b)
      if (b->p == p) { if (b->counted) counted_ -= b->bytes; free_buf(*b); bufs_.erase(b); return; }
  }
  void clear() {
    for (const Buf& b : bufs_) free_buf(b);
    bufs_.clear(); counted_ = 0;
  }
  size_t bytes() const { return counted_; }   // counted allocations only
  bool empty() const { return bufs_.empty(); }
};

// ---- the scratch of one call on a handle's stream -----------------------------------------------------------------------------
// Bound to the handle's stream and error string.  The first HIP error is kept and every later step is skipped; copies run on the
// stream; finish() synchronises it once and reports the error under the caller's prefix.  Buffers go when it goes out of scope, behind
// a synchronisation of the stream: on an error path work that reads them may still be in flight (success paths have synchronised
// already, and an idle stream costs nothing).
struct CallScratch {
  hipStream_t stream;
  std::string& err;
  hipError_t e = hipSuccess;
  DevBufs bufs;
  template <class H> explicit CallScratch(H* h) : stream(h->stream), err(h->err) {}
  ~CallScratch() { if (!bufs.empty()) hipStreamSynchronize(stream); }
  bool ok() const { return e == hipSuccess; }
  void chk(hipError_t r) { if (e == hipSuccess) e = r; }
  template <typename T> T* alloc(size_t n, bool pinned) {   // n = 0: no buffer (nullptr)
    T* p = nullptr;
    if (ok() && n) chk(bufs.alloc(&p, n, pinned));
    return p;
  }
  template <typename T> T* dev(size_t n) { return alloc<T>(n, false); }
  // callers in the return-code style: max(n, 1) elements now, a failure reported at once under the caller's prefix
  template <typename T> int get(T** p, size_t n, const char* what) {
    const hipError_t r = bufs.alloc(p, n);
    if (r == hipSuccess) return PBD_OK;
    err = pbd_alloc_error(what, r);
    return PBD_ERR_HIP;
  }
  void up(void* d, const void* s, size_t bytes) { if (ok() && bytes) chk(hipMemcpyAsync(d, s, bytes, hipMemcpyHostToDevice, stream)); }
  void up2d(void* d, size_t dpitch, const void* s, size_t spitch, size_t row, size_t rows) {
    if (ok() && row && rows) chk(hipMemcpy2DAsync(d, dpitch, s, spitch, row, rows, hipMemcpyHostToDevice, stream));
  }
  void down(void* d, const void* s, size_t bytes) { if (ok() && bytes) chk(hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToHost, stream)); }
  void zero(void* d, size_t bytes) { if (ok()) chk(hipMemsetAsync(d, 0, bytes, stream)); }
  void launched() { if (ok()) chk(hipGetLastError()); }
  int status(const char* what) {   // the latched error under the caller's prefix, without waiting
    if (ok()) return PBD_OK;
    err = std::string(what) + hipGetErrorString(e);
    return PBD_ERR_HIP;
  }
  int finish(const char* what) {
    chk(hipStreamSynchronize(stream));
    return status(what);
  }
};

// ---- the scratch of one handle-less call --------------------------------------------------------------------------------------
// The calling thread's device is remembered and restored; the call's work runs on a stream of its own (hipSetDevice(device) is the
// caller's first step: the stream and the buffers then belong to that device).  On every path out the stream is drained before
// anything is freed: work that reads the buffers may still be in flight after an error.
struct DeviceRun {
  int prev = -1;
  hipStream_t stream = nullptr;
  DevBufs bufs;
  DeviceRun() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
  DeviceRun(const DeviceRun&) = delete;
  DeviceRun& operator=(const DeviceRun&) = delete;
  hipError_t open() { return hipStreamCreateWithFlags(&stream, hipStreamNonBlocking); }
  template <typename T> hipError_t alloc(T** p, size_t n) { return bufs.alloc(p, n); }
  ~DeviceRun() {
    if (stream) hipStreamSynchronize(stream);
    bufs.clear();
    if (stream) hipStreamDestroy(stream);
    if (prev >= 0) hipSetDevice(prev);
    (void)hipGetLastError();
  }
};
