// probe_call.hpp - TEST INFRASTRUCTURE ONLY: the host side every wrapper of the device probe shares (probe.hip, probe_reduce.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <vector>

namespace fsp {

// device buffers of one wrapper call; the first failing HIP call is kept and every later step is skipped
struct Call {
  hipError_t err = hipSuccess;
  std::vector<void *> bufs;
  struct Back { void *host; void *dev; size_t bytes; };
  std::vector<Back> backs;
  bool ok() const { return err == hipSuccess; }
  void check(hipError_t e) { if (err == hipSuccess && e != hipSuccess) err = e; }
  void *alloc(size_t bytes) {
    void *d = nullptr;
    if (ok()) { check(hipMalloc(&d, bytes ? bytes : 1)); if (ok()) bufs.push_back(d); else d = nullptr; }
    return d;
  }
  template <typename T> const T *in(const T *host, size_t count) {
    void *d = alloc(count * sizeof(T));
    if (ok() && count) check(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
    return (const T *)d;
  }
  template <typename T> T *out(T *host, size_t count) {
    void *d = alloc(count * sizeof(T));
    if (ok()) { check(hipMemset(d, 0, count * sizeof(T))); backs.push_back({host, d, count * sizeof(T)}); }
    return (T *)d;
  }
  int finish() {
    if (ok()) check(hipGetLastError());
    if (ok()) check(hipDeviceSynchronize());
    for (const Back &b : backs) if (ok() && b.bytes) check(hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost));
    for (void *d : bufs) check(hipFree(d));
    return (int)err;
  }
};
constexpr int kBadArg = (int)hipErrorInvalidValue;

}  // namespace fsp
