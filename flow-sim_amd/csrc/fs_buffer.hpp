// fs_buffer.hpp - the owner of one device (hipMalloc) or pinned host (hipHostMalloc) allocation: move-only, knows its size in bytes,
// frees on reset() and on destruction.  Every buffer of a batch (fs_abi.hip: fs_batch) is one; they are freed with the batch, under its
// device, while its stream and events still exist.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace fs {

template <bool Pinned> class Buffer {
 public:
  Buffer() = default;
  Buffer(const Buffer &) = delete;
  Buffer &operator=(const Buffer &) = delete;
  Buffer(Buffer &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
  Buffer &operator=(Buffer &&o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
    return *this;
  }
  ~Buffer() { reset(); }

  // exactly `bytes`: kept when it already is that size, else freed and allocated anew (contents undefined)
  hipError_t ensure(size_t bytes) {
    if (p_ && bytes_ == bytes) return hipSuccess;
    reset();
    const hipError_t e = Pinned ? hipHostMalloc(&p_, bytes, hipHostMallocDefault) : hipMalloc(&p_, bytes);
    if (e != hipSuccess) p_ = nullptr; else bytes_ = bytes;
    return e;
  }
  // at least `bytes`: grown, never shrunk (a later call of the same size allocates nothing); *grew says whether the memory is new
  hipError_t reserve(size_t bytes, bool *grew = nullptr) {
    const bool grow = bytes_ < bytes;
    if (grew) *grew = grow;
    return grow ? ensure(bytes) : hipSuccess;
  }
  void reset() {
    if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr; bytes_ = 0;
  }
  template <typename R = void> R *get() const { return static_cast<R *>(p_); }
  explicit operator bool() const { return p_ != nullptr; }
  size_t bytes() const { return bytes_; }

 private:
  void *p_ = nullptr;
  size_t bytes_ = 0;
};

using DeviceBuffer = Buffer<false>;
using PinnedBuffer = Buffer<true>;

}  // namespace fs
