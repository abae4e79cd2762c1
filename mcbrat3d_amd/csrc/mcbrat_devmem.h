// The owner of every allocation of the host library: DeviceBuffer<T> for device memory, PinnedBuffer<T> for mapped pinned host
// memory.  A buffer frees what it holds when it is reset, allocated again, moved over or destroyed, so no function of
// mcbrat_api.hip frees by hand and none leaks on an early return.  Plain C++17, no HIP: the four seam functions below are defined
// in mcbrat_api.hip over the HIP runtime, and tests/device_buffer_check.cpp defines them over malloc to hold the owner to its rules.
#pragma once
#include <cstddef>
#include <utility>

namespace mcbrat {

// The seam.  The allocators return 0 or the runtime's error code (a hipError_t, as a plain int) and leave *ptr null on failure.
int device_alloc(void **ptr, size_t bytes);
void device_free(void *ptr);
int pinned_alloc(void **ptr, size_t bytes);
void pinned_free(void *ptr);

template <typename T, int (*Alloc)(void **, size_t), void (*Free)(void *)>
class OwnedBuffer {
 public:
  OwnedBuffer() = default;
  OwnedBuffer(const OwnedBuffer &) = delete;
  OwnedBuffer &operator=(const OwnedBuffer &) = delete;
  OwnedBuffer(OwnedBuffer &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  OwnedBuffer &operator=(OwnedBuffer &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      n_ = std::exchange(o.n_, 0);
    }
    return *this;
  }
  ~OwnedBuffer() { reset(); }

  T *get() const { return p_; }
  size_t capacity() const { return n_; }  // ELEMENTS allocated
  explicit operator bool() const { return p_ != nullptr; }

  void reset() {
    if (p_) Free(p_);
    p_ = nullptr;
    n_ = 0;
  }
  // Always fresh memory, also when the size is unchanged (the poison build of the library fills what is fresh).  The old block
  // goes first; a failure leaves the buffer empty.
  int allocate(size_t n) {
    reset();
    void *q = nullptr;
    const int status = Alloc(&q, sizeof(T) * n);
    if (status != 0) return status;
    p_ = static_cast<T *>(q);
    n_ = n;
    return 0;
  }
  // Grow only: what is large enough stays.
  int reserve(size_t n) { return n_ >= n ? 0 : allocate(n); }

 private:
  T *p_ = nullptr;
  size_t n_ = 0;
};

template <typename T>
using DeviceBuffer = OwnedBuffer<T, device_alloc, device_free>;
template <typename T>
using PinnedBuffer = OwnedBuffer<T, pinned_alloc, pinned_free>;

}  // namespace mcbrat
