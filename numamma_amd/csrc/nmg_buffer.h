// nmg_buffer.h -- the engine's two owning memory types: DevBuf<T> (device
// memory, hipMalloc / hipFree) and PinBuf<T> (pinned host memory,
// hipHostMalloc / hipHostFree).  Move-only; the destructor frees.  Neither
// synchronises anything: a block that a launch in flight may still read is
// released only after its caller has waited for that launch.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>

namespace nmg {

struct DevMem {
  hipError_t get(void** p, size_t bytes) const { return hipMalloc(p, bytes); }
  void put(void* p) const { (void)hipFree(p); }
};

struct PinMem {
  unsigned flags = hipHostMallocDefault;
  static PinMem portable() { return PinMem{hipHostMallocPortable}; }  // usable from every device
  hipError_t get(void** p, size_t bytes) const { return hipHostMalloc(p, bytes, flags); }
  void put(void* p) const { (void)hipHostFree(p); }
};

template <class T, class Mem>
class OwnedBuf {
 public:
  OwnedBuf() = default;
  explicit OwnedBuf(Mem mem) : mem_(mem) {}
  OwnedBuf(const OwnedBuf&) = delete;
  OwnedBuf& operator=(const OwnedBuf&) = delete;
  OwnedBuf(OwnedBuf&& o) noexcept : p_(o.p_), cap_(o.cap_), mem_(o.mem_) {
    o.p_ = nullptr;
    o.cap_ = 0;
  }
  OwnedBuf& operator=(OwnedBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      cap_ = o.cap_;
      mem_ = o.mem_;
      o.p_ = nullptr;
      o.cap_ = 0;
    }
    return *this;
  }
  ~OwnedBuf() { reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t cap() const { return cap_; }  // elements

  // Frees what is held, then allocates exactly n elements (n == 0: a small
  // block, so that the pointer is never null after a success).  On failure
  // the buffer is empty.
  hipError_t alloc(size_t n) {
    reset();
    void* q = nullptr;
    const hipError_t e = mem_.get(&q, n ? n * sizeof(T) : 16);
    if (e != hipSuccess) return e;
    p_ = static_cast<T*>(q);
    cap_ = n;
    return hipSuccess;
  }
  // Grows only; the contents are not kept.
  hipError_t reserve(size_t n) { return n <= cap_ ? hipSuccess : alloc(n); }
  void reset() {
    if (p_) mem_.put(p_);
    p_ = nullptr;
    cap_ = 0;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
  Mem mem_;
};

template <class T>
using DevBuf = OwnedBuf<T, DevMem>;

// (PinBuf<T>(PinMem::portable()) for a block that other devices copy from)
template <class T>
using PinBuf = OwnedBuf<T, PinMem>;

}  // namespace nmg
