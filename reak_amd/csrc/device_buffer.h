// device_buffer.h -- the one owner of device and pinned host memory in librkh.so: every hipMalloc / hipHostMalloc and
// its free happen here.  Handles and one-shot entry points hold their memory in these; device tables and launchers take
// plain pointers from get().
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <type_traits>

#include "../../include/rkh.h"

namespace rkh {

void set_error(const std::string& msg);

// Move-only array of n elements of T (T = void: n bytes) in device memory, or in pinned host memory (Pinned).  The
// destructor frees; a moved-from buffer is empty and frees nothing.
template <class T, bool Pinned = false>
class Buffer {
 public:
  Buffer() = default;
  Buffer(Buffer&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, n_ = o.n_;
      o.p_ = nullptr, o.n_ = 0;
    }
    return *this;
  }
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  ~Buffer() { reset(); }

  T* get() const { return p_; }
  size_t size() const { return n_; }  // elements allocated (0 after a failed alloc)
  explicit operator bool() const { return p_ != nullptr; }
  void reset() {
    if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr, n_ = 0;
  }
  // n uninitialised elements.  What the buffer held before is freed first, its contents discarded (growing scratch:
  // `if (need > b.size()) alloc(need)`).
  rkh_status alloc(size_t n) {
    reset();
    void* p = nullptr;
    const rkh_status st = check(Pinned ? hipHostMalloc(&p, n * kElem, hipHostMallocDefault) : hipMalloc(&p, n * kElem),
                                (Pinned ? "hipHostMalloc of " : "hipMalloc of ") + std::to_string(n * kElem) + " bytes");
    if (st == RKH_OK) p_ = static_cast<T*>(p), n_ = n;
    return st;
  }
  // device memory only: n elements, all bytes zero (a blocking hipMemset)
  rkh_status alloc_zeroed(size_t n) {
    static_assert(!Pinned, "pinned memory is filled by the host");
    const rkh_status st = alloc(n);
    return st != RKH_OK ? st : check(hipMemset(p_, 0, n * kElem), "hipMemset of a new buffer");
  }

 private:
  static constexpr size_t kElem = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
  static rkh_status check(hipError_t e, const std::string& what) {  // as RKH_HIP: the error text, OOM apart
    if (e == hipSuccess) return RKH_OK;
    set_error(what + ": " + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? RKH_ERR_OOM : RKH_ERR_DEVICE;
  }
  T* p_ = nullptr;
  size_t n_ = 0;
};
template <class T> using DeviceBuffer = Buffer<T, false>;
template <class T> using PinnedBuffer = Buffer<T, true>;

}  // namespace rkh
