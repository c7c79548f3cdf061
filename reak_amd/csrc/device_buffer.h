// device_buffer.h -- the one owner of device and pinned host memory in librkh.so: every hipMalloc / hipHostMalloc and
// its free happen here.  Handles and one-shot entry points hold their memory in these; device tables and launchers take
// plain pointers from get().  A batch RRT planner holds ONE allocation, a DeviceArena, and carves its buffers out of it
// (arena_layout.h); a context keeps the arenas of destroyed planners for the next one (rkh_internal.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <type_traits>

#include "../../include/rkh.h"
#include "arena_layout.h"

namespace rkh {

void set_error(const std::string& msg);
// Frees the arenas every live context keeps for reuse; returns the bytes freed (rkh_api_nn.hip).  A device allocation
// that runs out of memory calls it and tries once more: nothing starves beside a parked slab.
size_t release_cached_memory();

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
    hipError_t e = Pinned ? hipHostMalloc(&p, n * kElem, hipHostMallocDefault) : hipMalloc(&p, n * kElem);
    if (!Pinned && e == hipErrorOutOfMemory && release_cached_memory() > 0) {
      (void)hipGetLastError();  // the first attempt's error is dealt with
      e = hipMalloc(&p, n * kElem);
    }
    const rkh_status st = check(e, (Pinned ? "hipHostMalloc of " : "hipMalloc of ") + std::to_string(n * kElem) + " bytes");
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

// Move-only slab of device memory that its holder carves into ranges (arena_layout.h: 256-byte aligned offsets, a guard
// tail behind the last range).  One hipMalloc however many ranges; the contents are whatever the memory held before.
class DeviceArena {
 public:
  rkh_status alloc(size_t bytes) { return slab_.alloc(bytes); }
  void reset() { slab_.reset(); }
  size_t size() const { return slab_.size(); }
  explicit operator bool() const { return bool(slab_); }
  void* get() const { return slab_.get(); }
  // the range as an array of T; null for a range of no bytes
  template <class T>
  T* at(const ArenaRange& r) const {
    return r.bytes ? reinterpret_cast<T*>(static_cast<char*>(slab_.get()) + r.off) : nullptr;
  }

 private:
  DeviceBuffer<void> slab_;
};

}  // namespace rkh
