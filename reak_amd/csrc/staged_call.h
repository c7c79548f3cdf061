// staged_call.h -- the transfers around the launch of a one-shot entry point: the caller's arrays to the device, the
// launch, the results back.  A StagedCall is bound to one stream for one call and owns every device buffer of it.  The
// rule it keeps: the stream is idle before anything is freed or the entry returns, on every way out.  Host only, over
// device_buffer.h (every allocation goes through DeviceBuffer::alloc and its retry); it names no kernel.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "device_buffer.h"

namespace rkh {

// Waits for the stream when its scope ends: for the few places that keep buffers of their own beside a launch (a cached
// arena, a workspace, a table of device pointers).  Declared behind the buffers it protects.
struct StreamWait {
  hipStream_t s;
  ~StreamWait() { (void)hipStreamSynchronize(s); }
};

// in / out / scratch each allocate max(n, min_n) elements and return the device array; a call of n = 0 copies nothing.
// The first failure is latched (its text is the thread's last error): nothing is enqueued after it and every later
// array is null, so an entry checks status() once, before it launches.  Host memory handed to in() and out() -- the
// caller's, or a local declared BEFORE the StagedCall -- outlives it: the destructor is where the stream is waited for.
class StagedCall {
 public:
  static constexpr int kNoFill = -1;  // fill: a byte value for the whole allocation (hipMemsetAsync), or none

  explicit StagedCall(hipStream_t s) : s_(s) { bufs_.reserve(16), back_.reserve(8); }
  StagedCall(const StagedCall&) = delete;
  StagedCall& operator=(const StagedCall&) = delete;
  ~StagedCall() { (void)hipStreamSynchronize(s_); }  // then bufs_ frees

  // n elements of host, copied to the device
  template <class T>
  T* in(const T* host, size_t n, size_t min_n = 0) {
    T* d = scratch<T>(n, min_n);
    if (d && n) check(hipMemcpyAsync(d, host, n * sizeof(T), hipMemcpyHostToDevice, s_), "hipMemcpyAsync to the device");
    return st_ == RKH_OK ? d : nullptr;
  }
  // n elements that fetch() copies to host; host = null: allocated, never copied back
  template <class T>
  T* out(T* host, size_t n, size_t min_n = 0, int fill = kNoFill) {
    T* d = scratch<T>(n, min_n, fill);
    if (d && host && n) back_.push_back(Back{host, d, n * sizeof(T)});
    return d;
  }
  template <class T>
  T* scratch(size_t n, size_t min_n = 0, int fill = kNoFill) {
    if (st_ != RKH_OK) return nullptr;
    const size_t bytes = std::max(n, min_n) * sizeof(T);
    bufs_.emplace_back();
    st_ = bufs_.back().alloc(bytes);
    void* d = bufs_.back().get();
    if (d && fill != kNoFill) check(hipMemsetAsync(d, fill, bytes, s_), "hipMemsetAsync of a new buffer");
    return st_ == RKH_OK ? static_cast<T*>(d) : nullptr;
  }

  rkh_status status() const { return st_; }

  // the copies out() remembered, then the wait for the stream: the entry's last step with the device
  rkh_status fetch() {
    for (const Back& b : back_)
      if (st_ == RKH_OK) check(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, s_), "hipMemcpyAsync to the host");
    back_.clear();
    if (st_ == RKH_OK) check(hipStreamSynchronize(s_), "hipStreamSynchronize");
    return st_;
  }

 private:
  struct Back {
    void* host;
    const void* dev;
    size_t bytes;
  };
  void check(hipError_t e, const char* what) {  // as RKH_HIP
    if (e == hipSuccess) return;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    st_ = e == hipErrorOutOfMemory ? RKH_ERR_OOM : RKH_ERR_DEVICE;
  }
  hipStream_t s_;
  rkh_status st_ = RKH_OK;
  std::vector<DeviceBuffer<void>> bufs_;
  std::vector<Back> back_;
};

}  // namespace rkh
