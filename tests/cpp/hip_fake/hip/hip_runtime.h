// A stand-in for <hip/hip_runtime.h> that a host compiler reads: the calls device_buffer.h and staged_call.h make, over
// malloc and free, with one stream.  What makes it a test instrument:
//   * every hipMemcpyAsync / hipMemsetAsync (and every hip_fake::launch) is DEFERRED until hipStreamSynchronize, or
//     until a hipFree has to wait for the stream: a path that lets host memory go, or leaves a scope, with work queued
//     touches freed memory when the queue runs, and AddressSanitizer reports it;
//   * it counts the live allocations and logs every call, allocation size and copy;
//   * it fails the k-th call (hipMalloc: hipErrorOutOfMemory, any other: hipErrorUnknown), without doing its work.
// tests/cpp/staged_call_test.cpp is its user.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
enum hipMemcpyKind { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };
typedef struct ihipStream_t* hipStream_t;
enum { hipHostMallocDefault = 0 };

namespace hip_fake {

enum CallKind { kMalloc, kHostMalloc, kMemset, kMemcpyAsync, kMemsetAsync, kSynchronize };

struct Copy {
  hipMemcpyKind kind;
  size_t bytes;
};

struct State {
  std::vector<std::function<void()>> queue;  // the stream's pending work, in order
  std::map<void*, size_t> live;              // allocations not freed yet
  std::vector<CallKind> calls;               // every counted call, in order (frees and error queries are not counted)
  std::vector<size_t> alloc_bytes;           // of every successful hipMalloc
  std::vector<Copy> copies;                  // of every hipMemcpyAsync enqueued
  size_t memsets = 0;                        // hipMemsetAsync enqueued
  size_t fail_at = 0;                        // 1-based index of the call to fail; 0: none
  bool failed = false;
  size_t enqueued_after_failure = 0;
  size_t frees_that_waited = 0;  // hipFree / hipHostFree calls that found work queued
};
inline State& state() {
  static State s;
  return s;
}
inline void reset(size_t fail_at = 0) {
  State& s = state();
  s = State();
  s.fail_at = fail_at;
}
inline void drain() {
  State& s = state();
  std::vector<std::function<void()>> q;
  q.swap(s.queue);
  for (auto& f : q) f();
}
// true: this call is the one to fail
inline bool count(CallKind k) {
  State& s = state();
  s.calls.push_back(k);
  if (s.calls.size() != s.fail_at) return false;
  s.failed = true;
  return true;
}
inline void enqueue(std::function<void()> f) {
  State& s = state();
  if (s.failed) ++s.enqueued_after_failure;
  s.queue.push_back(std::move(f));
}
// a "kernel": host code that runs in stream order
inline void launch(hipStream_t, std::function<void()> f) { enqueue(std::move(f)); }

inline hipError_t allocate(CallKind k, void** p, size_t bytes) {
  *p = nullptr;
  if (count(k)) return k == kMalloc ? hipErrorOutOfMemory : hipErrorUnknown;
  if (bytes == 0) return hipSuccess;
  *p = std::malloc(bytes);
  if (!*p) return hipErrorOutOfMemory;
  state().live[*p] = bytes;
  if (k == kMalloc) state().alloc_bytes.push_back(bytes);
  return hipSuccess;
}
inline hipError_t release(void* p) {
  State& s = state();
  if (!s.queue.empty()) ++s.frees_that_waited, drain();
  if (p && s.live.erase(p) != 1) return hipErrorInvalidValue;
  std::free(p);
  return hipSuccess;
}

}  // namespace hip_fake

inline hipError_t hipMalloc(void** p, size_t bytes) { return hip_fake::allocate(hip_fake::kMalloc, p, bytes); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return hip_fake::allocate(hip_fake::kHostMalloc, p, bytes); }
inline hipError_t hipFree(void* p) { return hip_fake::release(p); }
inline hipError_t hipHostFree(void* p) { return hip_fake::release(p); }
inline hipError_t hipGetLastError() { return hipSuccess; }
inline const char* hipGetErrorString(hipError_t e) {
  return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : e == hipErrorInvalidValue ? "invalid value" : "unknown error";
}
inline hipError_t hipMemset(void* p, int value, size_t bytes) {  // blocking
  if (hip_fake::count(hip_fake::kMemset)) return hipErrorUnknown;
  hip_fake::drain();
  std::memset(p, value, bytes);
  return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
  if (hip_fake::count(hip_fake::kMemcpyAsync)) return hipErrorUnknown;
  hip_fake::enqueue([=] { std::memcpy(dst, src, bytes); });
  hip_fake::state().copies.push_back(hip_fake::Copy{kind, bytes});
  return hipSuccess;
}
inline hipError_t hipMemsetAsync(void* p, int value, size_t bytes, hipStream_t) {
  if (hip_fake::count(hip_fake::kMemsetAsync)) return hipErrorUnknown;
  hip_fake::enqueue([=] { std::memset(p, value, bytes); });
  ++hip_fake::state().memsets;
  return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t) {
  if (hip_fake::count(hip_fake::kSynchronize)) return hipErrorUnknown;
  hip_fake::drain();
  return hipSuccess;
}
