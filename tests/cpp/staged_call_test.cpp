// StagedCall (reak_amd/csrc/staged_call.h) over the fake runtime of tests/cpp/hip_fake, which defers every asynchronous
// copy and fill until the stream is waited for.  One representative call -- two inputs (one from a local vector), three
// outputs (one without a host), a zeroed scratch array, a min = 1 array of no elements -- runs clean, then once with each
// of its runtime calls failing in turn.  Compiled by the host compiler with AddressSanitizer and UBSan, run directly.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "staged_call.h"

namespace {
std::string g_error;
size_t g_release = 0;  // what release_cached_memory() frees, once
}  // namespace
namespace rkh {
void set_error(const std::string& msg) { g_error = msg; }
size_t release_cached_memory() {
  const size_t r = g_release;
  g_release = 0;
  return r;
}
}  // namespace rkh

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s (k = %zu)\n", __FILE__, __LINE__, #cond, hip_fake::state().fail_at); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

namespace {

constexpr size_t kNa = 37, kNb = 5;
constexpr double kUntouched = -777.0;

struct Host {  // the caller's side
  std::vector<double> a, sum, aux;
  std::vector<uint32_t> tag;
  float none = 3.5f;
  Host() : a(kNa), sum(kNa, kUntouched), aux(kNa, kUntouched), tag(kNb, 0xDEADu) {
    for (size_t i = 0; i < kNa; ++i) a[i] = 0.25 * double(i) - 3.0;
  }
};

// shaped like an entry point: stage, check once, launch, fetch.  launch_fails: the launcher refuses after the staging
rkh_status representative_call(Host& h, bool launch_fails, bool* launched) {
  hipStream_t s = nullptr;
  std::vector<uint32_t> b(kNb);  // a host source that dies with this scope: declared before the call
  for (size_t j = 0; j < kNb; ++j) b[j] = uint32_t(100 + j);
  rkh::StagedCall call(s);
  const double* d_a = call.in(h.a.data(), kNa);
  const uint32_t* d_b = call.in(b.data(), b.size());
  double* d_sum = call.out(h.sum.data(), kNa);
  uint32_t* d_tag = call.out(h.tag.data(), kNb);
  double* d_aux = call.out<double>(nullptr, kNa);  // no host: allocated, never copied back
  uint64_t* d_zero = call.scratch<uint64_t>(4, 0, 0);
  float* d_none = call.out(&h.none, 0, 1);  // no elements, one allocated
  if (call.status() != RKH_OK) {
    CHECK(!d_none);  // everything behind the failure is null
    return call.status();
  }
  CHECK(d_a && d_b && d_sum && d_tag && d_aux && d_zero && d_none);
  if (launch_fails) return RKH_ERR_UNSUPPORTED;
  *launched = true;
  hip_fake::launch(s, [=] {
    for (size_t i = 0; i < kNa; ++i) d_sum[i] = 2.0 * d_a[i] + double(d_zero[i % 4]), d_aux[i] = -d_a[i];
    for (size_t j = 0; j < kNb; ++j) d_tag[j] = d_b[j] ^ 0xA5u;
    d_none[0] = 1.0f;
  });
  return call.fetch();
}

void check_scope_end(bool failure_absorbed = false) {
  const hip_fake::State& f = hip_fake::state();
  CHECK(f.queue.empty());
  CHECK(f.live.empty());
  CHECK(f.frees_that_waited == 0);  // the stream was idle before anything was freed
  CHECK(failure_absorbed || f.enqueued_after_failure == 0);
}

void check_outputs(const Host& h, bool written) {
  for (size_t i = 0; i < kNa; ++i) {
    CHECK(h.sum[i] == (written ? 2.0 * h.a[i] : kUntouched));
    CHECK(h.aux[i] == kUntouched);
  }
  for (size_t j = 0; j < kNb; ++j) CHECK(h.tag[j] == (written ? (uint32_t(100 + j) ^ 0xA5u) : 0xDEADu));
  CHECK(h.none == 3.5f);
}

}  // namespace

int main() {
  using namespace hip_fake;
  // clean
  std::vector<CallKind> calls;
  {
    reset();
    Host h;
    bool launched = false;
    CHECK(representative_call(h, false, &launched) == RKH_OK && launched);
    check_scope_end();
    check_outputs(h, true);
    const State& f = state();
    const std::vector<size_t> want_allocs = {kNa * 8, kNb * 4, kNa * 8, kNb * 4, kNa * 8, 4 * 8, 4};
    CHECK(f.alloc_bytes == want_allocs);
    CHECK(f.copies.size() == 4 && f.memsets == 1);
    CHECK(f.copies[0].kind == hipMemcpyHostToDevice && f.copies[0].bytes == kNa * 8);
    CHECK(f.copies[1].kind == hipMemcpyHostToDevice && f.copies[1].bytes == kNb * 4);
    CHECK(f.copies[2].kind == hipMemcpyDeviceToHost && f.copies[2].bytes == kNa * 8);
    CHECK(f.copies[3].kind == hipMemcpyDeviceToHost && f.copies[3].bytes == kNb * 4);
    calls = f.calls;
    CHECK(calls.size() == 7 + 4 + 1 + 2);  // the second wait is the destructor's
    CHECK(calls[calls.size() - 2] == kSynchronize && calls.back() == kSynchronize);
  }
  // the launcher refuses: the scope ends with the inputs still queued
  {
    reset();
    Host h;
    bool launched = false;
    CHECK(representative_call(h, true, &launched) == RKH_ERR_UNSUPPORTED && !launched);
    check_scope_end();
    check_outputs(h, false);
  }
  // every call fails in turn
  for (size_t k = 1; k <= calls.size(); ++k) {
    reset(k);
    g_error.clear();
    Host h;
    bool launched = false;
    const rkh_status st = representative_call(h, false, &launched);
    const bool last_wait = k == calls.size();  // the destructor's: the entry has answered by then
    const rkh_status want = last_wait ? RKH_OK : calls[k - 1] == kMalloc ? RKH_ERR_OOM : RKH_ERR_DEVICE;
    CHECK(st == want);
    CHECK(state().failed);
    CHECK(last_wait || !g_error.empty());
    CHECK(launched == (k > 7 + 2 + 1));  // a staging failure is seen before the launch
    check_scope_end();
    if (k <= 7 + 2 + 1) check_outputs(h, false);
  }
  // an allocation that succeeds once cached memory is released: DeviceBuffer::alloc's retry is the path taken
  {
    reset(1);
    g_release = 64;
    Host h;
    bool launched = false;
    CHECK(representative_call(h, false, &launched) == RKH_OK && launched);
    check_scope_end(true);
    check_outputs(h, true);
    CHECK(state().calls.size() == calls.size() + 1 && state().calls[1] == kMalloc);
  }
  std::printf("staged call ok: %zu runtime calls, each failed once\n", calls.size());
  return 0;
}
