// svp_walk_dir.hip -- the collision-tested walk over the SVP space with a direction per row: forward (move_pt_toward, what
// rkh_svp_edge_check computes) or backward (move_pt_back_to: the profile a -> b walked from b, the last free point kept).
// The scalar rules of a row are svp_walk_rules.h's, the arithmetic svp_device.h's; a forward row equals svp_space.hip's
// walk bit for bit, a backward row the twin rkh.h states (tests/svp_back_ref.py).
//
// Kernels, in the staged form of svp_space.hip's walk and over the same workspace (SvpWalk, svp_walk_layout):
//   rl1dir_walk_solve_kernel   one lane per row: T, peaks, dt, the point count of the row's loop; rows without a point
//                              finish here, the others enter the live list
//   rl1dir_walk_points_kernel  one lane per (live row, point of the pass): the point in space coordinates and model units,
//                              and its bounds verdict; point j is at the row's next time moved j steps in its direction
//   rl1dir_walk_scan_kernel    one lane per live row: the pass's verdicts in order; first failure, last good point, count;
//                              unfinished rows enter the next pass's list
// The forward half restates svp_space.hip's three kernels, whose text and register counts are pinned by
// tests/test_svp_space_resources.py; folding the two is a later clean-up.
// Entries: rkh_svp_edge_check_back (every row backward), rkh_diag_svp_edge_check_dir (a direction byte per row).
#include <cmath>
#include <cstring>

#include "rkh_internal.h"
#include "staged_call.h"
#include "svp_device.h"
#include "svp_walk_rules.h"

namespace rkh {
namespace {

constexpr uint32_t kDirThreads = 256;

__device__ __forceinline__ double dir_fraction(const SvpWalk& w, uint32_t e) { return w.fraction ? w.fraction[e] : 1.0; }
__device__ __forceinline__ bool dir_back(const uint8_t* back, uint32_t e) { return back && back[e] != 0; }

__device__ __forceinline__ void dir_copy_end(const SvpWalk& w, uint32_t e, uint32_t D, SvpWalkEnd end, double* dst) {
  const double* src = (end == kSvpWalkEndA ? w.a : w.b) + size_t(e) * D;
  for (uint32_t c = 0; c < D; ++c) dst[c] = src[c];
}

// what the walk returns after its loop: an end of the profile, or the (untested) point at dt
__device__ __forceinline__ void dir_walk_finish(const SvpDev& sp, const SvpWalk& w, bool back, uint32_t e) {
  const uint32_t D = 2 * uint32_t(sp.n);
  double* out = w.out + size_t(e) * D;
  const SvpWalkEnd end = svp_walk_result(back, dir_fraction(w, e));
  if (end == kSvpWalkEndPoint)
    svp_point(sp, w.a + size_t(e) * D, w.b + size_t(e) * D, w.peak + size_t(e) * sp.n, w.T[e], w.dt[e], out, nullptr);
  else
    dir_copy_end(w, e, D, end, out);
  w.reached[e] = 1;
}

__global__ __launch_bounds__(256) void rl1dir_walk_solve_kernel(const SvpDev sp, const SvpWalk w,
                                                                const uint8_t* __restrict__ d_back) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= w.B) return;
  const uint32_t D = 2 * uint32_t(sp.n);
  const bool back = dir_back(d_back, e);
  const double T = svp_reach(sp, w.a + size_t(e) * D, w.b + size_t(e) * D, w.peak + size_t(e) * sp.n);
  w.T[e] = T;
  w.n_checked[e] = 0;
  w.reached[e] = 0;
  bool over = false;
  uint32_t K = 0;
  double dt = 0.0;
  if (T < INFINITY) {
    dt = svp_walk_dt(back, T, dir_fraction(w, e));
    K = svp_walk_count(back, sp.min_interval, T, dt, kSvpWalkMaxPoints, &over);
  }
  if (!(T < INFINITY) || over) {
    dir_copy_end(w, e, D, svp_walk_origin(back), w.out + size_t(e) * D);
    if (over) atomicOr(&w.counters[2], 1u);
    return;
  }
  w.dt[e] = dt;
  w.K[e] = K;
  w.k_done[e] = 0;
  w.d_next[e] = svp_walk_first(back, sp.min_interval, T);
  if (K == 0) {
    dir_walk_finish(sp, w, back, e);
    return;
  }
  dir_copy_end(w, e, D, svp_walk_origin(back), w.last + size_t(e) * D);
  w.list[0][atomicAdd(&w.counters[0], 1u)] = e;
}

__global__ __launch_bounds__(256) void rl1dir_walk_points_kernel(const SvpDev sp, const SvpWalk w,
                                                                 const uint8_t* __restrict__ d_back, uint32_t cur,
                                                                 uint32_t live) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= live * kSvpWalkPass) return;
  const uint32_t e = w.list[cur][i / kSvpWalkPass], j = i % kSvpWalkPass;
  const uint32_t D = 2 * uint32_t(sp.n);
  const double* a = w.a + size_t(e) * D;
  double* x = w.pts + size_t(i) * D;
  double* xm = w.pts_model + size_t(i) * D;
  if (w.k_done[e] + j < w.K[e]) {
    const double d = svp_walk_advance(dir_back(d_back, e), w.d_next[e], sp.min_interval, j);
    svp_point(sp, a, w.b + size_t(e) * D, w.peak + size_t(e) * sp.n, w.T[e], d, x, xm);
    w.inb[i] = svp_in_bounds(sp, x) ? 1 : 0;
  } else {  // past the row's last point: the distance launch still reads the row
    for (uint32_t c = 0; c < uint32_t(sp.n); ++c) {
      x[2 * c] = a[2 * c], x[2 * c + 1] = a[2 * c + 1];
      xm[2 * c] = a[2 * c] * sp.speed[c], xm[2 * c + 1] = a[2 * c + 1] * sp.accel[c];
    }
    w.inb[i] = 1;
  }
}

// has_dist = 0: the scene has no proxy pair, every point is collision-free
__global__ __launch_bounds__(256) void rl1dir_walk_scan_kernel(const SvpDev sp, const SvpWalk w,
                                                               const uint8_t* __restrict__ d_back, uint32_t cur, uint32_t live,
                                                               int has_dist) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= live) return;
  const uint32_t e = w.list[cur][i];
  const uint32_t D = 2 * uint32_t(sp.n);
  const uint32_t K = w.K[e];
  const bool back = dir_back(d_back, e);
  uint32_t k = w.k_done[e], nc = w.n_checked[e];
  int good = -1;
  bool failed = false;
  uint32_t j = 0;
  for (; j < kSvpWalkPass && k + j < K; ++j) {
    const size_t row = size_t(i) * kSvpWalkPass + j;
    ++nc;
    if (!w.inb[row] || (has_dist && w.dist[row] < 0.0)) {
      failed = true;
      break;
    }
    good = int(j);
  }
  w.n_checked[e] = nc;
  const double* lastp = good >= 0 ? w.pts + (size_t(i) * kSvpWalkPass + uint32_t(good)) * D : w.last + size_t(e) * D;
  if (failed) {
    for (uint32_t c = 0; c < D; ++c) w.out[size_t(e) * D + c] = lastp[c];
    return;
  }
  k += j;
  if (k == K) {
    dir_walk_finish(sp, w, back, e);
    return;
  }
  for (uint32_t c = 0; c < D; ++c) w.last[size_t(e) * D + c] = lastp[c];
  w.d_next[e] = svp_walk_advance(back, w.d_next[e], sp.min_interval, kSvpWalkPass);
  w.k_done[e] = k;
  w.list[1 - cur][atomicAdd(&w.counters[1 - cur], 1u)] = e;
}

rkh_status bad(const char* who, const char* what) {
  set_error(std::string(who) + ": " + what);
  return RKH_ERR_BAD_ARG;
}

}  // namespace

rkh_status launch_svp_walk_dir(const char* who, const rkh_scene& scene, const SvpDev& sp, const SvpWalk& w, const uint8_t* d_back,
                               uint32_t* passes) {
  const uint32_t B = w.B;
  hipStream_t s = scene.ctx->stream;
  if (passes) *passes = 0;
  if (B == 0) return RKH_OK;
  StreamWait wait_on_exit{s};
  RKH_HIP(hipMemsetAsync(w.counters, 0, 3 * 4, s));
  hipLaunchKernelGGL(rl1dir_walk_solve_kernel, dim3((B + kDirThreads - 1) / kDirThreads), dim3(kDirThreads), 0, s, sp, w, d_back);
  RKH_HIP(hipGetLastError());
  uint32_t cnt[3] = {0, 0, 0};
  RKH_HIP(hipMemcpyAsync(cnt, w.counters, sizeof(cnt), hipMemcpyDeviceToHost, s));
  RKH_HIP(hipStreamSynchronize(s));
  if (cnt[2]) {
    set_error(std::string(who) + ": an edge has more than 1 048 576 points to test (min_interval against its reach time)");
    return RKH_ERR_CAPACITY;
  }
  const int has_dist = scene.n_pairs > 0 ? 1 : 0;
  uint32_t pass = 0;
  for (uint32_t live = cnt[0], c = 0; live > 0; c = 1 - c, ++pass) {
    if (live > B || pass > kSvpWalkMaxPoints / kSvpWalkPass) {
      set_error(std::string(who) + ": the live list is inconsistent");
      return RKH_ERR_DEVICE;
    }
    const uint32_t n_rows = live * kSvpWalkPass;
    hipLaunchKernelGGL(rl1dir_walk_points_kernel, dim3((n_rows + kDirThreads - 1) / kDirThreads), dim3(kDirThreads), 0, s, sp, w,
                       d_back, c, live);
    RKH_HIP(hipGetLastError());
    if (has_dist) RKH_TRY(launch_min_distance(s, scene, w.pts_model, n_rows, w.dist));
    RKH_HIP(hipMemsetAsync(w.counters + (1 - c), 0, 4, s));
    hipLaunchKernelGGL(rl1dir_walk_scan_kernel, dim3((live + kDirThreads - 1) / kDirThreads), dim3(kDirThreads), 0, s, sp, w, d_back,
                       c, live, has_dist);
    RKH_HIP(hipGetLastError());
    RKH_HIP(hipMemcpyAsync(cnt, w.counters, sizeof(cnt), hipMemcpyDeviceToHost, s));
    RKH_HIP(hipStreamSynchronize(s));
    live = cnt[1 - c];
  }
  if (passes) *passes = pass;
  return RKH_OK;
}

namespace {

// rkh_svp_edge_check's arguments with a direction: back_all, or a host byte per row (back, may be null = forward)
rkh_status edge_check_dir(const char* who, rkh_scene* scene, const rkh_svp_space* space, const double* a, const double* b, uint32_t B,
                          const double* fraction, bool back_all, const uint8_t* back, double* out, double* reach_time,
                          uint32_t* n_checked, uint8_t* reached) {
  if (!scene) return bad(who, "scene is NULL");
  SvpDev sp;
  RKH_TRY(svp_space_dev(who, space, scene->host.n_dof, &sp));
  if (B == 0) return RKH_OK;
  if (!a || !b || !out) return bad(who, "a required pointer is NULL");
  if (B > (1u << 24)) {
    set_error(std::string(who) + ": at most 16 777 216 edges per call");
    return RKH_ERR_CAPACITY;
  }
  const size_t D = 2 * size_t(sp.n);
  rkh_ctx* ctx = scene->ctx;
  hipStream_t s = ctx->stream;
  RKH_HIP(hipSetDevice(ctx->device));
  // one slab for the call: the walk's workspace, then the direction bytes
  const bool with_dir = back_all || back != nullptr;
  const size_t walk_bytes = svp_walk_layout(sp.n, B, fraction != nullptr, nullptr, nullptr);
  const size_t bytes = walk_bytes + (with_dir ? arena_align_up(B) : 0);
  DeviceArena arena;
  RKH_TRY(ctx_take_arena(ctx, bytes + kArenaGuardBytes, true, &arena));
  struct GiveBack {  // the stream is idle before the slab goes back to its context
    rkh_ctx* ctx;
    hipStream_t s;
    DeviceArena* arena;
    ~GiveBack() {
      (void)hipStreamSynchronize(s);
      ctx_give_arena(ctx, std::move(*arena));
    }
  } give_back{ctx, s, &arena};
  SvpWalk w;
  svp_walk_layout(sp.n, B, fraction != nullptr, arena.get(), &w);
  uint8_t* d_back = with_dir ? static_cast<uint8_t*>(arena.get()) + walk_bytes : nullptr;
  RKH_HIP(hipMemcpyAsync(const_cast<double*>(w.a), a, B * D * 8, hipMemcpyHostToDevice, s));
  RKH_HIP(hipMemcpyAsync(const_cast<double*>(w.b), b, B * D * 8, hipMemcpyHostToDevice, s));
  if (fraction) RKH_HIP(hipMemcpyAsync(const_cast<double*>(w.fraction), fraction, size_t(B) * 8, hipMemcpyHostToDevice, s));
  if (back_all) RKH_HIP(hipMemsetAsync(d_back, 1, B, s));
  else if (back) RKH_HIP(hipMemcpyAsync(d_back, back, B, hipMemcpyHostToDevice, s));
  RKH_TRY(launch_svp_walk_dir(who, *scene, sp, w, d_back, nullptr));
  RKH_HIP(hipMemcpyAsync(out, w.out, B * D * 8, hipMemcpyDeviceToHost, s));
  if (reach_time) RKH_HIP(hipMemcpyAsync(reach_time, w.T, size_t(B) * 8, hipMemcpyDeviceToHost, s));
  if (n_checked) RKH_HIP(hipMemcpyAsync(n_checked, w.n_checked, size_t(B) * 4, hipMemcpyDeviceToHost, s));
  if (reached) RKH_HIP(hipMemcpyAsync(reached, w.reached, B, hipMemcpyDeviceToHost, s));
  RKH_HIP(hipStreamSynchronize(s));
  return RKH_OK;
}

}  // namespace
}  // namespace rkh

using namespace rkh;

extern "C" {

rkh_status rkh_svp_edge_check_back(rkh_scene* scene, const rkh_svp_space* space, const double* a, const double* b, uint32_t B,
                                   const double* fraction, double* out, double* reach_time, uint32_t* n_checked,
                                   uint8_t* reached) {
  return edge_check_dir("rkh_svp_edge_check_back", scene, space, a, b, B, fraction, true, nullptr, out, reach_time, n_checked,
                        reached);
}

rkh_status rkh_diag_svp_edge_check_dir(rkh_scene* scene, const rkh_svp_space* space, const double* a, const double* b, uint32_t B,
                                       const double* fraction, const uint8_t* back, double* out, double* reach_time,
                                       uint32_t* n_checked, uint8_t* reached) {
  return edge_check_dir("rkh_diag_svp_edge_check_dir", scene, space, a, b, B, fraction, false, back, out, reach_time, n_checked,
                        reached);
}

}  // extern "C"
