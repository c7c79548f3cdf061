// svp_shortcut.hip -- shortcutting of paths of SVP points under the reach-time metric (the definitions are at
// rkh_svp_shortcut_paths in include/rkh.h; the index rules are path_shortcut.h's, the search is path_shortcut.hip's, the
// walk is svp_space.hip's).  This module joins them:
//   1. rl1cut_pairs_kernel    one lane per candidate pair (i, j) of the current chunk: its two [2 n_dof] rows of the
//                             concatenated point table, copied into the walk's a / b rows.  No arithmetic on a coordinate.
//   2. launch_svp_walk        the staged collision-tested walk over the chunk's rows (fraction null = 1): T = d(p_i -> p_j),
//                             bit for bit rkh_svp_reach_time's, and the `reached` byte of rkh_svp_edge_check.
//   3. rl1cut_time_in_kernel  one lane per path, after the walks: the T of its pairs (v, v + 1) summed left to right.
//   4. shortcut_dp_kernel     as it stands: acc = reached, ok_mask = 0xFF, min_interval = 0, w = T.  +inf weights need no
//                             case of their own there: x + inf < y is never true.
// A module of its own: a kernel added to an existing module moves the code of the ones it holds.
//
// Memory.  The walk's workspace (svp_walk_layout) takes 1096 n_dof + 333 bytes per edge -- four [2 n_dof] rows, the peaks
// and 45 bytes of per-edge state, and per pass slot (32 per edge) two [2 n_dof] rows, a verdict byte and a distance -- so
// the pairs go through ONE workspace of min(E, chunk) edges, chunk after chunk; its T and reached members are re-pointed at
// the chunk's slice of two call-long [E] arrays (9 bytes per pair).  kSvpCutChunk = 262 144 pairs: a 6-joint chain's
// workspace is 6909 bytes per pair, 1.81 GB per call however many pairs the call has (12 joints: 3.54 GB).  Per call:
// 9 bytes per pair + (1096 n_dof + 333) min(pairs, 262 144) + 16 n_dof bytes per point.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "path_shortcut.h"
#include "rkh_internal.h"
#include "staged_call.h"
#include "svp_device.h"

namespace rkh {

namespace {
constexpr uint32_t kSvpCutThreads = 256;
constexpr uint32_t kSvpCutChunk = 1u << 18;  // pairs per walk (see above)
}  // namespace

// Pairs first .. first + count of the call go to rows 0 .. count of a / b.  D = 2 n_dof doubles per row: rows of the point
// table and of the workspace start on 16 bytes, so a row moves as D / 2 double2.
__global__ __launch_bounds__(256) void rl1cut_pairs_kernel(const double* __restrict__ points, uint32_t D,
                                                           const uint32_t* __restrict__ path_ptr,
                                                           const uint32_t* __restrict__ pair_ptr, uint32_t B, uint32_t max_span,
                                                           uint32_t first, uint32_t count, double* __restrict__ a,
                                                           double* __restrict__ b) {
  const uint32_t e = blockIdx.x * kSvpCutThreads + threadIdx.x;
  if (e >= count) return;
  const uint32_t g = first + e;
  const uint32_t p = segment_of(pair_ptr, B, g);  // (paths of one point own no pair and are never returned)
  const uint32_t row0 = path_ptr[p], L = path_ptr[p + 1] - row0;
  uint32_t i, j;
  shortcut_pair_at(L, max_span, g - pair_ptr[p], &i, &j);
  const double2* pi = reinterpret_cast<const double2*>(points + uint64_t(row0 + i) * D);
  const double2* pj = reinterpret_cast<const double2*>(points + uint64_t(row0 + j) * D);
  double2* ae = reinterpret_cast<double2*>(a + uint64_t(e) * D);
  double2* be = reinterpret_cast<double2*>(b + uint64_t(e) * D);
  for (uint32_t c = 0; c < D / 2; ++c) {
    ae[c] = pi[c];
    be[c] = pj[c];
  }
}

__global__ __launch_bounds__(256) void rl1cut_time_in_kernel(const uint32_t* __restrict__ path_ptr,
                                                             const uint32_t* __restrict__ pair_ptr, uint32_t B,
                                                             uint32_t max_span, const double* __restrict__ T,
                                                             double* __restrict__ time_in) {
  const uint32_t p = blockIdx.x * kSvpCutThreads + threadIdx.x;
  if (p >= B) return;
  const uint32_t L = path_ptr[p + 1] - path_ptr[p];
  const double* t = T + pair_ptr[p];
  double sum = 0.0;  // a path of one point has no hop
  for (uint32_t v = 0; v + 1 < L; ++v) sum = sum + t[shortcut_pair_index(L, max_span, v, v + 1)];
  time_in[p] = sum;
}

namespace {

rkh_status bad(const char* who, const char* what) {
  set_error(std::string(who) + ": " + what);
  return RKH_ERR_BAD_ARG;
}

// rkh_svp_shortcut_paths with the chunk size as an argument (rkh_diag_svp_shortcut_chunked), and with ms != null the
// whole sequence again `runs` times, its phases between events (rkh_diag_svp_shortcut_ms): ms[r][0..2] = pairs, walks,
// search (the input-time kernel included), each summed over the chunks.  The first, untimed sequence is the warm-up.
rkh_status svp_shortcut_run(const char* who, rkh_scene* scene, const rkh_svp_space* space, const double* points,
                            const uint32_t* path_ptr, uint32_t B, uint32_t max_span, uint32_t chunk_pairs, uint32_t* keep,
                            uint32_t* n_keep, double* time_in, double* time_out, uint32_t* n_blocked, uint32_t runs,
                            float* ms) {
  // (what needs no device is checked first, the scene last: the argument rules hold on a machine without one)
  SvpDev sp;
  RKH_TRY(svp_space_dev(who, space, scene ? scene->host.n_dof : -1, &sp));
  if (chunk_pairs == 0 || chunk_pairs > (1u << 24)) return bad(who, "chunk_pairs must be in [1, 16 777 216]");
  if (B == 0) return RKH_OK;
  if (!points || !path_ptr || !keep || !n_keep || !time_out) return bad(who, "a required pointer is NULL");
  std::vector<uint32_t> pair_ptr;
  RKH_TRY(shortcut_layout(who, path_ptr, B, max_span, &pair_ptr));
  const uint32_t D = 2 * uint32_t(sp.n);
  const uint32_t n_pts = path_ptr[B], E = pair_ptr[B];
  for (size_t k = 0; k < size_t(n_pts) * D; ++k)
    if (!std::isfinite(points[k])) return bad(who, "a point has a coordinate that is not finite");
  if (!scene) return bad(who, "scene is NULL");
  rkh_ctx* ctx = scene->ctx;
  hipStream_t s = ctx->stream;
  RKH_HIP(hipSetDevice(ctx->device));
  const uint32_t chunk = std::min(E, chunk_pairs);
  const size_t ws_bytes = svp_walk_layout(sp.n, chunk, false, nullptr, nullptr) + kArenaGuardBytes;

  StagedCall call(s);  // (pair_ptr was declared before it)
  const double* d_pts = call.in(points, size_t(n_pts) * D);
  const uint32_t* d_path_ptr = call.in(path_ptr, size_t(B) + 1);
  const uint32_t* d_pair_ptr = call.in(pair_ptr.data(), size_t(B) + 1);
  double* d_T = call.scratch<double>(E, 1);
  uint8_t* d_reached = call.scratch<uint8_t>(E, 1);
  char* d_ws = call.scratch<char>(ws_bytes);
  double* d_tin = call.out(time_in, B);
  ShortcutDpArgs dp;
  dp.path_ptr = d_path_ptr;
  dp.pair_ptr = d_pair_ptr;
  dp.B = B;
  dp.max_span = max_span;
  dp.acc = d_reached;
  dp.w = d_T;
  dp.ok_mask = 0xFFu;  // the walk's `reached` byte is the strict verdict
  dp.min_interval = 0.0;
  dp.keep = call.out(keep, n_pts, 0, 0xFF);  // the slots behind n_keep hold 0xFFFFFFFF
  dp.n_keep = call.out(n_keep, B);
  dp.cost_out = call.out(time_out, B);
  dp.n_blocked = call.out(n_blocked, B);
  RKH_TRY(call.status());
  SvpWalk w;
  svp_walk_layout(sp.n, chunk, false, d_ws, &w);

  hipEvent_t ev[2] = {nullptr, nullptr};
  struct Events {  // (the stream is idle wherever this scope is left: launch_svp_walk and StagedCall wait for it)
    hipEvent_t* ev;
    ~Events() {
      for (int k = 0; k < 2; ++k)
        if (ev[k]) (void)hipEventDestroy(ev[k]);
    }
  } events{ev};
  if (ms)
    for (auto& e : ev) RKH_HIP(hipEventCreate(&e));
  // one phase, and into *acc (if not null) its time between two events
  auto timed = [&](float* acc, auto&& launch) -> rkh_status {
    if (!acc) return launch();
    RKH_HIP(hipEventRecord(ev[0], s));
    RKH_TRY(launch());
    RKH_HIP(hipEventRecord(ev[1], s));
    RKH_HIP(hipEventSynchronize(ev[1]));
    float t = 0.0f;
    RKH_HIP(hipEventElapsedTime(&t, ev[0], ev[1]));
    *acc += t;
    return RKH_OK;
  };
  auto sequence = [&](float* t3) -> rkh_status {
    for (uint32_t first = 0; first < E; first += chunk) {
      const uint32_t count = std::min(chunk, E - first);
      w.B = count;
      w.T = d_T + first;
      w.reached = d_reached + first;
      RKH_TRY(timed(t3 ? t3 + 0 : nullptr, [&]() -> rkh_status {
        hipLaunchKernelGGL(rl1cut_pairs_kernel, dim3((count + kSvpCutThreads - 1) / kSvpCutThreads), dim3(kSvpCutThreads), 0, s,
                           d_pts, D, d_path_ptr, d_pair_ptr, B, max_span, first, count, const_cast<double*>(w.a),
                           const_cast<double*>(w.b));
        RKH_HIP(hipGetLastError());
        return RKH_OK;
      }));
      RKH_TRY(timed(t3 ? t3 + 1 : nullptr, [&]() { return launch_svp_walk(who, *scene, sp, w, nullptr); }));
    }
    return timed(t3 ? t3 + 2 : nullptr, [&]() -> rkh_status {
      hipLaunchKernelGGL(rl1cut_time_in_kernel, dim3((B + kSvpCutThreads - 1) / kSvpCutThreads), dim3(kSvpCutThreads), 0, s,
                         d_path_ptr, d_pair_ptr, B, max_span, d_T, d_tin);
      RKH_HIP(hipGetLastError());
      return launch_shortcut_dp(s, dp);
    });
  };
  RKH_TRY(sequence(nullptr));
  for (uint32_t r = 0; ms && r < runs; ++r) {
    ms[size_t(r) * 3 + 0] = ms[size_t(r) * 3 + 1] = ms[size_t(r) * 3 + 2] = 0.0f;
    RKH_TRY(sequence(ms + size_t(r) * 3));
  }
  RKH_TRY(call.fetch());
  // A goal no allowed hop sequence reaches: the points are not a trajectory.  The search leaves the one-vertex predecessor
  // walk {L - 1} there; the definition asks for no vertex at all.
  for (uint32_t b = 0; b < B; ++b)
    if (std::isinf(time_out[b])) {
      n_keep[b] = 0;
      if (n_blocked) n_blocked[b] = 0;
      for (uint32_t v = path_ptr[b]; v < path_ptr[b + 1]; ++v) keep[v] = kShortcutNil;
    }
  return RKH_OK;
}

}  // namespace
}  // namespace rkh

using namespace rkh;

extern "C" {

rkh_status rkh_svp_shortcut_paths(rkh_scene* scene, const rkh_svp_space* space, const double* points, const uint32_t* path_ptr,
                                  uint32_t B, uint32_t max_span, uint32_t* keep, uint32_t* n_keep, double* time_in,
                                  double* time_out, uint32_t* n_blocked) {
  return svp_shortcut_run("rkh_svp_shortcut_paths", scene, space, points, path_ptr, B, max_span, kSvpCutChunk, keep, n_keep,
                          time_in, time_out, n_blocked, 0, nullptr);
}

rkh_status rkh_diag_svp_shortcut_chunked(rkh_scene* scene, const rkh_svp_space* space, const double* points,
                                         const uint32_t* path_ptr, uint32_t B, uint32_t max_span, uint32_t chunk_pairs,
                                         uint32_t* keep, uint32_t* n_keep, double* time_in, double* time_out,
                                         uint32_t* n_blocked) {
  return svp_shortcut_run("rkh_diag_svp_shortcut_chunked", scene, space, points, path_ptr, B, max_span, chunk_pairs, keep,
                          n_keep, time_in, time_out, n_blocked, 0, nullptr);
}

rkh_status rkh_diag_svp_shortcut_ms(rkh_scene* scene, const rkh_svp_space* space, const double* points, const uint32_t* path_ptr,
                                    uint32_t B, uint32_t max_span, uint32_t runs, float* ms) {
  if (!scene || !space || !points || !path_ptr || !ms || B == 0 || runs == 0) return RKH_ERR_BAD_ARG;
  std::vector<uint32_t> keep(path_ptr[B]), n_keep(B);
  std::vector<double> time_out(B);
  return svp_shortcut_run("rkh_diag_svp_shortcut_ms", scene, space, points, path_ptr, B, max_span, kSvpCutChunk, keep.data(),
                          n_keep.data(), nullptr, time_out.data(), nullptr, runs, ms);
}

}  // extern "C"
