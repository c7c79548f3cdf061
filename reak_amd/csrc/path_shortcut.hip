// path_shortcut.hip -- shortcutting of solution paths as a batch operation (the definitions are at rkh_shortcut_paths in
// include/rkh.h; the index rules in path_shortcut.h).  Three launches serve B paths:
//   1. shortcut_pairs_kernel   one thread per candidate pair (i, j) of the whole batch: its two rows of the concatenated
//                              point table (EdgeIO::src_idx / tgt_idx) and its weight w(i, j), the left-to-right fp64
//                              euclidean norm the walk kernels compute (norm_n); the thread of a path's first pair also
//                              sums the path's consecutive hops (cost_in).
//   2. launch_edge_check       ONE quasi-static walk launch over all pairs, EDGE_STEER_BOTH: bit 1 of the accept byte =
//                              the predicate loop ran to its end.  The walk kernels are the ones every planner uses.
//   3. shortcut_dp_kernel      one workgroup per path: the shortest path through the visibility DAG, exactly.
// A module of its own: a kernel added to an existing module moves the code of the ones it holds.
//
// The search.  dist[0] = 0, dist[j] = min over allowed i < j of dist[i] + w(i, j), the lowest i winning ties.  Vertices
// are settled in index order (every hop goes up), so for i = 0, 1, ... the owner of vertex i publishes dist[i] -- final,
// all its predecessors are below it -- through LDS, one barrier, and every owner of a j > i within the span relaxes its
// vertex with that ONE fp64 addition under strict <.  Thread t owns the vertices t, t + 256, t + 512, t + 768 and keeps
// their (best, pred) in registers; no reduction, no atomics, and i ascends for every j, so the result is bit for bit
// the sequential double loop's.  The published value alternates between two LDS words: the word of step i is rewritten
// in step i + 2, which every thread enters only after the barrier of step i + 1, behind its read of step i.  The weights
// and verdicts of row i + 1 are loaded before the barrier of step i (they do not depend on any distance).
// Then the predecessor walk (one thread, through LDS), and in parallel the kept vertices and the count of kept hops whose
// strict verdict is false.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "path_shortcut.h"
#include "rkh_internal.h"
#include "staged_call.h"

namespace rkh {

namespace {
constexpr int kShortcutThreads = 256;
constexpr int kShortcutSlots = int(kShortcutMaxPoints) / kShortcutThreads;  // vertices a thread of the search owns
}  // namespace

__global__ __launch_bounds__(kShortcutThreads) void shortcut_pairs_kernel(
    const double* __restrict__ points, int n, const uint32_t* __restrict__ path_ptr, const uint32_t* __restrict__ pair_ptr,
    uint32_t B, uint32_t max_span, uint32_t* __restrict__ src_idx, uint32_t* __restrict__ tgt_idx, double* __restrict__ w,
    double* __restrict__ cost_in) {
  const uint32_t g = blockIdx.x * uint32_t(kShortcutThreads) + threadIdx.x;
  if (g >= pair_ptr[B]) return;
  const uint32_t b = segment_of(pair_ptr, B, g);  // (paths of one point own no pair and are never returned)
  const uint32_t first = path_ptr[b], L = path_ptr[b + 1] - first;
  uint32_t i, j;
  shortcut_pair_at(L, max_span, g - pair_ptr[b], &i, &j);
  auto hop = [&](uint32_t u, uint32_t v) {  // |p_u - p_v|: s = s + d * d in coordinate order, one sqrt
    const double* pu = points + uint64_t(first + u) * n;
    const double* pv = points + uint64_t(first + v) * n;
    double s = 0.0;
    for (int d = 0; d < n; ++d) {
      const double diff = pu[d] - pv[d];
      s = s + diff * diff;
    }
    return sqrt(s);
  };
  src_idx[g] = first + i;
  tgt_idx[g] = first + j;
  w[g] = hop(i, j);
  if (g == pair_ptr[b] && cost_in) {  // the path's first pair: the input cost, summed left to right
    double c = 0.0;
    for (uint32_t v = 0; v + 1 < L; ++v) c = c + hop(v, v + 1);
    cost_in[b] = c;
  }
}

// (ShortcutDpArgs, the arguments of one launch of the search: rkh_internal.h -- svp_shortcut.hip launches it as well)
__global__ __launch_bounds__(kShortcutThreads) void shortcut_dp_kernel(ShortcutDpArgs a) {
  __shared__ double s_pub[2];
  __shared__ uint32_t s_pred[kShortcutMaxPoints];
  __shared__ uint32_t s_rev[kShortcutMaxPoints];
  __shared__ uint32_t s_n;
  const uint32_t b = blockIdx.x;
  if (b >= a.B) return;  // (block-uniform)
  const uint32_t first = a.path_ptr[b], L = a.path_ptr[b + 1] - first;  // 1 <= L <= kShortcutMaxPoints (the host checked)
  const uint32_t span = shortcut_span(L, a.max_span);
  const uint32_t tid = threadIdx.x;
  const uint8_t* __restrict__ acc = a.acc + a.pair_ptr[b];
  const double* __restrict__ w = a.w + a.pair_ptr[b];
  const uint32_t ok_mask = a.ok_mask;
  const double min_interval = a.min_interval;
  auto verdict = [&](uint32_t p, double wp) { return (uint32_t(acc[p]) & ok_mask) != 0u || wp < min_interval; };

  double best[kShortcutSlots];
  uint32_t pred[kShortcutSlots];
#pragma unroll
  for (int k = 0; k < kShortcutSlots; ++k) {
    best[k] = INFINITY;
    pred[k] = kShortcutNil;
  }
  if (tid == 0) best[0] = 0.0;
  // weight and verdict of (i, j) for this thread's vertices j; outside row i: +inf and false (never taken)
  auto load_row = [&](uint32_t i, double* wv, bool* okv) {
    const uint32_t row = shortcut_pair_index(L, a.max_span, i, i + 1);
    const uint32_t j_max = (i + span < L - 1) ? i + span : L - 1;
#pragma unroll
    for (int k = 0; k < kShortcutSlots; ++k) {
      const uint32_t j = tid + uint32_t(k) * kShortcutThreads;
      wv[k] = INFINITY;
      okv[k] = false;
      if (j > i && j <= j_max) {
        const uint32_t p = row + (j - i - 1);
        wv[k] = w[p];
        okv[k] = verdict(p, wv[k]);
      }
    }
  };
  double w_cur[kShortcutSlots], w_next[kShortcutSlots];
  bool ok_cur[kShortcutSlots], ok_next[kShortcutSlots];
#pragma unroll
  for (int k = 0; k < kShortcutSlots; ++k) {
    w_cur[k] = w_next[k] = INFINITY;
    ok_cur[k] = ok_next[k] = false;
  }
  if (L > 1) load_row(0, w_cur, ok_cur);
  for (uint32_t i = 0; i + 1 < L; ++i) {  // (block-uniform bounds)
    if (i + 2 < L) load_row(i + 1, w_next, ok_next);
    if (tid == (i & uint32_t(kShortcutThreads - 1))) {  // the owner of vertex i publishes its distance
      const uint32_t slot = i / kShortcutThreads;
      double v = best[0];
#pragma unroll
      for (int k = 1; k < kShortcutSlots; ++k)
        if (slot == uint32_t(k)) v = best[k];
      s_pub[i & 1u] = v;
    }
    __syncthreads();
    const double d_i = s_pub[i & 1u];
#pragma unroll
    for (int k = 0; k < kShortcutSlots; ++k) {
      const uint32_t j = tid + uint32_t(k) * kShortcutThreads;
      const double c = d_i + w_cur[k];
      if (j > i && shortcut_allowed(i, j, span, ok_cur[k]) && c < best[k]) {
        best[k] = c;
        pred[k] = i;
      }
      w_cur[k] = w_next[k];
      ok_cur[k] = ok_next[k];
    }
  }
#pragma unroll
  for (int k = 0; k < kShortcutSlots; ++k) {
    const uint32_t j = tid + uint32_t(k) * kShortcutThreads;
    if (j < L) s_pred[j] = pred[k];
    if (j == L - 1) a.cost_out[b] = best[k];
  }
  __syncthreads();
  if (tid == 0) s_n = shortcut_walk(s_pred, L, s_rev);
  __syncthreads();
  const uint32_t n = s_n;
  for (uint32_t k = tid; k < n; k += kShortcutThreads) a.keep[first + (n - 1 - k)] = s_rev[k];
  // hops of the returned path whose strict verdict is false (hop k: s_rev[k + 1] -> s_rev[k], a candidate pair)
  uint32_t blocked = 0;
  for (uint32_t base = 0; base + 1 < n; base += kShortcutThreads) {  // (block-uniform bounds)
    const uint32_t k = base + tid;
    bool bad = false;
    if (k + 1 < n) {
      const uint32_t p = shortcut_pair_index(L, a.max_span, s_rev[k + 1], s_rev[k]);
      bad = !verdict(p, w[p]);
    }
    blocked += uint32_t(__syncthreads_count(bad ? 1 : 0));
  }
  if (tid == 0) {
    a.n_keep[b] = n;
    if (a.n_blocked) a.n_blocked[b] = blocked;
  }
}

// The pair offsets of B paths, and everything the entry points check about path_ptr before anything is launched.
rkh_status shortcut_layout(const char* who, const uint32_t* path_ptr, uint32_t B, uint32_t max_span,
                           std::vector<uint32_t>* pair_ptr) {
  if (path_ptr[0] != 0) {
    set_error(std::string(who) + ": path_ptr must ascend from 0");
    return RKH_ERR_BAD_ARG;
  }
  for (uint32_t b = 0; b < B; ++b)
    if (path_ptr[b + 1] <= path_ptr[b]) {
      set_error(std::string(who) + ": path_ptr must ascend from 0 and no path may be empty");
      return RKH_ERR_BAD_ARG;
    }
  pair_ptr->assign(size_t(B) + 1, 0u);
  uint64_t total = 0;
  for (uint32_t b = 0; b < B; ++b) {
    const uint32_t L = path_ptr[b + 1] - path_ptr[b];
    if (L > kShortcutMaxPoints) {
      set_error(std::string(who) + ": a path of more than " + std::to_string(kShortcutMaxPoints) + " points");
      return RKH_ERR_CAPACITY;
    }
    total += shortcut_pair_count(L, max_span);
    if (total > kShortcutMaxPairs) {
      set_error(std::string(who) + ": more than " + std::to_string(kShortcutMaxPairs) + " candidate pairs (lower max_span)");
      return RKH_ERR_CAPACITY;
    }
    (*pair_ptr)[b + 1] = uint32_t(total);
  }
  return RKH_OK;
}

rkh_status launch_shortcut_dp(hipStream_t s, const ShortcutDpArgs& a) {
  if (a.B == 0) return RKH_OK;
  hipLaunchKernelGGL(shortcut_dp_kernel, dim3(a.B), dim3(kShortcutThreads), 0, s, a);
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

namespace {

// rkh_shortcut_paths, and with ms != null its three launches timed `runs` times between events after one warm-up
// (rkh_diag_shortcut_ms): ms[r][0..2] = pairs, walks, search.
rkh_status shortcut_run(const char* who, rkh_scene* scene, const rkh_qs_space* space, const double* points,
                        const uint32_t* path_ptr, uint32_t B, uint32_t max_span, uint32_t* keep, uint32_t* n_keep,
                        double* cost_in, double* cost_out, uint32_t* n_blocked, uint32_t runs, float* ms) {
  if (!scene || !space) return RKH_ERR_BAD_ARG;
  if (B == 0) return RKH_OK;
  if (!points || !path_ptr || !keep || !n_keep || !cost_out) return RKH_ERR_BAD_ARG;
  const int n = scene->host.n_dof;
  if (space->n_dof != n) {
    set_error(std::string(who) + ": rkh_qs_space.n_dof does not match the scene");
    return RKH_ERR_BAD_ARG;
  }
  if (!(space->min_interval > 0.0)) {
    set_error("rkh_qs_space: min_interval must be positive");
    return RKH_ERR_BAD_ARG;
  }
  std::vector<uint32_t> pair_ptr;
  RKH_TRY(shortcut_layout(who, path_ptr, B, max_span, &pair_ptr));
  const uint32_t T = path_ptr[B], E = pair_ptr[B];
  for (size_t k = 0; k < size_t(T) * n; ++k)
    if (!std::isfinite(points[k])) {
      set_error(std::string(who) + ": a point has a coordinate that is not finite");
      return RKH_ERR_BAD_ARG;
    }
  QsDev qs;
  std::memset(&qs, 0, sizeof(qs));
  qs.min_interval = space->min_interval;
  qs.fraction = 1.0;
  qs_set_speed(qs, space->speed_limits, n);
  for (int d = 0; d < n; ++d) {
    qs.lower[d] = space->lower[d];
    qs.upper[d] = space->upper[d];
  }
  hipStream_t s = scene->ctx->stream;
  // per pair: two row indices, the weight, the verdict byte, and what every walk writes (end point, points tested):
  // 8 n + 25 bytes.  A call that does not fit the device's memory is refused with RKH_ERR_OOM (rkh.h says so).
  StagedCall call(s);  // (pair_ptr was declared before it)
  const double* d_pts = call.in(points, size_t(T) * n);
  const uint32_t* d_path_ptr = call.in(path_ptr, size_t(B) + 1);
  const uint32_t* d_pair_ptr = call.in(pair_ptr.data(), size_t(B) + 1);
  uint32_t* d_src = call.scratch<uint32_t>(E, 1);
  uint32_t* d_tgt = call.scratch<uint32_t>(E, 1);
  double* d_w = call.scratch<double>(E, 1);
  double* d_cin = call.out(cost_in, B, 0, 0);  // a path of one point has no pair: its input cost is 0

  EdgeIO io;  // pair e walks row src_idx[e] -> row tgt_idx[e] of the one point table
  io.src = d_pts;
  io.src_idx = d_src;
  io.src_stride = uint32_t(n);
  io.tgt = d_pts;
  io.tgt_idx = d_tgt;
  io.tgt_stride = uint32_t(n);
  io.B = E;
  io.x_out = call.scratch<double>(size_t(E) * n, n);
  io.steps_free = call.scratch<uint32_t>(E, 1);
  io.accept = call.scratch<uint8_t>(E, 1, 0);
  io.mode = EDGE_STEER_BOTH;
  io.err_flag = scene->d_err.get();
  ShortcutDpArgs dp;
  dp.path_ptr = d_path_ptr;
  dp.pair_ptr = d_pair_ptr;
  dp.B = B;
  dp.max_span = max_span;
  dp.acc = io.accept;
  dp.w = d_w;
  dp.ok_mask = 2u;  // EDGE_STEER_BOTH: the walk ran to its end
  dp.min_interval = space->min_interval;
  dp.keep = call.out(keep, T, 0, 0xFF);  // the slots behind n_keep hold 0xFFFFFFFF
  dp.n_keep = call.out(n_keep, B);
  dp.cost_out = call.out(cost_out, B);
  dp.n_blocked = call.out(n_blocked, B);
  RKH_TRY(call.status());
  auto launch_pairs = [&]() -> rkh_status {
    if (E == 0) return RKH_OK;
    hipLaunchKernelGGL(shortcut_pairs_kernel, dim3((E + kShortcutThreads - 1) / kShortcutThreads), dim3(kShortcutThreads), 0, s,
                       d_pts, n, d_path_ptr, d_pair_ptr, B, max_span, d_src, d_tgt, d_w, d_cin);
    RKH_HIP(hipGetLastError());
    return RKH_OK;
  };
  auto launch_walks = [&]() { return launch_edge_check(s, *scene, qs, io, E); };
  auto launch_search = [&]() { return launch_shortcut_dp(s, dp); };
  RKH_TRY(launch_pairs());
  RKH_TRY(launch_walks());
  RKH_TRY(launch_search());
  if (ms) {  // the launches above were the warm-up
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    for (auto& e : ev) RKH_HIP(hipEventCreate(&e));
    rkh_status st = RKH_OK;
    for (uint32_t r = 0; st == RKH_OK && r < runs; ++r) {
      hipError_t e = hipEventRecord(ev[0], s);
      if (e == hipSuccess) st = launch_pairs();
      if (e == hipSuccess) e = hipEventRecord(ev[1], s);
      if (e == hipSuccess && st == RKH_OK) st = launch_walks();
      if (e == hipSuccess) e = hipEventRecord(ev[2], s);
      if (e == hipSuccess && st == RKH_OK) st = launch_search();
      if (e == hipSuccess) e = hipEventRecord(ev[3], s);
      if (e == hipSuccess) e = hipEventSynchronize(ev[3]);
      for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipEventElapsedTime(&ms[size_t(r) * 3 + k], ev[k], ev[k + 1]);
      if (e != hipSuccess && st == RKH_OK) {
        set_error(std::string(who) + ": " + hipGetErrorString(e));
        st = RKH_ERR_DEVICE;
      }
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    RKH_TRY(st);
  }
  return call.fetch();
}

}  // namespace
}  // namespace rkh

using namespace rkh;

extern "C" {

rkh_status rkh_shortcut_paths(rkh_scene* scene, const rkh_qs_space* space, const double* points, const uint32_t* path_ptr,
                              uint32_t B, uint32_t max_span, uint32_t* keep, uint32_t* n_keep, double* cost_in,
                              double* cost_out, uint32_t* n_blocked) {
  return shortcut_run("rkh_shortcut_paths", scene, space, points, path_ptr, B, max_span, keep, n_keep, cost_in, cost_out,
                      n_blocked, 0, nullptr);
}

rkh_status rkh_diag_shortcut_ms(rkh_scene* scene, const rkh_qs_space* space, const double* points, const uint32_t* path_ptr,
                                uint32_t B, uint32_t max_span, uint32_t runs, float* ms) {
  if (!scene || !space || !points || !path_ptr || !ms || B == 0 || runs == 0) return RKH_ERR_BAD_ARG;
  std::vector<uint32_t> keep(path_ptr[B]), n_keep(B);
  std::vector<double> cost_out(B);
  return shortcut_run("rkh_diag_shortcut_ms", scene, space, points, path_ptr, B, max_span, keep.data(), n_keep.data(), nullptr,
                      cost_out.data(), nullptr, runs, ms);
}

rkh_status rkh_diag_shortcut_dp(rkh_ctx* ctx, const uint32_t* path_ptr, uint32_t B, uint32_t max_span, const uint8_t* ok,
                                const double* w, uint32_t* keep, uint32_t* n_keep, double* cost_out, uint32_t* n_blocked) {
  if (!ctx) return RKH_ERR_BAD_ARG;
  if (B == 0) return RKH_OK;
  if (!path_ptr || !keep || !n_keep || !cost_out) return RKH_ERR_BAD_ARG;
  std::vector<uint32_t> pair_ptr;
  RKH_TRY(shortcut_layout("rkh_diag_shortcut_dp", path_ptr, B, max_span, &pair_ptr));
  const uint32_t T = path_ptr[B], E = pair_ptr[B];
  if (E && (!ok || !w)) return RKH_ERR_BAD_ARG;
  for (uint32_t e = 0; e < E; ++e)
    if (!(w[e] >= 0.0) || std::isinf(w[e])) {
      set_error("rkh_diag_shortcut_dp: weights must be finite and >= 0");
      return RKH_ERR_BAD_ARG;
    }
  hipStream_t s = ctx->stream;
  StagedCall call(s);  // (pair_ptr was declared before it)
  ShortcutDpArgs dp;
  dp.path_ptr = call.in(path_ptr, size_t(B) + 1);
  dp.pair_ptr = call.in(pair_ptr.data(), size_t(B) + 1);
  dp.B = B;
  dp.max_span = max_span;
  dp.acc = call.in(ok, E, 1);
  dp.w = call.in(w, E, 1);
  dp.ok_mask = 0xFFu;  // any non-zero byte is a true verdict
  dp.min_interval = 0.0;
  dp.keep = call.out(keep, T, 0, 0xFF);  // the slots behind n_keep hold 0xFFFFFFFF
  dp.n_keep = call.out(n_keep, B);
  dp.cost_out = call.out(cost_out, B);
  dp.n_blocked = call.out(n_blocked, B);
  RKH_TRY(call.status());
  RKH_TRY(launch_shortcut_dp(s, dp));
  return call.fetch();
}

}  // extern "C"
