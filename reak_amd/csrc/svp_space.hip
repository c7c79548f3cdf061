// svp_space.hip -- the order-1 rate-limited joint space with SVP profiles (svp_device.h) on the device: reach time,
// nearest neighbours under the reach-time metric, the collision-tested edge walk and the profile sampled as a trajectory.
//
// Kernels (none reads a scene; the walk stages its points around rkh::launch_min_distance, which serves every scene kind):
//   svp_reach_kernel         one lane per pair: T and the peak velocities of the common-time solve
//   svp_nearest_kernel       one workgroup per (query, slice of the points): every lane solves whole pairs into an LDS
//                            array of the slice's distances, then the block draws its k smallest in (distance, index) order
//   svp_nearest_merge_kernel one workgroup per query: k-way merge of the slices' sorted lists
//   svp_walk_solve_kernel    one lane per edge: T, peaks, dt = T fraction, the point count of the loop; edges without a
//                            point finish here, the others enter the live list
//   svp_walk_points_kernel   one lane per (live edge, point of the pass): the point in space coordinates and model units,
//                            and its bounds verdict
//   svp_walk_scan_kernel     one lane per live edge: the pass's verdicts in order; first failure, last good point, count;
//                            unfinished edges enter the next pass's list
//   svp_interp_kernel        one lane per (pair, time)
// The walk's launches are launch_svp_walk (rkh_internal.h), over device rows and a caller-owned workspace: rkh_svp_edge_check
// wraps it with the arena and the copies, the batch RRT (svp_planner.hip) calls it on its own rows.
#include <cmath>
#include <cstring>

#include "rkh_internal.h"
#include "staged_call.h"
#include "svp_device.h"

namespace rkh {
namespace {

constexpr uint32_t kSvpThreads = 256;
constexpr uint32_t kSvpSliceMin = 256;    // points of a slice of the nearest sweep: a multiple of 256 in [256, 4096],
constexpr uint32_t kSvpSliceMax = 4096;   // chosen by svp_slice() (one double of LDS per point)
constexpr uint32_t kSvpMaxSlices = 4096;  // slices the merge kernel keeps a cursor for
constexpr uint32_t kSvpMaxK = 64;
constexpr uint32_t kSvpPass = 32;              // points per live edge and pass of the walk
constexpr uint32_t kSvpMaxPoints = 1u << 20;   // tested points of one edge (a walk that would test more is refused)
constexpr uint32_t kNoIndex = 0xFFFFFFFFu;

// Points per slice: the sweep should offer about 2048 workgroups (8 per compute unit) where the work allows it -- one
// query over 100 000 points runs as 391 slices of 256 -- and large launches take the largest slice, so that the merge
// stays small.
uint32_t svp_slice(uint64_t n_pts, uint32_t B) {
  const uint64_t per = (n_pts * B + 2047) / 2048;
  uint64_t slice = (per + kSvpSliceMin - 1) / kSvpSliceMin * kSvpSliceMin;
  slice = std::min<uint64_t>(std::max<uint64_t>(slice, kSvpSliceMin), kSvpSliceMax);
  return uint32_t(slice);
}

__global__ __launch_bounds__(256) void svp_reach_kernel(const SvpDev sp, const double* __restrict__ a,
                                                        const double* __restrict__ b, uint32_t B, double* __restrict__ time,
                                                        double* __restrict__ peak) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B) return;
  const size_t row = size_t(e) * 2 * sp.n;
  time[e] = svp_reach(sp, a + row, b + row, peak ? peak + size_t(e) * sp.n : nullptr);
}

__device__ __forceinline__ bool svp_less(double d1, uint32_t i1, double d2, uint32_t i2) {
  return (d1 < d2) || (d1 == d2 && i1 < i2);
}

// smallest (d, i) of the block, with the value v that travels with it; every lane returns it.  red: 4 x (double, 2 x uint32)
__device__ __forceinline__ void svp_block_min(double& d, uint32_t& i, uint32_t& v, double* red_d, uint32_t* red_i) {
  for (int m = 32; m >= 1; m >>= 1) {
    const double od = __shfl_xor(d, m, 64);
    const uint32_t oi = __shfl_xor(i, m, 64), ov = __shfl_xor(v, m, 64);
    if (svp_less(od, oi, d, i)) d = od, i = oi, v = ov;
  }
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red_d[wave] = d, red_i[2 * wave] = i, red_i[2 * wave + 1] = v;
  __syncthreads();
  d = red_d[0], i = red_i[0], v = red_i[1];
  for (uint32_t w = 1; w < kSvpThreads / 64; ++w)
    if (svp_less(red_d[w], red_i[2 * w], d, i)) d = red_d[w], i = red_i[2 * w], v = red_i[2 * w + 1];
  __syncthreads();
}

// grid (n_slices, B).  LDS: [slice] distances, [2 n] query, the reduction's 4 x 16 bytes.
// part_dist / part_idx: [B][n_slices][k], ascending by (distance, index), padded with (+inf, kNoIndex).
__global__ __launch_bounds__(256) void svp_nearest_kernel(const SvpDev sp, const double* __restrict__ pts, uint32_t n_pts,
                                                          const double* __restrict__ queries, uint32_t slice, uint32_t k,
                                                          int direction, double* __restrict__ part_dist,
                                                          uint32_t* __restrict__ part_idx) {
  extern __shared__ double svp_lds[];
  double* dist = svp_lds;
  double* qv = dist + slice;
  double* red_d = qv + 2 * kSvpMaxDof;
  uint32_t* red_i = reinterpret_cast<uint32_t*>(red_d + 4);
  const uint32_t tid = threadIdx.x, s = blockIdx.x, q = blockIdx.y;
  const uint32_t D = 2 * uint32_t(sp.n);
  if (tid < D) qv[tid] = queries[size_t(q) * D + tid];
  __syncthreads();
  const uint32_t base = s * slice;
  for (uint32_t j = tid; j < slice; j += kSvpThreads) {
    const uint32_t g = base + j;
    double d = INFINITY;
    if (g < n_pts) {
      const double* p = pts + size_t(g) * D;
      d = direction ? svp_reach(sp, qv, p, nullptr) : svp_reach(sp, p, qv, nullptr);
    }
    dist[j] = d;
  }
  __syncthreads();
  double prev_d = -1.0;  // every distance is >= 0: all entries come after (-1, 0)
  uint32_t prev_j = 0;
  bool more = true;
  const size_t out = (size_t(q) * gridDim.x + s) * k;
  for (uint32_t r = 0; r < k; ++r) {
    double bd = INFINITY;
    uint32_t bj = kNoIndex, unused = 0;
    if (more) {
      for (uint32_t j = tid; j < slice; j += kSvpThreads) {
        const double d = dist[j];
        if (d < INFINITY && svp_less(prev_d, prev_j, d, j) && svp_less(d, j, bd, bj)) bd = d, bj = j;
      }
      svp_block_min(bd, bj, unused, red_d, red_i);
      more = bd < INFINITY;
      prev_d = bd, prev_j = bj;
    }
    if (tid == 0) part_dist[out + r] = bd, part_idx[out + r] = more ? base + bj : kNoIndex;
  }
}

// grid (B).  LDS: [n_slices] cursors (uint32), the reduction's 4 x 16 bytes.
__global__ __launch_bounds__(256) void svp_nearest_merge_kernel(const double* __restrict__ part_dist,
                                                                const uint32_t* __restrict__ part_idx, uint32_t n_slices,
                                                                uint32_t k, uint32_t* __restrict__ idx,
                                                                double* __restrict__ dist) {
  extern __shared__ double svp_lds[];
  double* red_d = svp_lds;
  uint32_t* red_i = reinterpret_cast<uint32_t*>(red_d + 4);
  uint32_t* head = red_i + 8;
  const uint32_t tid = threadIdx.x, q = blockIdx.x;
  for (uint32_t s = tid; s < n_slices; s += kSvpThreads) head[s] = 0;
  __syncthreads();
  const size_t in = size_t(q) * n_slices * k;
  bool more = true;
  for (uint32_t r = 0; r < k; ++r) {
    double bd = INFINITY;
    uint32_t bi = kNoIndex, bs = 0;
    if (more) {
      for (uint32_t s = tid; s < n_slices; s += kSvpThreads) {
        const uint32_t h = head[s];
        if (h < k) {
          const double d = part_dist[in + size_t(s) * k + h];
          const uint32_t i = part_idx[in + size_t(s) * k + h];
          if (d < INFINITY && svp_less(d, i, bd, bi)) bd = d, bi = i, bs = s;
        }
      }
      svp_block_min(bd, bi, bs, red_d, red_i);
      more = bd < INFINITY;
      if (more && tid == 0) head[bs] += 1;
      __syncthreads();
    }
    if (tid == 0) dist[size_t(q) * k + r] = bd, idx[size_t(q) * k + r] = more ? bi : kNoIndex;
  }
}

// ---- the walk -----------------------------------------------------------------------------------------------------------
// (SvpWalk, the workspace the three kernels share: rkh_internal.h)
__device__ __forceinline__ double svp_fraction(const SvpWalk& w, uint32_t e) { return w.fraction ? w.fraction[e] : 1.0; }

// what the walk returns after its loop: b, a, or the (untested) point at dt
__device__ __forceinline__ void svp_walk_finish(const SvpDev& sp, const SvpWalk& w, uint32_t e) {
  const uint32_t D = 2 * uint32_t(sp.n);
  const double* a = w.a + size_t(e) * D;
  const double* b = w.b + size_t(e) * D;
  double* out = w.out + size_t(e) * D;
  const double f = svp_fraction(w, e);
  if (f == 1.0) {
    for (uint32_t c = 0; c < D; ++c) out[c] = b[c];
  } else if (f == 0.0) {
    for (uint32_t c = 0; c < D; ++c) out[c] = a[c];
  } else {
    svp_point(sp, a, b, w.peak + size_t(e) * sp.n, w.T[e], w.dt[e], out, nullptr);
  }
  w.reached[e] = 1;
}

__global__ __launch_bounds__(256) void svp_walk_solve_kernel(const SvpDev sp, const SvpWalk w) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= w.B) return;
  const uint32_t D = 2 * uint32_t(sp.n);
  const double* a = w.a + size_t(e) * D;
  const double T = svp_reach(sp, a, w.b + size_t(e) * D, w.peak + size_t(e) * sp.n);
  w.T[e] = T;
  w.n_checked[e] = 0;
  w.reached[e] = 0;
  bool over = false;
  uint32_t K = 0;
  double dt = 0.0;
  if (T < INFINITY) {
    dt = T * svp_fraction(w, e);
    K = svp_count_points(sp.min_interval, dt, kSvpMaxPoints, &over);
  }
  if (!(T < INFINITY) || over) {
    for (uint32_t c = 0; c < D; ++c) w.out[size_t(e) * D + c] = a[c];
    if (over) atomicOr(&w.counters[2], 1u);
    return;
  }
  w.dt[e] = dt;
  w.K[e] = K;
  w.k_done[e] = 0;
  w.d_next[e] = sp.min_interval;
  if (K == 0) {
    svp_walk_finish(sp, w, e);
    return;
  }
  for (uint32_t c = 0; c < D; ++c) w.last[size_t(e) * D + c] = a[c];
  w.list[0][atomicAdd(&w.counters[0], 1u)] = e;
}

__global__ __launch_bounds__(256) void svp_walk_points_kernel(const SvpDev sp, const SvpWalk w, uint32_t cur, uint32_t live) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= live * kSvpPass) return;
  const uint32_t e = w.list[cur][i / kSvpPass], j = i % kSvpPass;
  const uint32_t D = 2 * uint32_t(sp.n);
  const double* a = w.a + size_t(e) * D;
  double* x = w.pts + size_t(i) * D;
  double* xm = w.pts_model + size_t(i) * D;
  if (w.k_done[e] + j < w.K[e]) {
    double d = w.d_next[e];
    for (uint32_t c = 0; c < j; ++c) d += sp.min_interval;
    svp_point(sp, a, w.b + size_t(e) * D, w.peak + size_t(e) * sp.n, w.T[e], d, x, xm);
    w.inb[i] = svp_in_bounds(sp, x) ? 1 : 0;
  } else {  // past the edge's last point: the distance launch still reads the row
    for (uint32_t c = 0; c < uint32_t(sp.n); ++c) {
      x[2 * c] = a[2 * c], x[2 * c + 1] = a[2 * c + 1];
      xm[2 * c] = a[2 * c] * sp.speed[c], xm[2 * c + 1] = a[2 * c + 1] * sp.accel[c];
    }
    w.inb[i] = 1;
  }
}

// has_dist = 0: the scene has no proxy pair, every point is collision-free
__global__ __launch_bounds__(256) void svp_walk_scan_kernel(const SvpDev sp, const SvpWalk w, uint32_t cur, uint32_t live,
                                                            int has_dist) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= live) return;
  const uint32_t e = w.list[cur][i];
  const uint32_t D = 2 * uint32_t(sp.n);
  const uint32_t K = w.K[e];
  uint32_t k = w.k_done[e], nc = w.n_checked[e];
  int good = -1;
  bool failed = false;
  uint32_t j = 0;
  for (; j < kSvpPass && k + j < K; ++j) {
    const size_t row = size_t(i) * kSvpPass + j;
    ++nc;
    if (!w.inb[row] || (has_dist && w.dist[row] < 0.0)) {
      failed = true;
      break;
    }
    good = int(j);
  }
  w.n_checked[e] = nc;
  const double* lastp = good >= 0 ? w.pts + (size_t(i) * kSvpPass + uint32_t(good)) * D : w.last + size_t(e) * D;
  if (failed) {
    for (uint32_t c = 0; c < D; ++c) w.out[size_t(e) * D + c] = lastp[c];
    return;
  }
  k += j;
  if (k == K) {
    svp_walk_finish(sp, w, e);
    return;
  }
  for (uint32_t c = 0; c < D; ++c) w.last[size_t(e) * D + c] = lastp[c];
  double d = w.d_next[e];
  for (uint32_t c = 0; c < kSvpPass; ++c) d += sp.min_interval;
  w.d_next[e] = d;
  w.k_done[e] = k;
  w.list[1 - cur][atomicAdd(&w.counters[1 - cur], 1u)] = e;
}

__global__ __launch_bounds__(256) void svp_interp_kernel(const SvpDev sp, const double* __restrict__ a,
                                                         const double* __restrict__ b, const double* __restrict__ T,
                                                         const double* __restrict__ peak, const double* __restrict__ t,
                                                         uint32_t B, uint32_t M, double* __restrict__ out) {
  const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= uint64_t(B) * M) return;
  const uint32_t e = uint32_t(i / M);
  const uint32_t D = 2 * uint32_t(sp.n);
  const double* ae = a + size_t(e) * D;
  const double* be = b + size_t(e) * D;
  double* x = out + size_t(i) * D;
  const double Te = T[e], ti = t[i];
  if (!(Te < INFINITY) || !(ti > 0.0)) {
    for (uint32_t c = 0; c < D; ++c) x[c] = ae[c];
  } else if (ti >= Te) {
    for (uint32_t c = 0; c < D; ++c) x[c] = be[c];
  } else {
    svp_point(sp, ae, be, peak + size_t(e) * sp.n, Te, ti, x, nullptr);
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
rkh_status bad(const char* who, const char* what) {
  set_error(std::string(who) + ": " + what);
  return RKH_ERR_BAD_ARG;
}

}  // namespace

// everything the entries check about a space, and its device form.  scene_n < 0: no scene to agree with
rkh_status svp_space_dev(const char* who, const rkh_svp_space* sp, int scene_n, SvpDev* out) {
  if (!sp) return bad(who, "space is NULL");
  if (sp->struct_size != sizeof(rkh_svp_space)) return bad(who, "space->struct_size is not sizeof(rkh_svp_space)");
  const int n = sp->n_dof;
  if (n < 1 || n > kSvpMaxDof) return bad(who, "n_dof must be in [1, 12]");
  if (scene_n >= 0 && n != scene_n) return bad(who, "n_dof is not the scene's");
  if (!(sp->min_interval > 0.0) || !std::isfinite(sp->min_interval)) return bad(who, "min_interval must be positive and finite");
  std::memset(out, 0, sizeof(*out));
  out->n = n;
  out->min_interval = sp->min_interval;
  for (int i = 0; i < kSvpMaxDof; ++i) out->speed[i] = out->accel[i] = out->vm[i] = 1.0;
  for (int i = 0; i < n; ++i) {
    if (!(sp->lower[i] <= sp->upper[i])) return bad(who, "lower must not exceed upper");
    const double sl = sp->speed_limits[i], al = sp->accel_limits[i];
    if (!(sl >= 0.0) || !std::isfinite(sl) || !(al >= 0.0) || !std::isfinite(al))
      return bad(who, "speed and acceleration limits must be finite and not negative (0: 1)");
    out->lower[i] = sp->lower[i];
    out->upper[i] = sp->upper[i];
    out->speed[i] = sl != 0.0 ? sl : 1.0;
    out->accel[i] = al != 0.0 ? al : 1.0;
    out->vm[i] = out->speed[i] / out->accel[i];
  }
  return RKH_OK;
}

size_t svp_walk_layout(int n_dof, uint32_t B, bool with_fraction, void* base, SvpWalk* w) {
  const size_t D = 2 * size_t(n_dof), n = size_t(n_dof);
  size_t cur = 0;
  auto take = [&cur](size_t bytes) {
    ArenaRange r;
    r.off = cur, r.bytes = bytes;
    cur = arena_align_up(cur + bytes);
    return r;
  };
  const size_t rows = size_t(B) * kSvpPass;
  const ArenaRange r_a = take(B * D * 8), r_b = take(B * D * 8), r_f = take(with_fraction ? size_t(B) * 8 : 0), r_T = take(size_t(B) * 8),
                   r_peak = take(B * n * 8), r_dt = take(size_t(B) * 8), r_K = take(size_t(B) * 4), r_kd = take(size_t(B) * 4),
                   r_dn = take(size_t(B) * 8), r_last = take(B * D * 8), r_out = take(B * D * 8), r_nc = take(size_t(B) * 4),
                   r_re = take(B), r_l0 = take(size_t(B) * 4), r_l1 = take(size_t(B) * 4), r_cnt = take(3 * 4),
                   r_pts = take(rows * D * 8), r_ptm = take(rows * D * 8), r_inb = take(rows), r_dist = take(rows * 8);
  if (base && w) {
    char* const p = static_cast<char*>(base);
    auto at = [p](const ArenaRange& r) { return r.bytes ? static_cast<void*>(p + r.off) : nullptr; };
    w->a = static_cast<double*>(at(r_a)), w->b = static_cast<double*>(at(r_b)), w->fraction = static_cast<double*>(at(r_f));
    w->T = static_cast<double*>(at(r_T)), w->peak = static_cast<double*>(at(r_peak)), w->dt = static_cast<double*>(at(r_dt));
    w->K = static_cast<uint32_t*>(at(r_K)), w->k_done = static_cast<uint32_t*>(at(r_kd)), w->d_next = static_cast<double*>(at(r_dn));
    w->last = static_cast<double*>(at(r_last)), w->out = static_cast<double*>(at(r_out));
    w->n_checked = static_cast<uint32_t*>(at(r_nc)), w->reached = static_cast<uint8_t*>(at(r_re));
    w->list[0] = static_cast<uint32_t*>(at(r_l0)), w->list[1] = static_cast<uint32_t*>(at(r_l1));
    w->counters = static_cast<uint32_t*>(at(r_cnt));
    w->pts = static_cast<double*>(at(r_pts)), w->pts_model = static_cast<double*>(at(r_ptm));
    w->inb = static_cast<uint8_t*>(at(r_inb)), w->dist = static_cast<double*>(at(r_dist));
    w->B = B;
  }
  return cur;
}

rkh_status launch_svp_walk(const char* who, const rkh_scene& scene, const SvpDev& sp, const SvpWalk& w, uint32_t* passes) {
  const uint32_t B = w.B;
  hipStream_t s = scene.ctx->stream;
  if (passes) *passes = 0;
  if (B == 0) return RKH_OK;
  StreamWait wait_on_exit{s};
  RKH_HIP(hipMemsetAsync(w.counters, 0, 3 * 4, s));
  hipLaunchKernelGGL(svp_walk_solve_kernel, dim3((B + kSvpThreads - 1) / kSvpThreads), dim3(kSvpThreads), 0, s, sp, w);
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
    if (live > B || pass > kSvpMaxPoints / kSvpPass) {
      set_error(std::string(who) + ": the live list is inconsistent");
      return RKH_ERR_DEVICE;
    }
    const uint32_t n_rows = live * kSvpPass;
    hipLaunchKernelGGL(svp_walk_points_kernel, dim3((n_rows + kSvpThreads - 1) / kSvpThreads), dim3(kSvpThreads), 0, s, sp, w, c,
                       live);
    RKH_HIP(hipGetLastError());
    if (has_dist) RKH_TRY(launch_min_distance(s, scene, w.pts_model, n_rows, w.dist));
    RKH_HIP(hipMemsetAsync(w.counters + (1 - c), 0, 4, s));
    hipLaunchKernelGGL(svp_walk_scan_kernel, dim3((live + kSvpThreads - 1) / kSvpThreads), dim3(kSvpThreads), 0, s, sp, w, c, live,
                       has_dist);
    RKH_HIP(hipGetLastError());
    RKH_HIP(hipMemcpyAsync(cnt, w.counters, sizeof(cnt), hipMemcpyDeviceToHost, s));
    RKH_HIP(hipStreamSynchronize(s));
    live = cnt[1 - c];
  }
  if (passes) *passes = pass;
  return RKH_OK;
}

namespace {

rkh_status launch_svp_reach(hipStream_t s, const SvpDev& sp, const double* d_a, const double* d_b, uint32_t B, double* d_time,
                            double* d_peak) {
  hipLaunchKernelGGL(svp_reach_kernel, dim3((B + kSvpThreads - 1) / kSvpThreads), dim3(kSvpThreads), 0, s, sp, d_a, d_b, B,
                     d_time, d_peak);
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

struct NearestPlan {
  uint32_t slice = 0, n_slices = 0;
  size_t part_entries = 0;  // 0: one slice, the sweep writes the results itself
};
rkh_status svp_nearest_plan(const char* who, uint32_t n_pts, uint32_t B, uint32_t k, NearestPlan* p) {
  p->slice = svp_slice(n_pts, B);
  uint64_t ns = (uint64_t(n_pts) + p->slice - 1) / p->slice;
  if (ns > kSvpMaxSlices) {  // more points than 4096 slices of the chosen size: the largest slice
    p->slice = kSvpSliceMax;
    ns = (uint64_t(n_pts) + p->slice - 1) / p->slice;
  }
  if (ns > kSvpMaxSlices || B > 65535u) {
    set_error(std::string(who) + ": at most 16 777 216 points and 65 535 queries per call");
    return RKH_ERR_CAPACITY;
  }
  p->n_slices = uint32_t(ns);
  p->part_entries = ns > 1 ? size_t(B) * ns * k : 0;
  return RKH_OK;
}

rkh_status launch_svp_nearest(hipStream_t s, const SvpDev& sp, const NearestPlan& p, const double* d_pts, uint32_t n_pts,
                              const double* d_q, uint32_t B, uint32_t k, int direction, double* d_part_dist,
                              uint32_t* d_part_idx, uint32_t* d_idx, double* d_dist) {
  const size_t lds = (size_t(p.slice) + 2 * kSvpMaxDof + 4) * sizeof(double) + 8 * sizeof(uint32_t);
  const bool merge = p.n_slices > 1;
  hipLaunchKernelGGL(svp_nearest_kernel, dim3(p.n_slices, B), dim3(kSvpThreads), lds, s, sp, d_pts, n_pts, d_q, p.slice, k,
                     direction, merge ? d_part_dist : d_dist, merge ? d_part_idx : d_idx);
  RKH_HIP(hipGetLastError());
  if (merge) {
    const size_t lds_m = 4 * sizeof(double) + (8 + size_t(p.n_slices)) * sizeof(uint32_t);
    hipLaunchKernelGGL(svp_nearest_merge_kernel, dim3(B), dim3(kSvpThreads), lds_m, s, d_part_dist, d_part_idx, p.n_slices, k,
                       d_idx, d_dist);
    RKH_HIP(hipGetLastError());
  }
  return RKH_OK;
}

rkh_status nearest_args(const char* who, rkh_ctx* ctx, const rkh_svp_space* space, const void* points, const void* queries,
                        uint32_t k, int direction, const void* idx, const void* dist, SvpDev* sp) {
  RKH_TRY(svp_space_dev(who, space, -1, sp));
  if (k < 1 || k > kSvpMaxK) return bad(who, "k must be in [1, 64]");
  if (direction != 0 && direction != 1) return bad(who, "direction must be 0 (point -> query) or 1 (query -> point)");
  if (!points || !queries || !idx || !dist) return bad(who, "a required pointer is NULL");
  if (!ctx) return bad(who, "ctx is NULL");
  return RKH_OK;
}

}  // namespace
}  // namespace rkh

using namespace rkh;

extern "C" {

rkh_status rkh_svp_in_bounds(const rkh_svp_space* space, const double* pts, uint32_t B, uint8_t* ok) {
  SvpDev sp;
  RKH_TRY(svp_space_dev("rkh_svp_in_bounds", space, -1, &sp));
  if (B == 0) return RKH_OK;
  if (!pts || !ok) return bad("rkh_svp_in_bounds", "a required pointer is NULL");
  for (uint32_t e = 0; e < B; ++e) ok[e] = svp_in_bounds(sp, pts + size_t(e) * 2 * sp.n) ? 1 : 0;
  return RKH_OK;
}

rkh_status rkh_svp_reach_time(rkh_ctx* ctx, const rkh_svp_space* space, const double* a, const double* b, uint32_t B,
                              double* time, double* peak) {
  const char* who = "rkh_svp_reach_time";
  SvpDev sp;
  RKH_TRY(svp_space_dev(who, space, -1, &sp));
  if (B == 0) return RKH_OK;
  if (!a || !b || !time) return bad(who, "a required pointer is NULL");
  if (!ctx) return bad(who, "ctx is NULL");
  const size_t D = 2 * size_t(sp.n);
  hipStream_t s = ctx->stream;
  RKH_HIP(hipSetDevice(ctx->device));
  StagedCall call(s);
  const double* d_a = call.in(a, B * D);
  const double* d_b = call.in(b, B * D);
  double* d_t = call.out(time, B);
  double* d_p = peak ? call.out(peak, size_t(B) * sp.n) : nullptr;
  RKH_TRY(call.status());
  RKH_TRY(launch_svp_reach(s, sp, d_a, d_b, B, d_t, d_p));
  return call.fetch();
}

rkh_status rkh_svp_nearest(rkh_ctx* ctx, const rkh_svp_space* space, const double* points, uint32_t n_pts, const double* queries,
                           uint32_t B, uint32_t k, int32_t direction, uint32_t* idx, double* dist) {
  const char* who = "rkh_svp_nearest";
  SvpDev sp;
  if (space && (B == 0 || n_pts == 0)) {  // nothing to search or nobody asking: only the space and k are looked at
    RKH_TRY(svp_space_dev(who, space, -1, &sp));
    if (k < 1 || k > kSvpMaxK) return bad(who, "k must be in [1, 64]");
    if (direction != 0 && direction != 1) return bad(who, "direction must be 0 (point -> query) or 1 (query -> point)");
    if (B && (!idx || !dist)) return bad(who, "a required pointer is NULL");
    for (size_t i = 0; i < size_t(B) * k; ++i) idx[i] = kNoIndex, dist[i] = INFINITY;
    return RKH_OK;
  }
  RKH_TRY(nearest_args(who, ctx, space, points, queries, k, direction, idx, dist, &sp));
  NearestPlan plan;
  RKH_TRY(svp_nearest_plan(who, n_pts, B, k, &plan));
  const size_t D = 2 * size_t(sp.n);
  hipStream_t s = ctx->stream;
  RKH_HIP(hipSetDevice(ctx->device));
  StagedCall call(s);
  const double* d_pts = call.in(points, n_pts * D);
  const double* d_q = call.in(queries, B * D);
  uint32_t* d_idx = call.out(idx, size_t(B) * k);
  double* d_dist = call.out(dist, size_t(B) * k);
  double* d_pd = plan.part_entries ? call.scratch<double>(plan.part_entries) : nullptr;  // the slices' lists
  uint32_t* d_pi = plan.part_entries ? call.scratch<uint32_t>(plan.part_entries) : nullptr;
  RKH_TRY(call.status());
  RKH_TRY(launch_svp_nearest(s, sp, plan, d_pts, n_pts, d_q, B, k, direction, d_pd, d_pi, d_idx, d_dist));
  return call.fetch();
}

rkh_status rkh_svp_nearest_async(rkh_ctx* ctx, const rkh_svp_space* space, const double* d_points, uint32_t n_pts,
                                 const double* d_queries, uint32_t B, uint32_t k, int32_t direction, uint32_t* d_idx,
                                 double* d_dist) {
  const char* who = "rkh_svp_nearest_async";
  SvpDev sp;
  if (space && B == 0) return svp_space_dev(who, space, -1, &sp);
  // without points the sweep still runs, over one empty slice: it writes the padding
  RKH_TRY(nearest_args(who, ctx, space, n_pts ? static_cast<const void*>(d_points) : static_cast<const void*>(d_queries),
                       d_queries, k, direction, d_idx, d_dist, &sp));
  NearestPlan plan;
  RKH_TRY(svp_nearest_plan(who, n_pts, B, k, &plan));
  plan.n_slices = std::max(plan.n_slices, 1u);
  RKH_HIP(hipSetDevice(ctx->device));
  // the slices' lists live in the context and grow with the largest request (growing frees the old block, which waits
  // for the device: a steady stream of launches of one size never does)
  const size_t ws_bytes = plan.part_entries * (sizeof(double) + sizeof(uint32_t));
  if (ws_bytes > ctx->svp_ws.size()) RKH_TRY(ctx->svp_ws.alloc(ws_bytes));
  double* d_pd = static_cast<double*>(ctx->svp_ws.get());
  uint32_t* d_pi = reinterpret_cast<uint32_t*>(d_pd + plan.part_entries);
  return launch_svp_nearest(ctx->stream, sp, plan, d_points, n_pts, d_queries, B, k, direction, d_pd, d_pi, d_idx, d_dist);
}

rkh_status rkh_svp_edge_check(rkh_scene* scene, const rkh_svp_space* space, const double* a, const double* b, uint32_t B,
                              const double* fraction, double* out, double* reach_time, uint32_t* n_checked, uint8_t* reached) {
  const char* who = "rkh_svp_edge_check";
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
  // one slab for the call
  const size_t bytes = svp_walk_layout(sp.n, B, fraction != nullptr, nullptr, nullptr);
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
  RKH_HIP(hipMemcpyAsync(const_cast<double*>(w.a), a, B * D * 8, hipMemcpyHostToDevice, s));
  RKH_HIP(hipMemcpyAsync(const_cast<double*>(w.b), b, B * D * 8, hipMemcpyHostToDevice, s));
  if (fraction) RKH_HIP(hipMemcpyAsync(const_cast<double*>(w.fraction), fraction, size_t(B) * 8, hipMemcpyHostToDevice, s));
  RKH_TRY(launch_svp_walk(who, *scene, sp, w, nullptr));
  RKH_HIP(hipMemcpyAsync(out, w.out, B * D * 8, hipMemcpyDeviceToHost, s));
  if (reach_time) RKH_HIP(hipMemcpyAsync(reach_time, w.T, size_t(B) * 8, hipMemcpyDeviceToHost, s));
  if (n_checked) RKH_HIP(hipMemcpyAsync(n_checked, w.n_checked, size_t(B) * 4, hipMemcpyDeviceToHost, s));
  if (reached) RKH_HIP(hipMemcpyAsync(reached, w.reached, B, hipMemcpyDeviceToHost, s));
  RKH_HIP(hipStreamSynchronize(s));
  return RKH_OK;
}

rkh_status rkh_svp_interpolate(rkh_ctx* ctx, const rkh_svp_space* space, const double* a, const double* b, uint32_t B,
                               const double* t, uint32_t M, double* out, double* reach_time) {
  const char* who = "rkh_svp_interpolate";
  SvpDev sp;
  RKH_TRY(svp_space_dev(who, space, -1, &sp));
  if (B == 0) return RKH_OK;
  if (!a || !b || (M && (!t || !out))) return bad(who, "a required pointer is NULL");
  if (M == 0 && !reach_time) return RKH_OK;
  if (!ctx) return bad(who, "ctx is NULL");
  const size_t D = 2 * size_t(sp.n);
  if (uint64_t(B) * M > 0x7FFFFFFFull) {
    set_error(std::string(who) + ": too many (pair, time) samples for one launch");
    return RKH_ERR_CAPACITY;
  }
  hipStream_t s = ctx->stream;
  RKH_HIP(hipSetDevice(ctx->device));
  const size_t samples = size_t(B) * M;
  StagedCall call(s);
  const double* d_a = call.in(a, B * D);
  const double* d_b = call.in(b, B * D);
  double* d_T = call.out(reach_time, B);
  double* d_p = call.scratch<double>(size_t(B) * sp.n);
  const double* d_t = M ? call.in(t, samples) : nullptr;
  double* d_out = M ? call.out(out, samples * D) : nullptr;
  RKH_TRY(call.status());
  RKH_TRY(launch_svp_reach(s, sp, d_a, d_b, B, d_T, d_p));
  if (M) {
    hipLaunchKernelGGL(svp_interp_kernel, dim3(uint32_t((samples + kSvpThreads - 1) / kSvpThreads)), dim3(kSvpThreads), 0, s, sp,
                       d_a, d_b, d_T, d_p, d_t, B, M, d_out);
    RKH_HIP(hipGetLastError());
  }
  return call.fetch();
}

}  // extern "C"
