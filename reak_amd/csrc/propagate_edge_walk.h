// propagate_edge_walk.h -- HIP only: hipcc compiles it into the propagate*.hip units, no host compiler reads it (unlike the
// *_device.h headers).  The quasi-static edge walks: edge_walk and the staging of edge_check_kernel (planar scenes),
// the LDS layout of edge_points_kernel (3D scenes).  The kernels' own text: propagate_edge_check_kernel.inl,
// propagate_edge_points_kernel.inl.
#pragma once
#include "propagate_proximity.h"

namespace rkh {

// ---------------------------------------------------------------------------------------------
// Kernel: quasi-static edge walk interp_topo_move_position_toward_pred
// (ctrl/interpolation/interpolated_topologies.hpp:137-163) over joint positions (D = N), with
// manip_quasi_static_env::is_free (manip_free_workspace.hpp:154-156) as the predicate.
// Planar scenes (SceneDev::planar) only: 3D scenes walk in edge_points_kernel below, whose verdict may take the pairs
// in any order, while a planar verdict depends on the finder order (proximity_min_planar).
// One block of W waves per edge; its 4 * W 16-lane groups test that many consecutive interpolation points at a time
// (the points of a straight edge are independent), and the first colliding one is found from the groups' verdicts.
// dist_cur is accumulated by repeated addition exactly like the reference loop (":157 dist_cur += min_interval"),
// so the number of tested points is the same integer.  W (launch_edge_check) grows as the launch has fewer edges:
// 1 wave for thousands (the batch planner's rounds fill the machine with one wave per edge), up to 8 for a few hundred
// (a step of one or a few graph planners, which waits for its longest edge).
constexpr int kEdgeGL = 16;  // lanes per point
template <int N, int W>
struct BlockLdsQsW {
  static constexpr int G = (64 / kEdgeGL) * W;  // groups of the block = points per pass
  JointLds joints[N];
  double base[10];
  GroupWsQs<N> g[G];
  double pts[G][N];       // the groups' interpolation points (space coordinates)
  uint32_t masks[W];      // per wave: bit t = group t's point lies on the edge, bit 4 + t = it passed the predicate
};
template <int N, int W>
struct SmemLayoutQsW {
  static constexpr size_t block_bytes = (sizeof(BlockLdsQsW<N, W>) + 15) / 16 * 16;
  // env shapes, then (if it fits: edge_check_kernel's pairs_staged) the proxy pair list
  static size_t bytes(int n_env, int n_pairs_staged) {
    return block_bytes + size_t(n_env) * sizeof(ShapeDev) + size_t(n_pairs_staged) * sizeof(PairDev);
  }
};

// One edge walk of edge_check_kernel (the block's groups test G consecutive points per pass); PRISM: of
// planar_prismatic::edge_check_kernel, for chains with prismatic_joint_2D groups.
template <int N, int W, bool PRISM = false>
__device__ __forceinline__ void edge_walk(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs, int n_pairs,
                                          const QsDev& qs, const EdgeIO& io, BlockLdsQsW<N, W>& lds,
                                          const ShapeDev* __restrict__ env_lds, uint32_t e) {
  constexpr int GL = kEdgeGL, GPW = 64 / GL, G = GPW * W;  // lanes per group, groups per wave, groups of the block
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int g = tid / GL, gl = lane % GL, gb = (lane / GL) * GL;  // group of the block, lane of the group, its base lane in the wave
  GroupWsQs<N>& ws = lds.g[g];
  const uint32_t si = edge_source_row(io, e);
  const uint64_t trow = edge_target_row(io, e);
  const double a_d = (gl < N) ? io.src[uint64_t(si) * io.src_stride + gl] : 0.0;
  const double b_d = (gl < N) ? io.tgt[trow * io.tgt_stride + gl] : 0.0;
  const double lo = (gl < N) ? qs.lower[gl] : 0.0;
  const double hi = (gl < N) ? qs.upper[gl] : 0.0;
  const double speed = (gl < N) ? qs.speed[gl] : 1.0;  // rate-limited space: the model sees point * speed limit
  for (int t = gl; t < 2 * N; t += GL) ws.x[t] = 0.0;  // velocities stay zero (apply_to_model writes positions only)
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);

  // exact left-to-right euclidean norm of an N-vector held by lanes gl < N of every group
  auto norm_n = [&](double diff) {
    if (gl < N) ws.tmp[gl] = diff * diff;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < N; ++d) s = s + ws.tmp[d];
    __syncthreads();
    return sqrt(s);
  };
  if (io.mode == EDGE_POINT) {
    // is_free(target): hyperbox bounds, then proximity (manip_free_workspace.hpp:79-99,154-156); group 0 tests it
    if (gl < N) ws.x[2 * gl] = b_d * speed;
    const bool oob = (gl < N) && hyperbox_out(lo, hi, b_d);
    const unsigned long long mo = __ballot(oob);
    const bool group_oob = ((mo >> gb) & ((1ull << GL) - 1ull)) != 0ull;
    __syncthreads();
    const double dmin = proximity_min_planar<N, GL, PRISM>(sc, cp, lds.base, env_lds, pairs, n_pairs, ws, gl, gb);
    const bool is_free = !group_oob && !(dmin < 0.0);
    if (g == 0 && gl < N) io.x_out[uint64_t(e) * N + gl] = b_d;
    if (tid == 0) {
      io.steps_free[e] = 1;
      io.accept[e] = is_free ? 1 : 0;
    }
    return;
  }
  const double dist_tot = norm_n(a_d - b_d);
  const double fraction = io.frac ? io.frac[e] : qs.fraction;
  double result = a_d;       // component gl of the returned point
  uint32_t n_checked = 0;
  bool completed_walk = false;  // the predicate loop ran to dist_inter without a collision (EDGE_STEER_BOTH)
  if (dist_tot == INFINITY) {
    result = a_d;
  } else if (dist_tot < qs.min_interval) {
    result = a_d + (b_d - a_d) * fraction;  // vector_topology::move_position_toward, no predicate call
  } else {
    const double dist_inter = dist_tot * fraction;
    double cur = 0.0;          // dist_cur of the last tested point (0 + min_interval == min_interval exactly)
    double last_result = a_d;  // last point that passed the predicate
    bool collided = false;
    for (;;) {
      // dist_cur of this group's point and of the block's first and last ones: cur + min_interval, repeatedly
      double my = cur, last = cur;
#pragma unroll
      for (int t = 0; t < G; ++t) {
        if (t <= g) my = my + qs.min_interval;
        last = last + qs.min_interval;
      }
      if (!((cur + qs.min_interval) < dist_inter)) break;  // not even the first point is on the edge (block-uniform)
      const bool valid = my < dist_inter;
      const double pt = a_d + (b_d - a_d) * (my / dist_tot);
      if (gl < N) {
        ws.x[2 * gl] = pt * speed;
        lds.pts[g][gl] = pt;
      }
      const bool oob = (gl < N) && hyperbox_out(lo, hi, pt);
      const unsigned long long mo = __ballot(oob);
      const bool group_oob = ((mo >> gb) & ((1ull << GL) - 1ull)) != 0ull;
      __syncthreads();
      const double dmin = proximity_min_planar<N, GL, PRISM>(sc, cp, lds.base, env_lds, pairs, n_pairs, ws, gl, gb);
      const bool is_free = valid && !group_oob && !(dmin < 0.0);
      {  // the wave's verdicts -> LDS, then every thread scans the block's groups in edge order
        const unsigned long long mv = __ballot(valid && gl == 0), mf = __ballot(is_free && gl == 0);
        uint32_t m = 0;
#pragma unroll
        for (int t = 0; t < GPW; ++t)
          m |= (uint32_t((mv >> ((t * GL) & 63)) & 1ull) << t) | (uint32_t((mf >> ((t * GL) & 63)) & 1ull) << (4 + t));
        if (lane == 0) lds.masks[wave] = m;
      }
      __syncthreads();
      int first_bad = G;  // first valid group whose point fails the predicate
      int n_valid = 0;
#pragma unroll
      for (int t = G - 1; t >= 0; --t) {
        const uint32_t m = lds.masks[t / GPW];
        const bool v = (m >> (t % GPW)) & 1u, f = (m >> (4 + (t % GPW))) & 1u;
        if (v && !f) first_bad = t;
        if (v) n_valid = n_valid > t + 1 ? n_valid : t + 1;
      }
      if (first_bad < G) {
        n_checked += uint32_t(first_bad + 1);
        if (first_bad > 0 && gl < N) last_result = lds.pts[first_bad - 1][gl];
        collided = true;
        break;
      }
      n_checked += uint32_t(n_valid);
      if (gl < N) last_result = lds.pts[n_valid - 1][gl];
      if (n_valid < G) break;  // reached dist_inter without a collision
      cur = last;
      __syncthreads();         // the points and verdicts are rewritten by the next pass
    }
    completed_walk = !collided;
    if (collided) result = last_result;
    else if (fraction == 1.0) result = b_d;  // exact end fractions (:159-162)
    else if (fraction == 0.0) result = a_d;
    else result = a_d + (b_d - a_d) * fraction;
  }
  if (g == 0 && gl < N) io.x_out[uint64_t(e) * N + gl] = result;
  if (tid == 0) io.steps_free[e] = n_checked;
  if (io.mode != EDGE_PLAIN) {
    const double n_ar = norm_n(a_d - result);
    const double n_ab = dist_tot;
    const double n_rb = norm_n(result - b_d);
    const int acc = edge_accept(io.mode, n_ar, n_ab, n_rb, io.best_case, e, io.steer_tol, completed_walk ? 1 : 0);
    if (tid == 0) {
      if (acc != kNoAccept) io.accept[e] = uint8_t(acc);
      else if (io.mode == EDGE_GOAL_PROBE) io.goal_dist[si - 1] = goal_probe_interpolated(n_ab, n_rb);
    }
  }
}

template <int N, int W>
__device__ __forceinline__ const PairDev* edge_check_stage(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                                           int n_pairs, int pairs_staged, BlockLdsQsW<N, W>& lds,
                                                           ShapeDev* env_lds) {
  const int tid = threadIdx.x, lane = tid & 63;
  stage_chain<N>(sc, lds.joints, lds.base, lane);  // (every wave writes the same values)
  stage_env(sc, env_lds, lane);
  // and, when the launch made room for it, the pair list, which every point scans
  if (!pairs_staged) return pairs;
  PairDev* pl = reinterpret_cast<PairDev*>(env_lds + sc->n_env);
  for (int i = tid; i < n_pairs; i += 64 * W) pl[i] = pairs[i];
  return pl;
}

// ---------------------------------------------------------------------------------------------
// The same edge walk for 3D scenes, with ONE LANE PER POINT in the chain kinematics (edge_points_kernel).  A 16-lane
// group per point, as in edge_check_kernel, would run the serial base -> tip chain once per point: ~1.2 k fp64
// instructions per wave for 4 points.  Here a block of 4 waves takes G = 64 (32 for chains of more than 7 joints)
// consecutive points per pass and every phase is spread over what it is parallel in:
//   half-angle sin / cos   one (point, joint) per thread
//   joint end frames       one POINT per lane of the first wave: the serial chain, once per 64 points
//   robot shape poses      one (point, shape) per thread
//   bounding-sphere cull   one (point, pair) per thread -> survivors into the LDS queue
//   closed forms           one surviving (point, pair) per thread
// and the first colliding point comes out of two ballots.  is_free only asks whether SOME proxy pair is closer than 0
// (manip_free_workspace.hpp:154-156), so the pairs need no order: the cull is exactly findMinimumDistance's test
// against a running minimum of 0 (proxy_query_model.cpp:384-389), behind a cheaper test on squares that only ever skips
// what that one skips, and a pass nearly always needs ONE round of closed forms.  Should the survivors not fit the
// queue, the pair list is redone in slices that fit whatever survives.  Per-point data sit in LDS component-major
// ([..][G]: lanes of a wave = consecutive points = consecutive addresses).  Planar scenes, whose verdict depends on the
// finder order, walk in edge_check_kernel.
struct EdgePointsCfg {
  static constexpr int T = 256;                // threads per block
  static constexpr int QCAP = 1024;            // surviving (point, pair) combinations per round of closed forms
};
// G = points per pass: 64 for the launches of few edges (the step waits for its longest walk), 32 for the launches of
// thousands of edges (half the LDS, three blocks per CU) and for chains of more than 7 joints
template <int N, int G>
struct __attribute__((aligned(16))) EdgePointsLds {
  JointLds joints[N];
  double base[10];
  ShapeDev robot[2 * N];
  double a[N], b[N], res[N];      // the edge's end points; staging of an N-vector for the ordered sums
  double pts[N][G];               // the pass's interpolation points (space coordinates)
  double cs[N][2][G];             // cos, sin of the half joint angles
  double E[N][7][G];              // joint end frames: position, quaternion
  double R[2 * N][7][G];          // robot shapes, global pose
  uint32_t flags[G];              // bit 0: to be tested (on the edge, inside the bounds), bit 1: a pair closer than 0, bit 2: on the edge
  uint32_t q_cnt;
  uint32_t scan[2];               // first point that fails the predicate, points on the edge
  uint32_t queue[EdgePointsCfg::QCAP];
};
template <int N, int G>
struct EdgePointsSmem {
  static constexpr size_t block_bytes = (sizeof(EdgePointsLds<N, G>) + 15) / 16 * 16;
  static constexpr size_t bytes(int n_env, int n_pairs_staged) {
    return block_bytes + size_t(n_env) * sizeof(ShapeDev) + size_t(n_pairs_staged) * sizeof(PairDev);
  }
};

}  // namespace rkh
