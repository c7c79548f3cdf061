// propagate.hip -- RK4 forward-dynamics propagation of a KTE serial chain with a proximity
// (collision) test after every step, for batches of candidate edges (gfx950, wave64).
//
// What it replaces (paths relative to /root/reference/src/ReaK/):
//   steer loop        examples/misc/MEAQR_topology.hpp:503-565 (steer_with_constant_control pattern)
//   RK4               ctrl/sys_integrators/runge_kutta4_integrator_sys.hpp:53-97
//   x' = f(x,u)       ctrl/ctrl_sys/kte_nl_system.hpp:180-290 (apply_states_and_inputs, get_state_derivative)
//   KTE passes        ctrl/mbd_kte/kte_map_chain.hpp:71-89; revolute_joint.cpp:121-213; rigid_link.cpp:152-186;
//                     inertia.cpp:47-54,111-122; driving_actuator.cpp:31-39
//   mass matrix       ctrl/mbd_kte/mass_matrix_calculator.cpp:80-295 + core/kinetostatics/motion_jacobians.hpp:238-251
//   Cholesky solve    core/lin_alg/mat_cholesky.hpp:63-84,160-178,546-554
//   is_free           ctrl/topologies/manip_free_workspace.hpp:79-99 + geometry/proximity (proximity_device.h)
//
// Mapping onto the wave.  A block is one wave; a wave carries 64/GL candidate edges, GL lanes each
// (GL = 64: one wavefront per candidate, lowest latency; GL = 16: four candidates per wave, used when
// many planners oversubscribe the chip).  Within an edge's lane group:
//   * state x, RK4 temporaries, bounds: lane d < 2N owns component d (one register each)
//   * sin/cos of the N joint angles (half- and full-angle): lanes 0..2N-1 in parallel
//   * base->tip kinematic sweep and tip->base force sweep: serial by nature; every lane of the group runs
//     them on group-uniform values read by LDS broadcast (no cross-lane traffic), joints unrolled (template N)
//   * Jacobian columns Tcm(body b, coord c<=b): one lane per (b,c) pair; M(i,j): one lane per entry
//   * Cholesky: lane i owns row i (divisions of a column run in parallel), same per-element operation order
//   * proximity pairs: one lane per (robot shape, obstacle) pair, ballot for "any distance < 0"
// Chain parameters, obstacle table and all per-edge intermediates live in LDS.
// Compiled with -ffp-contract=off: products and sums round exactly as in the CPU reference; only
// sin/cos (OCML vs glibc) differ by ulps (stated tolerance: 1e-10 relative on propagated states).
//
// What the kernels call is in the propagate_*.h headers, the joint kind a template parameter PRISM; the text of the
// kernels that have prismatic forms too is in the propagate_*.inl files.  This unit holds the revolute kernels
// (kPrismatic = false: the prismatic branches compile away) and every public launcher; the prismatic forms are in
// propagate_prismatic.hip and propagate_planar_qs_prismatic.hip, the depth forms of the records in propagate_depth.hip.
#include "propagate_launch.h"
#include "propagate_records.h"

namespace rkh {

// ---- kernels ---------------------------------------------------------------------------------
// The revolute forms of the kernels whose text other units hold forms of too; the cycle probes and the record kernels
// (entries of their bodies) exist only here.
constexpr bool kPrismatic = false, kPlanarForm = false;
#include "propagate_steer_kernels.inl"
#include "propagate_edge_check_kernel.inl"
#include "propagate_edge_points_kernel.inl"

// Diagnostic kernel (not on the product path): `iters` back-to-back f-evals + proximity tests of one edge per
// wave, with s_memtime deltas per phase: [sincos, forward sweep, jacobian columns, force sweep, mass matrix,
// cholesky, proximity, total].
template <int N>
__global__ __launch_bounds__(64) void feval_cycles_kernel(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                                           int n_pairs, const double* __restrict__ x,
                                                           const double* __restrict__ u, int iters,
                                                           unsigned long long* __restrict__ out, double* __restrict__ sink_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  BlockLds<N, 64>& lds = *reinterpret_cast<BlockLds<N, 64>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + SmemLayout<N, 64>::block_bytes);
  const int lane = threadIdx.x;
  constexpr int D = 2 * N;
  stage_chain<N>(sc, lds.joints, lds.base, lane);
  stage_env(sc, env_lds, lane);
  GroupWs<N>& ws = lds.g[0];
  double xv = (lane < D) ? x[uint64_t(blockIdx.x) * D + lane] : 0.0;
  if (lane < N) ws.u[lane] = u[uint64_t(blockIdx.x) * N + lane];
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);
  unsigned long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool singular = false;
  double acc = 0.0;
  const unsigned long long t_begin = __builtin_readcyclecounter();
  for (int it = 0; it < iters; ++it) {
    if (lane < D) ws.x[lane] = xv;
    __syncthreads();
    const double dp = state_derivative<N, 64>(sc, cp, lds.joints, lds.base, ws, lds.sink[lane], lane, 0, &singular, st);
    xv = xv + 1e-4 * dp;
    if (lane < D) ws.x[lane] = xv;
    __syncthreads();
    const unsigned long long t0 = __builtin_readcyclecounter();
    acc += proximity_min<N, 64>(sc, cp, lds.base, env_lds, pairs, n_pairs, ws, lds.sink[lane], lane, 0, true, false);
    st[6] += __builtin_readcyclecounter() - t0;
  }
  st[7] = __builtin_readcyclecounter() - t_begin;
  if (lane == 0) {
    for (int i = 0; i < 8; ++i) out[blockIdx.x * 8 + i] = st[i];
    sink_out[blockIdx.x] = acc + xv + (singular ? 1.0 : 0.0);
  }
}

// Diagnostic kernel (not on the product path): state_derivative_duo, `iters` f-evals of one state per block of two
// waves; row 2 b of `out` = wave 0's stamps, row 2 b + 1 = wave 1's (8 counters each, see state_derivative_duo).
template <int N>
__global__ __launch_bounds__(128) void feval_cycles_duo_kernel(const SceneDev* __restrict__ sc, const double* __restrict__ x,
                                                                const double* __restrict__ u, int iters,
                                                                unsigned long long* __restrict__ out, double* __restrict__ sink_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  BlockLds<N, 64>& lds = *reinterpret_cast<BlockLds<N, 64>*>(smem_raw);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int D = 2 * N;
  stage_chain<N>(sc, lds.joints, lds.base, lane);
  GroupWs<N>& ws = lds.g[0];
  double xv = (lane < D) ? x[uint64_t(blockIdx.x) * D + lane] : 0.0;
  if (lane < N) ws.u[lane] = u[uint64_t(blockIdx.x) * N + lane];
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);
  unsigned long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool singular = false;
  const unsigned long long t_begin = __builtin_readcyclecounter();
  for (int it = 0; it < iters; ++it) {
    if (lane < D) ws.x[lane] = xv;
    __syncthreads();
    const double dp = state_derivative_duo<N>(sc, cp, lds.joints, lds.base, ws, lds.sink[lane], lane, wave, &singular, st);
    xv = xv + 1e-4 * dp;
  }
  st[7] = __builtin_readcyclecounter() - t_begin;
  if (lane == 0) {
    for (int i = 0; i < 8; ++i) out[(uint64_t(blockIdx.x) * 2 + wave) * 8 + i] = st[i];
    if (wave == 0) sink_out[blockIdx.x] = xv + (singular ? 1.0 : 0.0);
  }
}

#include "propagate_min_distance_kernel.inl"

template <int N>
__global__ __launch_bounds__(64) void min_distance_records_kernel(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                                                   const PairIdDev* __restrict__ ids, int n_pairs,
                                                                   const double* __restrict__ x, uint32_t B, RecordOut out) {
  min_distance_records_body<N, kRecClosed>(sc, pairs, ids, n_pairs, x, B, out);
}

template <int N>
__global__ __launch_bounds__(64) void min_distance_records_meshes_kernel(const SceneDev* __restrict__ sc,
                                                                          const PairDev* __restrict__ pairs,
                                                                          const PairIdDev* __restrict__ ids, int n_pairs,
                                                                          const double* __restrict__ x, uint32_t B, RecordOut out) {
  min_distance_records_body<N, kRecGjk>(sc, pairs, ids, n_pairs, x, B, out);
}

template <int N>
__global__ __launch_bounds__(64) void collision_records_kernel(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                                                const PairIdDev* __restrict__ ids, int n_pairs,
                                                                const double* __restrict__ x, uint32_t B, uint32_t cap,
                                                                RecordOut out) {
  collision_records_body<N, kRecClosed>(sc, pairs, ids, n_pairs, x, B, cap, out);
}

template <int N>
__global__ __launch_bounds__(64) void collision_records_meshes_kernel(const SceneDev* __restrict__ sc,
                                                                       const PairDev* __restrict__ pairs,
                                                                       const PairIdDev* __restrict__ ids, int n_pairs,
                                                                       const double* __restrict__ x, uint32_t B, uint32_t cap,
                                                                       RecordOut out) {
  collision_records_body<N, kRecGjk>(sc, pairs, ids, n_pairs, x, B, cap, out);
}

// ---- host launchers ------------------------------------------------------------------------
// (kept in their order: the order in which the kernels are first named decides the module's, and the inliner's choices)
template <int GL, bool GJK, bool DUO = false>
static rkh_status launch_propagate_t(hipStream_t s, const rkh_scene& scene, const DynDev& dyn, const EdgeIO& io,
                                     uint32_t edges_a, uint32_t edges_b, const EdgeIO* tab_a, const EdgeIO* tab_b,
                                     uint32_t n_problems, KernelGate gate) {
  uint32_t grid_a;
  const dim3 grid = steer_grid<GL>(edges_a, edges_b, n_problems, gate, &grid_a);
  const WaveArgs args = wave_args_of(scene, dyn, io, tab_a, tab_b, grid_a, gate);
  return with_chain_n<false>(scene.host.n_dof, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((propagate_kernel<N, GL, GJK, DUO>), grid, dim3(DUO ? 128 : 64),
                       (SmemLayout<N, GL>::bytes(scene.host.n_env)), s, args);
  });
}

rkh_status launch_propagate(hipStream_t s, const rkh_scene& scene, SteerMapping m, const DynDev& dyn, const EdgeIO& io,
                            uint32_t grid_edges, uint32_t grid_b, const EdgeIO* tab_a, const EdgeIO* tab_b,
                            uint32_t n_problems, double* d_lane_ws, KernelGate gate) {
  const uint32_t eb = tab_b ? grid_b : 0u;
  if (grid_edges + eb == 0 || n_problems == 0) return RKH_OK;
  rkh_status st;
  // a scene with prismatic joints never reaches a revolute form: whatever one-wave mapping was asked for is theirs
  // (planar chains with prismatic joints have forms of their own behind launch_propagate_planar)
  if (scene.host.has_prismatic && !scene.host.planar && m != SteerMapping::Pair) m = SteerMapping::Prismatic;
  switch (m) {
    case SteerMapping::Planar:
      return launch_propagate_planar(s, scene, dyn, io, grid_edges, eb, tab_a, tab_b, n_problems, gate);
    case SteerMapping::Prismatic:
      return prismatic::launch_propagate(s, scene, m, dyn, io, grid_edges, eb, tab_a, tab_b, n_problems, d_lane_ws, gate);
    case SteerMapping::Pair:
      return rkh::launch_propagate_pairs(s, scene, dyn, io, grid_edges, eb, tab_a, tab_b, n_problems, d_lane_ws, gate);
    case SteerMapping::Duo:
      st = launch_propagate_t<64, false, true>(s, scene, dyn, io, grid_edges, eb, tab_a, tab_b, n_problems, gate);
      break;
    case SteerMapping::Wave16:
      st = launch_propagate_t<16, true>(s, scene, dyn, io, grid_edges, eb, tab_a, tab_b, n_problems, gate);
      break;
    default:  // Wave; without vertex-set shapes the instantiation without the support-map query (no private segment)
      st = scene.host.has_meshes
               ? launch_propagate_t<64, true>(s, scene, dyn, io, grid_edges, eb, tab_a, tab_b, n_problems, gate)
               : launch_propagate_t<64, false>(s, scene, dyn, io, grid_edges, eb, tab_a, tab_b, n_problems, gate);
  }
  if (st != RKH_OK) return st;
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

rkh_status launch_state_derivative(hipStream_t s, const rkh_scene& scene, const double* d_x, const double* d_u, uint32_t B,
                                   double* d_pd, double* d_M, double* d_f, int* d_err) {
  if (B == 0) return RKH_OK;
  if (scene.host.planar) return launch_state_derivative_planar(s, scene, d_x, d_u, B, d_pd, d_M, d_f, d_err);
  if (scene.host.has_prismatic) return prismatic::launch_state_derivative(s, scene, d_x, d_u, B, d_pd, d_M, d_f, d_err);
  RKH_TRY(with_chain_n<false>(scene.host.n_dof, [&](auto c) {
    hipLaunchKernelGGL((state_derivative_kernel<decltype(c)::value>), dim3(B), dim3(64), 0, s, scene.d_scene.get(), d_x, d_u, B,
                       d_pd, d_M, d_f, d_err);
  }));
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

template <int N, bool GJK, int G>
static rkh_status launch_edge_points_t(hipStream_t s, dim3 grid, int n_env, const EdgeWalkArgs& ka) {
  static bool big_lds = false;  // (per instantiation: one flag per kernel function, see launch_edge_points)
  return launch_edge_points<N, G>(edge_points_kernel<N, GJK, G>, &big_lds, s, grid, n_env, ka);
}

// The form of a quasi-static edge walk launch.  3D scenes: edge_points_kernel, kEdgePointsWide points per pass for the
// launches edge_points_wide names, 32 otherwise, the support-map query only for scenes with vertex-set shapes.  Planar
// scenes: edge_check_kernel with edge_check_shape's W.  Both stage the pair list in LDS if it fits.
template <int N>
static rkh_status launch_edge_walk(hipStream_t s, dim3 grid, const rkh_scene& scene, EdgeWalkArgs ka) {
  const int n_env = scene.host.n_env;
  constexpr int GW = kEdgePointsWide<N>;
  const bool wide = edge_points_wide(grid);
  if (scene.host.planar) {
    const int w = edge_check_shape<N>(n_env, ka.n_pairs, uint64_t(grid.x) * grid.y, &ka.pairs_staged);
    return with_n<1, 2, 4, 8>(w, [&](auto cw) {
      constexpr int W = decltype(cw)::value;
      hipLaunchKernelGGL((edge_check_kernel<N, W>), grid, dim3(64 * W),
                         (SmemLayoutQsW<N, W>::bytes(n_env, ka.pairs_staged ? ka.n_pairs : 0)), s, ka);
    });
  }
  if (scene.host.has_meshes)
    return wide ? launch_edge_points_t<N, true, GW>(s, grid, n_env, ka) : launch_edge_points_t<N, true, 32>(s, grid, n_env, ka);
  return wide ? launch_edge_points_t<N, false, GW>(s, grid, n_env, ka) : launch_edge_points_t<N, false, 32>(s, grid, n_env, ka);
}

rkh_status launch_edge_check(hipStream_t s, const rkh_scene& scene, const QsDev& qs, const EdgeIO& io, uint32_t grid_edges,
                             uint32_t grid_b, const EdgeIO* tab_a, const EdgeIO* tab_b, uint32_t n_problems) {
  const uint32_t eb = tab_b ? grid_b : 0u;
  if (grid_edges + eb == 0 || n_problems == 0) return RKH_OK;
  if (scene.host.has_prismatic && scene.host.planar)
    return planar_prismatic::launch_edge_check(s, scene, qs, io, grid_edges, eb, tab_a, tab_b, n_problems);
  if (scene.host.has_prismatic)
    return prismatic::launch_edge_check(s, scene, qs, io, grid_edges, eb, tab_a, tab_b, n_problems);
  const EdgeWalkArgs ka = edge_walk_args_of(scene, qs, io, tab_a, tab_b, grid_edges);
  const dim3 grid(grid_edges + eb, n_problems);
  rkh_status st = RKH_OK;
  RKH_TRY(with_chain_n<false>(scene.host.n_dof, [&](auto c) { st = launch_edge_walk<decltype(c)::value>(s, grid, scene, ka); }));
  if (st != RKH_OK) return st;
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

// the f-eval cycle probes instrument the revolute forms only
rkh_status launch_feval_cycles_duo(hipStream_t s, const rkh_scene& scene, const double* d_x, const double* d_u, uint32_t B,
                                   int iters, unsigned long long* d_out, double* d_sink) {
  if (scene.host.has_prismatic) {
    set_error("rkh_diag_feval_cycles: scenes with prismatic joints are not instrumented");
    return RKH_ERR_UNSUPPORTED;
  }
  RKH_TRY(with_chain_n<false>(scene.host.n_dof, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((feval_cycles_duo_kernel<N>), dim3(B / 2), dim3(128), (SmemLayout<N, 64>::bytes(scene.host.n_env)), s,
                       scene.d_scene.get(), d_x, d_u, iters, d_out, d_sink);
  }));
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

rkh_status launch_feval_cycles(hipStream_t s, const rkh_scene& scene, const double* d_x, const double* d_u, uint32_t B,
                               int iters, unsigned long long* d_out, double* d_sink) {
  if (scene.host.has_prismatic) {
    set_error("rkh_diag_feval_cycles: scenes with prismatic joints are not instrumented");
    return RKH_ERR_UNSUPPORTED;
  }
  RKH_TRY(with_chain_n<false>(scene.host.n_dof, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((feval_cycles_kernel<N>), dim3(B), dim3(64), (SmemLayout<N, 64>::bytes(scene.host.n_env)), s,
                       scene.d_scene.get(), scene.d_pairs.get(), scene.n_pairs, d_x, d_u, iters, d_out, d_sink);
  }));
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

rkh_status launch_min_distance(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, double* d_dist) {
  if (B == 0) return RKH_OK;
  if (scene.host.has_prismatic && scene.host.planar) return planar_prismatic::launch_min_distance(s, scene, d_x, B, d_dist);
  if (scene.host.has_prismatic) return prismatic::launch_min_distance(s, scene, d_x, B, d_dist);
  RKH_TRY(with_chain_n<false>(scene.host.n_dof, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((min_distance_kernel<N>), dim3(B), dim3(64), (SmemLayoutQs<N, 64>::bytes(scene.host.n_env)), s,
                       scene.d_scene.get(), scene.d_pairs.get(), scene.n_pairs, d_x, B, d_dist);
  }));
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

// the record kernels exist once and serve both joint kinds (propagate_records.h)
rkh_status launch_min_distance_records(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, RecordOut out) {
  if (B == 0) return RKH_OK;
  return launch_records(scene, false, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((min_distance_records_kernel<N>), dim3(B), dim3(64), (SmemLayoutQs<N, 64>::bytes(scene.host.n_env)), s,
                       scene.d_scene.get(), scene.d_pairs.get(), scene.d_pair_ids.get(), scene.n_pairs, d_x, B, out);
  });
}

rkh_status launch_collision_records(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, uint32_t cap,
                                    RecordOut out) {
  if (B == 0) return RKH_OK;
  return launch_records(scene, false, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((collision_records_kernel<N>), dim3(B), dim3(64), (SmemLayoutQs<N, 64>::bytes(scene.host.n_env)), s,
                       scene.d_scene.get(), scene.d_pairs.get(), scene.d_pair_ids.get(), scene.n_pairs, d_x, B, cap, out);
  });
}

// The same for every 3D scene: with vertex-set shapes the support-map forms, without them the kernels above
rkh_status launch_min_distance_records_meshes(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, RecordOut out) {
  if (!scene.host.has_meshes) return launch_min_distance_records(s, scene, d_x, B, out);
  if (B == 0) return RKH_OK;
  return launch_records(scene, true, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((min_distance_records_meshes_kernel<N>), dim3(B), dim3(64), (SmemLayoutQs<N, 64>::bytes(scene.host.n_env)),
                       s, scene.d_scene.get(), scene.d_pairs.get(), scene.d_pair_ids.get(), scene.n_pairs, d_x, B, out);
  });
}

rkh_status launch_collision_records_meshes(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, uint32_t cap,
                                           RecordOut out) {
  if (!scene.host.has_meshes) return launch_collision_records(s, scene, d_x, B, cap, out);
  if (B == 0) return RKH_OK;
  return launch_records(scene, true, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((collision_records_meshes_kernel<N>), dim3(B), dim3(64), (SmemLayoutQs<N, 64>::bytes(scene.host.n_env)),
                       s, scene.d_scene.get(), scene.d_pairs.get(), scene.d_pair_ids.get(), scene.n_pairs, d_x, B, cap, out);
  });
}

}  // namespace rkh
