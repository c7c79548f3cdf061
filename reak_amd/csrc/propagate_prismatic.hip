// propagate_prismatic.hip -- the forms of the one-wave-per-edge steer kernel, the f-eval kernel, the distance query and
// the 3D edge walk for scenes with prismatic joints (SceneDev::has_prismatic): the kernel texts of the propagate_*.inl
// files with kPrismatic = true, as kernels of rkh::prismatic with their four launchers, for chains of 1, 2, 3, 4, 6 and
// 7 joints and without the duo, 16-lane, support-map and planar forms.  A translation unit of its own keeps the revolute
// kernels of propagate.hip exactly as they were (their code does not depend on what else is instantiated next to them).
#include "propagate_launch.h"

namespace rkh {
namespace prismatic {

constexpr bool kPrismatic = true, kPlanarForm = false;
#include "propagate_steer_kernels.inl"
#include "propagate_edge_points_kernel.inl"
#include "propagate_min_distance_kernel.inl"

// (kept in their order: the order in which the kernels are first named decides the module's, and the inliner's choices)
rkh_status launch_propagate(hipStream_t s, const rkh_scene& scene, SteerMapping, const DynDev& dyn, const EdgeIO& io,
                            uint32_t grid_edges, uint32_t grid_b, const EdgeIO* tab_a, const EdgeIO* tab_b,
                            uint32_t n_problems, double*, KernelGate gate) {
  const uint32_t eb = tab_b ? grid_b : 0u;
  if (grid_edges + eb == 0 || n_problems == 0) return RKH_OK;
  uint32_t grid_a;
  const dim3 grid = steer_grid<64>(grid_edges, eb, n_problems, gate, &grid_a);
  const WaveArgs args = wave_args_of(scene, dyn, io, tab_a, tab_b, grid_a, gate);
  RKH_TRY(with_chain_n<true>(scene.host.n_dof, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((propagate_kernel<N, 64, false>), grid, dim3(64), (SmemLayout<N, 64>::bytes(scene.host.n_env)), s, args);
  }));
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

rkh_status launch_state_derivative(hipStream_t s, const rkh_scene& scene, const double* d_x, const double* d_u, uint32_t B,
                                   double* d_pd, double* d_M, double* d_f, int* d_err) {
  if (B == 0) return RKH_OK;
  RKH_TRY(with_chain_n<true>(scene.host.n_dof, [&](auto c) {
    hipLaunchKernelGGL((state_derivative_kernel<decltype(c)::value>), dim3(B), dim3(64), 0, s, scene.d_scene.get(), d_x, d_u, B,
                       d_pd, d_M, d_f, d_err);
  }));
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

template <int N, int G>
static rkh_status launch_edge_points_t(hipStream_t s, dim3 grid, int n_env, const EdgeWalkArgs& ka) {
  static bool big_lds = false;  // (per instantiation: one flag per kernel function, see launch_edge_points)
  return launch_edge_points<N, G>(edge_points_kernel<N, false, G>, &big_lds, s, grid, n_env, ka);
}

rkh_status launch_edge_check(hipStream_t s, const rkh_scene& scene, const QsDev& qs, const EdgeIO& io, uint32_t grid_edges,
                             uint32_t grid_b, const EdgeIO* tab_a, const EdgeIO* tab_b, uint32_t n_problems) {
  const uint32_t eb = tab_b ? grid_b : 0u;
  if (grid_edges + eb == 0 || n_problems == 0) return RKH_OK;
  const EdgeWalkArgs ka = edge_walk_args_of(scene, qs, io, tab_a, tab_b, grid_edges);
  const dim3 grid(grid_edges + eb, n_problems);
  const int n_env = scene.host.n_env;
  rkh_status st = RKH_OK;
  RKH_TRY(with_chain_n<true>(scene.host.n_dof, [&](auto c) {
    constexpr int N = decltype(c)::value;
    st = edge_points_wide(grid) ? launch_edge_points_t<N, kEdgePointsWide<N>>(s, grid, n_env, ka)
                                : launch_edge_points_t<N, 32>(s, grid, n_env, ka);
  }));
  if (st != RKH_OK) return st;
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

rkh_status launch_min_distance(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, double* d_dist) {
  if (B == 0) return RKH_OK;
  RKH_TRY(with_chain_n<true>(scene.host.n_dof, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((min_distance_kernel<N>), dim3(B), dim3(64), (SmemLayoutQs<N, 64>::bytes(scene.host.n_env)), s,
                       scene.d_scene.get(), scene.d_pairs.get(), scene.n_pairs, d_x, B, d_dist);
  }));
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

}  // namespace prismatic
}  // namespace rkh
