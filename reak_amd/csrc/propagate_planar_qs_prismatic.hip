// propagate_planar_qs_prismatic.hip -- the position-level forms (quasi-static edge walk, distance query) for planar chains
// with prismatic_joint_2D groups (SceneDev::planar && has_prismatic): the kernel texts of propagate_edge_check_kernel.inl
// and propagate_min_distance_kernel.inl over proximity_min_planar<.., PRISM = true>, as kernels of rkh::planar_prismatic
// with their two launchers.  The unit holds these kernels and nothing else: a kernel added to propagate.hip's module
// would shift the code of the ones that holds.  (rkh::prismatic holds the forms of 3D chains.)
#include "propagate_launch.h"

namespace rkh {
namespace planar_prismatic {

constexpr bool kPrismatic = true, kPlanarForm = true;
#include "propagate_edge_check_kernel.inl"
#include "propagate_min_distance_kernel.inl"

rkh_status launch_edge_check(hipStream_t s, const rkh_scene& scene, const QsDev& qs, const EdgeIO& io, uint32_t grid_edges,
                             uint32_t grid_b, const EdgeIO* tab_a, const EdgeIO* tab_b, uint32_t n_problems) {
  const uint32_t eb = tab_b ? grid_b : 0u;
  if (grid_edges + eb == 0 || n_problems == 0) return RKH_OK;
  EdgeWalkArgs ka = edge_walk_args_of(scene, qs, io, tab_a, tab_b, grid_edges);
  const dim3 grid(grid_edges + eb, n_problems);
  const int n_env = scene.host.n_env;
  RKH_TRY(with_chain_n<true>(scene.host.n_dof, [&](auto c) {
    constexpr int N = decltype(c)::value;
    const int w = edge_check_shape<N>(n_env, ka.n_pairs, uint64_t(grid.x) * grid.y, &ka.pairs_staged);  // the revolute rule
    with_n<1, 2, 4, 8>(w, [&](auto cw) {
      constexpr int W = decltype(cw)::value;
      hipLaunchKernelGGL((edge_check_kernel<N, W>), grid, dim3(64 * W),
                         (SmemLayoutQsW<N, W>::bytes(n_env, ka.pairs_staged ? ka.n_pairs : 0)), s, ka);
    });
  }));
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

}  // namespace planar_prismatic
}  // namespace rkh
