// propagate_depth.hip -- the depth forms of the record kernels (min_distance_depth_kernel, collision_depth_kernel: the
// two record kernels' bodies over pair_distance_depth / pair_record_depth of proximity_record_device.h, i.e. with the
// penetration depth and contact normal of epa_device.h for vertex-set pairs) and the pair-by-pair gjk_pair_depth_kernel of
// the diagnostic entry: the bodies of propagate_records.h with MODE = kRecDepth, with their three launchers and nothing
// else.  A module of their own: the polytope arrays give them a private segment, and a kernel added to propagate.hip's
// module has moved the registers of the ones it holds.
#include "propagate_launch.h"
#include "propagate_records.h"

namespace rkh {

template <int N>
__global__ __launch_bounds__(64) void min_distance_depth_kernel(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                                                 const PairIdDev* __restrict__ ids, int n_pairs,
                                                                 const double* __restrict__ x, uint32_t B, RecordOut out,
                                                                 double* __restrict__ normal) {
  min_distance_records_body<N, kRecDepth>(sc, pairs, ids, n_pairs, x, B, out, normal);
}

template <int N>
__global__ __launch_bounds__(64) void collision_depth_kernel(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                                              const PairIdDev* __restrict__ ids, int n_pairs,
                                                              const double* __restrict__ x, uint32_t B, uint32_t cap, RecordOut out,
                                                              double* __restrict__ normal) {
  collision_records_body<N, kRecDepth>(sc, pairs, ids, n_pairs, x, B, cap, out, normal);
}

__global__ __launch_bounds__(64) void gjk_pair_depth_kernel(const rkh_shape* __restrict__ a, const rkh_shape* __restrict__ b,
                                                             uint32_t n, const double* __restrict__ pool, double* __restrict__ dist,
                                                             double* __restrict__ point1, double* __restrict__ point2,
                                                             double* __restrict__ normal) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  auto conv = [](const rkh_shape& s) {
    ShapeG g;
    g.kind = s.kind;
    g.pos = mk3(s.pose.pos[0], s.pose.pos[1], s.pose.pos[2]);
    g.q = d4{s.pose.quat[0], s.pose.quat[1], s.pose.quat[2], s.pose.quat[3]};
    g.d0 = s.dims[0]; g.d1 = s.dims[1]; g.d2 = s.dims[2];
    return g;
  };
  const ProxRecordN r = pair_record_depth(PR_GJK, conv(a[i]), conv(b[i]), pool);
  dist[i] = r.dist;
  st3(point1 + 3 * size_t(i), r.p1);
  st3(point2 + 3 * size_t(i), r.p2);
  st3(normal + 3 * size_t(i), r.nrm);
}

// A scene without vertex-set shapes has no pair for the depth forms to answer differently, but its records still gain
// their normals: the same kernels serve it.
rkh_status launch_min_distance_records_depth(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, RecordOut out,
                                             double* d_normal) {
  if (B == 0) return RKH_OK;
  return launch_records(scene, true, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((min_distance_depth_kernel<N>), dim3(B), dim3(64), (SmemLayoutQs<N, 64>::bytes(scene.host.n_env)), s,
                       scene.d_scene.get(), scene.d_pairs.get(), scene.d_pair_ids.get(), scene.n_pairs, d_x, B, out, d_normal);
  });
}

rkh_status launch_collision_records_depth(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, uint32_t cap,
                                          RecordOut out, double* d_normal) {
  if (B == 0) return RKH_OK;
  return launch_records(scene, true, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((collision_depth_kernel<N>), dim3(B), dim3(64), (SmemLayoutQs<N, 64>::bytes(scene.host.n_env)), s,
                       scene.d_scene.get(), scene.d_pairs.get(), scene.d_pair_ids.get(), scene.n_pairs, d_x, B, cap, out, d_normal);
  });
}

rkh_status launch_gjk_pair_depth(hipStream_t s, const rkh_shape* d_a, const rkh_shape* d_b, uint32_t n, const double* d_pool,
                                 double* d_dist, double* d_point1, double* d_point2, double* d_normal) {
  if (n == 0) return RKH_OK;
  hipLaunchKernelGGL(gjk_pair_depth_kernel, dim3((n + 63) / 64), dim3(64), 0, s, d_a, d_b, n, d_pool, d_dist, d_point1, d_point2,
                     d_normal);
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

}  // namespace rkh
