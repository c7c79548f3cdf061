// propagate_launch.h -- HIP only: hipcc compiles it into the propagate*.hip units, no host compiler reads it (unlike the
// *_device.h headers).  The argument structs of the steer and edge walk kernels and the host-side rules their launchers
// share: chain sizes, argument fills, grids, launch shapes.  Each unit writes its own hipLaunchKernelGGL lines.
#pragma once
#include <algorithm>

#include "propagate_edge_walk.h"
#include "propagate_feval.h"

namespace rkh {

// The arguments of the steer kernels, read through the kernarg segment pointer (propagate_steer_kernels.inl)
struct WaveArgs {
  const SceneDev* sc;
  const PairDev* pairs;
  int n_pairs;
  DynDev dyn;
  EdgeIO io_a, io_b;
  const EdgeIO* tab_a;
  const EdgeIO* tab_b;
  uint32_t grid_a;
  KernelGate gate;
};
typedef const __attribute__((address_space(4))) WaveArgs* WaveArgP;
RKH_DI WaveArgP wave_args() {
  WaveArgP a = (WaveArgP)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(a));
  return a;
}

// The arguments of both edge walk kernels (edge_check_kernel, edge_points_kernel), which read them through the kernarg
// segment pointer: a by-value record indexed at run time -- qs.speed[j], the choice between io_a and io_b -- would be
// copied to scratch.
struct EdgeWalkArgs {
  const SceneDev* sc;
  const PairDev* pairs;
  int n_pairs;
  QsDev qs;
  EdgeIO io_a, io_b;
  const EdgeIO* tab_a;
  const EdgeIO* tab_b;
  uint32_t grid_a;
  int pairs_staged;
};
typedef const __attribute__((address_space(4))) EdgeWalkArgs* EdgeWalkArgP;

// The chain sizes the one-wave kernels are instantiated for (12 joints: the revolute forms only)
template <bool PRISM, class F>
rkh_status with_chain_n(int n, F&& f) {
  if constexpr (PRISM) return with_n<1, 2, 3, 4, 6, 7>(n, f);
  else return with_n<1, 2, 3, 4, 6, 7, 12>(n, f);
}

// The grid of a steer launch of 64 / GL edges per block, and the blocks of its first edge group (*grid_a)
template <int GL>
dim3 steer_grid(uint32_t edges_a, uint32_t edges_b, uint32_t n_problems, const KernelGate& gate, uint32_t* grid_a) {
  constexpr uint32_t G = 64 / GL;
  const uint32_t ga = (edges_a + G - 1) / G, gbk = (edges_b + G - 1) / G;
  *grid_a = ga;
  if (!gate.wave_base) return dim3(ga + gbk, n_problems);
  // compact mapping (G = 1): the kernel only runs while the round has fewer than gate.hi edges in total, so that many
  // blocks are enough -- instead of (bound per problem) x problems blocks that find nothing when the gate is closed
  const uint64_t all = uint64_t(ga + gbk) * n_problems;
  return dim3(uint32_t(std::min<uint64_t>(all, gate.hi)), 1);
}

// The arguments of a steer launch from a scene (its verdict pairs)
inline WaveArgs wave_args_of(const rkh_scene& scene, const DynDev& dyn, const EdgeIO& io, const EdgeIO* tab_a,
                             const EdgeIO* tab_b, uint32_t grid_a, const KernelGate& gate) {
  return WaveArgs{scene.d_scene.get(), scene.d_pairs.get(), scene.n_pairs_verdict, dyn, io, EdgeIO(), tab_a, tab_b, grid_a, gate};
}

// The arguments of an edge walk launch from a scene (pairs_staged = 0: the launch decides)
inline EdgeWalkArgs edge_walk_args_of(const rkh_scene& scene, const QsDev& qs, const EdgeIO& io, const EdgeIO* tab_a,
                                      const EdgeIO* tab_b, uint32_t grid_a) {
  return EdgeWalkArgs{scene.d_scene.get(), scene.d_pairs.get(), scene.n_pairs_verdict, qs, io, EdgeIO(), tab_a, tab_b, grid_a, 0};
}

// The number of waves W of a planar edge_check_kernel launch, by the number of edges (1 for launches of 4096 edges and
// more, 4 below that, 8 below 512) and by what fits 64 KB of LDS (2 where 4 does not fit, 1 where neither does), and
// whether the pair list rides in LDS too.
template <int N>
int edge_check_shape(int n_env, int n_pairs, uint64_t n_edges, int* staged) {
  auto fit = [&](size_t with_pairs, size_t without) { return with_pairs <= 65536 ? 2 : (without <= 65536 ? 1 : 0); };
  const int f1 = fit(SmemLayoutQsW<N, 1>::bytes(n_env, n_pairs), SmemLayoutQsW<N, 1>::bytes(n_env, 0));
  const int f2 = fit(SmemLayoutQsW<N, 2>::bytes(n_env, n_pairs), SmemLayoutQsW<N, 2>::bytes(n_env, 0));
  const int f4 = fit(SmemLayoutQsW<N, 4>::bytes(n_env, n_pairs), SmemLayoutQsW<N, 4>::bytes(n_env, 0));
  const int f8 = fit(SmemLayoutQsW<N, 8>::bytes(n_env, n_pairs), SmemLayoutQsW<N, 8>::bytes(n_env, 0));
  int w = 1;
  *staged = f1 == 2;
  if (n_edges < 4096) {
    if (f4) w = 4, *staged = f4 == 2;
    else if (f2) w = 2, *staged = f2 == 2;
  }
  if (n_edges < 512 && f8) w = 8, *staged = f8 == 2;
  return w;
}

// The points per pass G of an edge_points_kernel launch: 64 for launches of fewer than 2048 edges and chains of at most
// 7 joints (kEdgePointsWide), 32 otherwise
template <int N>
constexpr int kEdgePointsWide = N <= 7 ? 64 : 32;
inline bool edge_points_wide(dim3 grid) { return uint64_t(grid.x) * grid.y < 2048; }

// A launch of `kern`, an edge_points_kernel form of <N, G>: the pair list is staged in LDS if it fits, and more than the
// default 64 KB of dynamic LDS is asked for once per kernel function (*big_lds: the caller's flag of this `kern`).
template <int N, int G, class K>
rkh_status launch_edge_points(K kern, bool* big_lds, hipStream_t s, dim3 grid, int n_env, EdgeWalkArgs ka) {
  // a scene holds fewer than kMaxEnvShapes environment shapes: they always fit next to the block's data
  static_assert(EdgePointsSmem<N, G>::bytes(kMaxEnvShapes, 0) <= 160 * 1024, "edge_points_kernel: LDS over 160 KB");
  const size_t with_pairs = EdgePointsSmem<N, G>::bytes(n_env, ka.n_pairs);
  ka.pairs_staged = with_pairs <= 160 * 1024;
  const size_t smem = ka.pairs_staged ? with_pairs : EdgePointsSmem<N, G>::bytes(n_env, 0);
  if (smem > 65536 && !*big_lds) {
    RKH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    *big_lds = true;
  }
  hipLaunchKernelGGL(kern, grid, dim3(256), smem, s, ka);
  return RKH_OK;
}

// the checks and the chain-size dispatch of every record launch (the depth forms' too)
template <class F>
rkh_status launch_records(const rkh_scene& scene, bool meshes, F&& f) {
  if (scene.host.planar || (scene.host.has_meshes && !meshes) || !scene.d_pair_ids.get() || scene.n_pairs > kMaxRecordPairs) {
    set_error(meshes ? "record queries: 3D scenes only" : "record queries: 3D scenes without vertex-set shapes only");
    return RKH_ERR_UNSUPPORTED;
  }
  RKH_TRY((with_n<1, 2, 3, 4, 6, 7, 12>(scene.host.n_dof, f)));
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

}  // namespace rkh
