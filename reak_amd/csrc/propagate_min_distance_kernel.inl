// propagate_min_distance_kernel.inl -- HIP only; the text of min_distance_kernel.  A unit includes it inside
// the namespace its form lives in (rkh, rkh::prismatic, rkh::planar_prismatic), after propagate_launch.h and with two
// constants of that namespace in scope (see propagate_steer_kernels.inl): `constexpr bool kPrismatic`, the joint kind, and
// `constexpr bool kPlanarForm`, true for the form that serves planar chains only (proximity_min_planar with the joint
// kind as given; proximity_min sends a revolute planar scene there at run time).

// Kernel: exact minimum proxy-pair distance for B states (no culling).
template <int N>
__global__ __launch_bounds__(64) void min_distance_kernel(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                                           int n_pairs, const double* __restrict__ x, uint32_t B,
                                                           double* __restrict__ dist) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  BlockLdsQs<N, 64>& lds = *reinterpret_cast<BlockLdsQs<N, 64>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + SmemLayoutQs<N, 64>::block_bytes);
  const uint32_t e = blockIdx.x;
  if (e >= B) return;
  const int lane = threadIdx.x;
  constexpr int D = 2 * N;
  stage_chain<N>(sc, lds.joints, lds.base, lane);
  stage_env(sc, env_lds, lane);
  GroupWsQs<N>& ws = lds.g[0];
  if (lane < D) ws.x[lane] = x[uint64_t(e) * D + lane];
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);
  double dmin;
  if constexpr (kPlanarForm) {
    dmin = proximity_min_planar<N, 64, kPrismatic>(sc, cp, lds.base, env_lds, pairs, n_pairs, ws, lane, 0);
  } else {  // (prismatic scenes hold no vertex sets: their form leaves the support-map query out)
    dmin = proximity_min<N, 64, GroupWsQs<N>, !kPrismatic, kPrismatic>(sc, cp, lds.base, env_lds, pairs, n_pairs, ws,
                                                                       lds.sink[lane], lane, 0, false, false);
  }
  if (lane == 0) dist[e] = dmin;
}
