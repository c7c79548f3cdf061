// propagate_edge_check_kernel.inl -- HIP only; the text of edge_check_kernel.  A unit includes it inside the
// namespace its form lives in (rkh: propagate.hip; rkh::planar_prismatic: propagate_planar_qs_prismatic.hip), after
// propagate_launch.h and with that namespace's `constexpr bool kPrismatic` in scope (see propagate_steer_kernels.inl).
template <int N, int W>
__global__ __launch_bounds__(64 * W) void edge_check_kernel(EdgeWalkArgs) {
  EdgeWalkArgP ka = (EdgeWalkArgP)__builtin_amdgcn_kernarg_segment_ptr();
  const SceneDev* __restrict__ sc = ka->sc;
  const int n_pairs = ka->n_pairs;
  const uint32_t grid_a = ka->grid_a;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  BlockLdsQsW<N, W>& lds = *reinterpret_cast<BlockLdsQsW<N, W>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + SmemLayoutQsW<N, W>::block_bytes);
  const bool group_b = blockIdx.x >= grid_a;
  const EdgeIO* iok = (const EdgeIO*)(group_b ? &ka->io_b : &ka->io_a);
  const EdgeIO io = ka->tab_a ? (group_b ? ka->tab_b[blockIdx.y] : ka->tab_a[blockIdx.y]) : *iok;
  const uint32_t B = io.d_B ? *io.d_B : io.B;
  const uint32_t e = group_b ? blockIdx.x - grid_a : blockIdx.x;
  if (e >= B) return;
  const PairDev* pairs = edge_check_stage<N, W>(sc, ka->pairs, n_pairs, ka->pairs_staged, lds, env_lds);
  edge_walk<N, W, kPrismatic>(sc, pairs, n_pairs, *(const QsDev*)&ka->qs, io, lds, env_lds, e);
}
