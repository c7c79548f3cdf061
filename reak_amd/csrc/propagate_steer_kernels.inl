// propagate_steer_kernels.inl -- HIP only; the text of propagate_kernel and state_derivative_kernel.
// A unit includes it inside the namespace its forms live in (rkh: propagate.hip; rkh::prismatic: propagate_prismatic.hip),
// after propagate_launch.h and with that namespace's `constexpr bool kPrismatic`, the joint kind, in scope.  (Not a
// function the entries call: a callee is simplified before it is inlined, and the kernels change)

// ---------------------------------------------------------------------------------------------
// Kernel: steer edges.  Two edge groups per launch (planner: this round's steer candidates + the
// previous round's goal probes); 64/GL edges per wave.
// GL = 64 (one wave per edge, the latency mapping: rounds of fewer waves than the chip has SIMDs) may use the whole
// register file of its SIMD; four edges per wave (GL = 16) is the throughput form and keeps two waves per SIMD.
// DUO (GL = 64 only): two waves per edge.  Both run this body in step -- the same loads, the same RK4 glue, the same
// control flow, so every block barrier is met by both -- and differ inside state_derivative_duo; only the first wave
// writes results.
template <int N, int GL, bool GJK, bool DUO = false>
__global__ __launch_bounds__(DUO ? 128 : 64, GL == 64 ? 1 : 2) void propagate_kernel(WaveArgs) {
  static_assert(!DUO || GL == 64, "two waves per edge: one edge per block");
  // Every argument is read through the kernarg segment pointer at its point of use (by-value parameters are loaded in the
  // entry block and stay live in scalar registers; once those run out they are spilled into vector-register lanes, and
  // the EdgeIO / DynDev / KernelGate copies alone are ~170 dwords: the kernel then needed 256 registers + 185 spilled)
  const SceneDev* __restrict__ sc = wave_args()->sc;
  const PairDev* __restrict__ pairs = wave_args()->pairs;
  const int n_pairs = wave_args()->n_pairs;
  const uint32_t grid_a = wave_args()->grid_a;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  if (steer_gate_closed(&wave_args()->gate)) return;  // the planner's per-round choice between the kernel mappings
  constexpr int G = 64 / GL;
  BlockLds<N, GL>& lds = *reinterpret_cast<BlockLds<N, GL>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + SmemLayout<N, GL>::block_bytes);
  // blockIdx.y selects the planning problem when per-problem EdgeIO tables are given
  bool group_b = blockIdx.x >= grid_a;
  uint32_t problem = blockIdx.y;
  uint32_t blk = group_b ? blockIdx.x - grid_a : blockIdx.x;
  if (wave_args()->gate.wave_base) {  // compact mapping (one edge per wave): block L of a 1-D grid takes working edge L
    const uint32_t L = blockIdx.x;
    if (L >= wave_args()->gate.wave_base[wave_args()->gate.n_segments]) return;
    const uint32_t seg = segment_of(wave_args()->gate.wave_base, wave_args()->gate.n_segments, L);
    problem = seg >> 1;
    group_b = (seg & 1u) != 0u;
    blk = L - wave_args()->gate.wave_base[seg];
  }
  auto edge_io = [&]() -> const EdgeIO* {
    WaveArgP A = wave_args();
    if (A->tab_a) return (group_b ? A->tab_b : A->tab_a) + problem;
    const char* ka = (const char*)(const void*)A;
    return (const EdgeIO*)(ka + (group_b ? offsetof(WaveArgs, io_b) : offsetof(WaveArgs, io_a)));
  };
  const uint32_t B = edge_io()->d_B ? *edge_io()->d_B : edge_io()->B;
  const int lane = DUO ? int(threadIdx.x & 63u) : int(threadIdx.x);
  const int wave = DUO ? int(threadIdx.x >> 6) : 0;
  const bool writer = !DUO || wave == 0;  // the wave whose results leave the block
  const int g = lane / GL, gl = lane % GL, gb = g * GL;
  const uint32_t e0 = blk * G;
  if (e0 >= B) return;
  const uint32_t e = e0 + g;
  const bool edge_valid = e < B;
  const uint32_t ec = edge_valid ? e : e0;  // idle groups shadow the wave's first edge, results discarded
  constexpr int D = 2 * N;
  stage_chain<N>(sc, lds.joints, lds.base, lane);
  stage_env(sc, env_lds, lane);
  GroupWs<N>& ws = lds.g[g];
  const uint32_t si = edge_source_row(*edge_io(), ec);
  const uint64_t trow = edge_target_row(*edge_io(), ec);
  const double a_d = (gl < D) ? edge_io()->src[uint64_t(si) * edge_io()->src_stride + gl] : 0.0;
  const double b_d = (gl < D) ? edge_io()->tgt[trow * edge_io()->tgt_stride + gl] : 0.0;
  const double lo = (gl < D) ? wave_args()->dyn.lower[gl] : 0.0;
  const double hi = (gl < D) ? wave_args()->dyn.upper[gl] : 0.0;
  if (gl < D) ws.b[gl] = b_d;
  double* __restrict__ record = (edge_valid && writer) ? edge_io()->record : nullptr;
  const int record_stride = edge_io()->record_stride;
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);

  double x = a_d;
  uint32_t n_free = 0;
  bool singular = false;   // a live edge met a singular mass matrix
  bool alive = true;       // this edge is still stepping
  uint32_t n_exec = 0;     // steps integrated for this edge (KernelGate::steps_exec)
  if (record && gl < D) record[(uint64_t(e) * record_stride + 0) * D + gl] = x;

  // steps of this edge: the launch's schedule, or (EdgeIO::frac) those of the edge's own travel fraction
  int n_steps = wave_args()->dyn.n_steps;
  if (edge_io()->frac) n_steps = edge_step_count(edge_io()->frac[ec], wave_args()->dyn.full_time, wave_args()->dyn.dt);
  if (edge_io()->mode == EDGE_POINT) {  // is_free(target): bounds, then proximity; no propagation
    n_steps = 0;
    x = b_d;
    const bool oob = (gl < D) && hyperbox_out(lo, hi, x);
    const unsigned long long m = __ballot(oob);
    const unsigned long long gm = (GL == 64) ? m : ((m >> gb) & ((1ull << (GL & 63)) - 1ull));
    bool free_pt = gm == 0ull;
    if (gl < D) ws.x[gl] = x;
    __syncthreads();
    const double dmin = proximity_min<N, GL, GroupWs<N>, GJK, kPrismatic>(sc, cp, lds.base, env_lds, pairs, n_pairs, ws, lds.sink[lane], gl, gb, true, !free_pt);
    if (dmin < 0.0) free_pt = false;
    if (edge_valid && gl == 0 && writer) edge_io()->accept[e] = free_pt ? 1 : 0;
  }

  for (int k = 0; k < n_steps; ++k) {
    // distance(x_current, x_goal) > goal_proximity_threshold
    const double dist = group_norm<N>(ws, x - b_d, gl);
    if (!(dist > wave_args()->dyn.goal_tol)) alive = false;
    if (!__any(alive)) break;
    if (alive) ++n_exec;
    // PD law, zero-order hold over the step
    if (gl < D) ws.x[gl] = x;
    __syncthreads();
    if (gl < N)
      ws.u[gl] = pd_input(wave_args()->dyn.kp, wave_args()->dyn.kd, wave_args()->dyn.u_max, ws.b[2 * gl], ws.x[2 * gl],
                          ws.b[2 * gl + 1], ws.x[2 * gl + 1]);
    // runge_kutta4_integrate_impl, time_step = dt: one call site for f(x,u), the stages of rk4_stage (steer_edge.h) in a
    // rolled loop.  The re-prime after the last iteration is dead in the reference and is not evaluated.
    const double h = wave_args()->dyn.dt;
    double xe = x;  // end_point
    {
      double w = xe, k1 = 0.0, k2 = 0.0, k3 = 0.0;
      bool sing_now = false;
      const int n_evals = 4 * wave_args()->dyn.inner[k];
#pragma unroll 1
      for (int ev = 0; ev < n_evals; ++ev) {
        if (gl < D) ws.x[gl] = xe;
        __syncthreads();
        const double dp = DUO ? state_derivative_duo<N>(sc, cp, lds.joints, lds.base, ws, lds.sink[lane], gl, wave, &sing_now)
                              : state_derivative<N, GL, kPrismatic>(sc, cp, lds.joints, lds.base, ws, lds.sink[lane], gl, gb, &sing_now);
        rk4_stage(ev & 3, h, dp, xe, w, k1, k2, k3);
      }
      if (sing_now && alive) {
        singular = true;
        alive = false;
      }
    }
    // is_free(x_next): hyperbox bounds, then proximity
    const bool oob = (gl < D) && hyperbox_out(lo, hi, xe);
    {
      const unsigned long long m = __ballot(oob);
      const unsigned long long gm = (GL == 64) ? m : ((m >> gb) & ((1ull << (GL & 63)) - 1ull));
      if (gm != 0ull) alive = false;
    }
    if (!__any(alive)) break;
    if (gl < D) ws.x[gl] = xe;
    __syncthreads();
    const double dmin = proximity_min<N, GL, GroupWs<N>, GJK, kPrismatic>(sc, cp, lds.base, env_lds, pairs, n_pairs, ws, lds.sink[lane], gl, gb, true, !alive);
    if (dmin < 0.0) alive = false;
    if (alive) {
      x = xe;
      ++n_free;
      if (record && gl < D) record[(uint64_t(e) * record_stride + n_free) * D + gl] = x;
    }
  }
  if (singular && gl == 0 && edge_valid && writer) atomicExch(edge_io()->err_flag, int(RKH_ERR_SINGULAR));
  if (edge_valid && gl < D && writer) edge_io()->x_out[uint64_t(e) * D + gl] = x;
  if (edge_valid && gl == 0 && writer) edge_io()->steps_free[e] = n_free;
  if (wave_args()->gate.steps_exec && edge_valid && gl == 0 && n_exec && writer)
    atomicAdd(wave_args()->gate.steps_exec, (unsigned long long)n_exec);
  if (edge_io()->mode != EDGE_PLAIN) {
    const double n_ar = group_norm<N>(ws, a_d - x, gl);
    const double n_ab = group_norm<N>(ws, a_d - b_d, gl);
    const double n_rb = group_norm<N>(ws, x - b_d, gl);
    const int acc = edge_accept(edge_io()->mode, n_ar, n_ab, n_rb, edge_io()->best_case, ec, edge_io()->steer_tol, kNoWalk);
    if (edge_valid && gl == 0 && writer) {
      if (acc != kNoAccept) edge_io()->accept[e] = uint8_t(acc);
      else if (edge_io()->mode == EDGE_GOAL_PROBE) edge_io()->goal_dist[si - 1] = goal_probe_steerable(n_ab, n_rb);
    }
  }
}

// Kernel: x' = f(x,u) for B states (one wave each); also exports M and the bias force.
template <int N>
__global__ __launch_bounds__(64) void state_derivative_kernel(const SceneDev* __restrict__ sc, const double* __restrict__ x,
                                                               const double* __restrict__ u, uint32_t B,
                                                               double* __restrict__ pd, double* __restrict__ M,
                                                               double* __restrict__ f, int* __restrict__ err_flag) {
  __shared__ BlockLds<N, 64> lds;
  const uint32_t e = blockIdx.x;
  if (e >= B) return;
  const int lane = threadIdx.x;
  constexpr int D = 2 * N;
  stage_chain<N>(sc, lds.joints, lds.base, lane);
  GroupWs<N>& ws = lds.g[0];
  if (lane < D) ws.x[lane] = x[uint64_t(e) * D + lane];
  if (lane < N) ws.u[lane] = u[uint64_t(e) * N + lane];
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);
  bool singular = false;
  const double dp = state_derivative<N, 64, kPrismatic>(sc, cp, lds.joints, lds.base, ws, lds.sink[lane], lane, 0, &singular);
  if (lane < D) pd[uint64_t(e) * D + lane] = dp;
  if (singular && lane == 0) atomicExch(err_flag, int(RKH_ERR_SINGULAR));
  // exports for the kernel-level parity tests: the symmetric M is rebuilt from Mf (ws.M now holds its
  // Cholesky factor); the bias force was parked in ws.tmp by state_derivative.
  if (M)
    for (int t = lane; t < N * N; t += 64) {
      const int i = t / N, j = t % N;
      const int lo = i < j ? i : j, hi = i < j ? j : i;
      M[uint64_t(e) * N * N + t] = (i == j) ? ws.Mf[i][i] : 0.5 * (ws.Mf[lo][hi] + ws.Mf[hi][lo]);
    }
  if (f && lane < N) f[uint64_t(e) * N + lane] = ws.tmp[lane];
}
