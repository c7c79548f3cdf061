// propagate_edge_points_kernel.inl -- HIP only; the text of edge_points_kernel (its mapping: propagate_edge_walk.h).
// A unit includes it inside the namespace its forms live in (rkh: propagate.hip; rkh::prismatic:
// propagate_prismatic.hip), after propagate_launch.h and with that namespace's `constexpr bool kPrismatic` in scope
// (see propagate_steer_kernels.inl).
template <int N, bool GJK, int G>
__global__ __launch_bounds__(256) void edge_points_kernel(EdgeWalkArgs) {
  EdgeWalkArgP ka = (EdgeWalkArgP)__builtin_amdgcn_kernarg_segment_ptr();
  const SceneDev* __restrict__ sc = ka->sc;
  const PairDev* __restrict__ pairs = ka->pairs;
  const int n_pairs = ka->n_pairs, pairs_staged = ka->pairs_staged;
  const uint32_t grid_a = ka->grid_a;
  const EdgeIO* __restrict__ tab_a = ka->tab_a;
  const EdgeIO* __restrict__ tab_b = ka->tab_b;
  const auto& qs = ka->qs;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr int T = EdgePointsCfg::T, QCAP = EdgePointsCfg::QCAP;
  EdgePointsLds<N, G>& lds = *reinterpret_cast<EdgePointsLds<N, G>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + EdgePointsSmem<N, G>::block_bytes);
  const bool group_b = blockIdx.x >= grid_a;
  const EdgeIO* iop = tab_a ? (group_b ? &tab_b[blockIdx.y] : &tab_a[blockIdx.y]) : nullptr;
  const __attribute__((address_space(4))) EdgeIO* iok = group_b ? &ka->io_b : &ka->io_a;
#define RKH_IO(f) (iop ? iop->f : iok->f)
  const uint32_t B = RKH_IO(d_B) ? *RKH_IO(d_B) : RKH_IO(B);
  const uint32_t e = group_b ? blockIdx.x - grid_a : blockIdx.x;
  if (e >= B) return;
  const int tid = threadIdx.x, lane = tid & 63;
  stage_chain<N>(sc, lds.joints, lds.base, lane);  // (every wave writes the same values)
  stage_env(sc, env_lds, lane);
  {
    const int n_words = sc->n_robot * int(sizeof(ShapeDev) / sizeof(double));
    for (int i = tid; i < n_words; i += T) reinterpret_cast<double*>(lds.robot)[i] = reinterpret_cast<const double*>(sc->robot)[i];
    if (pairs_staged) {
      PairDev* pl = reinterpret_cast<PairDev*>(env_lds + sc->n_env);
      for (int i = tid; i < n_pairs; i += T) pl[i] = pairs[i];
      pairs = pl;
    }
  }
  const int mode = RKH_IO(mode);
  if (tid < N) {
    const uint32_t si = edge_source_row(RKH_IO(src_idx), RKH_IO(d_src_first), e);
    const uint64_t trow = edge_target_row(RKH_IO(tgt_idx), RKH_IO(d_tgt_off), e);
    lds.a[tid] = RKH_IO(src)[uint64_t(si) * RKH_IO(src_stride) + tid];
    lds.b[tid] = RKH_IO(tgt)[trow * RKH_IO(tgt_stride) + tid];
  }
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);
  const int n_robot = sc->n_robot;

  // exact left-to-right euclidean norm of the N-vector whose component d thread d holds (vect_distance_metrics.hpp:126-137)
  auto norm_n = [&](double diff) {
    if (tid < N) lds.res[tid] = diff * diff;
    __syncthreads();
    double sacc = 0.0;
#pragma unroll
    for (int d = 0; d < N; ++d) sacc = sacc + lds.res[d];
    __syncthreads();
    return sqrt(sacc);
  };
  // is_free's proximity half for the points flagged 1 in lds.flags (their coordinates in lds.pts): sets bit 1 of the
  // flag of every point with a proxy pair closer than 0.  Block-uniform control flow throughout.
  auto test_points = [&](int n_pts) {
    for (int idx = tid; idx < G * N; idx += T) {   // half-angle sin / cos (revolute_joint_3D::doMotion)
      const int t = idx % G, j = idx / G;
      if (t >= n_pts) continue;
      double sn, cs;
      sincos(0.5 * (lds.pts[j][t] * qs.speed[j]), &sn, &cs);
      lds.cs[j][0][t] = cs;
      lds.cs[j][1][t] = sn;
    }
    __syncthreads();
    if (tid < G) {  // revolute_joint_3D / rigid_link_3D kinematics, position + orientation only: this lane's point
      const int t = tid;
      d3 pos = ld3(lds.base);
      d4 Q = ld4(lds.base + 3);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int jb = j * 32;
        if (sc->branch_start[j]) {  // a new branch: base frame * mount pose (rigid_link_3D::doMotion from frame 0)
          const d4 bq = ld4(lds.base + 3);
          pos = ld3(lds.base) + mul(rotmat(bq), ld3(sc->mount_pos[j]));
          Q = qmul(bq, ld4(sc->mount_quat[j]));
        }
        const d3 axis_n = cget3(cp, jb + JC_AXISN);
        const double c2 = lds.cs[j][0][t], s2 = lds.cs[j][1][t];
        d4 EQ;
        if (kPrismatic && ((sc->prismatic_mask >> j) & 1u)) {  // prismatic_joint_3D: translate by R(Q) (q a), keep Q
          pos = pos + mul(rotmat(Q), (lds.pts[j][t] * qs.speed[j]) * cget3(cp, jb + JC_AXIS));
          EQ = Q;
        } else {
          const d4 tq = d4{c2, axis_n.x * s2, axis_n.y * s2, axis_n.z * s2};
          EQ = qmul(Q, tq);
        }
        lds.E[j][0][t] = pos.x; lds.E[j][1][t] = pos.y; lds.E[j][2][t] = pos.z;
        lds.E[j][3][t] = EQ.w; lds.E[j][4][t] = EQ.x; lds.E[j][5][t] = EQ.y; lds.E[j][6][t] = EQ.z;
        const m33 Rm = rotmat(EQ);
        pos = pos + mul(Rm, cget3(cp, jb + JC_OFFP));
        Q = qmul(EQ, d4{cget(cp, jb + JC_OFFQ), cget(cp, jb + JC_OFFQ + 1), cget(cp, jb + JC_OFFQ + 2),
                        cget(cp, jb + JC_OFFQ + 3)});
      }
    }
    __syncthreads();
    for (int idx = tid; idx < G * n_robot; idx += T) {  // robot shapes -> global pose (pose_3D::getGlobalPose, pose_3D.hpp:102-110)
      const int t = idx % G, r = idx / G;
      const ShapeDev& sh = lds.robot[r];
      const int j = sh.link;
      const d3 pp = d3{lds.E[j][0][t], lds.E[j][1][t], lds.E[j][2][t]};
      const d4 pq = d4{lds.E[j][3][t], lds.E[j][4][t], lds.E[j][5][t], lds.E[j][6][t]};
      const d3 gp = pp + qrot(pq, ld3(sh.pos));
      const d4 gq = qmul(pq, ld4(sh.quat));
      lds.R[r][0][t] = gp.x; lds.R[r][1][t] = gp.y; lds.R[r][2][t] = gp.z;
      lds.R[r][3][t] = gq.w; lds.R[r][4][t] = gq.x; lds.R[r][5][t] = gq.y; lds.R[r][6][t] = gq.z;
    }
    __syncthreads();
    // bounding-sphere cull of every (pair, point), survivors -> queue -> closed forms (see above)
    int p_lo = 0, p_step = n_pairs;
    while (p_lo < n_pairs) {
      const int p_hi = (p_lo + p_step < n_pairs) ? p_lo + p_step : n_pairs;
      {  // a wave's lanes are consecutive points of ONE pair (two pairs when G = 32): the pair's constants are uniform
        constexpr int PPB = T / G;   // pairs per block iteration
        const int t = tid % G;
        const bool live = lds.flags[t] == 5u;
        auto cull = [&](int p) {
          const PairDev pr = pairs[p];
          const ShapeDev& rs = lds.robot[pr.robot];
          const ShapeDev& es = env_lds[pr.env];
          const d3 ca = d3{lds.R[pr.robot][0][t], lds.R[pr.robot][1][t], lds.R[pr.robot][2][t]}, cb = ld3(es.pos);
          const d3 dc = pr.s1_is_robot ? cb - ca : ca - cb;
          const double r1 = pr.s1_is_robot ? rs.brad : es.brad, r2 = pr.s1_is_robot ? es.brad : rs.brad;
          const double sq = ((0.0 + dc.x * dc.x) + dc.y * dc.y) + dc.z * dc.z, rr = r1 + r2;
          if (sq > (rr * rr) * (1.0 + 1e-9)) return false;   // clearly apart: the exact test below skips it too
          return !(sqrt(sq) - r1 - r2 > 0.0);                // |c2 - c1| - r1 - r2 > 0 (proxy_query_model.cpp:384-389, minimum 0)
        };
        int p = p_lo + tid / G;
        for (; p + 3 * PPB < p_hi; p += 4 * PPB) {  // four independent pairs in flight
          const bool k0 = cull(p), k1 = cull(p + PPB), k2 = cull(p + 2 * PPB), k3 = cull(p + 3 * PPB);
          if (live) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const bool k = u == 0 ? k0 : (u == 1 ? k1 : (u == 2 ? k2 : k3));
              if (k) {
                const uint32_t slot = atomicAdd(&lds.q_cnt, 1u);
                if (slot < uint32_t(QCAP)) lds.queue[slot] = uint32_t(t) | (uint32_t(p + u * PPB) << 8);
              }
            }
          }
        }
        for (; p < p_hi; p += PPB) {
          if (live && cull(p)) {
            const uint32_t slot = atomicAdd(&lds.q_cnt, 1u);
            if (slot < uint32_t(QCAP)) lds.queue[slot] = uint32_t(t) | (uint32_t(p) << 8);
          }
        }
      }
      __syncthreads();
      const uint32_t cnt = lds.q_cnt;
      __syncthreads();
      if (tid == 0) lds.q_cnt = 0u;
      if (cnt > uint32_t(QCAP)) {  // (block-uniform) does not fit: slices of QCAP / G pairs always do
        p_step = QCAP / G;
        __syncthreads();
        continue;
      }
      for (uint32_t i = tid; i < cnt; i += T) {
        const uint32_t ent = lds.queue[i];
        const int t = int(ent & 255u);
        if (lds.flags[t] != 5u) continue;              // this point already has a colliding pair
        const PairDev pr = pairs[ent >> 8];
        const ShapeDev& rs = lds.robot[pr.robot];
        const ShapeDev& es = env_lds[pr.env];
        ShapeG A, Bv;
        A.kind = rs.kind;
        A.pos = d3{lds.R[pr.robot][0][t], lds.R[pr.robot][1][t], lds.R[pr.robot][2][t]};
        A.q = d4{lds.R[pr.robot][3][t], lds.R[pr.robot][4][t], lds.R[pr.robot][5][t], lds.R[pr.robot][6][t]};
        A.d0 = rs.dims[0]; A.d1 = rs.dims[1]; A.d2 = rs.dims[2];
        Bv.kind = es.kind;
        Bv.pos = ld3(es.pos);
        Bv.q = ld4(es.quat);
        Bv.d0 = es.dims[0]; Bv.d1 = es.dims[1]; Bv.d2 = es.dims[2];
        const double d = pr.s1_is_robot ? pair_distance<GJK>(pr.routine, A, Bv, sc->mesh_verts)
                                        : pair_distance<GJK>(pr.routine, Bv, A, sc->mesh_verts);
        if (d < 0.0) atomicOr(&lds.flags[t], 2u);
      }
      __syncthreads();
      p_lo = p_hi;
    }
  };
  // hyperbox bounds of point t (manip_free_workspace.hpp:79-99; lower > upper: a wrapped coordinate)
  auto out_of_bounds = [&](int t) {
    bool oob = false;
#pragma unroll
    for (int d = 0; d < N; ++d) oob |= hyperbox_out(qs.lower[d], qs.upper[d], lds.pts[d][t]);
    return oob;
  };

  const double a_d = tid < N ? lds.a[tid] : 0.0, b_d = tid < N ? lds.b[tid] : 0.0;
  if (mode == EDGE_POINT) {
    // is_free(target): hyperbox bounds, then proximity (manip_free_workspace.hpp:79-99,154-156)
    if (tid < N) lds.pts[tid][0] = b_d;
    if (tid == 0) lds.q_cnt = 0u;
    __syncthreads();
    if (tid < G) lds.flags[tid] = (tid == 0 && !out_of_bounds(0)) ? 5u : 0u;
    __syncthreads();
    test_points(1);
    if (tid < N) RKH_IO(x_out)[uint64_t(e) * N + tid] = b_d;
    if (tid == 0) {
      RKH_IO(steps_free)[e] = 1;
      RKH_IO(accept)[e] = (lds.flags[0] == 5u) ? 1 : 0;
    }
    return;
  }
  const double dist_tot = norm_n(a_d - b_d);
  const double fraction = RKH_IO(frac) ? RKH_IO(frac)[e] : qs.fraction;
  double result = a_d;       // component tid of the returned point
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
      // dist_cur of this thread's point and of the pass's last one: cur + min_interval, repeatedly (":157 dist_cur += min_interval")
      double my = cur, last = cur;
      const int t_mine = tid < G ? tid : 0;
#pragma unroll 8
      for (int t = 0; t < G; ++t) {
        if (t <= t_mine) my = my + qs.min_interval;
        last = last + qs.min_interval;
      }
      if (!((cur + qs.min_interval) < dist_inter)) break;  // not even the first point is on the edge (block-uniform)
      if (tid < G) {
        const bool valid = my < dist_inter;
        const double f = my / dist_tot;
#pragma unroll
        for (int d = 0; d < N; ++d) lds.pts[d][tid] = lds.a[d] + (lds.b[d] - lds.a[d]) * f;
        lds.flags[tid] = valid ? (out_of_bounds(tid) ? 4u : 5u) : 0u;
      }
      if (tid == 0) lds.q_cnt = 0u;
      __syncthreads();
      test_points(G);
      if (tid < 64) {  // the first point on the edge that fails the predicate, and how many points are on the edge
        const uint32_t fl = tid < G ? lds.flags[tid] : 0u;
        const unsigned long long mv = __ballot((fl & 4u) != 0u), mf = __ballot(fl == 5u);
        const unsigned long long bad = mv & ~mf;
        if (tid == 0) {
          lds.scan[0] = bad ? uint32_t(__builtin_ctzll(bad)) : uint32_t(G);
          lds.scan[1] = uint32_t(__builtin_popcountll(mv));
        }
      }
      __syncthreads();
      const int first_bad = int(lds.scan[0]), n_valid = int(lds.scan[1]);
      if (first_bad < G) {
        n_checked += uint32_t(first_bad + 1);
        if (first_bad > 0 && tid < N) last_result = lds.pts[tid][first_bad - 1];
        collided = true;
        break;
      }
      n_checked += uint32_t(n_valid);
      if (tid < N) last_result = lds.pts[tid][n_valid - 1];
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
  if (tid < N) RKH_IO(x_out)[uint64_t(e) * N + tid] = result;
  if (tid == 0) RKH_IO(steps_free)[e] = n_checked;
  if (mode != EDGE_PLAIN) {
    const double n_ar = norm_n(a_d - result);
    const double n_ab = dist_tot;
    const double n_rb = norm_n(result - b_d);
    const int acc = edge_accept(mode, n_ar, n_ab, n_rb, RKH_IO(best_case), e, RKH_IO(steer_tol), completed_walk ? 1 : 0);
    if (tid == 0) {
      if (acc != kNoAccept) RKH_IO(accept)[e] = uint8_t(acc);
      else if (mode == EDGE_GOAL_PROBE)
        RKH_IO(goal_dist)[edge_source_row(RKH_IO(src_idx), RKH_IO(d_src_first), e) - 1] = goal_probe_interpolated(n_ab, n_rb);
    }
  }
#undef RKH_IO
}
