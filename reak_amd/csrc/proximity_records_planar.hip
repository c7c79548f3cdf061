// proximity_records_planar.hip -- the record queries of planar scenes (rkh_min_distance_records_2d,
// rkh_collision_records_2d): what proxy_query_pair_2D::findMinimumDistance()->getLastResult() and gatherCollisionPoints
// hold (geometry/proximity/proxy_query_model.cpp:163-187 and :189-208; proximity_record_2D.hpp:47-58).
//
// A translation unit of its own that holds nothing else: the two kernels, what they share and their launchers.  One wave
// per state; chain constants, environment shapes and the frames of the configuration live in LDS, the pair list is read
// from memory in finder order (pair index = finder rank: the planar builder keeps createProxFinderList's order, :75-161).
// One form serves revolute and prismatic planar chains: SceneDev::prismatic_mask is read at run time (uniform over the
// launch) and the revolute arithmetic is exactly proximity_min_planar's where the bit is clear, so the distances are
// rkh_min_distance's bit for bit on both kinds of chain.
#include <hip/hip_runtime.h>

#include <cmath>

#include "proximity_record_planar_device.h"
#include "rkh_internal.h"

namespace rkh {

constexpr int kMaxPlanarRobotShapes = 2 * kMaxDof;
constexpr int kMaxPlanarRecordPairs = kMaxPlanarRobotShapes * kMaxEnvShapes;  // every pair of a planar scene has a finder

template <int N>
struct __attribute__((aligned(16))) PlanarRecordLds {
  double joint[N][6];  // prismatic axis (2), link offset position (2), link offset rotation (cos, sin)
  double base[4];      // chain base: position (2), rotation (cos, sin)
  double x[2 * N];     // the state (q, qd interleaved)
  double cs[N][2];     // cos / sin of the revolute joint angles
  double Epos[N][2], Erot[N][2];  // joint end frames
  double Rpos[kMaxPlanarRobotShapes][2], Rrot[kMaxPlanarRobotShapes][2];  // robot shapes, global pose
};
template <int N>
constexpr size_t planar_record_lds_bytes(int n_env) {
  return ((sizeof(PlanarRecordLds<N>) + 15) / 16) * 16 + size_t(n_env) * sizeof(ShapeDev);
}

// Stages chain and environment, then revolute_joint_2D / prismatic_joint_2D / rigid_link_2D kinematics of state row e
// and pose_2D::getGlobalPose of the robot shapes (the arithmetic of proximity_min_planar).  Ends on a block barrier.
template <int N>
__device__ __forceinline__ void planar_record_frames(const SceneDev* __restrict__ sc, PlanarRecordLds<N>& lds,
                                                     ShapeDev* __restrict__ env_lds, const double* __restrict__ x, uint32_t e,
                                                     int lane) {
  for (int i = lane; i < N * 6; i += 64) {
    const int j = i / 6, k = i % 6;
    const JointDev& J = sc->joints[j];
    lds.joint[j][k] = k < 2 ? J.axis[k] : (k < 4 ? J.off_pos[k - 2] : J.off_quat[k - 4]);
  }
  if (lane < 2) lds.base[lane] = sc->base_pos[lane];
  else if (lane < 4) lds.base[lane] = sc->base_quat[lane - 2];
  {
    const int n_words = sc->n_env * int(sizeof(ShapeDev) / sizeof(double));
    const double* src = reinterpret_cast<const double*>(sc->env);
    double* dst = reinterpret_cast<double*>(env_lds);
    for (int i = lane; i < n_words; i += 64) dst[i] = src[i];
  }
  if (lane < 2 * N) lds.x[lane] = x[uint64_t(e) * (2 * N) + lane];
  __syncthreads();
  const uint32_t prismatic = sc->prismatic_mask;
  if (lane < N && !((prismatic >> lane) & 1u)) {
    double sn, cs;
    sincos(lds.x[2 * lane], &sn, &cs);
    lds.cs[lane][0] = cs;
    lds.cs[lane][1] = sn;
  }
  __syncthreads();
  {
    d2 pos = mk2(lds.base[0], lds.base[1]);
    d2 R = mk2(lds.base[2], lds.base[3]);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      d2 ER;
      if ((prismatic >> j) & 1u) {  // prismatic_joint_2D: the base moved by R (q a), same rotation
        pos = pos + rrot(R, lds.x[2 * j] * mk2(lds.joint[j][0], lds.joint[j][1]));
        ER = R;
      } else {
        ER = rmul(R, mk2(lds.cs[j][0], lds.cs[j][1]));
      }
      if (lane == 0) {
        lds.Epos[j][0] = pos.x;
        lds.Epos[j][1] = pos.y;
        lds.Erot[j][0] = ER.x;
        lds.Erot[j][1] = ER.y;
      }
      pos = pos + rrot(ER, mk2(lds.joint[j][2], lds.joint[j][3]));
      R = rmul(ER, mk2(lds.joint[j][4], lds.joint[j][5]));
    }
  }
  __syncthreads();
  const int n_robot = sc->n_robot < kMaxPlanarRobotShapes ? sc->n_robot : kMaxPlanarRobotShapes;
  for (int r = lane; r < n_robot; r += 64) {
    const ShapeDev& sh = sc->robot[r];
    const int j = sh.link;
    const d2 pp = mk2(lds.Epos[j][0], lds.Epos[j][1]);
    const d2 pr = mk2(lds.Erot[j][0], lds.Erot[j][1]);
    const d2 gp = pp + rrot(pr, mk2(sh.pos[0], sh.pos[1]));
    const d2 gr = rmul(pr, mk2(sh.quat[0], sh.quat[1]));
    lds.Rpos[r][0] = gp.x;
    lds.Rpos[r][1] = gp.y;
    lds.Rrot[r][0] = gr.x;
    lds.Rrot[r][1] = gr.y;
  }
  __syncthreads();
}

// Pair pr at those frames: (shape1, shape2) in the finder's own order, and the gap of their bounding circles
// (|c2 - c1| - r1 - r2, proxy_query_model.cpp:176-180 / :196-200)
template <int N>
RKH_DI double planar_record_pair_shapes(const SceneDev* __restrict__ sc, const ShapeDev* __restrict__ env_lds,
                                        const PlanarRecordLds<N>& lds, const PairDev pr, ShapeP* s1, ShapeP* s2) {
  const ShapeDev& rs = sc->robot[pr.robot];
  const ShapeDev& es = env_lds[pr.env];
  ShapeP A, Bv;
  A.kind = rs.kind;
  A.pos = mk2(lds.Rpos[pr.robot][0], lds.Rpos[pr.robot][1]);
  A.rot = mk2(lds.Rrot[pr.robot][0], lds.Rrot[pr.robot][1]);
  A.d0 = rs.dims[0]; A.d1 = rs.dims[1];
  Bv.kind = es.kind;
  Bv.pos = mk2(es.pos[0], es.pos[1]);
  Bv.rot = mk2(es.quat[0], es.quat[1]);
  Bv.d0 = es.dims[0]; Bv.d1 = es.dims[1];
  *s1 = pr.s1_is_robot ? A : Bv;
  *s2 = pr.s1_is_robot ? Bv : A;
  const double r1 = pr.s1_is_robot ? rs.brad : es.brad;
  const double r2 = pr.s1_is_robot ? es.brad : rs.brad;
  return norm_2(to_parent(*s2, mk2(0.0, 0.0)) - to_parent(*s1, mk2(0.0, 0.0))) - r1 - r2;
}

// slot `at` of the record arrays: the record of pair p (p < 0: no record)
template <int N>
RKH_DI void planar_write_pair_record(const SceneDev* __restrict__ sc, const ShapeDev* __restrict__ env_lds,
                                     const PlanarRecordLds<N>& lds, const PairDev* __restrict__ pairs,
                                     const PairIdDev* __restrict__ ids, int p, const RecordOut& out, uint64_t at, double dist) {
  ProxRecordP r;
  r.p1 = r.p2 = mk2(0.0, 0.0);
  uint32_t id1 = 0xFFFFFFFFu, id2 = 0xFFFFFFFFu;
  if (p >= 0) {
    const PairDev pr = pairs[p];
    ShapeP s1, s2;
    planar_record_pair_shapes<N>(sc, env_lds, lds, pr, &s1, &s2);
    r = pair_record_planar(pr.routine, s1, s2);
    id1 = ids[p].shape1;
    id2 = ids[p].shape2;
  }
  out.dist[at] = dist;  // the distance the pair was found with (pair_distance_planar); the point form's is the same
  out.point1[2 * at] = r.p1.x;
  out.point1[2 * at + 1] = r.p1.y;
  out.point2[2 * at] = r.p2.x;
  out.point2[2 * at + 1] = r.p2.y;
  out.shape1[at] = id1;
  out.shape2[at] = id2;
}

// Kernel: mProxFinders[min_i] after the loop of proxy_query_model.cpp:163-187 for B states, one wave per state.  The
// cull against the running minimum uses a radius the caps of a capped rectangle reach beyond, so the winner depends on
// the finder order and the loop is replayed as the sequence it is.  Lanes compute (cull value, distance) of 64 finders
// at a time.  Inside a tile the next finder to take over is the FIRST one that is neither culled by the running minimum
// nor at or above it: min_dist only falls, so a finder the present minimum culls or beats stays culled or beaten, and
// nothing in front of that first one can take over before it.  Each takeover is one ballot and one cross-lane read, in
// wave-uniform control flow.  Finder 0 is computed whatever its cull value says.
template <int N>
__global__ __launch_bounds__(64) void planar_min_distance_records_kernel(const SceneDev* __restrict__ sc,
                                                                          const PairDev* __restrict__ pairs,
                                                                          const PairIdDev* __restrict__ ids, int n_pairs,
                                                                          const double* __restrict__ x, uint32_t B, RecordOut out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  PlanarRecordLds<N>& lds = *reinterpret_cast<PlanarRecordLds<N>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + planar_record_lds_bytes<N>(0));
  const uint32_t e = blockIdx.x;
  if (e >= B) return;  // (the whole wave)
  const int lane = threadIdx.x;
  planar_record_frames<N>(sc, lds, env_lds, x, e, lane);
  double min_dist = INFINITY;
  int min_i = -1;
  for (int p0 = 0; p0 < n_pairs; p0 += 64) {
    const int p = p0 + lane;
    double d = INFINITY, c = INFINITY;
    if (p < n_pairs) {
      const PairDev pr = pairs[p];
      ShapeP s1, s2;
      c = planar_record_pair_shapes<N>(sc, env_lds, lds, pr, &s1, &s2);
      d = pair_distance_planar(pr.routine, s1, s2);
    }
    // every lane of the wave is here: the ballots and cross-lane reads below run in uniform control flow
    if (p0 == 0) {
      min_dist = __shfl(d, 0, 64);
      min_i = 0;
    }
    const bool follower = p < n_pairs && p != 0;
    for (;;) {
      const unsigned long long takes = __ballot(follower && !(c > min_dist) && d < min_dist);
      if (takes == 0ull) break;
      const int l = __builtin_ctzll(takes);
      min_dist = __shfl(d, l, 64);
      min_i = p0 + l;
    }
  }
  if (lane == 0) planar_write_pair_record<N>(sc, env_lds, lds, pairs, ids, min_i, out, e, min_dist);
}

// Kernel: proxy_query_pair_2D::gatherCollisionPoints (:189-208) for B states, one wave per state.  Lanes cull and
// measure 64 finders at a time (bounding circles apart, "> 0.0": skipped; distance < 0: a collision).  The pair index is
// the finder rank, so a ballot per tile and the count of set bits below a lane's own give every collision its place in
// finder order; the lane that owns one evaluates its point form and writes the slot if it is below cap.
template <int N>
__global__ __launch_bounds__(64) void planar_collision_records_kernel(const SceneDev* __restrict__ sc,
                                                                       const PairDev* __restrict__ pairs,
                                                                       const PairIdDev* __restrict__ ids, int n_pairs,
                                                                       const double* __restrict__ x, uint32_t B, uint32_t cap,
                                                                       RecordOut out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  PlanarRecordLds<N>& lds = *reinterpret_cast<PlanarRecordLds<N>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + planar_record_lds_bytes<N>(0));
  const uint32_t e = blockIdx.x;
  if (e >= B) return;  // (the whole wave)
  const int lane = threadIdx.x;
  planar_record_frames<N>(sc, lds, env_lds, x, e, lane);
  const uint64_t row = uint64_t(e) * cap;
  uint32_t total = 0;
  for (int p0 = 0; p0 < n_pairs; p0 += 64) {
    const int p = p0 + lane;
    bool hit = false;
    double d = INFINITY;
    if (p < n_pairs) {
      const PairDev pr = pairs[p];
      ShapeP s1, s2;
      const double gap = planar_record_pair_shapes<N>(sc, env_lds, lds, pr, &s1, &s2);
      if (!(gap > 0.0)) {
        d = pair_distance_planar(pr.routine, s1, s2);
        hit = d < 0.0;
      }
    }
    // every lane of the wave is here
    const unsigned long long hits = __ballot(hit);
    const uint32_t slot = total + uint32_t(__popcll(hits & ((1ull << lane) - 1ull)));
    if (hit && slot < cap) planar_write_pair_record<N>(sc, env_lds, lds, pairs, ids, p, out, row + slot, d);
    total += uint32_t(__popcll(hits));
  }
  if (lane == 0) out.n_found[e] = total;
  const uint32_t n_out = total < cap ? total : cap;
  for (uint32_t k = n_out + lane; k < cap; k += 64) planar_write_pair_record<N>(sc, env_lds, lds, pairs, ids, -1, out, row + k, INFINITY);
}

// ---- host launchers --------------------------------------------------------------------------------------------------
template <class F>
static rkh_status launch_records_2d(const rkh_scene& scene, F&& f) {
  if (!scene.host.planar || !scene.d_pair_ids.get() || scene.n_pairs > kMaxPlanarRecordPairs ||
      scene.host.n_robot > kMaxPlanarRobotShapes || scene.host.n_env > kMaxEnvShapes) {
    set_error("planar record queries: planar (2D) scenes only");
    return RKH_ERR_UNSUPPORTED;
  }
  RKH_TRY((with_n<1, 2, 3, 4, 6, 7>(scene.host.n_dof, f)));
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

rkh_status launch_min_distance_records_2d(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, RecordOut out) {
  if (B == 0) return RKH_OK;
  return launch_records_2d(scene, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((planar_min_distance_records_kernel<N>), dim3(B), dim3(64), planar_record_lds_bytes<N>(scene.host.n_env),
                       s, scene.d_scene.get(), scene.d_pairs.get(), scene.d_pair_ids.get(), scene.n_pairs, d_x, B, out);
  });
}

rkh_status launch_collision_records_2d(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, uint32_t cap,
                                       RecordOut out) {
  if (B == 0) return RKH_OK;
  return launch_records_2d(scene, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((planar_collision_records_kernel<N>), dim3(B), dim3(64), planar_record_lds_bytes<N>(scene.host.n_env), s,
                       scene.d_scene.get(), scene.d_pairs.get(), scene.d_pair_ids.get(), scene.n_pairs, d_x, B, cap, out);
  });
}

}  // namespace rkh
