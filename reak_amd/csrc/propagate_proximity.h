// propagate_proximity.h -- HIP only: hipcc compiles it into the propagate*.hip units, no host compiler reads it (unlike the
// *_device.h headers).  The proximity test of a configuration (proximity_frames, proximity_min, proximity_min_planar).
// The text of the distance query kernel: propagate_min_distance_kernel.inl.
#pragma once
#include "propagate_lds.h"
#include "proximity_device.h"
#include "proximity_planar_device.h"

namespace rkh {

// Planar scenes (SceneDev::planar): revolute_joint_2D / rigid_link_2D kinematics (revolute_joint.cpp:30-47,
// rigid_link.cpp:87-99), pose_2D::getGlobalPose of the robot shapes, then proxy_query_pair_2D::findMinimumDistance
// (proxy_query_model.cpp:163-189) replayed in finder order: every lane computes one pair's cull value and distance,
// and the sequence "skip if cull > running minimum, else take the minimum" is resolved lane by lane.
// PRISM (the rkh::planar_prismatic kernels): joints whose bit is set in SceneDev::prismatic_mask are prismatic_joint_2D
// (prismatic_joint.cpp:44-46,60): the end frame is the base moved by R (q a), no sincos.  The mask is uniform over the
// launch, and the handovers through LDS keep the barriers of the revolute form.
template <int N, int GL, bool PRISM = false, typename WS>
__device__ double proximity_min_planar(const SceneDev* __restrict__ sc, const CPack<N>& cp, const double* __restrict__ base,
                                       const ShapeDev* __restrict__ env_lds, const PairDev* __restrict__ pairs, int n_pairs,
                                       WS& ws, int gl, int gb) {
  for (int jj = gl; jj < N; jj += GL) {
    if (PRISM && ((sc->prismatic_mask >> jj) & 1u)) continue;
    double sn, cs;
    sincos(ws.x[2 * jj], &sn, &cs);
    ws.cs[jj][0] = cs;
    ws.cs[jj][1] = sn;
  }
  __syncthreads();
  {
    d2 pos = mk2(base[0], base[1]);
    d2 R = mk2(base[3], base[4]);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int jb = j * 32;
      d2 ER;
      if (PRISM && ((sc->prismatic_mask >> j) & 1u)) {
        pos = pos + rrot(R, ws.x[2 * j] * mk2(cget(cp, jb + JC_AXIS), cget(cp, jb + JC_AXIS + 1)));
        ER = R;
      } else {
        ER = rmul(R, mk2(ws.cs[j][0], ws.cs[j][1]));
      }
      if (gl == 0) {
        ws.Epos[j][0] = pos.x;
        ws.Epos[j][1] = pos.y;
        ws.Equat[j][0] = ER.x;
        ws.Equat[j][1] = ER.y;
      }
      pos = pos + rrot(ER, mk2(cget(cp, jb + JC_OFFP), cget(cp, jb + JC_OFFP + 1)));
      R = rmul(ER, mk2(cget(cp, jb + JC_OFFQ), cget(cp, jb + JC_OFFQ + 1)));
    }
  }
  __syncthreads();
  for (int r = gl; r < sc->n_robot; r += GL) {
    const ShapeDev& sh = sc->robot[r];
    const int j = sh.link;
    const d2 pp = mk2(ws.Epos[j][0], ws.Epos[j][1]);
    const d2 pr = mk2(ws.Equat[j][0], ws.Equat[j][1]);
    const d2 gp = pp + rrot(pr, mk2(sh.pos[0], sh.pos[1]));
    const d2 gr = rmul(pr, mk2(sh.quat[0], sh.quat[1]));
    ws.Rpos[r][0] = gp.x;
    ws.Rpos[r][1] = gp.y;
    ws.Rquat[r][0] = gr.x;
    ws.Rquat[r][1] = gr.y;
  }
  __syncthreads();
  double min_dist = INFINITY;
  for (int p0 = 0; p0 < n_pairs; p0 += GL) {
    const int p = p0 + gl;
    double d = INFINITY, c = INFINITY;
    if (p < n_pairs) {
      const PairDev pr = pairs[p];
      const ShapeDev& rs = sc->robot[pr.robot];
      const ShapeDev& es = env_lds[pr.env];
      ShapeP A, Bv;
      A.kind = rs.kind;
      A.pos = mk2(ws.Rpos[pr.robot][0], ws.Rpos[pr.robot][1]);
      A.rot = mk2(ws.Rquat[pr.robot][0], ws.Rquat[pr.robot][1]);
      A.d0 = rs.dims[0]; A.d1 = rs.dims[1];
      Bv.kind = es.kind;
      Bv.pos = mk2(es.pos[0], es.pos[1]);
      Bv.rot = mk2(es.quat[0], es.quat[1]);
      Bv.d0 = es.dims[0]; Bv.d1 = es.dims[1];
      const ShapeP& s1 = pr.s1_is_robot ? A : Bv;
      const ShapeP& s2 = pr.s1_is_robot ? Bv : A;
      const double r1 = pr.s1_is_robot ? rs.brad : es.brad;
      const double r2 = pr.s1_is_robot ? es.brad : rs.brad;
      c = norm_2(to_parent(s2, mk2(0.0, 0.0)) - to_parent(s1, mk2(0.0, 0.0))) - r1 - r2;
      d = pair_distance_planar(pr.routine, s1, s2);
    }
    const int cnt = (n_pairs - p0 < GL) ? (n_pairs - p0) : GL;
    for (int l = 0; l < cnt; ++l) {
      const double cl = __shfl(c, gb + l, 64), dl = __shfl(d, gb + l, 64);
      if (p0 + l == 0) min_dist = dl;                       // the first finder is always computed
      else if (!(cl > min_dist) && dl < min_dist) min_dist = dl;
    }
  }
  return min_dist;
}

// Proximity of the configuration in ws.x (joint angles): minimum distance over computed pairs.
// With cull_positive, pairs whose bounding spheres are apart are skipped (they cannot make the verdict
// "colliding"; proxy_query_model.cpp:386-389 culls the same way against the running minimum) and the scan
// stops once every edge of the wave has met a negative distance.
// Global poses of the robot shapes at the configuration in ws.x (ws.Rpos / ws.Rquat), every lane group for its own
// point; ends on a block barrier.
template <int N, int GL, typename WS, bool PRISM = false>
__device__ __forceinline__ void proximity_frames(const SceneDev* __restrict__ sc, const ShapeDev* __restrict__ robot,
                                                 const CPack<N>& cp, const double* __restrict__ base, WS& ws,
                                                 double* __restrict__ sink, int gl) {
  const bool lead = (gl == 0);
  // half-angle sin/cos, one joint per lane (strided: a 16-lane group may carry more than 16 / 2 joints)
  for (int jj = gl; jj < N; jj += GL) {
    double sn, cs;
    sincos(0.5 * ws.x[2 * jj], &sn, &cs);
    ws.cs[jj][0] = cs;
    ws.cs[jj][1] = sn;
  }
  __syncthreads();
  {  // revolute_joint_3D / rigid_link_3D kinematics, position + orientation only
    d3 pos = ld3(base);
    d4 Q = ld4(base + 3);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int jb = j * 32;
      if (sc->branch_start[j]) {  // a new branch: base frame * mount pose (rigid_link_3D::doMotion from frame 0)
        const d4 bq = ld4(base + 3);
        pos = ld3(base) + mul(rotmat(bq), ld3(sc->mount_pos[j]));
        Q = qmul(bq, ld4(sc->mount_quat[j]));
      }
      const d3 axis_n = cget3(cp, jb + JC_AXISN);
      const double c2 = ws.cs[j][0], s2 = ws.cs[j][1];
      d4 EQ;
      if (PRISM && ((sc->prismatic_mask >> j) & 1u)) {  // prismatic_joint_3D: translate by R(Q) (q a), keep Q
        pos = pos + mul(rotmat(Q), ws.x[2 * j] * cget3(cp, jb + JC_AXIS));
        EQ = Q;
      } else {
        const d4 tq = d4{c2, axis_n.x * s2, axis_n.y * s2, axis_n.z * s2};
        EQ = qmul(Q, tq);
      }
      st3(lead ? ws.Epos[j] : sink, pos);
      st4(lead ? ws.Equat[j] : sink, EQ);
      const m33 R = rotmat(EQ);
      pos = pos + mul(R, cget3(cp, jb + JC_OFFP));
      Q = qmul(EQ, d4{cget(cp, jb + JC_OFFQ), cget(cp, jb + JC_OFFQ + 1), cget(cp, jb + JC_OFFQ + 2),
                      cget(cp, jb + JC_OFFQ + 3)});
    }
  }
  __syncthreads();
  // robot shapes -> global pose (pose_3D::getGlobalPose, pose_3D.hpp:102-110)
  for (int r = gl; r < sc->n_robot; r += GL) {
    const ShapeDev& sh = robot[r];
    const int j = sh.link;
    const d3 pp = ld3(ws.Epos[j]);
    const d4 pq = ld4(ws.Equat[j]);
    st3(ws.Rpos[r], pp + qrot(pq, ld3(sh.pos)));
    st4(ws.Rquat[r], qmul(pq, ld4(sh.quat)));
  }
  __syncthreads();
}

template <int N, int GL, typename WS, bool GJK = true, bool PRISM = false>
__device__ double proximity_min(const SceneDev* __restrict__ sc, const CPack<N>& cp,
                                const double* __restrict__ base, const ShapeDev* __restrict__ env_lds,
                                const PairDev* __restrict__ pairs, int n_pairs, WS& ws,
                                double* __restrict__ sink, int gl, int gb, bool cull_positive, bool group_done) {
  if (!PRISM && sc->planar) return proximity_min_planar<N, GL>(sc, cp, base, env_lds, pairs, n_pairs, ws, gl, gb);
  proximity_frames<N, GL, WS, PRISM>(sc, sc->robot, cp, base, ws, sink, gl);
  double dmin = INFINITY;
  bool hit = group_done;  // finished edges of the wave do not hold the scan open
  for (int p0 = 0; p0 < n_pairs; p0 += GL) {
    const int p = p0 + gl;
    double d = INFINITY;
    if (p < n_pairs && !hit) {
      const PairDev pr = pairs[p];
      const ShapeDev& rs = sc->robot[pr.robot];
      const ShapeDev& es = env_lds[pr.env];
      ShapeG A, Bv;
      A.kind = rs.kind;
      A.pos = ld3(ws.Rpos[pr.robot]);
      A.q = ld4(ws.Rquat[pr.robot]);
      A.d0 = rs.dims[0]; A.d1 = rs.dims[1]; A.d2 = rs.dims[2];
      Bv.kind = es.kind;
      Bv.pos = ld3(es.pos);
      Bv.q = ld4(es.quat);
      Bv.d0 = es.dims[0]; Bv.d1 = es.dims[1]; Bv.d2 = es.dims[2];
      bool skip = false;
      if (cull_positive) {
        // transformToGlobal(0) of both shapes, then |c2 - c1| - r1 - r2 (proxy_query_model.cpp:384-389)
        const d3 c1 = pr.s1_is_robot ? pose_to_parent(A.pos, A.q, mk3(0, 0, 0)) : pose_to_parent(Bv.pos, Bv.q, mk3(0, 0, 0));
        const d3 c2p = pr.s1_is_robot ? pose_to_parent(Bv.pos, Bv.q, mk3(0, 0, 0)) : pose_to_parent(A.pos, A.q, mk3(0, 0, 0));
        const double r1 = pr.s1_is_robot ? rs.brad : es.brad;
        const double r2 = pr.s1_is_robot ? es.brad : rs.brad;
        skip = (norm_2(c2p - c1) - r1 - r2 > 0.0);
      }
      if (!skip) d = pr.s1_is_robot ? pair_distance<GJK>(pr.routine, A, Bv, sc->mesh_verts) : pair_distance<GJK>(pr.routine, Bv, A, sc->mesh_verts);
    }
    if (d < dmin) dmin = d;
    if (cull_positive) {
      // per-edge "any lane found a negative distance", then stop when every edge of the wave has one
      const unsigned long long m = __ballot(d < 0.0);
      const unsigned long long gm = (GL == 64) ? m : ((m >> gb) & ((1ull << (GL & 63)) - 1ull));
      hit = hit || (gm != 0ull);
      if (__all(hit)) break;
    }
  }
  // group min
#pragma unroll
  for (int off = GL / 2; off > 0; off >>= 1) {
    const double o = __shfl_xor(dmin, off, 64);
    if (o < dmin) dmin = o;
  }
  return dmin;
}

}  // namespace rkh
