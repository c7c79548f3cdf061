// scene.hip -- C-ABI: scene flattening (KTE program -> serial-chain tables, proxy pair list) and the
// kernel-level entry points rkh_state_derivative / rkh_min_distance / rkh_propagate (include/rkh.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "proximity_device.h"
#include "rkh_internal.h"
#include "staged_call.h"

using namespace rkh;

namespace rkh {

// quaternion::getRotMat (rotations_3D.hpp:986-999), host copy used once per scene for the constant link offsets
static void host_rotmat(const double* q, double* R) {
  const double t01 = 2.0 * q[0] * q[1], t02 = 2.0 * q[0] * q[2], t03 = 2.0 * q[0] * q[3];
  const double t11 = 2.0 * q[1] * q[1], t12 = 2.0 * q[1] * q[2], t13 = 2.0 * q[1] * q[3];
  const double t22 = 2.0 * q[2] * q[2], t23 = 2.0 * q[2] * q[3], t33 = 2.0 * q[3] * q[3];
  const double r[9] = {1.0 - t22 - t33, t12 - t03, t02 + t13, t12 + t03, 1.0 - t11 - t33, t23 - t01,
                       t13 - t02,       t01 + t23, 1.0 - t11 - t22};
  std::memcpy(R, r, sizeof(r));
}

static thread_local const double* g_mesh_vertices = nullptr;
static thread_local uint32_t g_n_mesh_vertices = 0;

static bool mesh_range_ok(const rkh_shape& s) {
  const double first = s.dims[0], cnt = s.dims[1];
  return first >= 0.0 && cnt >= 1.0 && first == std::floor(first) && cnt == std::floor(cnt) &&
         first + cnt <= double(g_n_mesh_vertices);
}

static double bounding_radius(const rkh_shape& s) {
  switch (s.kind) {
    case RKH_SHAPE_MESH: {  // about the local origin, like the reference's shapes
      double r2 = 0.0;
      for (int i = 0; i < int(s.dims[1]); ++i) {
        const double* v = g_mesh_vertices + 3 * (size_t(s.dims[0]) + i);
        r2 = std::max(r2, v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      }
      return std::sqrt(r2);
    }
    case RKH_SHAPE_SPHERE: return s.dims[0];
    case RKH_SHAPE_BOX: {
      double acc = 0.0;
      for (int i = 0; i < 3; ++i) acc += s.dims[i] * s.dims[i];
      return std::sqrt(acc) * 0.5;
    }
    case RKH_SHAPE_CCYLINDER: return s.dims[0] * 0.5 + s.dims[1];
    case RKH_SHAPE_PLANE: {  // plane.cpp:31-33
      double acc = 0.0;
      for (int i = 0; i < 2; ++i) acc += s.dims[i] * s.dims[i];
      return std::sqrt(acc) * 0.5;
    }
    case RKH_SHAPE_CYLINDER: return std::sqrt(s.dims[1] * s.dims[1] + 0.25 * s.dims[0] * s.dims[0]);  // cylinder.cpp:33-35
  }
  return 0.0;
}

// createProxFinderList's cascade of kinds for one pair (the host twin of pair_routine() in proximity_device.h)
static int host_pair_routine(int ka, int kb, bool* a_is_shape1) {
  auto other = [&](int first_kind) { return (ka == first_kind) ? kb : ka; };
  *a_is_shape1 = true;
  if (ka == RKH_SHAPE_MESH || kb == RKH_SHAPE_MESH) {  // the build's GJK query (no reference finder)
    const int ko = other(RKH_SHAPE_MESH);
    return (ko == RKH_SHAPE_SPHERE || ko == RKH_SHAPE_CCYLINDER || ko == RKH_SHAPE_BOX || ko == RKH_SHAPE_MESH) ? 12 : 0;
  }
  if (ka == RKH_SHAPE_PLANE || kb == RKH_SHAPE_PLANE) {
    *a_is_shape1 = (ka == RKH_SHAPE_PLANE);
    switch (other(RKH_SHAPE_PLANE)) {
      case RKH_SHAPE_PLANE: return 6;
      case RKH_SHAPE_SPHERE: return 7;
      case RKH_SHAPE_CCYLINDER: return 8;
      case RKH_SHAPE_CYLINDER: return 9;
      case RKH_SHAPE_BOX: return 10;
    }
    return 0;
  }
  if (ka == RKH_SHAPE_SPHERE || kb == RKH_SHAPE_SPHERE) {
    *a_is_shape1 = (ka == RKH_SHAPE_SPHERE);
    switch (other(RKH_SHAPE_SPHERE)) {
      case RKH_SHAPE_SPHERE: return 1;
      case RKH_SHAPE_CCYLINDER: return 2;
      case RKH_SHAPE_CYLINDER: return 11;
      case RKH_SHAPE_BOX: return 3;
    }
    return 0;
  }
  if (ka == RKH_SHAPE_CCYLINDER || kb == RKH_SHAPE_CCYLINDER) {
    *a_is_shape1 = (ka == RKH_SHAPE_CCYLINDER);
    switch (other(RKH_SHAPE_CCYLINDER)) {
      case RKH_SHAPE_CCYLINDER: return 4;
      case RKH_SHAPE_BOX: return 5;
    }
    return 0;
  }
  return 0;  // cylinder-cylinder, cylinder-box, box-box: no finder in the reference
}

// The time loops of the steer pattern and of runge_kutta4_integrate_impl depend only on (fraction, dt,
// steps): evaluate them on the host in the same fp64 arithmetic and hand the kernel integer counts.
rkh_status build_dyn_dev(const rkh_dyn_space& sp, double fraction, DynDev* out) {
  if (sp.n_dof < 1 || sp.n_dof > kMaxDof || sp.steps_per_edge < 0 || sp.steps_per_edge > kMaxSteps || !(sp.dt > 0.0)) {
    set_error("rkh_dyn_space: n_dof / steps_per_edge / dt out of range");
    return RKH_ERR_BAD_ARG;
  }
  DynDev d;
  std::memset(&d, 0, sizeof(d));
  d.dt = sp.dt; d.kp = sp.kp; d.kd = sp.kd; d.u_max = sp.u_max; d.goal_tol = sp.goal_tol;
  for (int i = 0; i < 2 * sp.n_dof; ++i) {
    d.lower[i] = sp.lower[i];
    d.upper[i] = sp.upper[i];
  }
  // the schedule is evaluated over the whole step budget (edges with their own travel fraction, EdgeIO::frac, cut it
  // on the device with the same comparison); n_steps = its length for this call's fraction
  d.full_time = sp.steps_per_edge * sp.dt;
  const double T_goal = fraction * d.full_time;
  double current_time = 0.0;
  int k = 0, n = 0;
  while (k < kMaxSteps) {
    if (current_time < T_goal) n = k + 1;
    double t = current_time;
    const double end_time = current_time + sp.dt;
    int it = 0;
    while (t < end_time) {  // runge_kutta4_integrator_sys.hpp:73-96
      t += sp.dt * 0.5;
      t += sp.dt * 0.5;
      ++it;
    }
    d.inner[k] = int8_t(it);
    current_time += sp.dt;
    ++k;
  }
  k = n;
  d.n_steps = k;
  *out = d;
  return RKH_OK;
}

// diagnostic: GJK on n world-anchored pairs (rkh_diag_gjk_distance)
__global__ void gjk_pairs_kernel(const rkh_shape* __restrict__ a, const rkh_shape* __restrict__ b, uint32_t n,
                                 const double* __restrict__ pool, double* __restrict__ out) {
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
  out[i] = gjk_distance(to_gjk(conv(a[i]), pool), to_gjk(conv(b[i]), pool));
}

// its twin with the points: gjk_record on the same pairs (rkh_diag_gjk_records)
__global__ void gjk_pair_records_kernel(const rkh_shape* __restrict__ a, const rkh_shape* __restrict__ b, uint32_t n,
                                        const double* __restrict__ pool, double* __restrict__ dist, double* __restrict__ point1,
                                        double* __restrict__ point2) {
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
  const GjkRecord r = gjk_record(to_gjk(conv(a[i]), pool), to_gjk(conv(b[i]), pool));
  dist[i] = r.dist;
  point1[3 * size_t(i)] = r.p1.x; point1[3 * size_t(i) + 1] = r.p1.y; point1[3 * size_t(i) + 2] = r.p1.z;
  point2[3 * size_t(i)] = r.p2.x; point2[3 * size_t(i) + 1] = r.p2.y; point2[3 * size_t(i) + 2] = r.p2.z;
}


static thread_local SteerMapping g_steer_mapping = SteerMapping::Wave;
void note_steer_mapping(SteerMapping m) { g_steer_mapping = m; }
}  // namespace rkh

// The chain as the kinematics kernels walk it (kinematics_device.h): a copy of the joint groups of SceneDev.
static void fill_kin_chain(rkh_scene* sc) {
  const SceneDev& S = sc->host;
  KinChain& K = sc->kin;
  std::memset(&K, 0, sizeof(K));
  K.n_dof = S.n_dof;
  K.planar = S.planar;
  std::memcpy(K.base_pos, S.base_pos, sizeof(K.base_pos));
  std::memcpy(K.base_quat, S.base_quat, sizeof(K.base_quat));
  for (int j = 0; j < S.n_dof; ++j) {
    KinJoint& J = K.joints[j];
    std::memcpy(J.axis, S.joints[j].axis, sizeof(J.axis));
    std::memcpy(J.axis_n, S.joints[j].axis_n, sizeof(J.axis_n));
    std::memcpy(J.off_pos, S.joints[j].off_pos, sizeof(J.off_pos));
    std::memcpy(J.off_quat, S.joints[j].off_quat, sizeof(J.off_quat));
    std::memcpy(J.mount_pos, S.mount_pos[j], sizeof(J.mount_pos));
    std::memcpy(J.mount_quat, S.mount_quat[j], sizeof(J.mount_quat));
    J.prismatic = int32_t((S.prismatic_mask >> j) & 1u);
    J.branch_start = S.branch_start[j];
  }
}

// One entry of rkh_scene::frame_table.  Frame ids are the caller's; an id the table cannot hold stays unknown to the
// kinematics entries (they answer RKH_ERR_BAD_ARG for it).
static void note_frame(rkh_scene* sc, int frame, KinFrameKind kind, int first, int last, uint32_t up) {
  if (frame < 0 || frame >= 65536) return;
  if (size_t(frame) >= sc->frame_table.size()) sc->frame_table.resize(size_t(frame) + 1, KinFrameRef{KIN_INVALID, 0, 0, 0u});
  sc->frame_table[frame] = KinFrameRef{kind, first, last, up};
}
static uint32_t frame_up(const rkh_scene* sc, int frame) {
  return (frame >= 0 && size_t(frame) < sc->frame_table.size()) ? sc->frame_table[frame].up : 0u;
}

// the last step of both scene builders: the handle is the caller's only once everything is on the device
static rkh_status upload_scene(rkh_ctx* ctx, std::unique_ptr<rkh_scene> sc, const std::vector<PairDev>& pairs,
                               rkh_scene** out, const std::vector<PairIdDev>& pair_ids = std::vector<PairIdDev>()) {
  SceneDev& S = sc->host;
  sc->n_pairs = int(pairs.size());
  if (sc->n_pairs_verdict < 0 || sc->n_pairs_verdict > sc->n_pairs) sc->n_pairs_verdict = sc->n_pairs;
  RKH_HIP(hipSetDevice(ctx->device));
  if (S.has_meshes && g_n_mesh_vertices > 0) {
    RKH_TRY(sc->d_mesh_verts.alloc(size_t(g_n_mesh_vertices) * 3));
    RKH_HIP(hipMemcpy(sc->d_mesh_verts.get(), g_mesh_vertices, size_t(g_n_mesh_vertices) * 3 * sizeof(double), hipMemcpyHostToDevice));
    S.mesh_verts = sc->d_mesh_verts.get();
  }
  RKH_TRY(sc->d_scene.alloc(1));
  RKH_HIP(hipMemcpy(sc->d_scene.get(), &S, sizeof(SceneDev), hipMemcpyHostToDevice));
  RKH_TRY(sc->d_pairs.alloc(std::max<size_t>(1, pairs.size())));
  if (!pairs.empty()) RKH_HIP(hipMemcpy(sc->d_pairs.get(), pairs.data(), pairs.size() * sizeof(PairDev), hipMemcpyHostToDevice));
  if (pair_ids.size() == pairs.size()) {  // the record queries' table
    RKH_TRY(sc->d_pair_ids.alloc(std::max<size_t>(1, pair_ids.size())));
    if (!pair_ids.empty())
      RKH_HIP(hipMemcpy(sc->d_pair_ids.get(), pair_ids.data(), pair_ids.size() * sizeof(PairIdDev), hipMemcpyHostToDevice));
  }
  RKH_TRY(sc->d_err.alloc_zeroed(1));
  RKH_TRY(sc->d_clear_stats.alloc_zeroed(2));
  fill_kin_chain(sc.get());
  RKH_TRY(sc->d_kin.alloc(1));
  RKH_HIP(hipMemcpy(sc->d_kin.get(), &sc->kin, sizeof(KinChain), hipMemcpyHostToDevice));
  *out = sc.release();
  return RKH_OK;
}

// Planar chain (manip_3R_arm.cpp:75-150 pattern): {revolute_joint_2D | prismatic_joint_2D, rigid_link_2D} per joint, 2D
// shapes only.  Given at the position level the scene serves the quasi-static entry points and the dynamics entry
// points refuse it.  A prismatic_joint_2D (prismatic_joint.cpp:33-123) may stand in any group: its bit goes into
// SceneDev::prismatic_mask and its axis into JointDev::axis[0..1], and the launchers pick the planar prismatic forms.
static bool is_planar_joint(int kind) { return kind == RKH_KTE_REVOLUTE_JOINT_2D || kind == RKH_KTE_PRISMATIC_JOINT_2D; }

static rkh_status create_planar_scene(rkh_ctx* ctx, const rkh_kte_op* prog, int n_ops, const rkh_chain_base* base,
                                      const rkh_shape* shapes, int n_shapes, rkh_scene** out) {
  // position level: {joint, rigid_link_2D} per joint; with dynamics: {driving_actuator_gen, inertia_gen, joint,
  // rigid_link_2D, inertia_2D on the link's end frame} per joint; joint = revolute_joint_2D or prismatic_joint_2D
  for (int k = 0; k < n_ops; ++k)
    if (prog[k].kind == RKH_KTE_PRISMATIC_JOINT_3D) {
      set_error("rkh_scene_create: prismatic_joint_3D is not supported in planar chains (a planar chain takes "
                "prismatic_joint_2D)");
      return RKH_ERR_UNSUPPORTED;
    }
  const bool dynamics = prog[0].kind == RKH_KTE_DRIVING_ACTUATOR_GEN;
  const int per = dynamics ? 5 : 2;
  const int n = n_ops / per;
  if (n_ops % per != 0 || n < 1 || n > kMaxDof) {
    set_error("rkh_scene_create: a planar chain is a sequence of {revolute_joint_2D or prismatic_joint_2D, rigid_link_2D} "
              "pairs, or of {driving_actuator_gen, inertia_gen, revolute_joint_2D or prismatic_joint_2D, rigid_link_2D, "
              "inertia_2D} groups");
    return RKH_ERR_UNSUPPORTED;
  }
  std::unique_ptr<rkh_scene> sc(new rkh_scene());
  sc->ctx = ctx;
  SceneDev& S = sc->host;
  std::memset(&S, 0, sizeof(S));
  S.n_dof = n;
  S.planar = 1;
  S.planar_dynamics = dynamics ? 1 : 0;
  for (int i = 0; i < 2; ++i) {
    S.base_pos[i] = base->pose.pos[i];
    S.base_quat[i] = base->pose.quat[i];
    S.base_acc[i] = base->acceleration[i];
  }
  std::vector<int> joint_end_frame(n);
  std::vector<uint32_t> robot_src, env_src;  // the caller's shape index of every robot / environment slot
  int prev_end = 0;
  for (int j = 0; j < n; ++j) {
    const rkh_kte_op& rev = prog[per * j + (dynamics ? 2 : 0)], &lnk = prog[per * j + (dynamics ? 3 : 1)];
    if (!is_planar_joint(rev.kind) || lnk.kind != RKH_KTE_RIGID_LINK_2D || rev.coord != j ||
        rev.base_frame != prev_end || lnk.base_frame != rev.end_frame) {
      set_error("rkh_scene_create: planar op group " + std::to_string(j) + " does not continue the serial chain");
      return RKH_ERR_UNSUPPORTED;
    }
    JointDev& J = S.joints[j];
    if (dynamics) {
      const rkh_kte_op& act = prog[per * j], &gen = prog[per * j + 1], &in2 = prog[per * j + 4];
      if (act.kind != RKH_KTE_DRIVING_ACTUATOR_GEN || act.coord != j || act.joint_op != per * j + 2 ||
          gen.kind != RKH_KTE_INERTIA_GEN || gen.coord != j || gen.upstream != (1u << j) ||
          in2.kind != RKH_KTE_INERTIA_2D || in2.end_frame != lnk.end_frame || in2.upstream != ((1u << (j + 1)) - 1u)) {
        set_error("rkh_scene_create: planar op group " + std::to_string(j) +
                  " is not {actuator, inertia_gen, revolute_joint_2D or prismatic_joint_2D, rigid_link_2D, inertia_2D} of "
                  "one serial joint");
        return RKH_ERR_UNSUPPORTED;
      }
      J.joint_inertia = gen.mass;
      J.mass = in2.mass;
      J.inertia[0] = in2.inertia[0];
    }
    if (j == 0) note_frame(sc.get(), 0, KIN_BASE, 0, 0, 0u);
    note_frame(sc.get(), rev.end_frame, KIN_JOINT_END, 0, j, frame_up(sc.get(), rev.base_frame) | (1u << j));
    note_frame(sc.get(), lnk.end_frame, KIN_LINK_END, 0, j, frame_up(sc.get(), lnk.base_frame));
    prev_end = lnk.end_frame;
    joint_end_frame[j] = rev.end_frame;
    if (rev.kind == RKH_KTE_PRISMATIC_JOINT_2D) {  // mAxis as given: the joint does not normalise it
      S.prismatic_mask |= 1u << j;
      J.axis[0] = rev.axis[0];
      J.axis[1] = rev.axis[1];
    }
    for (int i = 0; i < 2; ++i) {
      J.off_pos[i] = lnk.offset.pos[i];
      J.off_quat[i] = lnk.offset.quat[i];
    }
    S.mount_quat[j][0] = 1.0;
  }
  S.has_prismatic = S.prismatic_mask != 0u ? 1 : 0;
  for (int i = 0; i < n_shapes; ++i) {
    const rkh_shape& s = shapes[i];
    if (s.kind < RKH_SHAPE_CIRCLE || s.kind > RKH_SHAPE_CRECT) {
      set_error("rkh_scene_create: a planar chain takes 2D shapes only (circle, rectangle, capped_rectangle)");
      return RKH_ERR_UNSUPPORTED;
    }
    ShapeDev d;
    std::memset(&d, 0, sizeof(d));
    d.kind = s.kind;
    for (int k = 0; k < 2; ++k) {
      d.pos[k] = s.pose.pos[k];
      d.quat[k] = s.pose.quat[k];
      d.dims[k] = s.dims[k];
    }
    // circle.cpp:31-33 ; rectangle.cpp:31-33 and capped_rectangle.cpp:31-33: norm_2(mDimensions) * 0.5
    d.brad = (s.kind == RKH_SHAPE_CIRCLE) ? s.dims[0] : std::sqrt((0.0 + s.dims[0] * s.dims[0]) + s.dims[1] * s.dims[1]) * 0.5;
    if (s.anchor >= 0) {
      int link = -1;
      for (int j = 0; j < n; ++j)
        if (joint_end_frame[j] == s.anchor) link = j;
      if (link < 0 || S.n_robot >= 2 * kMaxDof) {
        set_error("rkh_scene_create: robot shapes must be anchored on a joint's end frame");
        return RKH_ERR_UNSUPPORTED;
      }
      d.link = link;
      S.robot[S.n_robot++] = d;
      robot_src.push_back(uint32_t(i));
    } else {
      if (S.n_env >= kMaxEnvShapes) {
        set_error("rkh_scene_create: too many environment shapes");
        return RKH_ERR_CAPACITY;
      }
      d.link = -1;
      S.env[S.n_env++] = d;
      env_src.push_back(uint32_t(i));
    }
  }
  for (int r = 0; r < S.n_robot; ++r) S.robot_n_reach[r] = S.n_env;
  // proxy_query_pair_2D::createProxFinderList (proxy_query_model.cpp:75-161), kept in its i-major / j-minor order:
  // findMinimumDistance (:163-189) culls against the running minimum with a radius the capped rectangle's caps
  // reach beyond, so the result depends on the order and the device replays the sequence
  // Every pair of kinds has a finder, so the pair index is the finder rank; the planar record queries
  // (proximity_records_planar.hip) report the caller's indices of the finder's (shape1, shape2) from pair_ids.
  std::vector<PairDev> pairs;
  std::vector<PairIdDev> pair_ids;
  for (int i = 0; i < S.n_robot; ++i)
    for (int j = 0; j < S.n_env; ++j) {
      const int ki = S.robot[i].kind, kj = S.env[j].kind;
      PairDev p;
      std::memset(&p, 0, sizeof(p));
      p.robot = uint16_t(i);
      p.env = uint16_t(j);
      if (ki == RKH_SHAPE_CIRCLE || kj == RKH_SHAPE_CIRCLE) {
        p.s1_is_robot = (ki == RKH_SHAPE_CIRCLE) ? 1 : 0;  // the circle is shape1
        const int ko = p.s1_is_robot ? kj : ki;
        p.routine = (ko == RKH_SHAPE_CIRCLE) ? 11 : (ko == RKH_SHAPE_CRECT ? 12 : 13);
      } else if (ki == RKH_SHAPE_CRECT || kj == RKH_SHAPE_CRECT) {
        p.s1_is_robot = (ki == RKH_SHAPE_CRECT) ? 1 : 0;  // the capped rectangle is shape1
        const int ko = p.s1_is_robot ? kj : ki;
        p.routine = (ko == RKH_SHAPE_CRECT) ? 14 : 15;
      } else {
        p.s1_is_robot = 1;  // rectangle-rectangle: model1's shape is shape1
        p.routine = 16;
      }
      pair_ids.push_back(PairIdDev{uint32_t(pairs.size()), p.s1_is_robot ? robot_src[i] : env_src[j],
                                   p.s1_is_robot ? env_src[j] : robot_src[i]});
      pairs.push_back(p);
    }
  return upload_scene(ctx, std::move(sc), pairs, out, pair_ids);
}

// The three rkh_diag_gjk_* entries after their checks: the distance alone (point1 = point2 = null), with the witness points,
// or with the points and the normal of the depth form.
static rkh_status gjk_pairs_run(rkh_ctx* ctx, const rkh_shape* a, const rkh_shape* b, uint32_t n, const double* mesh_vertices,
                                uint32_t n_mesh_vertices, double* dist, double* point1, double* point2, double* normal) {
  if (n == 0) return RKH_OK;
  RKH_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  StagedCall call(s);
  const rkh_shape* da = call.in(a, n);
  const rkh_shape* db = call.in(b, n);
  const double* dv = call.in(mesh_vertices, size_t(n_mesh_vertices) * 3, 1);
  double* dd = call.out(dist, n);
  double* dp1 = point1 ? call.out(point1, size_t(n) * 3) : nullptr;
  double* dp2 = point2 ? call.out(point2, size_t(n) * 3) : nullptr;
  double* dn3 = normal ? call.out(normal, size_t(n) * 3) : nullptr;
  RKH_TRY(call.status());
  if (!point1) {
    hipLaunchKernelGGL(rkh::gjk_pairs_kernel, dim3((n + 63) / 64), dim3(64), 0, s, da, db, n, dv, dd);
    RKH_HIP(hipGetLastError());
  } else if (!normal) {
    hipLaunchKernelGGL(rkh::gjk_pair_records_kernel, dim3((n + 63) / 64), dim3(64), 0, s, da, db, n, dv, dd, dp1, dp2);
    RKH_HIP(hipGetLastError());
  } else {
    RKH_TRY(launch_gjk_pair_depth(s, da, db, n, dv, dd, dp1, dp2, dn3));
  }
  return call.fetch();
}

extern "C" {

rkh_status rkh_scene_create(rkh_ctx* ctx, const rkh_kte_op* prog, int n_ops, const rkh_chain_base* base,
                            const rkh_shape* shapes, int n_shapes, rkh_scene** out) {
  return rkh_scene_create_with_meshes(ctx, prog, n_ops, base, shapes, n_shapes, nullptr, 0, out);
}

rkh_status rkh_scene_create_with_meshes(rkh_ctx* ctx, const rkh_kte_op* prog, int n_ops, const rkh_chain_base* base,
                                        const rkh_shape* shapes, int n_shapes, const double* mesh_vertices,
                                        uint32_t n_mesh_vertices, rkh_scene** out) {
  if (!ctx || !prog || !base || !out || n_ops < 1 || (n_shapes > 0 && !shapes)) return RKH_ERR_BAD_ARG;
  if (n_mesh_vertices > 0 && !mesh_vertices) return RKH_ERR_BAD_ARG;
  g_mesh_vertices = mesh_vertices;  // for bounding_radius() / validation while the scene is built (one host thread per ctx)
  g_n_mesh_vertices = n_mesh_vertices;
  // a planar chain: its first joint is a revolute_joint_2D, or it holds 2D elements and nothing three-dimensional (a
  // chain whose first joint is a misplaced prismatic_joint_3D is answered by the planar builder, which names it; a
  // prismatic_joint_2D among 3D elements is answered below)
  bool any_2d = false, any_3d = false;
  for (int k = 0; k < n_ops; ++k) {
    const int kd = prog[k].kind;
    any_2d = any_2d || kd == RKH_KTE_REVOLUTE_JOINT_2D || kd == RKH_KTE_RIGID_LINK_2D || kd == RKH_KTE_INERTIA_2D;
    any_3d = any_3d || kd == RKH_KTE_REVOLUTE_JOINT_3D || kd == RKH_KTE_RIGID_LINK_3D || kd == RKH_KTE_INERTIA_3D ||
             kd == RKH_KTE_FLEXIBLE_BEAM_3D;
  }
  const int first_joint = prog[0].kind == RKH_KTE_DRIVING_ACTUATOR_GEN && n_ops >= 3 ? prog[2].kind : prog[0].kind;
  if (first_joint == RKH_KTE_REVOLUTE_JOINT_2D || (!any_3d && (any_2d || first_joint == RKH_KTE_PRISMATIC_JOINT_2D)))
    return create_planar_scene(ctx, prog, n_ops, base, shapes, n_shapes, out);
  for (int k = 0; k < n_ops; ++k)
    if (prog[k].kind == RKH_KTE_PRISMATIC_JOINT_2D) {
      set_error("rkh_scene_create: prismatic_joint_2D is not supported in 3D chains (a 3D chain takes prismatic_joint_3D)");
      return RKH_ERR_UNSUPPORTED;
    }
  const bool has_beam = n_ops > 1 && prog[n_ops - 1].kind == RKH_KTE_FLEXIBLE_BEAM_3D;
  if (has_beam) --n_ops;  // the beam is validated below, after the chain
  // parse: [optional mount link from frame 0] {actuator, inertia_gen, revolute, link, inertia_3D} ...
  struct Group { int first_op; int mount_op; };
  std::vector<Group> groups;
  {
    int k = 0;
    while (k < n_ops) {
      Group g{0, -1};
      if (prog[k].kind == RKH_KTE_RIGID_LINK_3D && prog[k].base_frame == 0) {
        g.mount_op = k;
        ++k;
      }
      g.first_op = k;
      if (k + 5 > n_ops) {
        k = -1;
        break;
      }
      groups.push_back(g);
      k += 5;
    }
    if (k < 0 || groups.empty() || int(groups.size()) > kMaxDof) {
      set_error("rkh_scene_create: KTE program is not a chain of [mount link] {actuator, inertia_gen, revolute or "
                "prismatic joint, link, inertia_3D} groups (optionally followed by one flexible_beam_3D), or has too many joints");
      return RKH_ERR_UNSUPPORTED;
    }
  }
  const int n = int(groups.size());
  std::unique_ptr<rkh_scene> sc(new rkh_scene());
  sc->ctx = ctx;
  SceneDev& S = sc->host;
  std::memset(&S, 0, sizeof(S));
  S.n_dof = n;
  for (int i = 0; i < 3; ++i) {
    S.base_pos[i] = base->pose.pos[i];
    S.base_acc[i] = base->acceleration[i];
  }
  for (int i = 0; i < 4; ++i) S.base_quat[i] = base->pose.quat[i];
  std::vector<int> joint_end_frame(n), link_end_frame(n);
  int prev_end = 0;  // frame 0 = chain base
  bool first = true;
  int branch_first = 0;  // first joint of the current branch
  for (int j = 0; j < n; ++j) {
    const int k0 = groups[j].first_op;
    const rkh_kte_op& act = prog[k0], &gen = prog[k0 + 1], &rev = prog[k0 + 2], &lnk = prog[k0 + 3], &ine = prog[k0 + 4];
    bool starts_branch = false;
    int expect_base = prev_end;
    if (groups[j].mount_op >= 0) {  // a rigid link from the chain base carries this joint
      const rkh_kte_op& mt = prog[groups[j].mount_op];
      starts_branch = true;
      expect_base = mt.end_frame;
      for (int i = 0; i < 3; ++i) S.mount_pos[j][i] = mt.offset.pos[i];
      for (int i = 0; i < 4; ++i) S.mount_quat[j][i] = mt.offset.quat[i];
    } else if (!first && rev.base_frame == 0) {  // a second chain sitting directly on the base
      starts_branch = true;
      expect_base = 0;
      S.mount_quat[j][0] = 1.0;
    } else {
      S.mount_quat[j][0] = 1.0;
    }
    if (starts_branch) {
      S.branch_start[j] = 1;
      ++S.n_branches;
      branch_first = j;
    }
    S.branch_first[j] = branch_first;
    const uint32_t branch_mask = ((j + 1 >= 32 ? 0xFFFFFFFFu : ((1u << (j + 1)) - 1u))) & ~((1u << branch_first) - 1u);
    const bool ok = act.kind == RKH_KTE_DRIVING_ACTUATOR_GEN && gen.kind == RKH_KTE_INERTIA_GEN &&
                    (rev.kind == RKH_KTE_REVOLUTE_JOINT_3D || rev.kind == RKH_KTE_PRISMATIC_JOINT_3D) &&
                    lnk.kind == RKH_KTE_RIGID_LINK_3D &&
                    ine.kind == RKH_KTE_INERTIA_3D && act.coord == j && gen.coord == j && rev.coord == j &&
                    act.joint_op == k0 + 2 && gen.upstream == (1u << j) &&
                    (first && groups[j].mount_op < 0 ? rev.base_frame == 0 : rev.base_frame == expect_base) &&
                    lnk.base_frame == rev.end_frame && ine.end_frame == lnk.end_frame && ine.upstream == branch_mask;
    if (!ok) {
      set_error("rkh_scene_create: op group " + std::to_string(j) + " does not match the chain pattern");
      return RKH_ERR_UNSUPPORTED;
    }
    if (j == 0) note_frame(sc.get(), 0, KIN_BASE, 0, 0, 0u);
    if (groups[j].mount_op >= 0) note_frame(sc.get(), prog[groups[j].mount_op].end_frame, KIN_MOUNT, j, j, frame_up(sc.get(), 0));
    note_frame(sc.get(), rev.end_frame, KIN_JOINT_END, branch_first, j, frame_up(sc.get(), rev.base_frame) | (1u << j));
    note_frame(sc.get(), lnk.end_frame, KIN_LINK_END, branch_first, j, frame_up(sc.get(), lnk.base_frame));
    first = false;
    prev_end = lnk.end_frame;
    joint_end_frame[j] = rev.end_frame;
    link_end_frame[j] = lnk.end_frame;
    if (rev.kind == RKH_KTE_PRISMATIC_JOINT_3D) S.prismatic_mask |= 1u << j;
    JointDev& J = S.joints[j];
    for (int i = 0; i < 3; ++i) J.axis[i] = rev.axis[i];
    {  // axis_angle ctor normalisation (rotations_3D.hpp:1961-1974)
      double acc = 0.0;
      for (int i = 0; i < 3; ++i) acc += rev.axis[i] * rev.axis[i];
      const double tmp = std::sqrt(acc);
      if (tmp > 0.0000001) {
        for (int i = 0; i < 3; ++i) J.axis_n[i] = rev.axis[i] / tmp;
      } else {
        J.axis_n[0] = 1.0; J.axis_n[1] = 0.0; J.axis_n[2] = 0.0;
      }
    }
    J.joint_inertia = gen.mass;
    for (int i = 0; i < 3; ++i) J.off_pos[i] = lnk.offset.pos[i];
    for (int i = 0; i < 4; ++i) J.off_quat[i] = lnk.offset.quat[i];
    host_rotmat(J.off_quat, J.off_R);
    J.mass = ine.mass;
    for (int i = 0; i < 6; ++i) J.inertia[i] = ine.inertia[i];
  }
  S.has_prismatic = S.prismatic_mask != 0u ? 1 : 0;
  if (S.has_prismatic) {
    // a mount link on the first joint keeps the chain serial; any later branch start does not
    bool branching = false;
    for (int j = 1; j < n; ++j) branching = branching || S.branch_start[j] != 0;
    const char* why = branching ? "a branching chain" : (has_beam ? "a flexible_beam_3D" : nullptr);
    if (why) {
      set_error(std::string("rkh_scene_create: prismatic joints are supported in serial chains only, not with ") + why);
      return RKH_ERR_UNSUPPORTED;
    }
  }
  if (has_beam) {
    const rkh_kte_op& bm = prog[n_ops];
    int j1 = -1, j2 = -1;
    for (int j = 0; j < n; ++j) {
      if (link_end_frame[j] == bm.base_frame) j1 = j;
      if (bm.end_frame >= 0 && link_end_frame[j] == bm.end_frame) j2 = j;
    }
    if (j1 < 0 || (bm.end_frame >= 0 && j2 < 0) || j1 == j2) {
      set_error("rkh_scene_create: the flexible beam's anchors must be link end frames of the chain (anchor 2 may be a "
                "world anchor, end_frame = -1)");
      return RKH_ERR_UNSUPPORTED;
    }
    S.beam_on = 1;
    S.beam_j1 = j1;
    S.beam_j2 = j2;
    S.beam_rest = bm.axis[0];
    S.beam_k = bm.axis[1];
    S.beam_kt = bm.axis[2];
    for (int i = 0; i < 3; ++i) S.beam_pos[i] = bm.offset.pos[i];
    for (int i = 0; i < 4; ++i) S.beam_quat[i] = bm.offset.quat[i];
  }
  // shapes: robot model (anchored) / environment model (world).  The environment shapes are stored nearest-to-the-base
  // first (see SceneDev::robot_n_reach; the verdict "some pair is closer than 0" does not depend on the pair order).
  std::vector<int> robot_src, env_src;
  std::vector<int> order(n_shapes);
  {
    std::vector<double> key(n_shapes, -INFINITY);  // robot shapes first, in their given order
    for (int i = 0; i < n_shapes; ++i) {
      order[i] = i;
      const rkh_shape& s = shapes[i];
      if (s.anchor >= 0) continue;
      double d2 = 0.0;
      for (int k = 0; k < 3; ++k) d2 += (s.pose.pos[k] - S.base_pos[k]) * (s.pose.pos[k] - S.base_pos[k]);
      key[i] = std::sqrt(d2) - bounding_radius(s);
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[a] < key[b]; });
  }
  std::vector<double> env_key;
  for (int oi = 0; oi < n_shapes; ++oi) {
    const int i = order[oi];
    const rkh_shape& s = shapes[i];
    const bool kind_ok = (s.kind >= RKH_SHAPE_SPHERE && s.kind <= RKH_SHAPE_CCYLINDER) || s.kind == RKH_SHAPE_PLANE ||
                         s.kind == RKH_SHAPE_CYLINDER || (s.kind == RKH_SHAPE_MESH && mesh_range_ok(s));
    if (!kind_ok) {
      set_error("rkh_scene_create: unsupported shape kind");
      return RKH_ERR_UNSUPPORTED;
    }
    if (s.kind == RKH_SHAPE_MESH) S.has_meshes = 1;
    ShapeDev d;
    std::memset(&d, 0, sizeof(d));
    d.kind = s.kind;
    for (int k = 0; k < 3; ++k) { d.pos[k] = s.pose.pos[k]; d.dims[k] = s.dims[k]; }
    for (int k = 0; k < 4; ++k) d.quat[k] = s.pose.quat[k];
    d.brad = bounding_radius(s);
    if (s.anchor >= 0) {
      int link = -1;
      for (int j = 0; j < n; ++j)
        if (joint_end_frame[j] == s.anchor) link = j;
      if (link < 0 || S.n_robot >= 2 * kMaxDof) {
        set_error("rkh_scene_create: robot shapes must be anchored on a joint's end frame");
        return RKH_ERR_UNSUPPORTED;
      }
      d.link = link;
      S.robot[S.n_robot++] = d;
      robot_src.push_back(i);
    } else {
      if (S.n_env >= kMaxEnvShapes) {
        set_error("rkh_scene_create: too many environment shapes");
        return RKH_ERR_CAPACITY;
      }
      d.link = -1;
      for (int k = 0; k < 3; ++k) S.env_cull[S.n_env][k] = d.pos[k] - S.base_pos[k];  // relative to the chain base
      S.env_cull[S.n_env][3] = d.brad;
      if (d.kind <= RKH_SHAPE_CCYLINDER)
        S.env_kind_mask[d.kind == RKH_SHAPE_SPHERE ? 0 : (d.kind == RKH_SHAPE_BOX ? 1 : 2)][S.n_env / 64] |= 1ull << (S.n_env % 64);
      for (int k = RKH_SHAPE_SPHERE; k <= RKH_SHAPE_CYLINDER; ++k) {  // (meshes do not reach the kernel that reads this)
        bool first;
        if (host_pair_routine(k, d.kind, &first) != 0) S.env_finder_mask[k][S.n_env / 64] |= 1ull << (S.n_env % 64);
      }
      S.env[S.n_env++] = d;
      env_src.push_back(i);
      double d2 = 0.0;
      for (int k = 0; k < 3; ++k) d2 += (d.pos[k] - S.base_pos[k]) * (d.pos[k] - S.base_pos[k]);
      env_key.push_back(std::sqrt(d2) - d.brad);
    }
  }
  if (S.has_prismatic && S.has_meshes) {
    set_error("rkh_scene_create: prismatic joints are not supported together with mesh shapes");
    return RKH_ERR_UNSUPPORTED;
  }
  // robot shape r rides on a prismatic joint (its travel has no bound in the scene: no static reach, no plane pairs)
  auto on_prismatic = [&](int r) { return (S.prismatic_mask & ((2u << S.robot[r].link) - 1u)) != 0u; };
  S.clear_static = INFINITY;
  for (int r = 0; r < S.n_robot; ++r) {
    S.robot_n_reach[r] = S.robot_n_clear[r] = S.n_env;
    if (S.n_branches != 0 || S.planar) continue;  // serial 3D chains only: every joint hangs off the previous link
    if (on_prismatic(r)) continue;
    double reach = 0.0;
    for (int i = 0; i < S.robot[r].link; ++i) {
      const double* o = S.joints[i].off_pos;
      reach += std::sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]);
    }
    const double* lp = S.robot[r].pos;
    reach += std::sqrt(lp[0] * lp[0] + lp[1] * lp[1] + lp[2] * lp[2]) + S.robot[r].brad;
    reach *= 1.0 + 1e-9;  // the sums above are rounded
    int cnt = 0;
    while (cnt < S.n_env && env_key[cnt] <= reach + 1e-6) ++cnt;
    S.robot_n_reach[r] = cnt;
    // carried clearance: the obstacles up to kClearHorizon beyond the reach are measured by the cull as well; the
    // nearest one past that bounds every other pair of this shape in every configuration
    while (cnt < S.n_env && env_key[cnt] <= reach + kClearHorizon) ++cnt;
    S.robot_n_clear[r] = cnt;
    if (cnt < S.n_env) S.clear_static = std::min(S.clear_static, env_key[cnt] - reach);
  }
  // Lever arms of the carried clearance (SceneDev::clear_arm): the static reach sum above, started at joint i.  The bound
  // holds for serial 3D chains of revolute joints whose shapes all have a finite bounding radius about their position.
  S.has_clearance = (S.n_branches == 0 && !S.planar && !S.has_meshes && !S.has_prismatic) ? 1 : 0;
  for (int e = 0; e < S.n_env; ++e)
    if (S.env[e].kind == RKH_SHAPE_PLANE || !std::isfinite(S.env[e].brad)) S.has_clearance = 0;
  for (int i = 0; i < kMaxDof; ++i) S.clear_arm[i] = 0.0;
  if (!S.has_clearance)  // nothing is carried: the cull scans the static reach only
    for (int r = 0; r < S.n_robot; ++r) S.robot_n_clear[r] = S.robot_n_reach[r];
  for (int r = 0; r < S.n_robot && S.has_clearance; ++r) {
    if (S.robot[r].kind == RKH_SHAPE_PLANE || !std::isfinite(S.robot[r].brad)) S.has_clearance = 0;
    const double* lp = S.robot[r].pos;
    double arm = std::sqrt(lp[0] * lp[0] + lp[1] * lp[1] + lp[2] * lp[2]) + S.robot[r].brad;
    for (int i = S.robot[r].link; i >= 0; --i) {  // arm = reach of shape r from joint i's origin
      if (i < S.robot[r].link) {
        const double* o = S.joints[i].off_pos;
        arm += std::sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]);
      }
      S.clear_arm[i] = std::max(S.clear_arm[i], arm * (1.0 + 1e-9));  // the sums above are rounded
    }
  }
  // proxy_query_pair_3D::createProxFinderList (proxy_query_model.cpp:215-374), then grouped by routine so
  // that the lanes of a wave run the same closed form (the verdict does not depend on the pair order)
  std::vector<PairDev> pairs;
  // reach of every robot shape's CENTRE from the chain base (over all configurations), for the plane rule below
  std::vector<double> centre_reach(S.n_robot, 0.0);
  for (int r = 0; r < S.n_robot; ++r) {
    double reach = 0.0;
    for (int i = 0; i < n; ++i) {  // serial chain: the links below the shape's joint; branching chains: all of them
      if (S.n_branches == 0 && i >= S.robot[r].link) break;
      const double* o = S.joints[i].off_pos;
      reach += std::sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]);
      const double* mp = S.mount_pos[i];
      reach += std::sqrt(mp[0] * mp[0] + mp[1] * mp[1] + mp[2] * mp[2]);
    }
    const double* lp = S.robot[r].pos;
    centre_reach[r] = reach + std::sqrt(lp[0] * lp[0] + lp[1] * lp[1] + lp[2] * lp[2]);
  }
  for (int i = 0; i < S.n_robot; ++i)
    for (int j = 0; j < S.n_env; ++j) {
      const int ki = S.robot[i].kind, kj = S.env[j].kind;
      PairDev p;
      std::memset(&p, 0, sizeof(p));
      p.robot = uint16_t(i);
      p.env = uint16_t(j);
      bool robot_first = true;
      p.routine = uint8_t(host_pair_routine(ki, kj, &robot_first));
      if (p.routine == 0) continue;  // no finder in the reference
      p.s1_is_robot = robot_first ? 1 : 0;
      if ((ki == RKH_SHAPE_PLANE || kj == RKH_SHAPE_PLANE) && on_prismatic(i)) {
        set_error("rkh_scene_create: a plane cannot be paired with a shape carried by a prismatic joint (the plane rule "
                  "below needs a finite reach)");
        return RKH_ERR_UNSUPPORTED;
      }
      if (ki == RKH_SHAPE_PLANE || kj == RKH_SHAPE_PLANE) {
        // findMinimumDistance skips a finder whose bounding spheres are further apart than the running minimum
        // (proxy_query_model.cpp:384-389).  For bounded shapes that cannot change the minimum; a plane's bounding radius
        // (plane.cpp:31) is finite although the prox_plane_* routines treat it as infinite, so for a plane pair the skip
        // could.  The kernels evaluate every plane pair; that is the reference's result exactly when the pair can never
        // be skipped, i.e. the shapes' bounding spheres overlap in every configuration -- required here.
        double d2 = 0.0;
        for (int k = 0; k < 3; ++k) d2 += (S.env[j].pos[k] - S.base_pos[k]) * (S.env[j].pos[k] - S.base_pos[k]);
        if (std::sqrt(d2) + centre_reach[i] - S.env[j].brad - S.robot[i].brad > 0.0) {
          set_error("rkh_scene_create: a plane must be large enough that its bounding sphere (plane.cpp:31) always overlaps "
                    "the robot shapes' (otherwise the reference's result depends on the finder order)");
          return RKH_ERR_UNSUPPORTED;
        }
      }
      pairs.push_back(p);
    }
  // Pairs a robot shape can never reach (environment shape beyond its static reach, SceneDev::robot_n_reach: the bounding
  // spheres have a positive gap in EVERY configuration) go to the end of the list.  A verdict query ("is some pair closer
  // than 0") skips every pair whose spheres do not overlap anyway, so the verdict kernels -- steer and edge walks -- only
  // scan the first n_pairs_verdict entries (C2: 130 of 300); a distance query (rkh_min_distance) scans them all.
  auto unreachable = [&](const PairDev& q) { return int(q.env) >= S.robot_n_reach[q.robot] ? 1 : 0; };
  std::stable_sort(pairs.begin(), pairs.end(), [&](const PairDev& a, const PairDev& b) {
    const int ua = unreachable(a), ub = unreachable(b);
    return ua != ub ? ua < ub : a.routine < b.routine;
  });
  int n_verdict = 0;
  for (const PairDev& q : pairs) n_verdict += unreachable(q) ? 0 : 1;
  sc->n_pairs_verdict = n_verdict;
  // The record queries name a pair by the caller's shape indices and order the pairs as the reference's finder list
  // does: the robot shapes kept the caller's order above, the environment shapes were sorted by closeness.
  std::vector<uint32_t> env_rank(S.n_env, 0u);  // place of scene environment shape j among the caller's environment shapes
  for (int j = 0; j < S.n_env; ++j)
    for (int k = 0; k < S.n_env; ++k) env_rank[j] += env_src[k] < env_src[j] ? 1u : 0u;
  std::vector<PairIdDev> pair_ids(pairs.size());
  for (size_t k = 0; k < pairs.size(); ++k) {
    const PairDev& q = pairs[k];
    const uint32_t rid = uint32_t(robot_src[q.robot]), eid = uint32_t(env_src[q.env]);
    pair_ids[k].rank = uint32_t(q.robot) * uint32_t(S.n_env) + env_rank[q.env];
    pair_ids[k].shape1 = q.s1_is_robot ? rid : eid;
    pair_ids[k].shape2 = q.s1_is_robot ? eid : rid;
  }
  return upload_scene(ctx, std::move(sc), pairs, out, pair_ids);
}

rkh_status rkh_diag_gjk_distance(rkh_ctx* ctx, const rkh_shape* a, const rkh_shape* b, uint32_t n,
                                 const double* mesh_vertices, uint32_t n_mesh_vertices, double* dist) {
  if (!ctx || !a || !b || !dist) return RKH_ERR_BAD_ARG;
  return gjk_pairs_run(ctx, a, b, n, mesh_vertices, n_mesh_vertices, dist, nullptr, nullptr, nullptr);
}

rkh_status rkh_diag_gjk_records(rkh_ctx* ctx, const rkh_shape* a, const rkh_shape* b, uint32_t n, const double* mesh_vertices,
                                uint32_t n_mesh_vertices, double* dist, double* point1, double* point2) {
  if (!ctx || !a || !b || !dist || !point1 || !point2) return RKH_ERR_BAD_ARG;
  return gjk_pairs_run(ctx, a, b, n, mesh_vertices, n_mesh_vertices, dist, point1, point2, nullptr);
}

rkh_status rkh_diag_gjk_depth_records(rkh_ctx* ctx, const rkh_shape* a, const rkh_shape* b, uint32_t n, const double* mesh_vertices,
                                      uint32_t n_mesh_vertices, double* dist, double* point1, double* point2, double* normal) {
  if (!ctx || !a || !b || !dist || !point1 || !point2 || !normal) return RKH_ERR_BAD_ARG;
  return gjk_pairs_run(ctx, a, b, n, mesh_vertices, n_mesh_vertices, dist, point1, point2, normal);
}

rkh_status rkh_scene_destroy(rkh_scene* scene) {
  delete scene;  // (its buffers free themselves; hipFree waits for the device)
  return RKH_OK;
}
int rkh_scene_num_dof(const rkh_scene* scene) { return scene ? scene->host.n_dof : 0; }
int rkh_scene_num_pairs(const rkh_scene* scene) { return scene ? scene->n_pairs : 0; }

}  // extern "C"

namespace {
// dynamics entry points: branching chains are fine (wave-per-edge kernels); planar chains are position level only
rkh_status reject_branches(const rkh_scene* scene) {
  if (scene->host.planar && !scene->host.planar_dynamics) {
    set_error("this planar (2D) chain was given at position level (no actuators / inertias): quasi-static spaces only");
    return RKH_ERR_UNSUPPORTED;
  }
  return RKH_OK;
}
rkh_status check_err_flag(rkh_scene* scene) {
  int flag = 0;
  RKH_HIP(hipMemcpy(&flag, scene->d_err.get(), sizeof(int), hipMemcpyDeviceToHost));
  if (flag != 0) {
    RKH_HIP(hipMemset(scene->d_err.get(), 0, sizeof(int)));
    set_error("mass matrix is singular (Cholesky pivot < 1e-8)");
    return rkh_status(flag);
  }
  return RKH_OK;
}
// the record queries serve 3D scenes whose pairs all have a closed form
rkh_status records_supported(const rkh_scene* scene, const char* entry) {
  const char* why = scene->host.planar      ? "planar (2D) scenes: the records of proxy_query_pair_2D come from "
                                              "rkh_min_distance_records_2d / rkh_collision_records_2d"
                    : scene->host.has_meshes ? "scenes with mesh shapes: the support-map (GJK) query yields a distance and no points"
                    : scene->n_pairs > kMaxRecordPairs ? "more proxy pairs than the record kernels keep track of"
                                                       : nullptr;
  if (!why) return RKH_OK;
  set_error(std::string(entry) + ": not supported for " + why);
  return RKH_ERR_UNSUPPORTED;
}
// the _meshes entries serve every 3D scene
rkh_status records_meshes_supported(const rkh_scene* scene, const char* entry) {
  const char* why = scene->host.planar ? "planar (2D) scenes: the records of proxy_query_pair_2D come from "
                                         "rkh_min_distance_records_2d / rkh_collision_records_2d"
                    : scene->n_pairs > kMaxRecordPairs ? "more proxy pairs than the record kernels keep track of"
                                                       : nullptr;
  if (!why) return RKH_OK;
  set_error(std::string(entry) + ": not supported for " + why);
  return RKH_ERR_UNSUPPORTED;
}
// and their planar twins serve planar scenes
rkh_status records_2d_supported(const rkh_scene* scene, const char* entry) {
  if (scene->host.planar) return RKH_OK;
  set_error(std::string(entry) + ": not supported for 3D scenes: their records come from rkh_min_distance_records / "
            "rkh_collision_records");
  return RKH_ERR_UNSUPPORTED;
}
// Every record entry after its checks: the same transfers around launch(stream, d_x, out, d_normal).  width: the doubles
// of a point (3, planar scenes 2).  n_found = null: one record per state (the min-distance entries); else `cap` slots per
// state and their count (the collision entries; cap = 0 still allocates an element each).  normal: the depth entries'.
template <class Launch>
rkh_status records_run(rkh_scene* scene, int width, const double* x, uint32_t B, uint32_t cap, uint32_t* n_found, double* dist,
                       double* point1, double* point2, double* normal, uint32_t* shape1, uint32_t* shape2, Launch launch) {
  if (B == 0) return RKH_OK;
  const size_t slots = n_found ? size_t(B) * cap : size_t(B), min_n = n_found ? 1 : 0;
  hipStream_t s = scene->ctx->stream;
  StagedCall call(s);
  const double* dx = call.in(x, size_t(B) * 2 * scene->host.n_dof);
  RecordOut out;
  if (n_found) out.n_found = call.out(n_found, size_t(B));
  double* dn3 = normal ? call.out(normal, slots * 3, min_n) : nullptr;
  out.dist = call.out(dist, slots, min_n);
  out.point1 = call.out(point1, slots * width, min_n);
  out.point2 = call.out(point2, slots * width, min_n);
  out.shape1 = call.out(shape1, slots, min_n);
  out.shape2 = call.out(shape2, slots, min_n);
  RKH_TRY(call.status());
  RKH_TRY(launch(s, dx, out, dn3));
  return call.fetch();
}
}  // namespace

extern "C" {

rkh_status rkh_state_derivative(rkh_scene* scene, const double* x, const double* u, uint32_t B, double* pd, double* M,
                                double* f) {
  if (scene && reject_branches(scene) != RKH_OK) return RKH_ERR_UNSUPPORTED;
  if (!scene || !x || !u || !pd) return RKH_ERR_BAD_ARG;
  if (B == 0) return RKH_OK;
  const int n = scene->host.n_dof;
  hipStream_t s = scene->ctx->stream;
  StagedCall call(s);
  const double* dx = call.in(x, size_t(B) * 2 * n);
  const double* du = call.in(u, size_t(B) * n);
  double* dpd = call.out(pd, size_t(B) * 2 * n);
  double* dM = call.out(M, size_t(B) * n * n);
  double* df = call.out(f, size_t(B) * n);
  RKH_TRY(call.status());
  RKH_TRY(launch_state_derivative(s, *scene, dx, du, B, dpd, dM, df, scene->d_err.get()));
  RKH_TRY(call.fetch());
  return check_err_flag(scene);
}

rkh_status rkh_min_distance(rkh_scene* scene, const double* x, uint32_t B, double* dist) {
  if (!scene || !x || !dist) return RKH_ERR_BAD_ARG;
  if (B == 0) return RKH_OK;
  const int n = scene->host.n_dof;
  hipStream_t s = scene->ctx->stream;
  StagedCall call(s);
  const double* dx = call.in(x, size_t(B) * 2 * n);
  double* dd = call.out(dist, size_t(B));
  RKH_TRY(call.status());
  RKH_TRY(launch_min_distance(s, *scene, dx, B, dd));
  return call.fetch();
}

rkh_status rkh_min_distance_records(rkh_scene* scene, const double* x, uint32_t B, double* dist, double* point1,
                                    double* point2, uint32_t* shape1, uint32_t* shape2) {
  if (!scene || !x || !dist || !point1 || !point2 || !shape1 || !shape2) return RKH_ERR_BAD_ARG;
  RKH_TRY(records_supported(scene, "rkh_min_distance_records"));
  return records_run(scene, 3, x, B, 0, nullptr, dist, point1, point2, nullptr, shape1, shape2,
                     [&](hipStream_t s, const double* dx, RecordOut out, double*) {
                       return launch_min_distance_records(s, *scene, dx, B, out);
                     });
}

rkh_status rkh_min_distance_records_meshes(rkh_scene* scene, const double* x, uint32_t B, double* dist, double* point1,
                                           double* point2, uint32_t* shape1, uint32_t* shape2) {
  if (!scene || !x || !dist || !point1 || !point2 || !shape1 || !shape2) return RKH_ERR_BAD_ARG;
  RKH_TRY(records_meshes_supported(scene, "rkh_min_distance_records_meshes"));
  return records_run(scene, 3, x, B, 0, nullptr, dist, point1, point2, nullptr, shape1, shape2,
                     [&](hipStream_t s, const double* dx, RecordOut out, double*) {
                       return launch_min_distance_records_meshes(s, *scene, dx, B, out);
                     });
}

rkh_status rkh_min_distance_records_depth(rkh_scene* scene, const double* x, uint32_t B, double* dist, double* point1,
                                          double* point2, double* normal, uint32_t* shape1, uint32_t* shape2) {
  if (!scene || !x || !dist || !point1 || !point2 || !normal || !shape1 || !shape2) return RKH_ERR_BAD_ARG;
  RKH_TRY(records_meshes_supported(scene, "rkh_min_distance_records_depth"));
  return records_run(scene, 3, x, B, 0, nullptr, dist, point1, point2, normal, shape1, shape2,
                     [&](hipStream_t s, const double* dx, RecordOut out, double* dn3) {
                       return launch_min_distance_records_depth(s, *scene, dx, B, out, dn3);
                     });
}

rkh_status rkh_diag_distance_query_ms(rkh_scene* scene, const double* x, uint32_t B, int records, uint32_t runs, float* ms) {
  if (!scene || !x || !ms || B == 0) return RKH_ERR_BAD_ARG;
  const bool planar = scene->host.planar != 0;  // planar scenes: the _2d record kernel (points of two doubles)
  if (records && !planar) RKH_TRY(records_meshes_supported(scene, "rkh_diag_distance_query_ms"));
  const int n = scene->host.n_dof;
  hipStream_t s = scene->ctx->stream;
  const bool depth = records == 2 && !planar;  // the depth form of the 3D record kernel
  StagedCall call(s);  // nothing is copied back: the times are the answer
  const double* dx = call.in(x, size_t(B) * 2 * n);
  RecordOut out;
  out.dist = call.scratch<double>(size_t(B));
  out.point1 = call.scratch<double>(size_t(B) * 3);
  out.point2 = call.scratch<double>(size_t(B) * 3);
  double* dn3 = depth ? call.scratch<double>(size_t(B) * 3) : nullptr;
  out.shape1 = call.scratch<uint32_t>(size_t(B));
  out.shape2 = call.scratch<uint32_t>(size_t(B));
  RKH_TRY(call.status());
  hipEvent_t e0 = nullptr, e1 = nullptr;
  RKH_HIP(hipEventCreate(&e0));
  RKH_HIP(hipEventCreate(&e1));
  rkh_status st = RKH_OK;
  for (uint32_t r = 0; r < runs && st == RKH_OK; ++r) {
    hipError_t err = hipEventRecord(e0, s);
    st = !records ? launch_min_distance(s, *scene, dx, B, out.dist)
         : planar ? launch_min_distance_records_2d(s, *scene, dx, B, out)
         : depth  ? launch_min_distance_records_depth(s, *scene, dx, B, out, dn3)
                  : launch_min_distance_records_meshes(s, *scene, dx, B, out);  // (no meshes: the plain kernel)
    if (err == hipSuccess) err = hipEventRecord(e1, s);
    if (err == hipSuccess) err = hipEventSynchronize(e1);
    if (err == hipSuccess) err = hipEventElapsedTime(&ms[r], e0, e1);
    if (err != hipSuccess && st == RKH_OK) {
      set_error(std::string("rkh_diag_distance_query_ms: ") + hipGetErrorString(err));
      st = RKH_ERR_DEVICE;
    }
  }
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  return st;
}

rkh_status rkh_collision_records(rkh_scene* scene, const double* x, uint32_t B, uint32_t cap, uint32_t* n_found, double* dist,
                                 double* point1, double* point2, uint32_t* shape1, uint32_t* shape2) {
  if (!scene || !x || !n_found || !dist || !point1 || !point2 || !shape1 || !shape2) return RKH_ERR_BAD_ARG;
  RKH_TRY(records_supported(scene, "rkh_collision_records"));
  return records_run(scene, 3, x, B, cap, n_found, dist, point1, point2, nullptr, shape1, shape2,
                     [&](hipStream_t s, const double* dx, RecordOut out, double*) {
                       return launch_collision_records(s, *scene, dx, B, cap, out);
                     });
}

rkh_status rkh_collision_records_meshes(rkh_scene* scene, const double* x, uint32_t B, uint32_t cap, uint32_t* n_found,
                                        double* dist, double* point1, double* point2, uint32_t* shape1, uint32_t* shape2) {
  if (!scene || !x || !n_found || !dist || !point1 || !point2 || !shape1 || !shape2) return RKH_ERR_BAD_ARG;
  RKH_TRY(records_meshes_supported(scene, "rkh_collision_records_meshes"));
  return records_run(scene, 3, x, B, cap, n_found, dist, point1, point2, nullptr, shape1, shape2,
                     [&](hipStream_t s, const double* dx, RecordOut out, double*) {
                       return launch_collision_records_meshes(s, *scene, dx, B, cap, out);
                     });
}

rkh_status rkh_collision_records_depth(rkh_scene* scene, const double* x, uint32_t B, uint32_t cap, uint32_t* n_found,
                                       double* dist, double* point1, double* point2, double* normal, uint32_t* shape1,
                                       uint32_t* shape2) {
  if (!scene || !x || !n_found || !dist || !point1 || !point2 || !normal || !shape1 || !shape2) return RKH_ERR_BAD_ARG;
  RKH_TRY(records_meshes_supported(scene, "rkh_collision_records_depth"));
  return records_run(scene, 3, x, B, cap, n_found, dist, point1, point2, normal, shape1, shape2,
                     [&](hipStream_t s, const double* dx, RecordOut out, double* dn3) {
                       return launch_collision_records_depth(s, *scene, dx, B, cap, out, dn3);
                     });
}

rkh_status rkh_min_distance_records_2d(rkh_scene* scene, const double* x, uint32_t B, double* dist, double* point1,
                                       double* point2, uint32_t* shape1, uint32_t* shape2) {
  if (!scene || !x || !dist || !point1 || !point2 || !shape1 || !shape2) return RKH_ERR_BAD_ARG;
  RKH_TRY(records_2d_supported(scene, "rkh_min_distance_records_2d"));
  return records_run(scene, 2, x, B, 0, nullptr, dist, point1, point2, nullptr, shape1, shape2,
                     [&](hipStream_t s, const double* dx, RecordOut out, double*) {
                       return launch_min_distance_records_2d(s, *scene, dx, B, out);
                     });
}

rkh_status rkh_collision_records_2d(rkh_scene* scene, const double* x, uint32_t B, uint32_t cap, uint32_t* n_found,
                                    double* dist, double* point1, double* point2, uint32_t* shape1, uint32_t* shape2) {
  if (!scene || !x || !n_found || !dist || !point1 || !point2 || !shape1 || !shape2) return RKH_ERR_BAD_ARG;
  RKH_TRY(records_2d_supported(scene, "rkh_collision_records_2d"));
  return records_run(scene, 2, x, B, cap, n_found, dist, point1, point2, nullptr, shape1, shape2,
                     [&](hipStream_t s, const double* dx, RecordOut out, double*) {
                       return launch_collision_records_2d(s, *scene, dx, B, cap, out);
                     });
}

rkh_status rkh_propagate(rkh_scene* scene, const rkh_dyn_space* space, const double* a, const double* b, uint32_t B,
                         double fraction, double* x_out, uint32_t* steps_free, double* record) {
  if (scene && reject_branches(scene) != RKH_OK) return RKH_ERR_UNSUPPORTED;
  if (!scene || !space || !a || !b || !x_out || !steps_free) return RKH_ERR_BAD_ARG;
  if (space->n_dof != scene->host.n_dof) {
    set_error("rkh_propagate: rkh_dyn_space.n_dof does not match the scene");
    return RKH_ERR_BAD_ARG;
  }
  if (B == 0) return RKH_OK;
  DynDev dyn;
  RKH_TRY(build_dyn_dev(*space, fraction, &dyn));
  const int n = scene->host.n_dof, D = 2 * n;
  const int rec_stride = space->steps_per_edge + 1;
  hipStream_t s = scene->ctx->stream;
  StagedCall call(s);
  EdgeIO io;
  io.src = call.in(a, size_t(B) * D);
  io.src_stride = D;
  io.tgt = call.in(b, size_t(B) * D);
  io.tgt_stride = D;
  io.B = B;
  io.x_out = call.out(x_out, size_t(B) * D);
  io.steps_free = call.out(steps_free, size_t(B));
  io.record = record ? call.out(record, size_t(B) * rec_stride * D, 0, 0) : nullptr;
  io.record_stride = rec_stride;
  io.err_flag = scene->d_err.get();
  RKH_TRY(call.status());
  // the mapping (identical results): by default a call of few edges -- the adaptors steer ONE edge per call -- takes the
  // lowest-latency one (steer_mapping)
  const SteerMapping m = steer_mapping(scene->host, SteerEntry::Propagate, steer_request(), B, 1, 0);
  note_steer_mapping(m);
  DeviceBuffer<void> dws;  // the two-lanes form's workspace
  StreamWait dws_idle{s};
  if (m == SteerMapping::Pair) RKH_TRY(dws.alloc(propagate_pairs_workspace_bytes(n, B, 0, 1)));
  KernelGate gate;  // no gate; the two-lanes form carries its clearance bound unless RKH_STEER_CLEARANCE=0
  gate.clearance = steer_request().clearance;
  gate.clear_stats = scene->d_clear_stats.get();
  RKH_TRY(launch_propagate(s, *scene, m, dyn, io, B, 0, nullptr, nullptr, 1, static_cast<double*>(dws.get()), gate));
  RKH_TRY(call.fetch());
  return check_err_flag(scene);
}

rkh_status rkh_diag_feval_cycles(rkh_scene* scene, const double* x, const double* u, uint32_t B, int iters,
                                 uint64_t* cycles) {
  if (scene && reject_branches(scene) != RKH_OK) return RKH_ERR_UNSUPPORTED;
  if (!scene || !x || !u || !cycles || B == 0) return RKH_ERR_BAD_ARG;
  const int n = scene->host.n_dof;
  hipStream_t s = scene->ctx->stream;
  // the two-lanes-per-edge kernel writes one record of 8 counters per wave of states, and the two-waves-per-edge kernel
  // rows 2 b / 2 b + 1 for B / 2 states: both into zeroed rows
  const SteerMapping m = steer_mapping(scene->host, SteerEntry::CycleProbe, steer_request(), B, 1, 0);
  const bool sparse = m == SteerMapping::Pair || m == SteerMapping::Duo;
  StagedCall call(s);
  const double* dx = call.in(x, size_t(B) * 2 * n);
  const double* du = call.in(u, size_t(B) * n);
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are copied as they are");
  unsigned long long* dout = call.out(reinterpret_cast<unsigned long long*>(cycles), size_t(B) * 8, 0, sparse ? 0 : StagedCall::kNoFill);
  double* dsink = call.scratch<double>(size_t(B));
  RKH_TRY(call.status());
  if (m == SteerMapping::Pair) {
    RKH_TRY(launch_pair_cycles(s, *scene, dx, du, B, iters, dout, dsink));
  } else if (m == SteerMapping::Duo) {
    RKH_TRY((B >= 2) ? launch_feval_cycles_duo(s, *scene, dx, du, B, iters, dout, dsink) : RKH_ERR_BAD_ARG);
  } else {
    RKH_TRY(launch_feval_cycles(s, *scene, dx, du, B, iters, dout, dsink));
  }
  return call.fetch();
}

const char* rkh_steer_mapping_name(void) {
  switch (g_steer_mapping) {
    case SteerMapping::Auto: return "auto";
    case SteerMapping::Duo: return "duo";
    case SteerMapping::Wave16: return "wave16";
    case SteerMapping::Pair: return "pair";
    case SteerMapping::Planar: return "planar";
    case SteerMapping::Prismatic: return "prismatic";
    default: return "wave";
  }
}

rkh_status rkh_diag_proximity_counts(rkh_scene* scene, const double* x, uint32_t B, uint64_t counts[8]) {
  if (scene && reject_branches(scene) != RKH_OK) return RKH_ERR_UNSUPPORTED;
  if (!scene || !x || !counts || B == 0) return RKH_ERR_BAD_ARG;
  const int n = scene->host.n_dof;
  if (!scene_fits_lane_kernel(scene->host)) {
    set_error("proximity counts: a scene of the two-lanes steer mapping is needed");
    return RKH_ERR_UNSUPPORTED;
  }
  hipStream_t s = scene->ctx->stream;
  StagedCall call(s);
  const double* dx = call.in(x, size_t(B) * 2 * n);
  unsigned long long* dout = call.out(reinterpret_cast<unsigned long long*>(counts), 8, 0, 0);
  RKH_TRY(call.status());
  RKH_TRY(launch_pair_counts(s, *scene, dx, B, dout));
  RKH_TRY(call.fetch());
  // what the host knows: proxy pairs of the scene, and the ones inside the shapes' static reach
  counts[5] = uint64_t(scene->n_pairs);
  counts[6] = uint64_t(scene->n_pairs_verdict);
  counts[7] = 0;
  return RKH_OK;
}

rkh_status rkh_diag_proximity_clearance(rkh_scene* scene, const double* x, uint32_t B, float* out) {
  if (scene && reject_branches(scene) != RKH_OK) return RKH_ERR_UNSUPPORTED;
  if (!scene || !x || !out || B == 0) return RKH_ERR_BAD_ARG;
  const int n = scene->host.n_dof;
  if (!scene_fits_lane_kernel(scene->host)) {
    set_error("proximity clearance: a scene of the two-lanes steer mapping is needed");
    return RKH_ERR_UNSUPPORTED;
  }
  hipStream_t s = scene->ctx->stream;
  StagedCall call(s);
  const double* dx = call.in(x, size_t(B) * 2 * n);
  unsigned long long* dcnt = call.scratch<unsigned long long>(8, 0, 0);
  float* dout = call.out(out, size_t(B));
  RKH_TRY(call.status());
  RKH_TRY(launch_pair_counts(s, *scene, dx, B, dcnt, dout));
  RKH_TRY(call.fetch());
  if (!scene->host.has_clearance)  // the kernels carry nothing in such a scene
    for (uint32_t i = 0; i < B; ++i) out[i] = 0.0f;
  return RKH_OK;
}

rkh_status rkh_diag_steer_clearance_counts(rkh_scene* scene, uint64_t counts[2]) {
  if (!scene || !counts) return RKH_ERR_BAD_ARG;
  hipStream_t s = scene->ctx->stream;
  unsigned long long v[2] = {0, 0};
  RKH_HIP(hipStreamSynchronize(s));
  RKH_HIP(hipMemcpy(v, scene->d_clear_stats.get(), sizeof(v), hipMemcpyDeviceToHost));
  counts[0] = v[0];
  counts[1] = v[1];
  return RKH_OK;
}

rkh_status rkh_edge_check(rkh_scene* scene, const double* lower, const double* upper, double min_interval,
                          const double* a, const double* b, uint32_t B, double fraction, double* out,
                          uint32_t* n_checked) {
  if (!scene || !lower || !upper || !a || !b || !out || !n_checked || !(min_interval > 0.0)) return RKH_ERR_BAD_ARG;
  if (B == 0) return RKH_OK;
  const int n = scene->host.n_dof;
  QsDev qs;
  std::memset(&qs, 0, sizeof(qs));
  qs.min_interval = min_interval;
  qs.fraction = fraction;
  qs_set_speed(qs, nullptr, n);  // this entry point takes an ordinary joint space
  for (int i = 0; i < n; ++i) {
    qs.lower[i] = lower[i];
    qs.upper[i] = upper[i];
  }
  hipStream_t s = scene->ctx->stream;
  StagedCall call(s);
  EdgeIO io;
  io.src = call.in(a, size_t(B) * n);
  io.src_stride = n;
  io.tgt = call.in(b, size_t(B) * n);
  io.tgt_stride = n;
  io.B = B;
  io.x_out = call.out(out, size_t(B) * n);
  io.steps_free = call.out(n_checked, size_t(B));
  io.err_flag = scene->d_err.get();
  RKH_TRY(call.status());
  RKH_TRY(launch_edge_check(s, *scene, qs, io, B));
  return call.fetch();
}

}  // extern "C"
