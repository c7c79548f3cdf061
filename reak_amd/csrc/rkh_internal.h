// rkh_internal.h -- shared declarations of librkh.so (host side + device structs).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/rkh.h"
#include "../../include/rkh_diag.h"
#include "device_buffer.h"
#include "kinematics_device.h"  // KinChain, KinFrameRef
#include "knn_plan.h"    // KnnWorkspace, knn_plan, knn_carve
#include "steer_edge.h"  // EdgeMode, EdgeIO, KernelGate, kMaxSteps

namespace rkh {

void set_error(const std::string& msg);

#define RKH_HIP(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      ::rkh::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                     \
      return (_e == hipErrorOutOfMemory) ? RKH_ERR_OOM : RKH_ERR_DEVICE;                       \
    }                                                                                          \
  } while (0)

// returns the status of a step that failed
#define RKH_TRY(expr)                                                                          \
  do {                                                                                         \
    const rkh_status _st = (expr);                                                             \
    if (_st != RKH_OK) return _st;                                                             \
  } while (0)

// Calls f(std::integral_constant<int, N>()) for the N of Ns... equal to n: the chain sizes a launcher's kernels are
// instantiated for.  Any other n: RKH_ERR_UNSUPPORTED, with the list in the error message.
template <int... Ns, class F>
rkh_status with_n(int n, F&& f) {
  if ((... || (n == Ns && (f(std::integral_constant<int, Ns>()), true)))) return RKH_OK;
  std::string list;
  ((list += (list.empty() ? "" : ", ") + std::to_string(Ns)), ...);
  set_error("chains of " + std::to_string(n) + " joints: these kernels are instantiated for " + list + " joints");
  return RKH_ERR_UNSUPPORTED;
}

constexpr int kMaxDof = 12;         // joints of a scene (dynamics kernels: 1, 2, 3, 6; quasi-static kernels also 12)
constexpr int kMaxEnvShapes = 256;  // environment shapes resident in LDS

// ---- NN sweep (nn_sweep.hip) -----------------------------------------------------------------
// Vertex positions live row-major [n][D] in HBM (one contiguous 8*D-byte row per vertex): the sweep
// streams them linearly through LDS tiles and the propagate kernel gathers a parent with one row read.
struct NnStore {  // a view: the handle that fills it in owns the rows
  double* d_pos = nullptr;  // [capacity][D]
  uint64_t capacity = 0;
  int D = 0;
};

struct NnArgs {  // one 1-NN problem: tree rows, queries, outputs (device pointers)
  const double* pos = nullptr;        // [n][DP] vertex rows
  uint64_t n = 0;                      // vertex count (used if d_n == nullptr)
  const uint32_t* d_n = nullptr;       // vertex count read on the device (planner rounds enqueued without host sync)
  const double* q = nullptr;           // [B][D] queries
  const uint32_t* d_qoff = nullptr;    // optional row offset of the query block, read on the device
  uint32_t B = 0;
  const uint32_t* d_B = nullptr;       // query count read on the device
  double* part_dist = nullptr;         // [blocks][Bpad] per-block partial minima
  uint32_t* part_idx = nullptr;
  uint32_t* idx = nullptr;             // [B] results
  double* dist = nullptr;
  uint32_t* seed = nullptr;            // [B] optional: matrix-core sweeps start from a sampled minimum (all 0xFF between sweeps)
  // planner-regime sweep over the half-precision mirror of the tree (nn_mirror.hip)
  const void* mirror = nullptr;          // [ceil(capacity / 32)] slabs of 1 KB, nn_mirror.h
  const uint32_t* dx_max_bits = nullptr; // max over the rows of |x - x_h| (bits of a float)
  uint4* qfrag = nullptr;                // [B][2] B operands of the round's queries
  double* qinfo = nullptr;               // [B][3] |q_h|^2, |q - q_h|, |q|
  float* thr = nullptr;                  // [B] smallest estimate + band
  uint32_t* cand_cnt = nullptr;          // [B] rows at or below thr (zero between sweeps)
  uint32_t* cand_rows = nullptr;         // [B][nn1_mirror_cand_cap()]
  float* est = nullptr;                  // [nn1_mirror_max_slices()][est_stride] smallest estimate per (row slice, query)
  uint32_t est_stride = 0;
  uint16_t* open_list = nullptr;         // [nn1_mirror_max_slices()][est_stride] queries open in a row slice (nn_mirror.h)
  uint32_t* open_cnt = nullptr;          // [nn1_mirror_max_slices()] their number (written every round by the thr kernel)
};
// nn_mirror.hip
uint32_t nn1_mirror_queries();
uint32_t nn1_mirror_cand_cap();
uint32_t nn1_mirror_max_slices();
size_t nn1_mirror_bytes(uint64_t capacity_rows);
size_t nn1_mirror_query_bytes();
void nn1_mirror_carve(void* base, uint32_t b_max, NnArgs* a);
bool nn1_mirror_applies(int D, double coord_bound);
bool nn1_mirror_open_lists();  // RKH_NN_MIRROR_OPEN (default on)
rkh_status launch_mirror_fill(hipStream_t s, void* d_mirror, uint64_t capacity_rows);
rkh_status launch_mirror_build(hipStream_t s, void* d_mirror, const double* d_pos, uint64_t n, int D, int DP, double scale,
                               uint32_t* d_dx_max_bits);
rkh_status launch_nn1_mirror(hipStream_t s, int D, const NnArgs* d_table, uint32_t n_problems, uint64_t n_upper,
                             uint32_t B_upper, double x_norm_bound, double scale, const uint32_t* d_yblock_base,
                             bool open_lists, hipEvent_t ev0, hipEvent_t ev1);
int nn_padded_dims(int D);
rkh_status launch_nn1(hipStream_t s, int D, const NnArgs& single, const NnArgs* d_table, uint32_t n_problems,
                      uint64_t n_upper, uint32_t B, uint32_t part_capacity_blocks, hipEvent_t ev0 = nullptr,
                      hipEvent_t ev1 = nullptr, double coord_bound = 0.0, const uint32_t* d_yblock_base = nullptr,
                      bool table_has_seed = false);
// d_yblock_base (table launches, matrix-core kernel): [n_problems + 1] exclusive prefix of ceil(B_p / nn1_mfma_queries())
// over the problems; the grid's blocks then take the working (row slice, query block) pairs in dispatch order.
uint32_t nn1_mfma_queries();
// launch_nn1 with coord_bound > 0: every |coordinate| of rows and queries is <= coord_bound; sweeps with >= 32 queries
// then run the single-precision pre-filter variant (identical results).
// Partial minima per query (row slices) that launch_nn1 may write for at most B_max queries per problem.
uint32_t nn1_partial_blocks(int D, uint64_t n_upper, uint32_t B_max, uint32_t n_problems, double coord_bound);
// k-NN with radius (knn_sweep.hip).  ws: device workspace planned and carved by knn_plan.h (KnnWorkspace, knn_plan,
// knn_carve); *ws.overflow is set (non-zero) if a query met more than the candidate capacity.  After a first pass
// (launch_nnk / launch_nnk_table) that left the word set, the caller runs the exact retry of the same job(s) once
// (launch_nnk_retry / launch_nnk_table_retry: three launches that redo only the queries whose list overflowed and
// leave every other query's result as it is); the word is then set only for coincident vertices (knn_plan.h).
// list_cap > 0 (knn_list_cap_from_env(): RKH_KNN_LIST_CAP, rkh_diag.h) shortens the candidate lists to
// next_pow2(max(list_cap, 2 k)) slots inside the workspace planned for the full ones: first passes then overflow on
// ordinary data and the exact retry answers, with the same results.
uint32_t knn_list_cap_from_env();  // 0: not set
uint64_t knn_retry_count();        // exact retries launched in this process
inline rkh_status knn_plan_or_error(uint64_t n, uint32_t B, uint32_t k, KnnWorkspace* ws, size_t* bytes,
                                    uint32_t list_cap = 0) {
  const rkh_status st = knn_plan(n, B, k, ws, bytes);
  if (st != RKH_OK) {
    set_error("k-NN: k must be in [1, 1024]");
    return st;
  }
  if (list_cap) ws->cmax = std::min(ws->cmax, next_pow2(std::max(list_cap, 2 * k)));
  return st;
}
// what a caller reports when the word is still set after the retry
inline const char* knn_capacity_text() {
  return "k-NN candidate capacity exceeded: too many vertices at exactly the k-th nearest distance (coincident "
         "vertices; a smaller k or radius that ends before them avoids it)";
}
rkh_status launch_nnk(hipStream_t s, const NnStore& st, uint64_t n, const double* d_q, uint32_t B, uint32_t k,
                      double radius, uint32_t* d_idx, double* d_dist, uint32_t* d_count, const KnnWorkspace& ws);
rkh_status launch_nnk_retry(hipStream_t s, const NnStore& st, uint64_t n, const double* d_q, uint32_t B, uint32_t k,
                            double radius, uint32_t* d_idx, double* d_dist, uint32_t* d_count, const KnnWorkspace& ws);
// One k-NN job (one tree, B queries).  A launch serves either one job (by value) or a device table of jobs
// (blockIdx.z = job; RRT* / PRM batches: one query per problem, all problems in the same four launches).
struct KnnArgs {
  const double* pos = nullptr;  // [n][DP] vertex rows
  uint64_t n = 0;
  const double* q = nullptr;    // [B][D]
  int D = 0;
  uint32_t B = 0, k = 0;
  double radius = 0.0;
  KnnWorkspace ws;
  uint32_t m_pow2 = 0;          // next_pow2(ws.m_sub)
  uint32_t* out_idx = nullptr;  // [B][k]
  double* out_dist = nullptr;
  uint32_t* out_cnt = nullptr;  // [B]
};
// Launch a table of jobs (d_table on the device, h_table its host copy for grid sizing).  All jobs share D.
rkh_status launch_nnk_table(hipStream_t s, int D, const KnnArgs* d_table, const KnnArgs* h_table, uint32_t n_jobs);
rkh_status launch_nnk_table_retry(hipStream_t s, int D, const KnnArgs* d_table, const KnnArgs* h_table, uint32_t n_jobs);
rkh_status launch_fill_uniform(hipStream_t s, const NnStore& st, uint64_t n, uint64_t seed);

// ---- scene (propagate.hip) ---------------------------------------------------------------------
struct JointDev {  // one {actuator, rotor inertia, revolute joint, rigid link, link inertia} group
  double axis[3];     // revolute_joint_3D::mAxis as given
  double axis_n[3];   // axis_angle's normalised copy (rotations_3D.hpp:1961-1974)
  double joint_inertia;
  double off_pos[3];
  double off_quat[4];
  double off_R[9];   // rotmat(off_quat), row-major (same formula as the device would use)
  double mass;
  double inertia[6]; // a11,a12,a13,a22,a23,a33
};
struct ShapeDev {
  int32_t kind;
  int32_t link;      // robot shapes: joint index whose end frame anchors the shape; env: -1
  double pos[3];
  double quat[4];
  double dims[3];
  double brad;       // getBoundingRadius()
};
struct SceneDev {
  int32_t n_dof;
  int32_t n_robot;   // robot shapes (anchored)
  int32_t n_env;     // environment shapes
  int32_t beam_on;   // 1: the chain carries a flexible_beam_3D (see beam_j1 / beam_j2)
  double base_pos[3];
  double base_quat[4];
  double base_acc[3];
  JointDev joints[kMaxDof];
  ShapeDev robot[kMaxDof * 2];
  ShapeDev env[kMaxEnvShapes];
  // cull table of the environment: centre of the bounding sphere (pose.transformToGlobal(0) = the pose's position)
  // RELATIVE TO base_pos -- the fp32 cull of the two-lanes steer kernels must not depend on where the world sits -- and
  // its radius; one bit per shape and kind (sphere, box, capped cylinder) in chunks of 64 shapes
  double env_cull[kMaxEnvShapes][4];
  unsigned long long env_kind_mask[3][kMaxEnvShapes / 64];
  // Branching (quasi-static kernels only): joint j with branch_start[j] != 0 does not continue the previous link but
  // starts from the chain base through a fixed mount (rigid_link_3D from frame 0; identity if the joint sits on the base)
  int32_t branch_start[kMaxDof];
  int32_t n_branches;  // joints with branch_start (0 for a plain serial chain)
  int32_t beam_j1;     // the beam's anchor 1 is the link end frame of this joint
  int32_t beam_j2;     // anchor 2: link end frame of this joint, or -1 = the world anchor (beam_pos, beam_quat)
  int32_t planar_dynamics;  // planar chain given with its actuators and inertias: the dynamics entry points accept it
  int32_t planar;      // 1: planar chain (revolute_joint_2D / rigid_link_2D, 2D shapes): poses carry (x, y) and (cos, sin)
  int32_t branch_first[kMaxDof];  // first joint of the branch joint j belongs to
  double mount_pos[kMaxDof][3];
  double mount_quat[kMaxDof][4];
  // flexible_beam_3D (flexible_beam.cpp:155-193): rest length, stiffness, torsion stiffness, world anchor pose
  double beam_rest, beam_k, beam_kt;
  double beam_pos[3], beam_quat[4];
  // Static reach of the robot shapes (serial chains).  The environment shapes are stored in ascending order of
  // "closeness" = |centre - chain base| - bounding radius, and robot shape r can only ever touch the first
  // robot_n_reach[r] of them: its centre stays within (sum of the link offsets below its joint) + |local position| of the
  // chain base, plus its bounding radius.  Pairs beyond that have a positive bounding-sphere gap in every configuration,
  // i.e. they are the pairs the cull of proxy_query_pair_3D::findMinimumDistance (proxy_query_model.cpp:384-389) drops.
  int32_t robot_n_reach[kMaxDof * 2];
  // bit o of env_finder_mask[k][chunk]: the reference has a finder for (robot shape of kind k, environment shape o)
  // (createProxFinderList, proxy_query_model.cpp:215-374: no finder for box-box, cylinder-cylinder, cylinder-box and
  // capped cylinder-cylinder)
  unsigned long long env_finder_mask[9][kMaxEnvShapes / 64];
  int32_t has_meshes;      // 1: convex vertex sets among the shapes (GJK pairs; wave-per-edge and quasi-static kernels)
  const double* mesh_verts;  // device pointer: the vertex pool [n][3] the mesh shapes index into (dims[0], dims[1])
  // prismatic_joint_3D groups (serial chains only): bit j = joint j translates along JointDev::axis (mAxis as given)
  uint32_t prismatic_mask;
  int32_t has_prismatic;   // 1: prismatic_mask != 0 (the prismatic instantiations of the one-wave and quasi-static kernels)
  // Carried clearance of the two-lanes steer kernels (serial 3D revolute chains without vertex-set or plane shapes:
  // has_clearance).  clear_arm[i] bounds the distance of every point of every robot shape on joint i or beyond from
  // joint i's axis: max over the shapes r with link >= i of (link offsets i .. link - 1) + |local position| + bounding
  // radius, the robot_n_reach sum started at joint i.  Turning joint i by d moves such a point by at most clear_arm[i] |d|,
  // so between two configurations no point of the robot moves more than sum_i clear_arm[i] |dq_i|.
  // The bound is a clearance over ALL pairs with a finder: robot shape r's cull also looks at the obstacles up to
  // kClearHorizon beyond its static reach (the first robot_n_clear[r] >= robot_n_reach[r] of the table; they never
  // reach the queues), and every pair further out is at least clear_static away in every configuration.
  int32_t has_clearance;
  double clear_arm[kMaxDof];
  int32_t robot_n_clear[kMaxDof * 2];
  double clear_static;
};
constexpr double kClearHorizon = 0.25;  // m; more than the 20 steps of a C2 edge can move the arm (20 x 6.3 mm)

struct PairDev {
  uint8_t routine;      // PairRoutine (proximity_device.h)
  uint8_t s1_is_robot;  // 1: (shape1, shape2) = (robot, env); 0: (env, robot)
  uint16_t robot;
  uint16_t env;
  uint16_t pad;
};
// What the record queries report about pair p of d_pairs (same order): its place in the reference's finder list and the
// caller's indices of the finder's (shape1, shape2).  rank = (robot shape) * n_env + (environment shape), both counted in
// the order the caller gave them: i-major / j-minor like createProxFinderList (proxy_query_model.cpp:215-374), so ranks
// order the finders as mProxFinders does (pairs without a finder leave gaps).
struct PairIdDev {
  uint32_t rank;
  uint32_t shape1, shape2;
};
constexpr int kMaxRecordPairs = 128 * 64;  // collision_records_kernel keeps one bit per pair in two 64-bit masks per lane

}  // namespace rkh

struct rkh_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  // Arenas of destroyed batch RRT planners, kept for the next one: creating, solving and destroying a planner over and
  // over on one scene then maps its memory once (at 512 problems x 100 000 vertices a planner holds 26 GB).  At most
  // kArenaCacheSlots; rkh_ctx_release_cached_memory, an allocation that runs out of memory and rkh_ctx_destroy free them.
  std::vector<rkh::DeviceArena> arena_cache;
  // the slices' partial lists of rkh_svp_nearest_async (svp_space.hip); grows with the largest request
  rkh::DeviceBuffer<void> svp_ws;
};

namespace rkh {
constexpr size_t kArenaCacheSlots = 4;
// An arena of at least `bytes`: the smallest cached one that fits, else a new one -- after the cached ones are freed, so
// that nothing is hoarded beside a larger live slab.  cached = false: a new one, the cache untouched (RKH_ARENA_CACHE=0).
rkh_status ctx_take_arena(rkh_ctx* ctx, size_t bytes, bool cached, DeviceArena* out);
// The arena of a planner whose streams are idle goes back to its context, or is freed if the context is gone (or full).
void ctx_give_arena(rkh_ctx* ctx, DeviceArena&& arena);
}  // namespace rkh

struct rkh_nn {
  rkh_ctx* ctx = nullptr;
  rkh::DeviceBuffer<double> pos;  // the rows
  rkh::NnStore st;                // ... as the launchers take them
  uint64_t n = 0;
  // scratch for host-pointer queries; each grows with the largest request (its size() is its capacity)
  rkh::DeviceBuffer<double> d_q;
  rkh::DeviceBuffer<uint32_t> d_idx;
  rkh::DeviceBuffer<double> d_dist;
  rkh::DeviceBuffer<uint32_t> d_count;
  rkh::DeviceBuffer<double> d_part_dist;
  rkh::DeviceBuffer<uint32_t> d_part_idx;
  rkh::DeviceBuffer<uint32_t> d_seed;  // NnArgs::seed
  double max_abs_coord = 0.0;  // over the rows appended from the host (checked against coord_bound)
  std::vector<uint8_t> removed;  // tombstones (host copy; the device row of a removed vertex holds +inf)
  uint64_t n_removed = 0;
  uint32_t part_blocks = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // one-shot: bracket the next sweep kernel
  rkh::DeviceBuffer<void> d_knn_ws;  // k-NN workspace
  double coord_bound = 0.0;  // rkh_nn_set_coord_bound: |coordinate| bound enabling the single-precision pre-filters
};

struct rkh_scene {
  rkh_ctx* ctx = nullptr;
  rkh::SceneDev host;
  rkh::DeviceBuffer<rkh::SceneDev> d_scene;
  rkh::DeviceBuffer<rkh::PairDev> d_pairs;   // [n_pairs], sorted by routine
  rkh::DeviceBuffer<rkh::PairIdDev> d_pair_ids;  // [n_pairs]: finder rank and the caller's shape indices
  rkh::DeviceBuffer<double> d_mesh_verts;    // vertex pool of the mesh shapes
  rkh::DeviceBuffer<int> d_err;
  rkh::DeviceBuffer<unsigned long long> d_clear_stats;  // [2] KernelGate::clear_stats of every steer launch on this scene
  int n_pairs = 0;
  int n_pairs_verdict = -1;  // the first entries of d_pairs: pairs whose shapes can touch at all (verdict kernels scan these)
  // the kinematics entries (kinematics_frames.hip): the chain as their kernels walk it, and where every frame of the
  // caller's numbering (rkh_kte_op::base_frame / end_frame, rkh_shape::anchor) sits in it -- a host table, indexed by
  // frame id; the refs of the frames a call asks for are uploaded with the call
  rkh::KinChain kin;
  rkh::DeviceBuffer<rkh::KinChain> d_kin;
  std::vector<rkh::KinFrameRef> frame_table;
};

namespace rkh {

struct DynDev {  // rkh_dyn_space on the device (passed by value)
  double dt, kp, kd, u_max, goal_tol;
  double lower[2 * kMaxDof], upper[2 * kMaxDof];
  double full_time;         // steps_per_edge * dt (the travel time of fraction 1)
  int n_steps;              // RK4 steps for this fraction
  int8_t inner[kMaxSteps];  // runge_kutta4_integrate_impl loop iterations of step k (normally 1), whole step budget
};

struct QsDev {  // manip_quasi_static_env on the device (passed by value)
  double min_interval, fraction;
  double lower[kMaxDof], upper[kMaxDof];
  double speed[kMaxDof];  // joint = point * speed (rate-limited joint space; 1.0 otherwise)
};
inline void qs_set_speed(QsDev& qs, const double* speed_limits, int n) {
  for (int i = 0; i < kMaxDof; ++i) qs.speed[i] = (speed_limits && i < n && speed_limits[i] != 0.0) ? speed_limits[i] : 1.0;
}

// ---- steer mapping ---------------------------------------------------------------------------------------------------
// The kernel form that steers the edges of a dynamic-space launch.
enum class SteerMapping : uint8_t {
  Auto,       // batch planner rounds: the launches of steer_plan (round_plan.h), each gated on the device by the round's
              // edge count
  Duo,        // two waves per edge (state_derivative_duo)
  Wave,       // one wave per edge (the form with the support-map query for scenes with vertex-set shapes)
  Wave16,     // four edges per wave, 16 lanes each (the form with the support-map query)
  Pair,       // two lanes per edge, 32 edges per wave (propagate_pair.hip; prismatic chains: propagate_pair_prismatic.hip)
  Planar,     // planar chains: one lane per edge (propagate_planar.hip)
  Prismatic,  // chains with prismatic joints: one wave per edge, no support-map query (propagate_prismatic.hip)
};
enum class SteerEntry : uint8_t { BatchPlanner, GraphPlanner, Propagate, CycleProbe };

// The knobs of the mapping, read when a planner is created or rkh_propagate / the cycle probe is called.
struct SteerRequest {
  bool lanes_set = false;
  int lanes = 0;                 // RKH_LANES_PER_EDGE
  uint32_t duo_threshold = 512;  // RKH_DUO_THRESHOLD (0: never)
  bool clearance = true;         // RKH_STEER_CLEARANCE (0: the two-lanes kernels test every step)
};
inline SteerRequest steer_request() {
  SteerRequest r;
  if (const char* e = getenv("RKH_LANES_PER_EDGE")) r.lanes_set = true, r.lanes = atoi(e);
  if (const char* e = getenv("RKH_DUO_THRESHOLD")) r.duo_threshold = uint32_t(std::max(0, atoi(e)));
  if (const char* e = getenv("RKH_STEER_CLEARANCE")) r.clearance = atoi(e) != 0;
  return r;
}

// the two-lanes-per-edge kernel handles one serial chain of at most 7 joints, revolute or prismatic (rkh::prismatic
// forms), with at most a tip-to-world beam (a scene with prismatic joints has none)
inline bool scene_fits_lane_kernel(const SceneDev& S) {
  if (S.has_meshes) return false;  // GJK pairs run in the wave-per-edge / quasi-static kernels
  return S.n_dof <= 7 && S.n_branches == 0 && (!S.beam_on || (S.beam_j1 == S.n_dof - 1 && S.beam_j2 < 0));
}

// The steer plan: the one place that chooses the form steering a launch of `edges` edges per problem for n_problems
// problems (b_max: the batch planner's final bound of candidates per problem and round).
//   Batch planner (rkh_planner_create*, dynamic space), at create: RKH_LANES_PER_EDGE 0 -> Auto, 2 -> Pair, 16 -> Wave16,
//     any other value (128 included) -> Wave.  Unset: Auto if n_dof <= 6 and scene_fits_lane_kernel, else Wave16 if
//     n_problems * 2 * b_max > 4096 (a round offers more waves than the chip has slots), else Wave.  Auto rounds run
//     the forms steer_plan lists for their edge count (round_plan.h; Auto never sees vertex-set shapes).
//   rkh_propagate, every call: unset -> Duo if edges <= 512, else Wave; 2 -> Pair, 16 -> Wave16, 128 -> Duo, any other
//     value -> Wave.
//   Graph planners (dynamic space), every launch: Duo if edges * n_problems <= RKH_DUO_THRESHOLD (read at create), else
//     Wave; RKH_LANES_PER_EDGE does not apply.
//   Then for these three: Pair or Auto on a scene the lane kernel does not fit -> Wave; Wave16 with 2 n_dof > 16 (a
//     16-lane group holds at most 16 components) -> Wave; planar chains -> Planar; prismatic joints: Pair stays Pair
//     and the batch planner's Auto stays Auto (their rkh::prismatic forms), everything else -> Prismatic (one wave per
//     edge; the graph planners always); Duo on a scene with vertex-set shapes -> Wave (its support-map form).
//   Cycle probe (rkh_diag_feval_cycles), every call: 2 -> Pair, 128 -> Duo, any other value -> Wave; no scene rule (the
//     probes refuse prismatic scenes themselves).
//   rkh_diag_proximity_counts: scenes of scene_fits_lane_kernel only.
inline SteerMapping steer_mapping(const SceneDev& S, SteerEntry entry, const SteerRequest& req, uint64_t edges,
                                  uint32_t n_problems, uint32_t b_max) {
  using M = SteerMapping;
  M m = M::Wave;
  switch (entry) {
    case SteerEntry::BatchPlanner:
      if (req.lanes_set) m = req.lanes == 0 ? M::Auto : (req.lanes == 2 ? M::Pair : (req.lanes == 16 ? M::Wave16 : M::Wave));
      else if (S.n_dof <= 6 && scene_fits_lane_kernel(S)) m = M::Auto;
      else m = (uint64_t(n_problems) * 2 * b_max > 4096) ? M::Wave16 : M::Wave;
      break;
    case SteerEntry::Propagate:
      if (!req.lanes_set) m = edges <= 512 ? M::Duo : M::Wave;
      else m = req.lanes == 2 ? M::Pair : (req.lanes == 16 ? M::Wave16 : (req.lanes == 128 ? M::Duo : M::Wave));
      break;
    case SteerEntry::GraphPlanner:
      m = (edges * n_problems <= req.duo_threshold) ? M::Duo : M::Wave;
      break;
    case SteerEntry::CycleProbe:
      return req.lanes == 2 ? M::Pair : (req.lanes == 128 ? M::Duo : M::Wave);
  }
  if ((m == M::Pair || m == M::Auto) && !scene_fits_lane_kernel(S)) m = M::Wave;
  if (m == M::Wave16 && 2 * S.n_dof > 16) m = M::Wave;
  if (S.planar) return M::Planar;
  if (S.has_prismatic) return (m == M::Pair || (m == M::Auto && entry == SteerEntry::BatchPlanner)) ? m : M::Prismatic;
  if (m == M::Duo && S.has_meshes) m = M::Wave;
  return m;
}

// rkh_steer_mapping_name(): the mapping this thread's last rkh_propagate / rkh_planner_create* (dynamic space) was given
void note_steer_mapping(SteerMapping m);

// ---- launchers ------------------------------------------------------------------------------------------------------
// They read the scene's kind (planar, vertex-set shapes, prismatic joints) from scene.host; the verdict kernels
// (propagate, edge walk) scan its first n_pairs_verdict pairs, min_distance and the f-eval probes all n_pairs.  Edge
// launches take grid_edges (+ grid_b of a second group) edges per problem: `io` by value (n_problems = 1, no second
// group) or two device tables of n_problems entries each.
// launch_propagate runs the form `m` it is given (steer_mapping chooses it; Pair needs d_lane_ws).
rkh_status launch_propagate(hipStream_t s, const rkh_scene& scene, SteerMapping m, const DynDev& dyn, const EdgeIO& io,
                            uint32_t grid_edges, uint32_t grid_b = 0, const EdgeIO* tab_a = nullptr,
                            const EdgeIO* tab_b = nullptr, uint32_t n_problems = 1, double* d_lane_ws = nullptr,
                            KernelGate gate = KernelGate());
rkh_status launch_state_derivative(hipStream_t s, const rkh_scene& scene, const double* d_x, const double* d_u, uint32_t B,
                                   double* d_pd, double* d_M, double* d_f, int* d_err);
rkh_status launch_min_distance(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, double* d_dist);
rkh_status launch_edge_check(hipStream_t s, const rkh_scene& scene, const QsDev& qs, const EdgeIO& io, uint32_t grid_edges,
                             uint32_t grid_b = 0, const EdgeIO* tab_a = nullptr, const EdgeIO* tab_b = nullptr,
                             uint32_t n_problems = 1);
// The record queries (3D scenes without vertex-set shapes; chains with prismatic joints included): one launch each over
// all n_pairs.  Outputs as in rkh.h, on the device.
struct RecordOut {
  uint32_t* n_found = nullptr;  // collision records only
  double* dist = nullptr;
  double* point1 = nullptr;
  double* point2 = nullptr;
  uint32_t* shape1 = nullptr;
  uint32_t* shape2 = nullptr;
};
rkh_status launch_min_distance_records(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, RecordOut out);
rkh_status launch_collision_records(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, uint32_t cap,
                                    RecordOut out);
// The same for every 3D scene: scenes with vertex-set shapes go to the support-map forms of the two kernels (records of
// such pairs: gjk_record), all others to the launchers above.
rkh_status launch_min_distance_records_meshes(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, RecordOut out);
rkh_status launch_collision_records_meshes(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, uint32_t cap,
                                           RecordOut out);
// Their depth forms (propagate_depth.hip): vertex-set pairs with crossing cores carry a penetration depth, and every record
// a normal (d_normal: three doubles per slot of out); and the pair-by-pair form of rkh_diag_gjk_depth_records
rkh_status launch_min_distance_records_depth(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, RecordOut out,
                                             double* d_normal);
rkh_status launch_collision_records_depth(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, uint32_t cap,
                                          RecordOut out, double* d_normal);
rkh_status launch_gjk_pair_depth(hipStream_t s, const rkh_shape* d_a, const rkh_shape* d_b, uint32_t n, const double* d_pool,
                                 double* d_dist, double* d_point1, double* d_point2, double* d_normal);
// Their planar twins (proximity_records_planar.hip; planar scenes, revolute and prismatic joints): points of two doubles
// ([B][2], [B][cap][2]), finder rank = pair index.
rkh_status launch_min_distance_records_2d(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, RecordOut out);
rkh_status launch_collision_records_2d(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, uint32_t cap,
                                       RecordOut out);
// The same four for chains with prismatic joints (propagate_prismatic.hip); the ones above hand these scenes on.
namespace prismatic {
rkh_status launch_propagate(hipStream_t s, const rkh_scene& scene, SteerMapping m, const DynDev& dyn, const EdgeIO& io,
                            uint32_t grid_edges, uint32_t grid_b, const EdgeIO* tab_a, const EdgeIO* tab_b,
                            uint32_t n_problems, double* d_lane_ws, KernelGate gate);
rkh_status launch_state_derivative(hipStream_t s, const rkh_scene& scene, const double* d_x, const double* d_u, uint32_t B,
                                   double* d_pd, double* d_M, double* d_f, int* d_err);
rkh_status launch_min_distance(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, double* d_dist);
rkh_status launch_edge_check(hipStream_t s, const rkh_scene& scene, const QsDev& qs, const EdgeIO& io, uint32_t grid_edges,
                             uint32_t grid_b, const EdgeIO* tab_a, const EdgeIO* tab_b, uint32_t n_problems);
// the two-lanes-per-edge forms (propagate_pair_prismatic.hip); the ones below hand these scenes on
rkh_status launch_propagate_pairs(hipStream_t s, const rkh_scene& scene, const DynDev& dyn, const EdgeIO& io,
                                  uint32_t grid_edges, uint32_t grid_b, const EdgeIO* tab_a, const EdgeIO* tab_b,
                                  uint32_t n_problems, double* d_ws, KernelGate gate);
rkh_status launch_propagate_pair_steps(hipStream_t s, const rkh_scene& scene, const DynDev& dyn, const EdgeIO* tab_a,
                                       const EdgeIO* tab_b, uint32_t n_problems, const uint32_t* d_edge_base,
                                       uint4* d_list0, uint4* d_list1, uint32_t list_cap, uint32_t* d_cnt, double* d_ws,
                                       uint32_t blocks, KernelGate gate, unsigned long long* d_steps_exec,
                                       uint32_t carry_min_edges);
uint32_t pair_kernel_waves_per_cu(int n_dof, bool has_prismatic);
rkh_status launch_pair_counts(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B,
                              unsigned long long* d_out, float* d_clear_out = nullptr);
}  // namespace prismatic
rkh_status launch_feval_cycles_duo(hipStream_t s, const rkh_scene& scene, const double* d_x, const double* d_u, uint32_t B,
                                   int iters, unsigned long long* d_out, double* d_sink);
rkh_status launch_feval_cycles(hipStream_t s, const rkh_scene& scene, const double* d_x, const double* d_u, uint32_t B,
                               int iters, unsigned long long* d_out, double* d_sink);
// two-lanes-per-edge kernel (propagate_pair.hip): 32 edges per wave, two waves per SIMD; scenes: scene_fits_lane_kernel
size_t propagate_pairs_workspace_bytes(int n_dof, uint32_t edges_a, uint32_t edges_b, uint32_t n_problems);
rkh_status launch_propagate_pairs(hipStream_t s, const rkh_scene& scene, const DynDev& dyn, const EdgeIO& io,
                                  uint32_t grid_edges, uint32_t grid_b, const EdgeIO* tab_a, const EdgeIO* tab_b,
                                  uint32_t n_problems, double* d_ws, KernelGate gate);
// the same mapping, one launch per RK4 step over the live edges of all problems (see propagate_pair_step_kernel)
size_t propagate_pair_step_workspace_bytes(int n_dof, uint32_t blocks);
rkh_status launch_propagate_pair_steps(hipStream_t s, const rkh_scene& scene, const DynDev& dyn, const EdgeIO* tab_a,
                                       const EdgeIO* tab_b, uint32_t n_problems, const uint32_t* d_edge_base,
                                       uint4* d_list0, uint4* d_list1, uint32_t list_cap, uint32_t* d_cnt, double* d_ws,
                                       uint32_t blocks, KernelGate gate, unsigned long long* d_steps_exec,
                                       uint32_t carry_min_edges);
uint32_t pair_kernel_waves_per_cu(int n_dof, bool has_prismatic);
uint32_t pair_kernel_edges_per_wave();
rkh_status launch_pair_counts(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B,
                              unsigned long long* d_out, float* d_clear_out = nullptr);
rkh_status launch_pair_cycles(hipStream_t s, const rkh_scene& scene, const double* d_x, const double* d_u, uint32_t B,
                              int iters, unsigned long long* d_out, double* d_sink);
// planar chains (propagate_planar.hip): one lane per edge
rkh_status launch_propagate_planar(hipStream_t s, const rkh_scene& scene, const DynDev& dyn, const EdgeIO& io,
                                   uint32_t grid_edges, uint32_t grid_b, const EdgeIO* tab_a, const EdgeIO* tab_b,
                                   uint32_t n_problems, KernelGate gate);
rkh_status launch_state_derivative_planar(hipStream_t s, const rkh_scene& scene, const double* d_x, const double* d_u,
                                          uint32_t B, double* d_pd, double* d_M, double* d_f, int* d_err);
// the same two compiled for planar chains with prismatic_joint_2D groups (propagate_planar_prismatic.hip); the ones above
// hand these scenes on
namespace planar_prismatic {
rkh_status launch_propagate_planar(hipStream_t s, const rkh_scene& scene, const DynDev& dyn, const EdgeIO& io,
                                   uint32_t grid_edges, uint32_t grid_b, const EdgeIO* tab_a, const EdgeIO* tab_b,
                                   uint32_t n_problems, KernelGate gate);
rkh_status launch_state_derivative_planar(hipStream_t s, const rkh_scene& scene, const double* d_x, const double* d_u,
                                          uint32_t B, double* d_pd, double* d_M, double* d_f, int* d_err);
// and the position-level forms (propagate_planar_qs_prismatic.hip); launch_edge_check / launch_min_distance hand on
rkh_status launch_edge_check(hipStream_t s, const rkh_scene& scene, const QsDev& qs, const EdgeIO& io, uint32_t grid_edges,
                             uint32_t grid_b, const EdgeIO* tab_a, const EdgeIO* tab_b, uint32_t n_problems);
rkh_status launch_min_distance(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, double* d_dist);
}  // namespace planar_prismatic
rkh_status build_dyn_dev(const rkh_dyn_space& sp, double fraction, DynDev* out);

// ---- the staged walk of the SVP space (svp_space.hip) ----------------------------------------------------------------------
struct SvpDev;  // svp_device.h
// everything the rkh_svp_* entries check about a space, and its device form.  scene_n < 0: no scene to agree with
rkh_status svp_space_dev(const char* who, const rkh_svp_space* sp, int scene_n, SvpDev* out);
struct SvpWalk {  // the walk's workspace: device pointers into the caller's memory, by value
  const double* a;         // [B][2n]
  const double* b;
  const double* fraction;  // [B] or null = 1.0
  double* T;               // [B]
  double* peak;            // [B][n]
  double* dt;              // [B] T fraction
  uint32_t* K;             // [B] points of the edge's loop
  uint32_t* k_done;        // [B] points that passed
  double* d_next;          // [B] travel time of point k_done
  double* last;            // [B][2n] last point that passed
  double* out;             // [B][2n]
  uint32_t* n_checked;     // [B]
  uint8_t* reached;        // [B]
  uint32_t* list[2];       // [B] live edges of this pass / the next
  uint32_t* counters;      // [0], [1]: entries of list[0], list[1]; [2]: an edge with more than kSvpMaxPoints points
  double* pts;             // [live][kSvpPass][2n] space coordinates
  double* pts_model;       // the same in model units
  uint8_t* inb;            // [live][kSvpPass]
  double* dist;            // [live][kSvpPass]
  uint32_t B;
};
// Bytes of a workspace for at most B edges of n_dof joints (256-byte aligned ranges, no guard tail); with base, *w points
// into it (fraction null unless with_fraction; w->B = B).
size_t svp_walk_layout(int n_dof, uint32_t B, bool with_fraction, void* base, SvpWalk* w);
// The walk of rkh_svp_edge_check over the rows w.a, w.b, w.fraction of the first w.B edges, already on the device: the solve
// launch and the passes on the scene's context's stream, one read-back of the live count per pass; the stream is idle on
// return.  Results in w.out, w.T, w.n_checked, w.reached.  passes (may be null): passes run.  RKH_ERR_CAPACITY: an edge with
// more than 1 048 576 points to test.
rkh_status launch_svp_walk(const char* who, const rkh_scene& scene, const SvpDev& sp, const SvpWalk& w, uint32_t* passes);
// The same walk with a direction per row (svp_walk_dir.hip, the rules are svp_walk_rules.h's): d_back [w.B] on the device,
// d_back[e] != 0 walks the profile a_e -> b_e backward from b_e (rkh_svp_edge_check_back), 0 forward as launch_svp_walk does,
// bit for bit; d_back null: every row forward.  Same workspace, results, passes and errors.
rkh_status launch_svp_walk_dir(const char* who, const rkh_scene& scene, const SvpDev& sp, const SvpWalk& w, const uint8_t* d_back,
                               uint32_t* passes);

// ---- the search of path shortcutting (path_shortcut.hip; the index rules are path_shortcut.h's) ----------------------------
// One launch of the search.  All pointers are device pointers.  ok(i, j) = (acc[pair] & ok_mask) != 0 || w < min_interval:
// the accept bytes of an EDGE_STEER_BOTH walk with ok_mask = 2 and the space's min_interval (rkh_shortcut_paths), or verdict
// bytes with ok_mask = 0xFF and min_interval = 0 (rkh_diag_shortcut_dp; rkh_svp_shortcut_paths with the walk's `reached`).
struct ShortcutDpArgs {
  const uint32_t* path_ptr;  // [B + 1] rows of the point table
  const uint32_t* pair_ptr;  // [B + 1] pairs of the pair arrays
  uint32_t B, max_span;
  const uint8_t* acc;        // per pair
  const double* w;           // per pair
  uint32_t ok_mask;
  double min_interval;
  uint32_t* keep;            // [path_ptr[B]], path b at path_ptr[b]
  uint32_t* n_keep;          // [B]
  double* cost_out;          // [B]
  uint32_t* n_blocked;       // [B] or null
};
// The pair offsets of B paths, and everything the shortcut entries check about path_ptr before anything is launched.
rkh_status shortcut_layout(const char* who, const uint32_t* path_ptr, uint32_t B, uint32_t max_span,
                           std::vector<uint32_t>* pair_ptr);
rkh_status launch_shortcut_dp(hipStream_t s, const ShortcutDpArgs& a);
}  // namespace rkh
