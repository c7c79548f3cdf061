/* rkh.h -- C-ABI of the MI355X-native planning hot path (librkh.so).
 *
 * ReaK itself has no FFI for this path: the hot path sits behind C++ template concepts
 * (SURVEY.md 8(b)).  These entry points are what a ReaK-side adaptor binds (INTEGRATION.md shows
 * the C++ classes modelling ReaK's NNFinder / Steerable C_free / planner concepts on top of them).
 * Each function names the reference interface it replaces (paths relative to
 * /root/reference/src/ReaK/).
 *
 * Conventions: every function returns an rkh_status (0 = ok, negative = error); no exception
 * crosses the boundary; the caller owns every host buffer; one host thread per rkh_ctx; calls are
 * synchronous (they return after the device work finished) unless named *_async.
 * Pointers named d_* are device (HBM) pointers, all others are host pointers.
 * Profiling and diagnostic entry points (kernel timing for bench.py, per-phase cycle counts) are NOT part of this
 * boundary: they live in rkh_diag.h.  The C++ classes that model ReaK's concepts over these functions are in
 * rkh_adaptors.hpp.
 */
#ifndef RKH_H
#define RKH_H

#include <stddef.h>
#include <stdint.h>

#include "rkh_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum rkh_status {
  RKH_OK = 0,
  RKH_ERR_BAD_ARG = -1,     /* std::range_error in the reference (kte_nl_system.hpp:181-188) */
  RKH_ERR_OOM = -2,
  RKH_ERR_SINGULAR = -3,    /* singularity_error (mat_cholesky.hpp:80-82, manip_dynamics_model.cpp:206-214) */
  RKH_ERR_DEVICE = -4,      /* HIP runtime error; rkh_last_error() has the text */
  RKH_ERR_UNSUPPORTED = -5, /* KTE program / shape not covered by the HIP kernels */
  RKH_ERR_CAPACITY = -6
} rkh_status;

typedef struct rkh_ctx rkh_ctx;         /* one device + stream */
typedef struct rkh_nn rkh_nn;           /* device-resident vertex set for NN queries */
typedef struct rkh_scene rkh_scene;     /* KTE chain + proxy environment on the device */
typedef struct rkh_planner rkh_planner; /* batched RRT driver over a scene */
typedef struct rkh_rrtstar rkh_rrtstar; /* batched RRT* driver over a scene */
typedef struct rkh_prm rkh_prm;         /* batched PRM driver over a scene */
typedef struct rkh_birrt rkh_birrt;     /* batched bidirectional-RRT driver over a scene */

const char* rkh_last_error(void);
const char* rkh_version(void);
/* ABI number of this header: bumped whenever a public POD changes size or meaning (2: rkh_rrtstar_stats gained
 * pruned / skipped, rkh_qs_space gained speed_limits; 3: this handshake).  A binding checks once after loading:
 *   rkh_abi_check(RKH_ABI_VERSION, sizeof(rkh_dyn_space), sizeof(rkh_qs_space), ...) == RKH_OK
 * (RKH_ABI_CHECK() below spells the call out). */
#define RKH_ABI_VERSION 3u
uint32_t rkh_abi_version(void);
rkh_status rkh_abi_check(uint32_t abi_version, size_t sizeof_dyn_space, size_t sizeof_qs_space, size_t sizeof_rrt_params,
                         size_t sizeof_prm_params, size_t sizeof_planner_stats, size_t sizeof_rrtstar_stats,
                         size_t sizeof_prm_stats, size_t sizeof_birrt_stats, size_t sizeof_shape, size_t sizeof_kte_op);
#define RKH_ABI_CHECK()                                                                                                  \
  rkh_abi_check(RKH_ABI_VERSION, sizeof(rkh_dyn_space), sizeof(rkh_qs_space), sizeof(rkh_rrt_params), sizeof(rkh_prm_params), \
                sizeof(rkh_planner_stats), sizeof(rkh_rrtstar_stats), sizeof(rkh_prm_stats), sizeof(rkh_birrt_stats),   \
                sizeof(rkh_shape), sizeof(rkh_kte_op))

/* ---- context ------------------------------------------------------------------------------ */
rkh_status rkh_ctx_create(int device, rkh_ctx** out);
rkh_status rkh_ctx_destroy(rkh_ctx* ctx);
rkh_status rkh_ctx_synchronize(rkh_ctx* ctx);
/* hipStream_t of the context as void* (bench.py brackets launches with HIP events on it). */
void* rkh_ctx_stream(rkh_ctx* ctx);
/* A context keeps the device memory of destroyed batch RRT planners for the next rkh_planner_create* on it (creating,
 * solving and destroying planners over and over on one scene then maps memory once; RKH_ARENA_CACHE=0 in the environment
 * at create turns that off).  This frees what is kept; so does rkh_ctx_destroy, and any allocation of the library that
 * runs out of device memory before it gives up. */
rkh_status rkh_ctx_release_cached_memory(rkh_ctx* ctx);

/* ---- nearest neighbours -------------------------------------------------------------------
 * Replaces linear_neighbor_search<Graph> (ctrl/path_planning/topological_search.hpp:529-690):
 *   rkh_nn_query1  = min_dist_linear_search 1-NN            (topological_search.hpp:95-118)
 *   rkh_nn_queryk  = min_dist_linear_search k-NN + radius   (topological_search.hpp:244-274)
 * and any_knn_synchro::added_vertex (ctrl/path_planning/any_knn_synchro.hpp:69-76) = rkh_nn_append.
 * Distance is euclidean_distance_metric (ctrl/topologies/vect_distance_metrics.hpp:113-150),
 * evaluated in the reference's fp64 operation order; results are bit-identical to the CPU search,
 * including "first minimum wins" on ties.  Vertex ids are insertion indices. */
rkh_status rkh_nn_create(rkh_ctx* ctx, int dims, uint64_t capacity, rkh_nn** out);
rkh_status rkh_nn_destroy(rkh_nn* nn);
rkh_status rkh_nn_clear(rkh_nn* nn);
uint64_t rkh_nn_size(const rkh_nn* nn);
/* any_knn_synchro::removed_vertex (ctrl/path_planning/any_knn_synchro.hpp:77-84; called from
 * planning_visitor_base::vertex_to_be_removed, planning_visitors.hpp:213-216): vertex `index` is never returned by a
 * query again.  The store stays append-only -- indices of the other vertices do not change and rkh_nn_size still counts
 * the row -- and the row itself is overwritten with +inf coordinates: every sweep then computes an infinite distance for
 * it, which no comparison of the reference accepts (d < radius, d < best), at no extra bytes per sweep (a separate n/8
 * mask would add a read per row).  Removing a vertex twice is allowed.  rkh_nn_live_size counts the vertices left. */
rkh_status rkh_nn_remove(rkh_nn* nn, uint64_t index);
uint64_t rkh_nn_live_size(const rkh_nn* nn);
/* pts: n points, row-major [n][dims] */
rkh_status rkh_nn_append(rkh_nn* nn, const double* pts, uint64_t n);
/* q: [B][dims]; idx[B] (0xFFFFFFFF if the set is empty), dist[B] */
rkh_status rkh_nn_query1(rkh_nn* nn, const double* q, uint32_t B, uint32_t* idx, double* dist);
/* k-NN with radius: idx/dist are [B][k], nearest first, padded with 0xFFFFFFFF / +inf; count[B].
 * Among exactly equal distances the reference's order is std::heap-defined; this returns
 * ascending (distance, index).  k in [1, 1024] (else RKH_ERR_BAD_ARG).  RKH_ERR_CAPACITY only for coincident
 * vertices: more than 1024 vertices, besides the k nearest, at exactly the k-th nearest distance. */
rkh_status rkh_nn_queryk(rkh_nn* nn, const double* q, uint32_t B, uint32_t k, double radius, uint32_t* idx,
                         double* dist, uint32_t* count);
/* Device-pointer variants for callers that keep queries / results in HBM (bench, planner).
 * d_q: [B][dims] row-major in HBM; d_idx[B]; d_dist[B]. Asynchronous on the context stream. */
rkh_status rkh_nn_query1_async(rkh_nn* nn, const double* d_q, uint32_t B, uint32_t* d_idx, double* d_dist);
rkh_status rkh_nn_queryk_async(rkh_nn* nn, const double* d_q, uint32_t B, uint32_t k, double radius,
                               uint32_t* d_idx, double* d_dist, uint32_t* d_count);
/* Fill the set with n uniform points of the unit hypercube directly on the device (synthetic
 * trees for the sweep microbenchmark); deterministic in seed. */
/* Promise that every |coordinate| of the stored vertices and of all later queries is <= bound (for a hyperbox_topology:
 * the largest |corner coordinate|, ctrl/topologies/hyperbox_topology.hpp:97-103).  Sweeps of 5 or more queries then run a
 * single-precision pre-filter (the fp32 matrix instructions for 5..32 queries over at least 8192 vertices and for more
 * than 32 queries, as a split-bf16 estimate from 7 dimensions on) in front of the exact fp64 test; results stay
 * bit-identical for every bound in [1e-6, 1e6], whether the vertices fill it or lie far inside it.  bound = 0 (default)
 * switches the pre-filters off, and so does a bound outside [1e-6, 1e6].  (A planner derives its bound from its
 * hyperbox; with 1e-3 <= bound <= 32 and at most 12 dimensions its rounds search over a half-precision mirror of the
 * tree instead, kept in units of the power of two that brings the bound into [16, 32): reak_amd/csrc/nn_mirror.h.)
 * The promise is checked where the library holds the data on the host: rkh_nn_append and rkh_nn_query1 return
 * RKH_ERR_BAD_ARG for a coordinate beyond the bound, and so does this call if rows already stored exceed it.  Queries
 * handed over in HBM (rkh_nn_query1_async) are the caller's responsibility: a query outside the bound may return a
 * wrong neighbour. */
rkh_status rkh_nn_set_coord_bound(rkh_nn* nn, double bound);
rkh_status rkh_nn_fill_uniform(rkh_nn* nn, uint64_t n, uint64_t seed);

/* ---- scene: KTE chain + proximity environment ----------------------------------------------
 * rkh_scene_create flattens what the reference holds as kte_map_chain + mass_matrix_calc
 * (ctrl/mbd_kte/kte_map_chain.hpp, mass_matrix_calculator.cpp) and one proxy_query_pair_3D
 * (robot model = shapes with anchor >= 0, environment model = anchor -1;
 * geometry/proximity/proxy_query_model.cpp:215-402).  The HIP kernels cover serial chains of
 * {driving_actuator_gen, inertia_gen, revolute_joint_3D, rigid_link_3D, inertia_3D} groups
 * (the pattern of examples/robot_airship/old/CRS_A465_models.cpp:751-785); anything else returns
 * RKH_ERR_UNSUPPORTED.  A prismatic_joint_3D may take the place of the revolute joint in any group of a
 * SERIAL chain (the CRS A465's track, :300-346), also after the optional mount link; such a scene runs on the
 * one-wave-per-edge and quasi-static kernels.  Refused with a prismatic joint: branching chains, a
 * flexible_beam_3D, mesh shapes, and a plane paired with a shape the joint carries (its travel is unbounded).
 * PLANAR chains (2D shapes only) are sequences of {revolute_joint_2D | prismatic_joint_2D, rigid_link_2D} groups, or with
 * dynamics {driving_actuator_gen, inertia_gen, revolute_joint_2D | prismatic_joint_2D, rigid_link_2D, inertia_2D}, of 1,
 * 2, 3, 4, 6 or 7 joints.  A prismatic_joint_2D (ctrl/mbd_kte/prismatic_joint.cpp:33-123: doMotion :33-80, doForce
 * :82-102, applyReactionForce :120-123; the planar CRS A465 analog of examples/robot_airship/old/
 * CRS_A465_2D_analog.cpp:139-360 rides one) may stand in any group, in any mix with revolute joints; its axis is used as
 * given, and robot shapes anchor on any joint's end frame.  Such a scene runs on the rkh::planar_prismatic forms of the
 * planar kernels behind every entry point that serves planar scenes.  Refused (RKH_ERR_UNSUPPORTED): a
 * prismatic_joint_3D inside a planar chain, a prismatic_joint_2D inside a 3D chain, and the record queries on any
 * planar scene. */
rkh_status rkh_scene_create(rkh_ctx* ctx, const rkh_kte_op* prog, int n_ops, const rkh_chain_base* base,
                            const rkh_shape* shapes, int n_shapes, rkh_scene** out);
/* The same with convex vertex sets among the shapes (RKH_SHAPE_MESH): mesh_vertices = the pool [n_mesh_vertices][3] the
 * mesh shapes index into.  Pairs with a mesh are evaluated by GJK over support maps (sphere = point + radius, capped
 * cylinder = segment + radius, box, vertex set); the reference's closed forms stay in place for all other pairs.
 * BASELINE config C4 ("200 mesh obstacles, batched GJK").  Meshes pair with spheres, capped cylinders, boxes and
 * meshes; they have no finder against planes and cylinders. */
rkh_status rkh_scene_create_with_meshes(rkh_ctx* ctx, const rkh_kte_op* prog, int n_ops, const rkh_chain_base* base,
                                        const rkh_shape* shapes, int n_shapes, const double* mesh_vertices,
                                        uint32_t n_mesh_vertices, rkh_scene** out);
rkh_status rkh_scene_destroy(rkh_scene* scene);
int rkh_scene_num_dof(const rkh_scene* scene);
int rkh_scene_num_pairs(const rkh_scene* scene);

/* kte_nl_system::get_state_derivative (ctrl/ctrl_sys/kte_nl_system.hpp:239-290) for B (x,u) pairs:
 * x [B][2n] interleaved (q,qd), u [B][n]; pd [B][2n]; optional M [B][n][n], f [B][n].
 * Returns RKH_ERR_SINGULAR if any mass matrix pivot < 1e-8 (singularity_error). */
rkh_status rkh_state_derivative(rkh_scene* scene, const double* x, const double* u, uint32_t B, double* pd,
                                double* M, double* f);
/* manip_dk_proxy_env_impl::is_free's distance (ctrl/topologies/manip_free_workspace.hpp:79-99):
 * minimum proxy-pair distance for B states (apply_to_model + findMinimumDistance). */
rkh_status rkh_min_distance(rkh_scene* scene, const double* x, uint32_t B, double* dist);
/* The records behind that distance: what proxy_query_pair_3D::findMinimumDistance()->getLastResult() and
 * gatherCollisionPoints hold (geometry/proximity/proxy_query_model.cpp:376-400 and :402-421; proximity_record_3D.hpp:47-56).
 *   point1 / point2   mPoint1 on the finder's shape1, mPoint2 on its shape2, world frame.
 *   shape1 / shape2   the two shapes as indices into the shapes array given to rkh_scene_create, in the FINDER's order
 *                     (createProxFinderList, :225-370: the plane first, else the sphere, else the capped cylinder; equal
 *                     kinds: the robot's shape), not robot-then-environment.
 *   Finder order      i-major over the robot shapes, j-minor over the environment shapes, each in the caller's order.
 * rkh_min_distance_records, for B states: the winning finder's record.  The loop of :384-397 takes a new minimum only on
 * a strictly smaller distance and its bounding-sphere skip cannot drop a finder that would win (the shapes are bounded;
 * rkh_scene_create enforces the plane rule), so the winner is the first finder in finder order among those at the
 * minimum distance.  dist[b] is bit-identical to rkh_min_distance's.  A scene without finders: dist = +inf, shape ids
 * 0xFFFFFFFF, points 0.
 * rkh_collision_records, for B states: every finder whose bounding spheres are not apart (:409-411, "> 0.0" skips) and
 * whose distance is < 0.0 (:414), in finder order.  n_found[b] counts them all and may exceed cap; the first cap of
 * them are written to row b of the [B][cap] arrays; the slots behind them read dist +inf, shape ids 0xFFFFFFFF, points 0.
 * No pointer may be NULL (RKH_ERR_BAD_ARG); B == 0 is RKH_OK.  RKH_ERR_UNSUPPORTED, with an error text: scenes with
 * RKH_SHAPE_MESH shapes (these two entries know the closed forms only; the _meshes entries below serve such scenes)
 * and planar (2D) scenes (proxy_query_pair_2D's records come from the _2d entries below). */
rkh_status rkh_min_distance_records(rkh_scene* scene, const double* x, uint32_t B,
                                    double* dist,      /* [B]    */
                                    double* point1,    /* [B][3] */
                                    double* point2,    /* [B][3] */
                                    uint32_t* shape1,  /* [B]    */
                                    uint32_t* shape2); /* [B]    */
rkh_status rkh_collision_records(rkh_scene* scene, const double* x, uint32_t B, uint32_t cap,
                                 uint32_t* n_found,                             /* [B] */
                                 double* dist, double* point1, double* point2,  /* [B][cap], [B][cap][3], [B][cap][3] */
                                 uint32_t* shape1, uint32_t* shape2);           /* [B][cap] */
/* The same two queries for EVERY non-planar scene, scenes with RKH_SHAPE_MESH shapes included: arguments, array shapes,
 * finder order, tie rule, n_found / cap, unused slots, NULL and B == 0 rules as above; dist[b] of the first is
 * bit-identical to rkh_min_distance's.  A scene without mesh shapes runs the kernels of the two entries above and the
 * results are theirs bit for bit.  New names because the entries above are defined to refuse mesh scenes.
 * A finder with a mesh in it is not the reference's (it has no mesh shape) but the build's support-map (GJK) query, which
 * comes last in the cascade of kinds: mesh against sphere / capped cylinder / box / mesh, shape1 = model 1's (the
 * robot's) shape, shape2 = the environment's.  Its record holds the witnesses of the search.  Each shape is a convex
 * core swept by a radius r (sphere: centre; capped cylinder: axis segment; box and mesh: themselves, r = 0):
 *   cores apart     point1 = pA + r1 n, point2 = pB - r2 n, where (pA, pB) is a closest pair of points of the two cores
 *                   and n the unit vector from pA towards pB; dist = |pB - pA| - r1 - r2, which is negative when the
 *                   swept shapes overlap while their cores do not.  Where the closest pair is not unique (parallel
 *                   faces or edges) the points are one such pair, not a particular one.
 *   cores crossing  dist = -(r1 + r2) - 1e-9, as rkh_min_distance reports it, and point1 = point2 (to rounding) = one
 *                   point common to both cores.  The query computes NO penetration depth and the record invents none:
 *                   neither dist nor the points measure how deep the cores cross.
 * RKH_ERR_UNSUPPORTED, with an error text: planar (2D) scenes (the _2d entries below). */
rkh_status rkh_min_distance_records_meshes(rkh_scene* scene, const double* x, uint32_t B,
                                           double* dist,      /* [B]    */
                                           double* point1,    /* [B][3] */
                                           double* point2,    /* [B][3] */
                                           uint32_t* shape1,  /* [B]    */
                                           uint32_t* shape2); /* [B]    */
rkh_status rkh_collision_records_meshes(rkh_scene* scene, const double* x, uint32_t B, uint32_t cap,
                                        uint32_t* n_found,                             /* [B] */
                                        double* dist, double* point1, double* point2,  /* [B][cap], [B][cap][3], [B][cap][3] */
                                        uint32_t* shape1, uint32_t* shape2);           /* [B][cap] */
/* The _meshes entries with a PENETRATION DEPTH and a CONTACT NORMAL (the _meshes entries themselves hold what they held).
 * Finder order, caps, n_found, unused slots (normal: zeros), NULL and B == 0 rules, the refusal of planar scenes (the _2d
 * entries below) and a scene without finders are those of the _meshes entries; normal is one more array of the points'
 * shape.  What differs is the record of a support-map finder whose cores cross: the search goes on with the Expanding
 * Polytope Algorithm on the Minkowski difference of the two cores (reak_amd/csrc/epa_device.h), and
 *   cores crossing  depth = the least translation that brings the cores to touching, n = its unit direction, from shape1
 *                   towards shape2 (moving shape2 by depth n separates the cores; ties between directions: one of them);
 *                   dist = -(r1 + r2 + depth) - 1e-9 (the collision mark of rkh_min_distance is kept, so the verdict and
 *                   the set of colliding finders are the _meshes entries'); point1 = a point of shape1's surface where
 *                   that translation first makes contact, point2 = point1 - (depth + r1 + r2) n on shape2's.  Cores that
 *                   touch exactly have depth 0; cores that lie in one plane or line have depth 0 and n = its normal.
 *   cores apart     dist, point1, point2 as in the _meshes entries, bit for bit; normal = n.
 *   closed forms    dist, point1, point2 as in the plain entries; normal = (point2 - point1) / dist componentwise, zeros
 *                   where dist is 0 or not finite.  No more is claimed for it.
 * rkh_min_distance_records_depth takes the minimum over THESE distances, with the same tie rule (first in finder order
 * among equals): among crossing support-map finders the deepest wins, where the _meshes entry reports the first of those
 * at -(r1 + r2) - 1e-9.  dist[b] is therefore bit-identical to rkh_min_distance's only when the winner's cores are apart
 * or the winner is a closed form.  rkh_collision_records_depth lists exactly the finders rkh_collision_records_meshes
 * lists, with the same n_found.  A scene without mesh shapes: dist, the points and the ids are the plain entries' byte
 * for byte. */
rkh_status rkh_min_distance_records_depth(rkh_scene* scene, const double* x, uint32_t B,
                                          double* dist,      /* [B]    */
                                          double* point1,    /* [B][3] */
                                          double* point2,    /* [B][3] */
                                          double* normal,    /* [B][3] */
                                          uint32_t* shape1,  /* [B]    */
                                          uint32_t* shape2); /* [B]    */
rkh_status rkh_collision_records_depth(rkh_scene* scene, const double* x, uint32_t B, uint32_t cap,
                                       uint32_t* n_found,                             /* [B] */
                                       double* dist, double* point1, double* point2,  /* [B][cap], [B][cap][3], [B][cap][3] */
                                       double* normal,                                /* [B][cap][3] */
                                       uint32_t* shape1, uint32_t* shape2);           /* [B][cap] */
/* The same for planar (2D) scenes: what proxy_query_pair_2D::findMinimumDistance()->getLastResult() and
 * gatherCollisionPoints hold (proxy_query_model.cpp:163-187 and :189-208; proximity_record_2D.hpp:47-58: points are
 * vect<double,2>).  x as for rkh_min_distance; shape1 / shape2 and the finder order as above, with createProxFinderList's
 * 2D cascade (:75-161): the circle first, else the capped rectangle; rectangle / rectangle: the robot's shape.
 * rkh_min_distance_records_2d: the record of mProxFinders[min_i] after the loop of :163-187.  Unlike in 3D, the cull
 * against the running minimum can drop a finder that would win (capped_rectangle::getBoundingRadius is shorter than the
 * caps reach), so the winner is NOT the lowest distance but what the sequence leaves: finder 0 is always computed,
 * finder i >= 1 is skipped when |c2 - c1| - r1 - r2 > min_dist and otherwise takes over on a strictly smaller distance.
 * dist[b] is bit-identical to rkh_min_distance's.  A scene without finders: dist = +inf, shape ids 0xFFFFFFFF, points 0.
 * rkh_collision_records_2d: every finder whose bounding circles are not apart ("> 0.0" skips) and whose distance is
 * < 0.0, in finder order; n_found, cap and the unused slots as for rkh_collision_records.
 * No pointer may be NULL (RKH_ERR_BAD_ARG); B == 0 is RKH_OK.  RKH_ERR_UNSUPPORTED, with an error text: scenes that are
 * not planar (their records come from rkh_min_distance_records / rkh_collision_records). */
rkh_status rkh_min_distance_records_2d(rkh_scene* scene, const double* x, uint32_t B,
                                       double* dist,      /* [B]    */
                                       double* point1,    /* [B][2] */
                                       double* point2,    /* [B][2] */
                                       uint32_t* shape1,  /* [B]    */
                                       uint32_t* shape2); /* [B]    */
rkh_status rkh_collision_records_2d(rkh_scene* scene, const double* x, uint32_t B, uint32_t cap,
                                    uint32_t* n_found,                             /* [B] */
                                    double* dist, double* point1, double* point2,  /* [B][cap], [B][cap][2], [B][cap][2] */
                                    uint32_t* shape1, uint32_t* shape2);           /* [B][cap] */
/* steer_position_toward of the steerable dynamic free space (rkh_dyn_space) for B (a,b) pairs:
 * x_out [B][2n] last collision-free state, steps_free[B] accepted RK4 steps, record (optional)
 * [B][steps_per_edge+1][2n] the steer record. RK4 = runge_kutta4_integrate_impl
 * (ctrl/sys_integrators/runge_kutta4_integrator_sys.hpp:53-97). */
rkh_status rkh_propagate(rkh_scene* scene, const rkh_dyn_space* space, const double* a, const double* b,
                         uint32_t B, double fraction, double* x_out, uint32_t* steps_free, double* record);
/* Quasi-static edge walk interp_topo_move_position_toward_pred
 * (ctrl/interpolation/interpolated_topologies.hpp:137-163) over joint positions, for B (a,b) pairs:
 * lower/upper [n] joint box, out [B][n] last free point, n_checked[B] is_free calls made. */
rkh_status rkh_edge_check(rkh_scene* scene, const double* lower, const double* upper, double min_interval,
                          const double* a, const double* b, uint32_t B, double fraction, double* out,
                          uint32_t* n_checked);

/* ---- planner: rrt_planner::solve_planning_query (LINEAR_SEARCH_KNN, UNIDIRECTIONAL) ----------
 * (ctrl/path_planning/rrt_path_planner.tpp:66-145 -> generate_rrt, ctrl/graph_alg/rr_tree.hpp:179-199)
 * over the steerable dynamic space.  Expansion is speculative in batches but commits vertices in
 * exactly the order of the sequential algorithm, so vertex ids, parents and sample consumption
 * equal the CPU planner's on the same seed. */
typedef struct rkh_planner_stats {
  uint64_t num_vertices;   /* num_vertices(g), root included */
  uint64_t iterations;     /* samples consumed = generate_rrt loop iterations */
  uint64_t edges_checked;  /* steer_towards_position + goal probes committed */
  uint64_t edges_speculated; /* propagate kernel edges launched (incl. discarded speculation) */
  uint64_t rounds;         /* speculative batches */
  uint64_t num_solutions;
  double best_cost;
  uint32_t done;
} rkh_planner_stats;

rkh_status rkh_planner_create(rkh_scene* scene, const rkh_dyn_space* space, const rkh_rrt_params* prm,
                              rkh_planner** out);
/* A batch of n_problems independent planning problems (seeds / start-goal queries) on one scene.  They advance in
 * lock-step rounds and share every kernel launch, which is what fills the chip (the reference's evaluation mode is
 * Monte-Carlo over independent runs, ctrl/path_planning/planner_exec_engines.hpp:139-206).  Each problem is
 * still, bit for bit, the sequential planner on its own seed.  Every stats pointer below is an array of
 * rkh_planner_num_problems() entries. */
rkh_status rkh_planner_create_batch(rkh_scene* scene, const rkh_dyn_space* space, const rkh_rrt_params* prms,
                                    uint32_t n_problems, rkh_planner** out);
uint32_t rkh_planner_num_problems(const rkh_planner* p);
/* The same planner over the quasi-static free space manip_quasi_static_env (points = joint positions, steering =
 * move_position_toward with the min_interval collision walk, goal probe = interp_topo_get_distance_pred). */
rkh_status rkh_planner_create_qs_batch(rkh_scene* scene, const rkh_qs_space* space, const rkh_rrt_params* prms,
                                       uint32_t n_problems, rkh_planner** out);
rkh_status rkh_planner_destroy(rkh_planner* p);
/* Enqueue `rounds` speculative batches on the planner's stream (no host sync). */
rkh_status rkh_planner_enqueue(rkh_planner* p, uint32_t rounds);
/* Wait for the enqueued batches and refresh stats; *done is set once keep_going() turned false. */
rkh_status rkh_planner_sync(rkh_planner* p, rkh_planner_stats* stats);
/* Run to completion (keep_going() false): enqueue + sync until done. */
rkh_status rkh_planner_solve(rkh_planner* p, rkh_planner_stats* stats);
/* Copy the motion graph of one problem out: pos [num_vertices][2n], parent[num_vertices] (root 0xFFFFFFFF),
 * nn_seq[iterations], accept[iterations], goal_dist[num_vertices-1].  Any pointer may be NULL. */
rkh_status rkh_planner_get_tree(rkh_planner* p, uint32_t problem, double* pos, uint32_t* parent, uint32_t* nn_seq,
                                uint8_t* accept, double* goal_dist);
void* rkh_planner_stream(rkh_planner* p);

/* ---- RRT*: rrtstar_planner::solve_planning_query (LINEAR_SEARCH_KNN, UNIDIRECTIONAL, undirected motion graph) ----
 * (ctrl/path_planning/rrtstar_path_planner.tpp:298- -> generate_rrt_star, ctrl/graph_alg/rrt_star.hpp:169-190,530-570;
 * rrg_node_generator node_generators.hpp:137-172; star_neighborhood neighborhood_functors.hpp:95-102;
 * lazy_node_connector lazy_connector.hpp:79-123,230-275,332-372) over the quasi-static free space.
 * Iterations are sequential (rewiring); the two k-NN sweeps and all candidate edges of an iteration run batched on
 * the device, for all problems of the batch at once.  Vertex 0 = start, vertex 1 = goal. */
typedef struct rkh_rrtstar_stats {
  uint64_t num_vertices, samples, loop_iterations, num_solutions, rewires, edges_checked;
  double best_cost;
  uint64_t pruned, skipped; /* branch-and-bound: vertices removed / points dropped before a vertex was created */
} rkh_rrtstar_stats;
rkh_status rkh_rrtstar_create_qs_batch(rkh_scene* scene, const rkh_qs_space* space, const rkh_rrt_params* prms,
                                       uint32_t n_problems, rkh_rrtstar** out);
/* The same planner over the steerable dynamic free space (rkh_dyn_space: vertices are states (q, qd), every candidate
 * edge -- expand_to_nearest, can_be_connected in each direction -- is an RK4 propagation with collision checks, as in
 * rkh_planner_*).  For a space with an asymmetric metric the reference builds a directed motion graph
 * (motion_graph_structures.hpp:73-74) and runs rrg_node_generator's directed overload (node_generators.hpp:176-206) and
 * lazy_node_connector's (lazy_connector.hpp:418-460: connect_best_predecessor over the predecessor neighbourhood,
 * connect_successors :277-325 over the successor neighbourhood; both from min_dist_linear_search
 * topological_search.hpp:296-345).  This space's metric is the symmetric Euclidean state distance, under which the two
 * neighbourhoods coincide (one k-NN sweep serves both); what is directional is every can_be_connected call, and those
 * are evaluated per direction. */
rkh_status rkh_rrtstar_create_batch(rkh_scene* scene, const rkh_dyn_space* space, const rkh_rrt_params* prms,
                                    uint32_t n_problems, rkh_rrtstar** out);
/* USE_BRANCH_AND_BOUND_PRUNING_FLAG (rrtstar_path_planner.tpp:270-283; unidirectional planners, before the first solve):
 * generate_bnb_rrt_star (rrt_star.hpp:690-730) with branch_and_bound_connector (branch_and_bound_connector.hpp:105-330).
 * Once the goal has a predecessor, a new point whose straight-line bound |start p| + |p goal| exceeds the goal's cost is
 * dropped, and after every connection the vertices whose distance_accum + |v goal| exceeds it are removed from the graph
 * (vertex_to_be_removed -> the KNN synchro's removed_vertex: the vertex keeps its index, its row on the device becomes
 * +inf).  Kept as in the reference: with nothing but uniform sampling almost every later point is dropped, so a run is
 * normally ended by max_loop_iterations; children of a removed vertex keep their cost and stay candidate parents.
 * Defined here: ids are append-only (the reference's pooled container would re-use the hole), the pruning loop stops on
 * an empty queue. */
rkh_status rkh_rrtstar_set_branch_and_bound(rkh_rrtstar* p, int enabled);
rkh_status rkh_rrtstar_get_removed(rkh_rrtstar* p, uint32_t problem, uint8_t* removed);
rkh_status rkh_rrtstar_destroy(rkh_rrtstar* p);
/* stats: array of n_problems entries.  max_loop_iterations < 0: run until keep_going() is false. */
rkh_status rkh_rrtstar_solve(rkh_rrtstar* p, int64_t max_loop_iterations, rkh_rrtstar_stats* stats);
/* pos [num_vertices][n_dof], pred[num_vertices] (0xFFFFFFFF = unconnected), dist[num_vertices] (distance_accum),
 * near_seq[loop_iterations] (x_near returned by the node generator).  Any pointer may be NULL. */
rkh_status rkh_rrtstar_get_graph(rkh_rrtstar* p, uint32_t problem, double* pos, uint32_t* pred, double* dist,
                                 uint32_t* near_seq);
/* ---- bidirectional RRT*: generate_rrt_star_bidir (ctrl/graph_alg/rrt_star.hpp:197-236,612-659) with rrg_bidir_generator
 * (node_generators.hpp:215-277) and the bidirectional lazy_node_connector (lazy_connector.hpp:465-518), over the
 * quasi-static free space (the reference requires a reversible space, rrtstar_path_planner.tpp:70).  Every vertex
 * carries a predecessor / distance_accum towards the start (forward tree, root = vertex 0) and a successor /
 * fwd_distance_accum towards the goal (backward tree, root = vertex 1).  As in the reference, no solution is ever
 * registered: the goal has a successor (itself), so connect_successors never gives it a predecessor, which is what
 * vertex_added tests (planning_visitors.hpp:108-116); the graph grows to max_vertices.  Vertices that end up with both
 * links are counted (`joins`, best_join_cost = distance_accum + fwd_distance_accum).  A loop iteration can add two
 * vertices, so the graph may hold max_vertices + 3.  The handle type is rkh_rrtstar; rkh_rrtstar_destroy frees it. */
typedef struct rkh_birrtstar_stats {
  uint64_t num_vertices, samples, loop_iterations, rewires, fwd_rewires, joins, edges_checked;
  double best_join_cost;
} rkh_birrtstar_stats;
rkh_status rkh_birrtstar_create_qs_batch(rkh_scene* scene, const rkh_qs_space* space, const rkh_rrt_params* prms,
                                         uint32_t n_problems, rkh_rrtstar** out);
rkh_status rkh_birrtstar_solve(rkh_rrtstar* p, int64_t max_loop_iterations, rkh_birrtstar_stats* stats);
/* pos [num_vertices][n_dof]; pred / succ (0xFFFFFFFF = none); dist / fwd_dist; near_pred / near_succ [loop_iterations]:
 * the generator's x_pred / x_succ.  Any pointer may be NULL. */
rkh_status rkh_birrtstar_get_graph(rkh_rrtstar* p, uint32_t problem, double* pos, uint32_t* pred, double* dist, uint32_t* succ,
                                   double* fwd_dist, uint32_t* near_pred, uint32_t* near_succ);
/* ---- PRM: prm_planner::solve_planning_query (LINEAR_SEARCH_KNN, ADJ_LIST_MOTION_GRAPH, undirected graph) ----
 * (ctrl/path_planning/prm_path_planner.tpp:131-365 -> generate_prm, ctrl/graph_alg/probabilistic_roadmap.hpp:211-249,
 * 309-404; prm_node_connector prm_connector.hpp:68-182; prm_conn_visitor probabilistic_roadmap.hpp:75-196;
 * prm_density_calculator density_calculators.hpp:45-73; random_walk planning_visitors.hpp:403-432) over the
 * quasi-static free space.  One loop iteration (construct: rejection sampling + k-NN + can_be_connected to every
 * neighbour; expand: the 11 random-walk attempts from the lowest-density vertex + k-NN + connections) is one batched
 * device step for all problems.  Vertex 0 = start, vertex 1 = goal.  As in the reference (which instantiates
 * density_plan_visitor here), no solution is registered: the roadmap grows to max_vertices; merged_at_vertex is the
 * vertex count at which start and goal first shared a connected component (-1: never). */
typedef struct rkh_prm_stats {
  uint64_t num_vertices, num_edges, samples, rejected, loop_iterations, num_components, publish_calls;
  int64_t merged_at_vertex;
  uint64_t edges_checked, device_steps;
} rkh_prm_stats;
rkh_status rkh_prm_create_qs_batch(rkh_scene* scene, const rkh_qs_space* space, const rkh_prm_params* prms,
                                   uint32_t n_problems, rkh_prm** out);
/* The same planner over the steerable dynamic free space: vertices are states (q, qd); the rejection sampling tests
 * is_free(state), every random-walk attempt is steer_position_toward(v, target_dist / dist, p_rnd) -- an RK4 propagation
 * over that fraction of the edge time -- and every connection a full propagation judged by can_be_connected.  A walk
 * whose fraction asks for more RK4 steps than an edge's budget (64) is refused with RKH_ERR_UNSUPPORTED. */
rkh_status rkh_prm_create_batch(rkh_scene* scene, const rkh_dyn_space* space, const rkh_prm_params* prms, uint32_t n_problems,
                                rkh_prm** out);
rkh_status rkh_prm_destroy(rkh_prm* p);
/* stats: array of n_problems entries.  max_loop_iterations < 0: run until keep_going() is false. */
rkh_status rkh_prm_solve(rkh_prm* p, int64_t max_loop_iterations, rkh_prm_stats* stats);
/* pos [num_vertices][n_dof]; edge_u/edge_v/edge_w [num_edges] in insertion order; density, cc_root [num_vertices];
 * kind [loop_iterations] (0 construct, 1 expand, 2 expand failed -> Q.pop()); expanded [loop_iterations] (Q.top() of
 * expansion iterations, else 0xFFFFFFFF).  Any pointer may be NULL. */
rkh_status rkh_prm_get_graph(rkh_prm* p, uint32_t problem, double* pos, uint32_t* edge_u, uint32_t* edge_v,
                             double* edge_w, double* density, uint32_t* cc_root, uint8_t* kind, uint32_t* expanded);
/* ---- Roadmap queries: what prm_planner_visitor::publish_path (ctrl/path_planning/prm_path_planner.tpp:97-122) does and
 * the solve above never reaches -- a shortest-path search over the motion graph with EdgeProp::weight that writes
 * predecessor / distance_accum, and the predecessor walk from the goal (solution_path_factories.hpp).  They are queries
 * on the roadmap as it stands (finished, or stopped by max_loop_iterations and resumed later); the solve, its stats and
 * the roadmap are untouched and still no solution is registered during the solve.  The graph and its weights are what
 * rkh_prm_get_graph returns, over quasi-static and dynamic roadmaps alike.
 * Searches run on the device, one workgroup per (roadmap, source) pair (reak_amd/csrc/roadmap_paths.hip).  dist is the
 * minimum over paths of the left-to-right fp64 sum of the weights from the source: bit for bit what a sequential
 * Dijkstra computes.  The reference's search (BGL's astar_search, not in its tree; never run) yields these distances
 * too, but its choice among equal-cost predecessors follows its queue's history.  Defined here instead: pred[v] is the
 * LOWEST vertex id u among v's edges with dist[u] + w == dist[v]; a query point that is not a roadmap vertex counts as
 * lower than every id (RKH_PRM_QUERY_POINT).  The source itself: dist 0, pred 0xFFFFFFFF; an unreached vertex: dist +inf,
 * pred 0xFFFFFFFF. */
#define RKH_PRM_QUERY_POINT 0xFFFFFFFEu
/* distance_accum / predecessor of every vertex of problem's roadmap from each of S source vertices, the S searches in one
 * launch.  dist, pred [S][num_vertices]; either may be NULL, not both.  RKH_ERR_BAD_ARG: a source >= num_vertices, S > 0
 * without sources, problem out of range, both outputs NULL.  S == 0 is RKH_OK. */
rkh_status rkh_prm_shortest_paths(rkh_prm* p, uint32_t problem, const uint32_t* sources, uint32_t S,
                                  double* dist /* [S][num_vertices] */, uint32_t* pred /* [S][num_vertices] */);
/* start (vertex 0) -> goal (vertex 1) through the roadmap as it stands: cost = distance_accum of the goal, path = the
 * predecessor walk from the goal, start first.  Capacity, NULL path and n_path = 0 (goal not reached: cost +inf) as for
 * rkh_rrtstar_get_solution below.  The first call after a solve searches from vertex 0 in all problems of the batch in
 * one launch; the handle keeps a problem's tree until rkh_prm_solve adds a vertex or an edge to it. */
rkh_status rkh_prm_get_solution(rkh_prm* p, uint32_t problem, uint32_t* path, uint32_t capacity,
                                uint32_t* n_path, double* cost);
/* Multi-query: B (start, goal) pairs of points [B][n_dof] that need not be roadmap vertices (quasi-static roadmaps;
 * a dynamic roadmap: RKH_ERR_UNSUPPORTED, its connections are directional propagations between states).  Each point
 * is connected to its k nearest roadmap vertices strictly inside radius (the rule of rkh_nn_queryk: ascending
 * (distance, index)) by the quasi-static walk in the direction of travel, start -> u and u -> goal, judged by
 * can_be_connected (planning_visitors.hpp:385-395) with the problem's conn_tol and weighted like a roadmap edge
 * (|first point of the walk - its end point|).  A point that coincides with a roadmap vertex connects to it with weight 0.
 * cost[b] = min over the accepted goal connections v of dist[v] + w(v, goal), the lowest v winning ties, dist from the
 * accepted start connections; path[b] = the roadmap vertices between the two points in travel order, n_path[b] their
 * count (the first min(n_path[b], capacity) are written); no path: n_path[b] = 0, cost[b] = +inf.  path may be NULL.
 * One k-NN launch, one edge-walk launch and one search launch serve all B pairs.  A direct start -> goal walk is not
 * tried here: rkh_shortcut_paths on the answer (start, path vertices, goal) tries it as its pair (0, L - 1).
 * RKH_ERR_BAD_ARG: NULL starts / goals / cost / n_path with B > 0, k == 0,
 * problem out of range.  B == 0 is RKH_OK. */
rkh_status rkh_prm_query_paths(rkh_prm* p, uint32_t problem, const double* starts, const double* goals, uint32_t B,
                               uint32_t k, double radius, uint32_t capacity,
                               double* cost /* [B] */, uint32_t* path /* [B][capacity] */, uint32_t* n_path /* [B] */);
/* ---- Bidirectional RRT: rrt_planner with BIDIRECTIONAL_PLANNING (the reference's default flag,
 * ctrl/path_planning/rrt_path_planner.hpp:114) -> generate_bidirectional_rrt (ctrl/graph_alg/rr_tree.hpp:256-317),
 * joining_vertex_found (planning_visitors.hpp:223-231), two-graph solution registration
 * (solution_path_factories.hpp:359-408), over the quasi-static free space.  Tree 1 is rooted at the start, tree 2 at
 * the goal; one expansion (nearest neighbour + edge walk) is one batched device step for all problems. */
typedef struct rkh_birrt_stats {
  uint64_t num_vertices_1, num_vertices_2, loop_iterations, samples, num_solutions, joins, edges_checked;
  double best_cost;
} rkh_birrt_stats;
rkh_status rkh_birrt_create_qs_batch(rkh_scene* scene, const rkh_qs_space* space, const rkh_rrt_params* prms,
                                     uint32_t n_problems, rkh_birrt** out);
rkh_status rkh_birrt_destroy(rkh_birrt* p);
/* stats: array of n_problems entries.  max_loop_iterations < 0: run until keep_going() is false. */
rkh_status rkh_birrt_solve(rkh_birrt* p, int64_t max_loop_iterations, rkh_birrt_stats* stats);
/* pos1 [num_vertices_1][n_dof], parent1 (root: 0xFFFFFFFF), the same for tree 2; nn_seq / accept [2 * loop_iterations]:
 * nearest vertex and reached_new of every expansion (tree 1, tree 2, tree 1, ...).  Any pointer may be NULL. */
rkh_status rkh_birrt_get_trees(rkh_birrt* p, uint32_t problem, double* pos1, uint32_t* parent1, double* pos2,
                               uint32_t* parent2, uint32_t* nn_seq, uint8_t* accept);
/* ---- Solution paths (what register_*_solution_path_impl of ctrl/path_planning/solution_path_factories.hpp walks) ----
 * Vertex indices into the arrays of rkh_planner_get_tree / rkh_rrtstar_get_graph / rkh_birrt_get_trees, start first;
 * n_path = 0 if no solution is registered; the path pointers may be NULL to query the lengths; cost = the registered
 * solution cost (RRT: path + goal-probe distance of the last vertex; RRT*: distance_accum of the goal; bidirectional:
 * both tree paths + joining distance). */
rkh_status rkh_planner_get_solution(rkh_planner* p, uint32_t problem, uint32_t* path, uint32_t capacity,
                                    uint32_t* n_path, double* cost);
rkh_status rkh_rrtstar_get_solution(rkh_rrtstar* p, uint32_t problem, uint32_t* path, uint32_t capacity, uint32_t* n_path,
                                    double* cost);
rkh_status rkh_birrt_get_solution(rkh_birrt* p, uint32_t problem, uint32_t* path1, uint32_t* n_path1, uint32_t* path2,
                                  uint32_t* n_path2, uint32_t capacity, double* cost);
/* ---- Shortcutting: the paths above come straight off a random tree or roadmap and zig-zag.  This entry removes the
 * vertices a straight collision-free hop makes unnecessary, for B paths at once, exactly.  The reference has no
 * shortcutter; the walk it rests on is the one of rkh_edge_check.
 * Input: B paths over a quasi-static space (rate-limited spaces included; metric and interpolation in space coordinates).
 * Path b is the L_b >= 1 points points[path_ptr[b] .. path_ptr[b + 1]), each [n_dof], start first (the rows of
 * rkh_*_get_graph / get_tree picked by a solution's indices, with any off-roadmap start and goal point added).
 * Weight: w(i, j) = the left-to-right fp64 euclidean norm of p_i - p_j (s = s + d * d in coordinate order, a correctly
 * rounded sqrt, no contraction): what the walk computes as the length of the hop.
 * Strict verdict: ok(i, j) is the verdict of the full-fraction walk p_i -> p_j in the direction of travel: true if
 * w(i, j) < min_interval (move_position_toward makes no predicate call there), else iff the predicate loop ran to its end
 * without a failing point, i.e. the walk returns p_j bit for bit.  This is stricter than can_be_connected
 * (planning_visitors.hpp:385-395), which accepts a walk that stopped within conn_tol of its target; a shortcut must not.
 * Candidates: with span = max_span ? max_span : L - 1, all pairs (i, j) with 1 <= j - i <= span, in the order i ascending,
 * then j ascending; every one of them is walked, all paths' pairs in ONE walk launch.
 * Search: dist[0] = 0, dist[j] = min over the allowed i < j of dist[i] + w(i, j), that one fp64 addition; allowed means
 * j == i + 1 (the caller's own hops, whatever their verdict: roadmap edges were accepted under a tolerance) or ok(i, j) with
 * j - i <= span; the LOWEST i wins ties.  Bit for bit the sequential double loop (i ascending, update under strict <).  All
 * pairs are tried, so the result is the optimum over all subsequences of the path: a second pass cannot improve it.
 * Outputs per path: keep = the predecessor walk from L - 1, start first, as path-local indices, written at
 * keep[path_ptr[b] ..], n_keep[b] <= L_b of them (the path's slots behind them hold 0xFFFFFFFF); cost_in = the left-to-right sum of the consecutive hops; cost_out =
 * dist[L - 1] <= cost_in (the input is a candidate and fp addition is monotone); n_blocked = the hops of the RETURNED path
 * whose strict verdict is false (they can only be input hops; 0: the returned path passed the strict walk hop by hop).
 * The direct start -> goal connection is the pair (0, L - 1): n_keep == 2.
 * B == 0 is RKH_OK.  RKH_ERR_BAD_ARG: a NULL scene, space, points, path_ptr, keep, n_keep or cost_out; path_ptr not
 * ascending from 0; an empty path; space->n_dof != rkh_scene_num_dof; min_interval <= 0; a coordinate that is not finite.
 * RKH_ERR_CAPACITY: a path of more than 1024 points, or more than 2147483647 candidate pairs in the call (a path of L
 * points has L (L - 1) / 2 of them; max_span is the caller's way under it: about L * max_span).  Every pair takes
 * 8 n_dof + 25 bytes of device memory for the duration of the call (the walk's scratch included), so memory ends a call
 * (RKH_ERR_OOM) long before that count: 100 million pairs of a 3-joint chain take 4.9 GB.
 * Paths of dynamic states (rkh_dyn_space) are not served: their hops are propagations, not straight walks. */
rkh_status rkh_shortcut_paths(rkh_scene* scene, const rkh_qs_space* space, const double* points,
                              const uint32_t* path_ptr /* [B+1] */, uint32_t B, uint32_t max_span,
                              uint32_t* keep /* [path_ptr[B]] */, uint32_t* n_keep /* [B] */,
                              double* cost_in /* [B], may be NULL */, double* cost_out /* [B] */,
                              uint32_t* n_blocked /* [B], may be NULL */);

/* ---- Direct kinematics, Jacobians and pose IK -------------------------------------------------------------------------
 * Where a frame of the chain is, how it moves with the joints, and joint configurations that put it at a pose.  The
 * planners above work in joint space; these entries are the way between joint space and workspace.
 * Frames are named by the caller's own indices: the numbering of rkh_kte_op::base_frame / end_frame and rkh_shape::anchor
 * (frame 0 = the chain base, plus every joint end frame, link end frame and mount link end frame of the program).
 * q [B][n_dof] joint positions, qd [B][n_dof] joint rates or NULL for zero rates; frames [F].
 *
 * rkh_direct_kinematics answers manip_direct_kin_map::map_to_space (ctrl/topologies/direct_kinematics_topomap.hpp:57-103):
 * per (state, frame) what kte_map_chain::doMotion leaves in the frame with q'' = 0, in the conventions of a parentless
 * frame_3D: pos [B][F][3] and vel [B][F][3] in world coordinates, quat [B][F][4] (w, x, y, z), ang_vel [B][F][3] in the
 * frame's OWN coordinates.  The pose is computed in the operation order of the distance query, so it is bit for bit the
 * pose rkh_min_distance gives the shapes anchored on the frame.  Any output may be NULL, not all of them.
 * rkh_direct_kinematics_2d: the same for planar scenes (frame_2D): pos [B][F][2], rot [B][F][2] = (cos, sin),
 * vel [B][F][2], ang_vel [B][F].
 *
 * rkh_jacobians answers manipulator_kinematics_model::getJacobianMatrix / getJacobianMatrixAndDerivative
 * (ctrl/kte_models/manip_kinematics_model.cpp:70-77, manip_kinematics_helper.cpp:249-318) for one dependent frame per
 * asked frame: jac [B][F][6][n_dof], jac_dot the same shape (either may be NULL, not both; jac_dot with NULL qd is zeros).
 * Column i of frame f is all zeros unless joint i is upstream of f (mUpStreamJoints: a joint gives up[end] = up[base] |
 * bit(coord), a link up[end] = up[base], the base has none); otherwise it is jacobian_gen_3D::get_jac_relative_to
 * (core/kinetostatics/motion_jacobians.hpp:238-251) of the joint's generator -- revolute qd_avel = mAxis, prismatic
 * qd_vel = mAxis as given (revolute_joint.cpp:145-148, prismatic_joint.cpp:150-153), the rest 0 -- relative to f, written
 * in write_to_matrices' row order: velocity (3), angular velocity (3), both in f's own coordinates.  So
 * jac qd = (R(quat)^T vel, ang_vel) of rkh_direct_kinematics.
 * rkh_jacobians_2d: jacobian_gen_2D (:138-146), jac [B][F][3][n_dof], rows (vx, vy, omega) in f's coordinates.
 *
 * B == 0 or F == 0 is RKH_OK.  RKH_ERR_BAD_ARG: a frame index that is not a frame of the chain, NULL q or frames, every
 * output NULL.  RKH_ERR_UNSUPPORTED, with an error text: the 3D entries on a planar scene, the _2d entries on a 3D scene.
 * Every chain rkh_scene_create[_with_meshes] accepts is served. */
rkh_status rkh_direct_kinematics(rkh_scene* scene, const double* q, const double* qd, uint32_t B, const int32_t* frames,
                                 uint32_t F, double* pos /* [B][F][3] */, double* quat /* [B][F][4] */,
                                 double* vel /* [B][F][3] */, double* ang_vel /* [B][F][3] */);
rkh_status rkh_direct_kinematics_2d(rkh_scene* scene, const double* q, const double* qd, uint32_t B, const int32_t* frames,
                                    uint32_t F, double* pos /* [B][F][2] */, double* rot /* [B][F][2] */,
                                    double* vel /* [B][F][2] */, double* ang_vel /* [B][F] */);
rkh_status rkh_jacobians(rkh_scene* scene, const double* q, const double* qd, uint32_t B, const int32_t* frames, uint32_t F,
                         double* jac /* [B][F][6][n_dof] */, double* jac_dot /* [B][F][6][n_dof] */);
rkh_status rkh_jacobians_2d(rkh_scene* scene, const double* q, const double* qd, uint32_t B, const int32_t* frames, uint32_t F,
                            double* jac /* [B][F][3][n_dof] */, double* jac_dot /* [B][F][3][n_dof] */);
/* Pose IK for 3D chains: T targets x S seeds, all T S solves in one launch.  It stands where the reference's manipulator
 * applications run an inverse-kinematics step in front of the planner (chaser_kin_model->doInverseMotion(),
 * examples/robot_airship/CRS_planner_exec.cpp:309: closed forms per arm, else ctrl/kte_models/manip_clik_calculator.cpp over
 * an NLP solver); neither is restated.  Defined here instead, a damped
 * least-squares iteration per solve, q = clamp(seed, lower, upper), then for k = 0, 1, ...:
 *   1. (p, Q) = pose of `frame` at q, J = its Jacobian [6][n_dof] as rkh_jacobians defines it
 *   2. e_v = (p* - p) R(Q): the position error in the frame's coordinates
 *   3. dQ = Q^-1 Q*, negated if its w < 0; e_w = 2 (dQ.x, dQ.y, dQ.z)
 *   4. |e_v| <= tol_pos and |e_w| <= tol_rot: converged, stop, iters = k
 *   5. k == max_iters: stop, not converged, iters = k
 *   6. A = J J^T + damping^2 I (6 x 6); A y = e, e = (e_v, e_w), by decompose_Cholesky / backsub_Cholesky
 *      (lin_alg/mat_cholesky.hpp), the sequence of the f-eval; a pivot that is not positive: stop, not converged
 *   7. dq = J^T y; if max |dq_i| > max_step: dq = dq * (max_step / max |dq_i|)
 *   8. q = clamp(q + dq, lower, upper)
 * in fp64, every sum left to right (over the joints, then + damping^2; over the six rows), no contraction.
 * Then ONE launch of the distance query of rkh_min_distance over all T S results: free = (minimum distance > 0); a scene
 * without proxy pairs is free.
 * seeds [T][S][n_dof]; lower / upper [n_dof] (lower <= upper); q_out [T][S][n_dof]; res_pos / res_rot [T][S] the last |e_v| /
 * |e_w|; iters [T][S]; flags [T][S]: bit 0 converged, bit 1 free; best [T]: the lowest seed index that is converged and
 * free, else 0xFFFFFFFF.  Every output but q_out may be NULL.  T == 0 or S == 0 is RKH_OK.
 * RKH_ERR_BAD_ARG: params->struct_size != sizeof(rkh_ik_params) (the entry checks it itself), damping or max_step not
 * positive, a negative tolerance, lower > upper, a target that is not finite or whose quaternion is not unit to 1e-9, a
 * seed that is not finite, a frame that is not a frame of the chain, NULL targets / seeds / bounds / q_out.
 * RKH_ERR_UNSUPPORTED: planar scenes.  Not built: planar IK, position-only or partial-pose targets, null-space objectives
 * for redundant chains, the reference's closed-form arm solutions. */
typedef struct rkh_ik_params {
  uint32_t struct_size; /* sizeof(rkh_ik_params) */
  uint32_t max_iters;
  double damping, max_step, tol_pos, tol_rot;
} rkh_ik_params;
rkh_status rkh_inverse_kinematics(rkh_scene* scene, int32_t frame, const rkh_pose* targets /* [T] */, uint32_t T,
                                  const double* seeds /* [T][S][n_dof] */, uint32_t S, const double* lower, const double* upper,
                                  const rkh_ik_params* params, double* q_out /* [T][S][n_dof] */, double* res_pos /* [T][S] */,
                                  double* res_rot /* [T][S] */, uint32_t* iters /* [T][S] */, uint32_t* flags /* [T][S] */,
                                  uint32_t* best /* [T] */);

/* ---- the order-1 rate-limited joint space with SVP profiles (rkh_svp_space, rkh_types.h) ----------------------------------
 * These entries stand in for svp_Ndof_reach_time_metric, svp_Ndof_interpolator and the move_pt_toward of
 * svp_Ndof_reach_topologies.hpp over manip_quasi_static_env::is_free.  Points are [2 n_dof] doubles (p0, v0, p1, v1, ...).
 *
 * Reach time d(a -> b): per joint the minimum time of a ramp / cruise / ramp velocity profile
 * (svp_Ndof_compute_min_delta_time), T = their maximum, then per joint the peak velocity that takes exactly T
 * (svp_Ndof_compute_peak_velocity).  A joint without a solution in either pass (a velocity beyond vm, or the known gap of a
 * velocity-bounded double integrator that cannot stretch its time), or coordinates that are not finite, make d = +inf.
 * d is not symmetric.
 *
 * rkh_svp_in_bounds: svp_Ndof_is_in_bounds, on the host (no device needed): the point, the point where each joint could
 * stop (p + v |v| / (2 vm)) and the point it could have started from (p - v |v| / (2 vm)) inside [lower, upper], v inside
 * +-vm.  ok [B]: 1 or 0.
 * rkh_svp_reach_time: time [B] and, if not NULL, peak [B][n_dof] (zeros for an infinite pair).
 * rkh_svp_nearest: the k nearest of `points` per query.  direction 0: by d(point -> query), the predecessors an RRT extends
 * from; direction 1: by d(query -> point), the successors.  idx / dist [B][k] ascend by (distance, index); infinite
 * distances are never returned: a query with fewer than k finite neighbours is padded with 0xFFFFFFFF and +inf.  k in [1, 64];
 * at most 16 777 216 points and 65 535 queries per call (RKH_ERR_CAPACITY).
 * rkh_svp_nearest_async: the same with device pointers, enqueued on the context's stream: no host copy, no synchronisation.
 * The context keeps the scratch of launches that slice the points; it grows with the largest request.
 * rkh_svp_edge_check: the collision-tested walk.  T = d(a -> b); T = +inf: out = a, nothing tested.  Else dt = T fraction
 * (fraction NULL: 1.0), and the points at travel times d = min_interval, + min_interval, ... (repeated addition) below dt are
 * tested in order with "in bounds (above), and no proxy pair closer than 0" at q_i = p_i speed_limits[i],
 * qd_i = v_i accel_limits[i]; the first failure ends the walk at the last point that passed (a if none).  Without a failure:
 * fraction == 1.0 returns b, fraction == 0.0 returns a, any other the (untested) point at dt.  out [B][2 n_dof];
 * reach_time [B]; n_checked [B]: points tested, the failing one included; reached [B]: 1 where the loop ran to dt without a
 * failure.  Every output but out may be NULL.  An edge with more than 1 048 576 points to test: RKH_ERR_CAPACITY.
 * rkh_svp_edge_check_back: the same arguments, outputs, NULL rules and refusals; it stands in for move_pt_back_to
 * (svp_Ndof_reach_topologies.hpp) over is_free: the profile a -> b walked from its end backwards, the last free point kept.
 * In fp64 with these groupings:
 *     T, peak = reach(a, b)                       the common-time solve of d(a -> b)
 *     T == +inf:  out = b, n_checked = 0, reached = 0
 *     dt = T * (1.0 - fraction)                   fraction NULL: 1.0
 *     d = T - min_interval;  last = b
 *     while d > dt:                               strict
 *         x = point(a, b, peak, T, d);  ++n_checked
 *         not in bounds, or a proxy pair closer than 0 at x in model units:  out = last, reached = 0, stop
 *         last = x;  d -= min_interval            repeated subtraction
 *     reached = 1;  out = a if fraction == 1.0, b if fraction == 0.0, else point(a, b, peak, T, dt)   (untested, as forward)
 * More than 1 048 576 points to test (counted by the same repeated subtraction): RKH_ERR_CAPACITY.
 * rkh_svp_interpolate: the profile of each pair sampled at M times, t [B][M], out [B][M][2 n_dof], reach_time [B] (may be
 * NULL).  t <= 0: a; t >= T: b; an infinite pair: a at every time.
 *
 * B == 0, M == 0 or n_pts == 0 is RKH_OK.  RKH_ERR_BAD_ARG: space->struct_size != sizeof(rkh_svp_space), n_dof not in
 * [1, 12] or not the scene's, min_interval not positive and finite, lower > upper, a negative or non-finite limit, k or
 * direction out of range, a NULL required pointer.  Not built: the order-2 space (SAP), the temporal spaces, and batch
 * planners over this space other than the RRT and the bidirectional RRT below (no RRT*, PRM or SBA* over it), a walk
 * fused into one launch. */
rkh_status rkh_svp_in_bounds(const rkh_svp_space* space, const double* pts /* [B][2 n_dof] */, uint32_t B, uint8_t* ok /* [B] */);
rkh_status rkh_svp_reach_time(rkh_ctx* ctx, const rkh_svp_space* space, const double* a, const double* b, uint32_t B,
                              double* time /* [B] */, double* peak /* [B][n_dof], may be NULL */);
rkh_status rkh_svp_nearest(rkh_ctx* ctx, const rkh_svp_space* space, const double* points /* [n_pts][2 n_dof] */,
                           uint32_t n_pts, const double* queries /* [B][2 n_dof] */, uint32_t B, uint32_t k, int32_t direction,
                           uint32_t* idx /* [B][k] */, double* dist /* [B][k] */);
rkh_status rkh_svp_nearest_async(rkh_ctx* ctx, const rkh_svp_space* space, const double* d_points, uint32_t n_pts,
                                 const double* d_queries, uint32_t B, uint32_t k, int32_t direction, uint32_t* d_idx,
                                 double* d_dist);
rkh_status rkh_svp_edge_check(rkh_scene* scene, const rkh_svp_space* space, const double* a, const double* b, uint32_t B,
                              const double* fraction /* [B], NULL = 1.0 */, double* out /* [B][2 n_dof] */,
                              double* reach_time /* [B] */, uint32_t* n_checked /* [B] */, uint8_t* reached /* [B] */);
rkh_status rkh_svp_edge_check_back(rkh_scene* scene, const rkh_svp_space* space, const double* a, const double* b, uint32_t B,
                                   const double* fraction /* [B], NULL = 1.0 */, double* out /* [B][2 n_dof] */,
                                   double* reach_time /* [B] */, uint32_t* n_checked /* [B] */, uint8_t* reached /* [B] */);
rkh_status rkh_svp_interpolate(rkh_ctx* ctx, const rkh_svp_space* space, const double* a, const double* b, uint32_t B,
                               const double* t /* [B][M] */, uint32_t M, double* out /* [B][M][2 n_dof] */,
                               double* reach_time /* [B] */);

/* ---- batch RRT over the SVP space: device-resident trees, P problems per launch ------------------------------------------
 * P independent problems (rkh_svp_rrt_params, rkh_types.h) on one scene and one space grow in lock step, one RRT iteration
 * of every unfinished problem per round; trees, sample streams and all per-problem state stay on the device.  Each
 * problem's tree is, bit for bit, the tree of this sequential loop, whatever P is and whatever the other problems do:
 *
 *   sample stream: std::mt19937(seed); draw j gives u = y 2^-32; candidate k takes draws k D .. k D + D - 1 (D = 2 n_dof)
 *     in point order, coordinate c = lo_c + u (hi_c - lo_c) with (lo, hi) = (lower[i], upper[i]) for p_i and
 *     (-vm_i, +vm_i) for v_i: the rate-limited sampler (draw from the box, reject with rkh_svp_in_bounds), every draw an
 *     iteration.
 *   before the loop: has_goal and the whole edge start -> goal is free (rkh_svp_edge_check, fraction 1, reached): goal_parent = 0.
 *   while the goal is not reached, n_vertices < max_vertices and iterations < max_iterations:
 *     take the next candidate, ++iterations; not rkh_svp_in_bounds: next iteration;
 *     the 1-nearest vertex by d(vertex -> candidate), ties to the lower index; every distance +inf: next iteration;
 *     fraction = asked > 0 ? min(1, max_edge_time / asked) : 1; walk vertex -> candidate with that fraction as
 *     rkh_svp_edge_check does; n_checked == 0: next iteration;
 *     travelled = d(vertex -> out); commit only if it is finite, < 2 asked fraction and > steer_tol asked fraction:
 *     append out with its parent and travelled; has_goal and the whole edge out -> goal is free: goal_parent = the new vertex.
 *
 * rkh_svp_rrt_create_batch: P in [1, 16384]; runs the probes before the loop.  One arena of the context per planner.
 * rkh_svp_rrt_solve: rounds until every problem has ended or max_rounds of them have run (max_rounds < 0: no limit); a
 * later call resumes where the last stopped.  stats (may be NULL) are totals since create.  A round draws at most 1024
 * candidates per problem: a problem that found none in bounds among them makes no extension in that round.
 * rkh_svp_rrt_get_status: per problem; any pointer may be NULL.  goal_parent 0xFFFFFFFF: the goal is not reached.
 * rkh_svp_rrt_get_tree: the first min(V, capacity) vertices of one problem ([.][2 n_dof]), their parents (0xFFFFFFFF for
 * the start) and edge times (d(parent -> vertex); 0 for the start); *n_vertices = V.  Output pointers may be NULL.
 * rkh_svp_rrt_get_solution: start ... goal, the goal last, [n_points][2 n_dof]; duration = the sum of the edges' reach
 * times in path order.  n_points = 0 (and duration = 0) when the goal has not been reached; more points than capacity:
 * RKH_ERR_CAPACITY with *n_points set.
 *
 * RKH_ERR_BAD_ARG: a NULL required pointer, a struct of another size (space or any params), n_dof not the scene's,
 * max_vertices == 0, a start that is not finite or fails rkh_svp_in_bounds, P == 0 or P > 16384.  RKH_ERR_CAPACITY: an
 * edge with more than 1 048 576 points to test (the planner then refuses further rounds).  A failed create leaves no
 * planner behind (*out = NULL). */
typedef struct rkh_svp_rrt rkh_svp_rrt;
typedef struct rkh_svp_rrt_stats {
  uint64_t rounds;            /* rounds run */
  uint64_t problems_finished; /* problems that have ended */
  uint64_t iterations;        /* candidates drawn, over all problems */
  uint64_t vertices;          /* vertices, over all problems (the starts included) */
  uint64_t walk_passes;       /* passes of the staged walk, extensions and probes */
  uint64_t tested_points;     /* points tested by the walks */
  uint64_t window_refills;    /* refills of the problems' sample windows (64 candidates each) */
} rkh_svp_rrt_stats;
rkh_status rkh_svp_rrt_create_batch(rkh_scene* scene, const rkh_svp_space* space, const rkh_svp_rrt_params* params /* [P] */,
                                    uint32_t P, rkh_svp_rrt** out);
void rkh_svp_rrt_destroy(rkh_svp_rrt* planner);
rkh_status rkh_svp_rrt_solve(rkh_svp_rrt* planner, int64_t max_rounds, rkh_svp_rrt_stats* stats);
rkh_status rkh_svp_rrt_get_status(rkh_svp_rrt* planner, uint32_t* n_vertices /* [P] */, uint32_t* iterations /* [P] */,
                                  uint32_t* goal_parent /* [P] */);
rkh_status rkh_svp_rrt_get_tree(rkh_svp_rrt* planner, uint32_t problem, double* vertices /* [capacity][2 n_dof] */,
                                uint32_t* parent /* [capacity] */, double* edge_time /* [capacity] */, uint32_t capacity,
                                uint32_t* n_vertices);
rkh_status rkh_svp_rrt_get_solution(rkh_svp_rrt* planner, uint32_t problem, double* points /* [capacity][2 n_dof] */,
                                    uint32_t capacity, uint32_t* n_points, double* duration);

/* ---- batch bidirectional RRT over the SVP space: two device-resident trees per problem ---------------------------------------
 * The reach time is not symmetric, so a tree rooted at the goal cannot grow with forward walks: every edge of it must be a
 * profile that runs towards the goal.  Here tree 0 is rooted at the start and grows forward; tree 1 is rooted at the goal
 * and grows backward with rkh_svp_edge_check_back: the edge of its vertex v is the profile v -> parent(v), and
 * edge_time[v] = d(v -> parent(v)).  (The progress rule is steer_back_to_position's, the alternation
 * generate_bidirectional_rrt's; the reference's own bidirectional RRT steers both trees forward, which on this space gives
 * goal-tree edges nobody can traverse.)  One problem is a rkh_svp_rrt_params with has_goal = 1; max_vertices bounds each
 * tree; seed, max_iterations, max_edge_time and steer_tol mean what they do for rkh_svp_rrt.  One std::mt19937(seed)
 * candidate stream per problem, exactly the RRT's; both sides consume it in loop order.  Each problem's two trees are, bit
 * for bit, those of this sequential loop, whatever P is and whatever the other problems do:
 *
 *   target[0] = (goal, vertex 0 of tree 1);  target[1] = (start, vertex 0 of tree 0);  side = 0;  iterations = 0
 *   loop:
 *     n0 >= max_vertices or n1 >= max_vertices: end "max_vertices"
 *     (tp, tv) = target[side]
 *     tv is none:                                             # a sample is needed
 *         iterations >= max_iterations: end "max_iterations"
 *         ++iterations; q = next candidate; not rkh_svp_in_bounds(q): continue loop (same side)
 *         tp = q
 *     side 0: (idx, asked) = argmin over tree 0 of d(vertex -> tp); side 1: argmin over tree 1 of d(tp -> vertex)
 *             ties to the lower index; every distance +inf: not moved
 *     else:
 *         f = asked > 0 ? min(1, max_edge_time / asked) : 1          # rl1rrt_fraction
 *         side 0: forward walk (a = vertex, b = tp, f);  side 1: backward walk (a = tp, b = vertex, f)
 *         tv is a vertex and f == 1.0 and reached:  join = (idx, tv) on side 0, (tv, idx) on side 1;
 *                                                   join_time = asked;  end "joined"   # nothing is appended
 *         n_checked == 0: not moved
 *         else travelled = d(vertex -> out) on side 0, d(out -> vertex) on side 1;
 *              rl1rrt_progress(travelled, asked, f, steer_tol): append out to tree `side` with parent idx and
 *              edge time travelled: moved;  otherwise not moved
 *     target[1 - side] = moved ? (out, the new vertex) : none;   side = 1 - side
 *
 * A join does not look at n_checked: a connection shorter than min_interval tests nothing and counts, as the RRT's goal
 * probe does.  max_iterations ends a problem only when a sample is needed and none is left: a problem whose targets are
 * vertices goes on past iterations == max_iterations, and with max_iterations == 0 it runs until its first failed half
 * step.  There is no probe before the loop: the first half step is the attempt start -> goal.
 * What this planner is not known to be: faster.  On the C2 scene the unidirectional rkh_svp_rrt often needs fewer vertices,
 * because its goal probe walks the whole edge whatever max_edge_time is; nobody has measured either planner on a scene
 * where the goal sits in a pocket the probe rarely sees.
 *
 * rkh_svp_birrt_create_batch: P in [1, 16384].  One arena of the context per planner.
 * rkh_svp_birrt_solve: rounds (one half step of every unfinished problem) until every problem has ended or max_rounds have
 * run (< 0: no limit); a later call resumes.  stats (may be NULL): rkh_svp_rrt_stats, totals since create; vertices counts
 * both trees, roots included.  A round draws at most 1024 candidates per problem, as the RRT's.
 * rkh_svp_birrt_get_status: per problem; any pointer may be NULL.  join0 / join1: the joined vertices of tree 0 and tree 1,
 * 0xFFFFFFFF: no join.
 * rkh_svp_birrt_get_tree: as rkh_svp_rrt_get_tree, of tree 0 or 1.
 * rkh_svp_birrt_get_solution: the points start ... join0, join1 ... goal; duration summed in path order: tree-0 edge times
 * from the start, then join_time, then tree-1 edge times towards the goal.  n_points = 0 and duration = 0 without a join;
 * more points than capacity: RKH_ERR_CAPACITY with *n_points set.
 *
 * RKH_ERR_BAD_ARG: what rkh_svp_rrt_create_batch refuses, and has_goal == 0, a goal that is not finite or fails
 * rkh_svp_in_bounds (the message names "problem i"), tree > 1.  RKH_ERR_CAPACITY: an edge with more than 1 048 576 points to
 * test (the planner then refuses further rounds).  A failed create leaves no planner behind (*out = NULL). */
typedef struct rkh_svp_birrt rkh_svp_birrt;
rkh_status rkh_svp_birrt_create_batch(rkh_scene* scene, const rkh_svp_space* space, const rkh_svp_rrt_params* params /* [P] */,
                                      uint32_t P, rkh_svp_birrt** out);
void rkh_svp_birrt_destroy(rkh_svp_birrt* planner);
rkh_status rkh_svp_birrt_solve(rkh_svp_birrt* planner, int64_t max_rounds, rkh_svp_rrt_stats* stats);
rkh_status rkh_svp_birrt_get_status(rkh_svp_birrt* planner, uint32_t* n_vertices0 /* [P] */, uint32_t* n_vertices1 /* [P] */,
                                    uint32_t* iterations /* [P] */, uint32_t* join0 /* [P] */, uint32_t* join1 /* [P] */);
rkh_status rkh_svp_birrt_get_tree(rkh_svp_birrt* planner, uint32_t problem, uint32_t tree /* 0 | 1 */,
                                  double* vertices /* [capacity][2 n_dof] */, uint32_t* parent /* [capacity] */,
                                  double* edge_time /* [capacity] */, uint32_t capacity, uint32_t* n_vertices);
rkh_status rkh_svp_birrt_get_solution(rkh_svp_birrt* planner, uint32_t problem, double* points /* [capacity][2 n_dof] */,
                                      uint32_t capacity, uint32_t* n_points, double* duration);

/* ---- Shortcutting under the reach-time metric: a solution of the RRT above is a tree branch, a sequence of short extensions
 * towards random candidates, and far from the shortest duration its own vertices allow.  This entry is rkh_shortcut_paths
 * for paths of SVP points, B paths at once, exactly; that entry's definition holds with these substitutions and additions.
 * Input: path b is the L_b >= 1 points points[path_ptr[b] .. path_ptr[b + 1]), each [2 n_dof], start first (the rows of
 * rkh_svp_rrt_get_solution).
 * Weight: w(i, j) = the reach time d(p_i -> p_j), for i < j only (time runs forward; d is not symmetric): bit for bit what
 * rkh_svp_reach_time returns for the pair.  It may be +inf.
 * Strict verdict: ok(i, j) is the `reached` byte of rkh_svp_edge_check(p_i, p_j, fraction = NULL): the bounds rule and the
 * distance query at the travel times min_interval, + min_interval, ... below T all pass.  T < min_interval tests nothing
 * and gives true; T = +inf gives false.  The end points themselves are not tested, as in rkh_svp_edge_check.
 * Candidates: the span, the pair order and the walk of every pair are those of rkh_shortcut_paths.
 * Search: unchanged -- dist[0] = 0, dist[j] = min over the allowed i < j of dist[i] + w(i, j), allowed = j == i + 1 or
 * ok(i, j) within the span, the lowest i wins ties under strict <.  x + inf < y is never true, so an infinite weight is
 * never taken: a vertex behind an infinite consecutive hop is reachable only through a shortcut that bypasses it.
 * Outputs per path: keep / n_keep as there; time_in = the left-to-right sum of the consecutive hops' reach times (+inf if
 * any of them is); time_out = dist[L - 1] <= time_in; n_blocked = the hops of the RETURNED path whose strict verdict is
 * false.  They can only be input hops, and they do occur on planner output: a tree edge re-walked to its stored end point is
 * a new profile with new test points, not the extension the planner tested (0: the returned trajectory passed the walk hop by
 * hop).  A path of one point: n_keep = 1, keep = {0}, both times 0.
 * Unreachable goal: time_out = +inf means the points are not a trajectory and no shortcut repairs them: n_keep[b] = 0,
 * n_blocked[b] = 0 and every slot of keep that belongs to the path holds 0xFFFFFFFF.  The call is still RKH_OK and the other
 * paths are served.
 * B == 0 is RKH_OK.  RKH_ERR_BAD_ARG: everything the rkh_svp_* entries above refuse about a space (n_dof not the scene's
 * included); a NULL scene, points, path_ptr, keep, n_keep or time_out; path_ptr not ascending from 0; an empty path; a
 * coordinate that is not finite.  RKH_ERR_CAPACITY: a path of more than 1024 points; more than 2147483647 candidate pairs in
 * the call; an edge with more than 1 048 576 points to test.
 * Memory: the pairs go through the walk in chunks of 262 144, so a call takes 9 bytes per pair, 16 n_dof bytes per point and
 * (1096 n_dof + 333) min(pairs, 262 144) bytes of walk workspace: at most 1.81 GB for a 6-joint chain.
 * Not built: pruning of candidate pairs, shortcuts through new intermediate points. */
rkh_status rkh_svp_shortcut_paths(rkh_scene* scene, const rkh_svp_space* space, const double* points /* [path_ptr[B]][2 n_dof] */,
                                  const uint32_t* path_ptr /* [B+1] */, uint32_t B, uint32_t max_span,
                                  uint32_t* keep /* [path_ptr[B]] */, uint32_t* n_keep /* [B] */,
                                  double* time_in /* [B], may be NULL */, double* time_out /* [B] */,
                                  uint32_t* n_blocked /* [B], may be NULL */);

#ifdef __cplusplus
}
#endif
#endif
