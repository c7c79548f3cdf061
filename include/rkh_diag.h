/* rkh_diag.h -- profiling and diagnostic entry points of librkh.so.
 *
 * NOT part of the drop-in boundary (rkh.h): nothing here replaces a reference interface.  bench.py uses them to time
 * kernels with HIP events on the launch stream, the tests/diag_*.py scripts to read per-phase cycle counts.
 */
#ifndef RKH_DIAG_H
#define RKH_DIAG_H

#include "rkh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One-shot: the next rkh_nn_query1_async records the two hipEvent_t (passed as void*) immediately before and after
 * its sweep kernel on the context stream (bench.py times the kernel itself, not the launch sequence). */
rkh_status rkh_nn_set_events(rkh_nn* nn, void* ev_start, void* ev_stop);
/* Name of the sweep kernel the last query launched (for profile bookkeeping). */
const char* rkh_nn_kernel_name(void);
/* Exact retries of the k-NN search launched in this process so far: rkh_nn_queryk / rkh_prm_query_paths calls and
 * graph-planner steps whose first pass overflowed a candidate list (reak_amd/csrc/knn_plan.h).  RKH_KNN_LIST_CAP=N in the
 * environment -- read by every rkh_nn_queryk* and rkh_prm_query_paths call, and by a graph planner at create --
 * shortens the candidate lists to max(N, 2 k) slots, rounded up to a power of two: first passes then overflow on
 * ordinary data, which is how the tests make the planners take the retry.  Results do not depend on it. */
uint64_t rkh_diag_knn_retries(void);
/* The mapping the steer plan chose at this thread's last rkh_propagate or rkh_planner_create* over a dynamic space:
 * "auto", "duo", "wave", "wave16", "pair", "planar" or "prismatic" (one wave per edge, prismatic form). */
const char* rkh_steer_mapping_name(void);

/* Shader-clock cycles of `iters` back-to-back f-evals + proximity tests.  One-wave-per-edge kernel: one wave per state,
 * cycles[B][8] = {sincos, forward sweep, jacobian columns, force sweep, mass matrix, cholesky, proximity, total};
 * two-lanes-per-edge kernel (RKH_LANES_PER_EDGE = 2 in the environment): one record per wave of 32 states,
 * {frames + sincos, jacobian columns, mass matrix, force sweep, (assembly +) cholesky, proximity: joint frames, cull
 * (+ queueing), closed forms}. */
rkh_status rkh_diag_feval_cycles(rkh_scene* scene, const double* x, const double* u, uint32_t B, int iters,
                                 uint64_t* cycles);

/* GJK distance of n world-anchored shape pairs (a[i], b[i]), any kinds GJK knows (sphere, capped cylinder, box, mesh):
 * the check of the support-map query against the closed forms on primitive pairs. */
rkh_status rkh_diag_gjk_distance(rkh_ctx* ctx, const rkh_shape* a, const rkh_shape* b, uint32_t n,
                                 const double* mesh_vertices, uint32_t n_mesh_vertices, double* dist);
/* Its twin with the points: the record of the same search for each pair (gjk_record, reak_amd/csrc/gjk_device.h; the
 * definition is at rkh_min_distance_records_meshes in rkh.h).  dist[n] is rkh_diag_gjk_distance's value; point1[n][3] on
 * a[i], point2[n][3] on b[i], world frame. */
rkh_status rkh_diag_gjk_records(rkh_ctx* ctx, const rkh_shape* a, const rkh_shape* b, uint32_t n,
                                const double* mesh_vertices, uint32_t n_mesh_vertices, double* dist, double* point1,
                                double* point2);
/* And with the penetration depth and the contact normal: gjk_depth_record (reak_amd/csrc/epa_device.h; the definition is
 * at rkh_min_distance_records_depth in rkh.h) for each pair.  normal[n][3]: unit, from a[i] towards b[i]. */
rkh_status rkh_diag_gjk_depth_records(rkh_ctx* ctx, const rkh_shape* a, const rkh_shape* b, uint32_t n,
                                      const double* mesh_vertices, uint32_t n_mesh_vertices, double* dist, double* point1,
                                      double* point2, double* normal);

/* The planner-regime 1-NN sweep (half-precision mirror of the vertex rows + exact resolution of the one or two rows the
 * estimate leaves, reak_amd/csrc/nn_mirror.hip) on a caller's point cloud: n points [n][D], B queries [B][D], every
 * |coordinate| <= coord_bound, 1e-3 <= coord_bound <= 32 (else RKH_ERR_UNSUPPORTED), D <= 12.  The mirror is kept in
 * units of the power of two that brings coord_bound into [16, 32), so the cloud may fill the bound or be far smaller.
 * idx / dist: the nearest point of each query, first minimum wins (min_dist_linear_search,
 * topological_search.hpp:95-118), bit-identical to the fp64 sweeps (tests/test_nn_mirror_bounds_gpu.py). */
rkh_status rkh_diag_nn_mirror_query(rkh_ctx* ctx, const double* pts, uint64_t n, int D, const double* q, uint32_t B,
                                    double coord_bound, uint32_t* idx, double* dist);

/* With RKH_PROFILE_NN=1 in the environment at rkh_planner_create, every round brackets its NN sweep kernel with
 * HIP events on the planner stream: total kernel time, algorithmic bytes (n*D*8 per sweep) and launch count. */
rkh_status rkh_planner_nn_profile(rkh_planner* p, double* total_ms, uint64_t* total_bytes, uint64_t* launches);
/* Same profile: (vertex, query) pairs the profiled sweeps evaluated = sum over rounds and problems of n * B. */
rkh_status rkh_planner_nn_pairs(rkh_planner* p, uint64_t* pairs);
/* Same switch: HIP events around the steer launches (both kernel mappings) of every round: total time, rounds. */
rkh_status rkh_planner_steer_profile(rkh_planner* p, double* total_ms, uint64_t* launches);
/* Always on: RK4 steps the steer kernels of this planner integrated so far, over all edges (a step counts when it
 * starts from a live edge, the step that ends the edge included; steps skipped because the edge had ended do not).
 * The executed work of the steer launches -- an edge is launched for n_steps but stops at its first state that is not
 * free (MEAQR_topology.hpp:550-559). */
rkh_status rkh_planner_steer_steps(rkh_planner* p, uint64_t* executed_steps);
/* Samples the stream buffers of one problem hold at present (its sample stream and the two per-iteration logs): the
 * first buffers are ranges of the planner's arena, rkh_planner_sync replaces them with larger ones of their own. */
rkh_status rkh_diag_planner_sample_cap(rkh_planner* p, uint32_t problem, uint64_t* samples);

/* The proximity test of the two-lanes steer kernels on B states (2 n_dof doubles each), counting what reaches each of
 * its stages ("collide"): counts[0] = states tested, [1] = (robot shape, obstacle) pairs that pass the
 * static reach and the bounding cull, [2] = closed forms evaluated, [3] = golden-section searches (capped cylinder /
 * box), [4] = states found in collision, [5] = proxy pairs of the scene (the tests per state before any culling),
 * [6] = those within the shapes' static reach.  Scenes of the two-lanes mapping only (serial chains of 3, 6 or 7 joints,
 * revolute or prismatic). */
rkh_status rkh_diag_proximity_counts(rkh_scene* scene, const double* x, uint32_t B, uint64_t counts[8]);

/* The clearance bound the two-lanes steer kernels take out of that proximity test, per state (same device code): a
 * lower bound on the distance of the closest (robot shape, obstacle) pair, <= 0 when some pair passes the bounding cull
 * and in scenes the bound does not cover (branching or planar chains, prismatic joints, plane shapes), where the
 * kernels test every step.  out[B]. */
rkh_status rkh_diag_proximity_clearance(rkh_scene* scene, const double* x, uint32_t B, float* out);
/* Always on: what the carried bound saved in the two-lanes steer launches on this scene so far (rkh_propagate and the
 * planners created on it; planner launches are read after rkh_planner_sync).  counts[0] = edge-steps whose proximity
 * test the bound settled, counts[1] = wave-steps (32 edges) that ran the test.  RKH_STEER_CLEARANCE=0 in the
 * environment (read with the steer mapping's knobs) makes the kernels test every step. */
rkh_status rkh_diag_steer_clearance_counts(rkh_scene* scene, uint64_t counts[2]);
/* Always on: what the rounds of this planner did with the candidates they did not consume, summed over its problems
 * (waits for the planner's stream).  counts[0] = candidates discarded (a round of B candidates that consumes `cut` of
 * them discards B - cut; their samples come up again in the next round), counts[1] = candidates that took the stashed
 * result of such a discarded candidate instead of being steered again, because their nearest neighbour was still the
 * vertex the stashed edge started from (reak_amd/csrc/round_carry.h).  Only rounds that take the step-wise steer launch
 * with at least RKH_STEER_CARRY_MIN_EDGES edges (default: the built-in step-wise threshold) reuse; RKH_STEER_CARRY=0 in
 * the environment at rkh_planner_create* switches the reuse off. */
rkh_status rkh_diag_planner_carry_counts(rkh_planner* p, uint64_t counts[2]);

/* Goal probes of one problem of a batch RRT planner (waits for the planner's stream).  A vertex whose joint angles are
 * farther from the goal's than a steered edge can travel, plus 5 % of its distance to the goal, gets its goal-probe
 * result (+inf) when it is committed; only the other vertices' probes are steered (reak_amd/csrc/probe_reach.h).
 * counts[0] = probes settled at commit, counts[1] = probes a steer launch ran, counts[2] = probed_n (vertices
 * [1, probed_n) have their result), counts[3] = open probes waiting for a launch, counts[4] = the first vertex whose
 * probe is open (the vertex count if none is).  reach_q (may be null) = the travel bound in joint-angle norm, +inf where
 * the scene or the space gives no certificate or RKH_PROBE_REACH=0 was set at rkh_planner_create*.  Only rounds of at least
 * RKH_PROBE_REACH_MIN_EDGES edges (default: half the resident steer waves x 32 edges, the round carry's threshold)
 * settle probes. */
rkh_status rkh_diag_planner_probe_counts(rkh_planner* p, uint32_t problem, uint64_t counts[5], double* reach_q);

/* Kernel time of the distance query on B states: `runs` launches of rkh_min_distance's kernel (records == 0) or of
 * rkh_min_distance_records' (records != 0; on a planar scene rkh_min_distance_records_2d's, on a scene with mesh shapes
 * rkh_min_distance_records_meshes'; records == 2 on a 3D scene: rkh_min_distance_records_depth's) over the same device copy of x, each between two events on the context's stream; ms[runs] = the elapsed times.  No copies are timed
 * (tools/measure_record_query.py). */
rkh_status rkh_diag_distance_query_ms(rkh_scene* scene, const double* x, uint32_t B, int records, uint32_t runs, float* ms);

/* The roadmap search kernel (reak_amd/csrc/roadmap_paths.hip; the definition is at rkh_prm_shortest_paths in rkh.h) on a
 * caller's graph, so that graphs a planner never builds can be tested.  The graph is a CSR adjacency of n >= 1 vertices
 * (row_ptr[n + 1] ascending from 0, col / w [row_ptr[n]], col < n, w >= 0; an undirected edge is listed under both ends).
 * S searches run in one launch; search s starts from the seed list (seed_v[i], seed_d[i]), i in
 * [seed_ptr[s], seed_ptr[s + 1]): vertex seed_v[i] at distance seed_d[i] >= 0 (a roadmap vertex v as the source is the list
 * {(v, 0.0)}).  seed_mark[s] is the predecessor written where a seed is the vertex's distance: 0xFFFFFFFF for a vertex
 * source, RKH_PRM_QUERY_POINT for a query point's connections.  dist / pred [S][n] (either may be NULL), rounds [S] or
 * NULL: relaxation rounds each search ran.  Malformed input: RKH_ERR_BAD_ARG. */
rkh_status rkh_diag_sssp(rkh_ctx* ctx, uint32_t n, const uint32_t* row_ptr, const uint32_t* col, const double* w, uint32_t S,
                         const uint32_t* seed_ptr, const uint32_t* seed_v, const double* seed_d, const uint32_t* seed_mark,
                         double* dist, uint32_t* pred, uint32_t* rounds);
/* Time of the search launch alone on the roadmaps of a PRM handle (tools/measure_prm_queries.py).  problem == 0xFFFFFFFF:
 * one search from vertex 0 in every problem of the batch (the launch of rkh_prm_get_solution; sources / S unused);
 * else the S searches of rkh_prm_shortest_paths on that problem.  After one warm-up launch, `runs` launches, each between
 * two events on the handle's stream: ms[runs].  max_rounds: the most relaxation rounds any search took.  host_ms (may be
 * NULL): the time a single-thread std::priority_queue Dijkstra takes for the same searches over the same CSRs, once
 * (reference code for the comparison, not the code under test). */
rkh_status rkh_diag_prm_search_ms(rkh_prm* p, uint32_t problem, const uint32_t* sources, uint32_t S, uint32_t runs, float* ms,
                                  uint32_t* max_rounds, double* host_ms);

/* The search kernel of rkh_shortcut_paths (reak_amd/csrc/path_shortcut.hip; the definitions are at that entry in rkh.h) on
 * a caller's verdicts and weights, so that matrices no scene produces can be tested.  path_ptr [B + 1] as there (only the
 * lengths matter); ok / w hold one entry per candidate pair, path after path, each path's pairs in pair order (i ascending,
 * then j ascending, 1 <= j - i <= span): ok != 0 is a true strict verdict, w finite and >= 0.  Outputs as there.
 * RKH_ERR_BAD_ARG / RKH_ERR_CAPACITY as there, and BAD_ARG for a weight that is negative or not finite. */
rkh_status rkh_diag_shortcut_dp(rkh_ctx* ctx, const uint32_t* path_ptr, uint32_t B, uint32_t max_span,
                                const uint8_t* ok, const double* w, /* per candidate pair, in pair order */
                                uint32_t* keep, uint32_t* n_keep, double* cost_out, uint32_t* n_blocked);
/* Time of the three launches of rkh_shortcut_paths on the same arguments (tools/measure_shortcut.py): after one warm-up,
 * `runs` times the pair kernel, the walk launch and the search, each between two events on the context's stream:
 * ms[runs][3] = pairs, walks, search.  No copies are timed.  B > 0. */
rkh_status rkh_diag_shortcut_ms(rkh_scene* scene, const rkh_qs_space* space, const double* points, const uint32_t* path_ptr,
                                uint32_t B, uint32_t max_span, uint32_t runs, float* ms /* [runs][3] */);
/* Times of the kinematics launches on the same arguments (tools/measure_kinematics.py), events on the context's stream,
 * after one warm-up; no copies are timed.  rkh_diag_kinematics_ms: the one launch that answers rkh_direct_kinematics AND
 * rkh_jacobians (all six outputs, JacDot included; planar scenes: the _2d forms) with the clear of the two Jacobian arrays
 * in front of it, ms[runs].  rkh_diag_ik_ms: rkh_inverse_kinematics' solve launch and its distance launch,
 * ms[runs][2] = solves, distance query (0 for a scene without proxy pairs).  B, F, T, S, runs > 0. */
rkh_status rkh_diag_kinematics_ms(rkh_scene* scene, const double* q, const double* qd, uint32_t B, const int32_t* frames,
                                  uint32_t F, uint32_t runs, float* ms /* [runs] */);
rkh_status rkh_diag_ik_ms(rkh_scene* scene, int32_t frame, const rkh_pose* targets, uint32_t T, const double* seeds, uint32_t S,
                          const double* lower, const double* upper, const rkh_ik_params* params, uint32_t runs,
                          float* ms /* [runs][2] */);
/* The split of the batch SVP RRT's rounds (tools/measure_svp_rrt.py): enable = 1 brackets the phases of every later round
 * of the planner with events on the context's stream; ms (may be NULL) receives the totals so far of {sample, nearest +
 * steer, extension walk, commit, probe walk, finish} in milliseconds (the walks include their read-backs). */
rkh_status rkh_diag_svp_rrt_profile(rkh_svp_rrt* planner, int32_t enable, double* ms /* [6] */);
/* rkh_svp_shortcut_paths (rkh.h) with the chunk size as an argument: the candidate pairs go through the walk's workspace
 * chunk_pairs at a time (the entry itself uses 262 144), so that tests can put chunk boundaries inside a path's rows and
 * between paths.  chunk_pairs in [1, 16 777 216]; everything else, results included, as there. */
rkh_status rkh_diag_svp_shortcut_chunked(rkh_scene* scene, const rkh_svp_space* space, const double* points,
                                         const uint32_t* path_ptr, uint32_t B, uint32_t max_span, uint32_t chunk_pairs,
                                         uint32_t* keep, uint32_t* n_keep, double* time_in, double* time_out,
                                         uint32_t* n_blocked);
/* Time of the phases of rkh_svp_shortcut_paths on the same arguments (tools/measure_svp_shortcut.py): after one warm-up
 * of the whole sequence, `runs` times the pair kernel, the walk (its launches and the read-back of the live count per pass)
 * and the search with the input-time kernel, each between two events on the context's stream and summed over the chunks:
 * ms[runs][3] = pairs, walks, search.  The copies of the call are not timed.  B > 0. */
rkh_status rkh_diag_svp_shortcut_ms(rkh_scene* scene, const rkh_svp_space* space, const double* points, const uint32_t* path_ptr,
                                    uint32_t B, uint32_t max_span, uint32_t runs, float* ms /* [runs][3] */);
/* The directed walk launch with a direction byte per row from the host: back[e] != 0 walks row e as
 * rkh_svp_edge_check_back does, 0 as rkh_svp_edge_check does, bit for bit, in one launch; back NULL: every row forward.
 * Everything else as rkh_svp_edge_check.  For the tests and the measurement of launches that hold both directions (the
 * rounds of rkh_svp_birrt_*). */
rkh_status rkh_diag_svp_edge_check_dir(rkh_scene* scene, const rkh_svp_space* space, const double* a, const double* b, uint32_t B,
                                       const double* fraction /* [B], NULL = 1.0 */, const uint8_t* back /* [B] */,
                                       double* out /* [B][2 n_dof] */, double* reach_time /* [B] */,
                                       uint32_t* n_checked /* [B] */, uint8_t* reached /* [B] */);
/* The split of the batch bidirectional SVP RRT's rounds (tools/measure_svp_birrt.py), as rkh_diag_svp_rrt_profile: ms (may
 * be NULL) receives the totals so far of {sample, nearest, steer, walk, commit} in milliseconds (the walk includes its
 * read-backs). */
rkh_status rkh_diag_svp_birrt_profile(rkh_svp_birrt* planner, int32_t enable, double* ms /* [5] */);

#ifdef __cplusplus
}
#endif
#endif
