"""ctypes binding of the C-ABI in include/rkh.h (reak_amd/librkh.so = hand-written HIP kernels, gfx950).

There is no CPU fallback: if the shared library is missing or the GPU is absent the calls fail loudly.
The classes mirror the reference interfaces the kernels replace (paths relative to /root/reference/src/ReaK/):
  HipNeighborSearch  ~ linear_neighbor_search + any_knn_synchro  (ctrl/path_planning/topological_search.hpp:529-690)
  Scene              ~ kte_map_chain + mass_matrix_calc + proxy_query_pair_3D
  RrtPlanner         ~ rrt_planner::solve_planning_query          (ctrl/path_planning/rrt_path_planner.tpp:66-145)
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import types as T

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "librkh.so")

RKH_OK = 0
STATUS_NAMES = {0: "RKH_OK", -1: "RKH_ERR_BAD_ARG", -2: "RKH_ERR_OOM", -3: "RKH_ERR_SINGULAR", -4: "RKH_ERR_DEVICE",
                -5: "RKH_ERR_UNSUPPORTED", -6: "RKH_ERR_CAPACITY"}


class RkhError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {msg}")
        self.status = status


class SingularityError(RkhError):
    """singularity_error of the reference (core/lin_alg/mat_num_exceptions.hpp), status RKH_ERR_SINGULAR."""


class RrtStarStats(C.Structure):
    _fields_ = [("num_vertices", C.c_uint64), ("samples", C.c_uint64), ("loop_iterations", C.c_uint64),
                ("num_solutions", C.c_uint64), ("rewires", C.c_uint64), ("edges_checked", C.c_uint64),
                ("best_cost", C.c_double), ("pruned", C.c_uint64), ("skipped", C.c_uint64)]


class PrmStats(C.Structure):
    _fields_ = [("num_vertices", C.c_uint64), ("num_edges", C.c_uint64), ("samples", C.c_uint64),
                ("rejected", C.c_uint64), ("loop_iterations", C.c_uint64), ("num_components", C.c_uint64),
                ("publish_calls", C.c_uint64), ("merged_at_vertex", C.c_int64), ("edges_checked", C.c_uint64),
                ("device_steps", C.c_uint64)]


class BiRrtStats(C.Structure):
    _fields_ = [("num_vertices_1", C.c_uint64), ("num_vertices_2", C.c_uint64), ("loop_iterations", C.c_uint64),
                ("samples", C.c_uint64), ("num_solutions", C.c_uint64), ("joins", C.c_uint64),
                ("edges_checked", C.c_uint64), ("best_cost", C.c_double)]


class SvpRrtStats(C.Structure):
    """rkh_svp_rrt_stats (include/rkh.h): totals since the planner was created."""
    _fields_ = [("rounds", C.c_uint64), ("problems_finished", C.c_uint64), ("iterations", C.c_uint64),
                ("vertices", C.c_uint64), ("walk_passes", C.c_uint64), ("tested_points", C.c_uint64),
                ("window_refills", C.c_uint64)]


class PlannerStats(C.Structure):
    _fields_ = [
        ("num_vertices", C.c_uint64),
        ("iterations", C.c_uint64),
        ("edges_checked", C.c_uint64),
        ("edges_speculated", C.c_uint64),
        ("rounds", C.c_uint64),
        ("num_solutions", C.c_uint64),
        ("best_cost", C.c_double),
        ("done", C.c_uint32),
    ]


ABI_VERSION = 3  # RKH_ABI_VERSION of include/rkh.h this binding mirrors


def abi_sizes():
    """sizeof of the mirrored PODs, in the argument order of rkh_abi_check."""
    return [C.sizeof(T.DynSpace), C.sizeof(T.QsSpace), C.sizeof(T.RrtParams), C.sizeof(T.PrmParams), C.sizeof(PlannerStats),
            C.sizeof(RrtStarStats), C.sizeof(PrmStats), C.sizeof(BiRrtStats), C.sizeof(T.Shape), C.sizeof(T.KteOp)]


EXPORTS = [
    "rkh_last_error", "rkh_version", "rkh_abi_version", "rkh_abi_check", "rkh_ctx_create", "rkh_ctx_destroy", "rkh_ctx_synchronize", "rkh_ctx_stream",
    "rkh_ctx_release_cached_memory", "rkh_diag_planner_sample_cap",
    "rkh_nn_create", "rkh_nn_destroy", "rkh_nn_clear", "rkh_nn_size", "rkh_nn_remove", "rkh_nn_live_size", "rkh_nn_append", "rkh_nn_query1",
    "rkh_nn_queryk", "rkh_nn_query1_async", "rkh_nn_queryk_async", "rkh_nn_fill_uniform", "rkh_nn_kernel_name",
    "rkh_diag_knn_retries",
    "rkh_steer_mapping_name",
    "rkh_nn_set_coord_bound",
    "rkh_scene_create", "rkh_scene_create_with_meshes", "rkh_diag_gjk_distance", "rkh_diag_gjk_records", "rkh_diag_gjk_depth_records", "rkh_scene_destroy", "rkh_scene_num_dof", "rkh_scene_num_pairs", "rkh_state_derivative",
    "rkh_min_distance", "rkh_min_distance_records", "rkh_collision_records", "rkh_min_distance_records_meshes", "rkh_collision_records_meshes", "rkh_min_distance_records_depth", "rkh_collision_records_depth", "rkh_min_distance_records_2d", "rkh_collision_records_2d", "rkh_propagate", "rkh_edge_check", "rkh_planner_create", "rkh_planner_destroy",
    "rkh_planner_enqueue", "rkh_planner_sync", "rkh_planner_solve", "rkh_planner_get_tree", "rkh_planner_stream",
    "rkh_planner_nn_profile", "rkh_planner_nn_pairs", "rkh_planner_steer_profile", "rkh_planner_steer_steps", "rkh_diag_nn_mirror_query", "rkh_diag_feval_cycles", "rkh_diag_proximity_counts", "rkh_diag_distance_query_ms", "rkh_diag_proximity_clearance", "rkh_diag_steer_clearance_counts", "rkh_diag_planner_carry_counts", "rkh_diag_planner_probe_counts", "rkh_planner_create_batch", "rkh_planner_num_problems", "rkh_nn_set_events", "rkh_planner_create_qs_batch", "rkh_rrtstar_create_qs_batch", "rkh_rrtstar_create_batch", "rkh_birrtstar_create_qs_batch", "rkh_birrtstar_solve",
    "rkh_birrtstar_get_graph", "rkh_rrtstar_set_branch_and_bound", "rkh_rrtstar_get_removed", "rkh_rrtstar_destroy", "rkh_rrtstar_solve",
    "rkh_rrtstar_get_graph", "rkh_prm_create_qs_batch", "rkh_prm_create_batch", "rkh_prm_destroy", "rkh_prm_solve", "rkh_prm_get_graph", "rkh_prm_shortest_paths", "rkh_prm_get_solution", "rkh_prm_query_paths", "rkh_diag_sssp", "rkh_diag_prm_search_ms", "rkh_birrt_create_qs_batch", "rkh_birrt_destroy", "rkh_birrt_solve", "rkh_birrt_get_trees", "rkh_planner_get_solution", "rkh_rrtstar_get_solution", "rkh_birrt_get_solution",
    "rkh_shortcut_paths", "rkh_diag_shortcut_dp", "rkh_diag_shortcut_ms",
    "rkh_direct_kinematics", "rkh_direct_kinematics_2d", "rkh_jacobians", "rkh_jacobians_2d", "rkh_inverse_kinematics",
    "rkh_diag_kinematics_ms", "rkh_diag_ik_ms",
    "rkh_svp_in_bounds", "rkh_svp_reach_time", "rkh_svp_nearest", "rkh_svp_nearest_async", "rkh_svp_edge_check",
    "rkh_svp_interpolate",
    "rkh_svp_rrt_create_batch", "rkh_svp_rrt_destroy", "rkh_svp_rrt_solve", "rkh_svp_rrt_get_status", "rkh_svp_rrt_get_tree",
    "rkh_svp_rrt_get_solution", "rkh_diag_svp_rrt_profile",
    "rkh_svp_shortcut_paths", "rkh_diag_svp_shortcut_chunked", "rkh_diag_svp_shortcut_ms",
    "rkh_svp_edge_check_back", "rkh_diag_svp_edge_check_dir",
    "rkh_svp_birrt_create_batch", "rkh_svp_birrt_destroy", "rkh_svp_birrt_solve", "rkh_svp_birrt_get_status",
    "rkh_svp_birrt_get_tree", "rkh_svp_birrt_get_solution", "rkh_diag_svp_birrt_profile",
]


def build(verbose=False):
    """Compile every HIP source for gfx950 into reak_amd/librkh.so and the library it loads from its own directory,
    librkh_prismatic_pair.so (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-s", "-C", os.path.join(_HERE, "csrc")], check=True,
                   stdout=None if verbose else subprocess.DEVNULL, stderr=None if verbose else subprocess.DEVNULL)
    return _LIB_PATH


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(f"{_LIB_PATH} is missing: run reak_amd.lib.build() (or __graft_entry__.build()); "
                           "there is no CPU fallback for the HIP path")
    lib = C.CDLL(_LIB_PATH)
    vp, d, dp, u32, u32p, u64 = C.c_void_p, C.c_double, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint64
    lib.rkh_last_error.restype = C.c_char_p
    lib.rkh_version.restype = C.c_char_p
    lib.rkh_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.rkh_ctx_destroy.argtypes = [vp]
    lib.rkh_ctx_synchronize.argtypes = [vp]
    lib.rkh_ctx_stream.restype = vp
    lib.rkh_ctx_stream.argtypes = [vp]
    lib.rkh_ctx_release_cached_memory.argtypes = [vp]
    lib.rkh_nn_create.argtypes = [vp, C.c_int, u64, C.POINTER(vp)]
    lib.rkh_nn_destroy.argtypes = [vp]
    lib.rkh_nn_clear.argtypes = [vp]
    lib.rkh_nn_size.restype = u64
    lib.rkh_nn_size.argtypes = [vp]
    lib.rkh_nn_remove.argtypes = [vp, u64]
    lib.rkh_nn_live_size.restype = u64
    lib.rkh_nn_live_size.argtypes = [vp]
    lib.rkh_nn_append.argtypes = [vp, dp, u64]
    lib.rkh_nn_query1.argtypes = [vp, dp, u32, u32p, dp]
    lib.rkh_nn_queryk.argtypes = [vp, dp, u32, u32, d, u32p, dp, u32p]
    lib.rkh_nn_query1_async.argtypes = [vp, vp, u32, vp, vp]
    lib.rkh_nn_queryk_async.argtypes = [vp, vp, u32, u32, d, vp, vp, vp]
    lib.rkh_nn_fill_uniform.argtypes = [vp, u64, u64]
    lib.rkh_nn_set_coord_bound.argtypes = [vp, C.c_double]
    lib.rkh_nn_set_events.argtypes = [vp, vp, vp]
    lib.rkh_nn_kernel_name.restype = C.c_char_p
    lib.rkh_diag_knn_retries.restype = u64
    lib.rkh_diag_knn_retries.argtypes = []
    lib.rkh_steer_mapping_name.restype = C.c_char_p
    lib.rkh_scene_create.argtypes = [vp, C.POINTER(T.KteOp), C.c_int, C.POINTER(T.ChainBase), C.POINTER(T.Shape), C.c_int,
                                     C.POINTER(vp)]
    lib.rkh_scene_create_with_meshes.argtypes = [vp, C.POINTER(T.KteOp), C.c_int, C.POINTER(T.ChainBase), C.POINTER(T.Shape),
                                                 C.c_int, dp, u32, C.POINTER(vp)]
    lib.rkh_diag_gjk_distance.argtypes = [vp, C.POINTER(T.Shape), C.POINTER(T.Shape), u32, dp, u32, dp]
    lib.rkh_diag_gjk_records.argtypes = [vp, C.POINTER(T.Shape), C.POINTER(T.Shape), u32, dp, u32, dp, dp, dp]
    lib.rkh_diag_gjk_depth_records.argtypes = [vp, C.POINTER(T.Shape), C.POINTER(T.Shape), u32, dp, u32, dp, dp, dp, dp]
    lib.rkh_scene_destroy.argtypes = [vp]
    lib.rkh_scene_num_dof.argtypes = [vp]
    lib.rkh_scene_num_pairs.argtypes = [vp]
    lib.rkh_state_derivative.argtypes = [vp, dp, dp, u32, dp, dp, dp]
    lib.rkh_min_distance.argtypes = [vp, dp, u32, dp]
    lib.rkh_min_distance_records.argtypes = [vp, dp, u32, dp, dp, dp, u32p, u32p]
    lib.rkh_collision_records.argtypes = [vp, dp, u32, u32, u32p, dp, dp, dp, u32p, u32p]
    lib.rkh_min_distance_records_meshes.argtypes = [vp, dp, u32, dp, dp, dp, u32p, u32p]
    lib.rkh_collision_records_meshes.argtypes = [vp, dp, u32, u32, u32p, dp, dp, dp, u32p, u32p]
    lib.rkh_min_distance_records_depth.argtypes = [vp, dp, u32, dp, dp, dp, dp, u32p, u32p]
    lib.rkh_collision_records_depth.argtypes = [vp, dp, u32, u32, u32p, dp, dp, dp, dp, u32p, u32p]
    lib.rkh_min_distance_records_2d.argtypes = [vp, dp, u32, dp, dp, dp, u32p, u32p]
    lib.rkh_collision_records_2d.argtypes = [vp, dp, u32, u32, u32p, dp, dp, dp, u32p, u32p]
    lib.rkh_diag_distance_query_ms.argtypes = [vp, dp, u32, C.c_int, u32, C.POINTER(C.c_float)]
    lib.rkh_propagate.argtypes = [vp, C.POINTER(T.DynSpace), dp, dp, u32, d, dp, u32p, dp]
    lib.rkh_diag_feval_cycles.argtypes = [vp, dp, dp, u32, C.c_int, C.POINTER(C.c_uint64)]
    lib.rkh_diag_proximity_counts.argtypes = [vp, dp, u32, C.POINTER(C.c_uint64)]
    lib.rkh_diag_proximity_clearance.argtypes = [vp, dp, u32, C.POINTER(C.c_float)]
    lib.rkh_diag_steer_clearance_counts.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.rkh_edge_check.argtypes = [vp, dp, dp, d, dp, dp, u32, d, dp, u32p]
    lib.rkh_planner_create.argtypes = [vp, C.POINTER(T.DynSpace), C.POINTER(T.RrtParams), C.POINTER(vp)]
    lib.rkh_planner_create_batch.argtypes = [vp, C.POINTER(T.DynSpace), C.POINTER(T.RrtParams), u32, C.POINTER(vp)]
    lib.rkh_planner_create_qs_batch.argtypes = [vp, C.POINTER(T.QsSpace), C.POINTER(T.RrtParams), u32, C.POINTER(vp)]
    lib.rkh_rrtstar_create_qs_batch.argtypes = [vp, C.POINTER(T.QsSpace), C.POINTER(T.RrtParams), u32, C.POINTER(vp)]
    lib.rkh_rrtstar_destroy.argtypes = [vp]
    lib.rkh_rrtstar_solve.argtypes = [vp, C.c_int64, C.POINTER(RrtStarStats)]
    lib.rkh_rrtstar_get_graph.argtypes = [vp, u32, dp, u32p, dp, u32p]
    lib.rkh_rrtstar_set_branch_and_bound.argtypes = [vp, C.c_int]
    lib.rkh_rrtstar_get_removed.argtypes = [vp, u32, C.POINTER(C.c_uint8)]
    lib.rkh_birrtstar_solve.argtypes = [vp, C.c_int64, C.POINTER(BiRrtStarStats)]
    lib.rkh_birrtstar_get_graph.argtypes = [vp, u32, dp, u32p, dp, u32p, dp, u32p, u32p]
    lib.rkh_prm_create_qs_batch.argtypes = [vp, C.POINTER(T.QsSpace), C.POINTER(T.PrmParams), u32, C.POINTER(vp)]
    lib.rkh_prm_destroy.argtypes = [vp]
    lib.rkh_prm_solve.argtypes = [vp, C.c_int64, C.POINTER(PrmStats)]
    lib.rkh_planner_get_solution.argtypes = [vp, u32, u32p, u32, u32p, dp]
    lib.rkh_rrtstar_get_solution.argtypes = [vp, u32, u32p, u32, u32p, dp]
    lib.rkh_birrt_get_solution.argtypes = [vp, u32, u32p, u32p, u32p, u32p, u32, dp]
    lib.rkh_birrt_create_qs_batch.argtypes = [vp, C.POINTER(T.QsSpace), C.POINTER(T.RrtParams), u32, C.POINTER(vp)]
    lib.rkh_birrt_destroy.argtypes = [vp]
    lib.rkh_birrt_solve.argtypes = [vp, C.c_int64, C.POINTER(BiRrtStats)]
    lib.rkh_birrt_get_trees.argtypes = [vp, u32, dp, u32p, dp, u32p, u32p, C.POINTER(C.c_uint8)]
    lib.rkh_prm_get_graph.argtypes = [vp, u32, dp, u32p, u32p, dp, dp, u32p, C.POINTER(C.c_uint8), u32p]
    lib.rkh_prm_shortest_paths.argtypes = [vp, u32, u32p, u32, dp, u32p]
    lib.rkh_prm_get_solution.argtypes = [vp, u32, u32p, u32, u32p, dp]
    lib.rkh_prm_query_paths.argtypes = [vp, u32, dp, dp, u32, u32, d, u32, dp, u32p, u32p]
    lib.rkh_diag_sssp.argtypes = [vp, u32, u32p, u32p, dp, u32, u32p, u32p, dp, u32p, dp, u32p, u32p]
    lib.rkh_diag_prm_search_ms.argtypes = [vp, u32, u32p, u32, u32, C.POINTER(C.c_float), u32p, dp]
    u8p = C.POINTER(C.c_uint8)
    lib.rkh_shortcut_paths.argtypes = [vp, C.POINTER(T.QsSpace), dp, u32p, u32, u32, u32p, u32p, dp, dp, u32p]
    lib.rkh_diag_shortcut_dp.argtypes = [vp, u32p, u32, u32, u8p, dp, u32p, u32p, dp, u32p]
    lib.rkh_diag_shortcut_ms.argtypes = [vp, C.POINTER(T.QsSpace), dp, u32p, u32, u32, u32, C.POINTER(C.c_float)]
    i32p = C.POINTER(C.c_int32)
    lib.rkh_direct_kinematics.argtypes = [vp, dp, dp, u32, i32p, u32, dp, dp, dp, dp]
    lib.rkh_direct_kinematics_2d.argtypes = [vp, dp, dp, u32, i32p, u32, dp, dp, dp, dp]
    lib.rkh_jacobians.argtypes = [vp, dp, dp, u32, i32p, u32, dp, dp]
    lib.rkh_jacobians_2d.argtypes = [vp, dp, dp, u32, i32p, u32, dp, dp]
    lib.rkh_inverse_kinematics.argtypes = [vp, C.c_int32, C.POINTER(T.Pose), u32, dp, u32, dp, dp, C.POINTER(T.IkParams), dp, dp,
                                           dp, u32p, u32p, u32p]
    lib.rkh_diag_kinematics_ms.argtypes = [vp, dp, dp, u32, i32p, u32, u32, C.POINTER(C.c_float)]
    lib.rkh_diag_ik_ms.argtypes = [vp, C.c_int32, C.POINTER(T.Pose), u32, dp, u32, dp, dp, C.POINTER(T.IkParams), u32,
                                   C.POINTER(C.c_float)]
    svp = C.POINTER(T.SvpSpace)
    lib.rkh_svp_in_bounds.argtypes = [svp, dp, u32, u8p]
    lib.rkh_svp_reach_time.argtypes = [vp, svp, dp, dp, u32, dp, dp]
    lib.rkh_svp_nearest.argtypes = [vp, svp, dp, u32, dp, u32, u32, C.c_int32, u32p, dp]
    lib.rkh_svp_nearest_async.argtypes = [vp, svp, vp, u32, vp, u32, u32, C.c_int32, vp, vp]
    lib.rkh_svp_edge_check.argtypes = [vp, svp, dp, dp, u32, dp, dp, dp, u32p, u8p]
    lib.rkh_svp_interpolate.argtypes = [vp, svp, dp, dp, u32, dp, u32, dp, dp]
    lib.rkh_svp_rrt_create_batch.argtypes = [vp, svp, C.POINTER(T.SvpRrtParams), u32, C.POINTER(vp)]
    lib.rkh_svp_rrt_destroy.argtypes = [vp]
    lib.rkh_svp_rrt_destroy.restype = None
    lib.rkh_svp_rrt_solve.argtypes = [vp, C.c_int64, C.POINTER(SvpRrtStats)]
    lib.rkh_svp_rrt_get_status.argtypes = [vp, u32p, u32p, u32p]
    lib.rkh_svp_rrt_get_tree.argtypes = [vp, u32, dp, u32p, dp, u32, u32p]
    lib.rkh_svp_rrt_get_solution.argtypes = [vp, u32, dp, u32, u32p, dp]
    lib.rkh_diag_svp_rrt_profile.argtypes = [vp, C.c_int32, dp]
    lib.rkh_svp_shortcut_paths.argtypes = [vp, svp, dp, u32p, u32, u32, u32p, u32p, dp, dp, u32p]
    lib.rkh_diag_svp_shortcut_chunked.argtypes = [vp, svp, dp, u32p, u32, u32, u32, u32p, u32p, dp, dp, u32p]
    lib.rkh_diag_svp_shortcut_ms.argtypes = [vp, svp, dp, u32p, u32, u32, u32, C.POINTER(C.c_float)]
    lib.rkh_svp_edge_check_back.argtypes = [vp, svp, dp, dp, u32, dp, dp, dp, u32p, u8p]
    lib.rkh_diag_svp_edge_check_dir.argtypes = [vp, svp, dp, dp, u32, dp, u8p, dp, dp, u32p, u8p]
    lib.rkh_svp_birrt_create_batch.argtypes = [vp, svp, C.POINTER(T.SvpRrtParams), u32, C.POINTER(vp)]
    lib.rkh_svp_birrt_destroy.argtypes = [vp]
    lib.rkh_svp_birrt_destroy.restype = None
    lib.rkh_svp_birrt_solve.argtypes = [vp, C.c_int64, C.POINTER(SvpRrtStats)]
    lib.rkh_svp_birrt_get_status.argtypes = [vp, u32p, u32p, u32p, u32p, u32p]
    lib.rkh_svp_birrt_get_tree.argtypes = [vp, u32, u32, dp, u32p, dp, u32, u32p]
    lib.rkh_svp_birrt_get_solution.argtypes = [vp, u32, dp, u32, u32p, dp]
    lib.rkh_diag_svp_birrt_profile.argtypes = [vp, C.c_int32, dp]
    lib.rkh_planner_num_problems.restype = u32
    lib.rkh_planner_num_problems.argtypes = [vp]
    lib.rkh_planner_destroy.argtypes = [vp]
    lib.rkh_planner_enqueue.argtypes = [vp, u32]
    lib.rkh_planner_sync.argtypes = [vp, C.POINTER(PlannerStats)]
    lib.rkh_planner_solve.argtypes = [vp, C.POINTER(PlannerStats)]
    lib.rkh_planner_get_tree.argtypes = [vp, u32, dp, u32p, u32p, C.POINTER(C.c_uint8), dp]
    lib.rkh_planner_stream.restype = vp
    lib.rkh_planner_stream.argtypes = [vp]
    lib.rkh_planner_nn_profile.argtypes = [vp, dp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.rkh_planner_nn_pairs.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.rkh_planner_steer_profile.argtypes = [vp, dp, C.POINTER(C.c_uint64)]
    lib.rkh_planner_steer_steps.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.rkh_diag_planner_sample_cap.argtypes = [vp, u32, C.POINTER(C.c_uint64)]
    lib.rkh_diag_planner_carry_counts.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.rkh_diag_planner_probe_counts.argtypes = [vp, u32, C.POINTER(C.c_uint64), dp]
    lib.rkh_diag_nn_mirror_query.argtypes = [vp, dp, C.c_uint64, C.c_int, dp, C.c_uint32, C.c_double, C.POINTER(C.c_uint32), dp]
    lib.rkh_abi_version.restype = C.c_uint32
    lib.rkh_abi_check.argtypes = [C.c_uint32] + [C.c_size_t] * 10
    # the handshake of include/rkh.h: this binding's struct mirrors against the library's (RKH_ABI_CHECK)
    st = lib.rkh_abi_check(ABI_VERSION, *abi_sizes())
    if st != 0:
        raise RkhError(st, lib.rkh_last_error().decode())
    _lib = lib
    return lib


def _check(status):
    if status != RKH_OK:
        msg = load().rkh_last_error().decode()
        if status == -3:
            raise SingularityError(status, msg)
        raise RkhError(status, msg)


def diag_sssp(ctx, row_ptr, col, w, seed_lists, seed_marks):
    """rkh_diag_sssp: the roadmap search kernel on a caller's CSR graph.  seed_lists: one list of (vertex, distance) per
    search; seed_marks: the predecessor written where a seed is the distance.  Returns (dist [S][n], pred [S][n], rounds [S])."""
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint32)
    col = np.ascontiguousarray(col, dtype=np.uint32)
    w = np.ascontiguousarray(w, dtype=np.float64)
    n, S = len(row_ptr) - 1, len(seed_lists)
    seed_ptr = np.zeros(S + 1, dtype=np.uint32)
    seed_ptr[1:] = np.cumsum([len(sl) for sl in seed_lists])
    seed_v = np.array([v for sl in seed_lists for v, _ in sl] + [0], dtype=np.uint32)
    seed_d = np.array([x for sl in seed_lists for _, x in sl] + [0.0], dtype=np.float64)
    marks = np.ascontiguousarray(seed_marks, dtype=np.uint32)
    dist = np.zeros((S, n))
    pred = np.zeros((S, n), dtype=np.uint32)
    rounds = np.zeros(max(S, 1), dtype=np.uint32)
    colp = np.concatenate([col, np.zeros(1, np.uint32)])  # (never an empty buffer)
    wp = np.concatenate([w, np.zeros(1)])
    _check(ctx.lib.rkh_diag_sssp(ctx.h, n, T.u32ptr(row_ptr), T.u32ptr(colp), T.dptr(wp), S, T.u32ptr(seed_ptr), T.u32ptr(seed_v),
                                 T.dptr(seed_d), T.u32ptr(marks), T.dptr(dist), T.u32ptr(pred), T.u32ptr(rounds)))
    return dist, pred, rounds[:S]


def _path_table(paths, n):
    """(points [sum L][n], path_ptr [B + 1]) of a list of [L][n] arrays"""
    paths = [np.ascontiguousarray(p, dtype=np.float64).reshape(-1, n) for p in paths]
    path_ptr = np.zeros(len(paths) + 1, dtype=np.uint32)
    path_ptr[1:] = np.cumsum([len(p) for p in paths])
    pts = np.concatenate(paths + [np.zeros((1, n))])  # (never an empty buffer)
    return np.ascontiguousarray(pts), path_ptr


def _keep_lists(keep, n_keep, path_ptr):
    return [keep[path_ptr[b]:path_ptr[b] + n_keep[b]].copy() for b in range(len(n_keep))]


def diag_shortcut_dp(ctx, lengths, ok, w, max_span=0):
    """rkh_diag_shortcut_dp: the search kernel of rkh_shortcut_paths on a caller's verdicts and weights.  lengths: the
    point count of each path; ok / w: one entry per candidate pair, path after path, in pair order.  Returns
    (keep lists, cost_out [B], n_blocked [B])."""
    B = len(lengths)
    path_ptr = np.zeros(B + 1, dtype=np.uint32)
    path_ptr[1:] = np.cumsum(lengths)
    ok = np.concatenate([np.ascontiguousarray(ok, dtype=np.uint8).reshape(-1), np.zeros(1, np.uint8)])
    w = np.concatenate([np.ascontiguousarray(w, dtype=np.float64).reshape(-1), np.zeros(1)])
    keep = np.zeros(max(int(path_ptr[B]), 1), dtype=np.uint32)
    n_keep, n_blocked = np.zeros(max(B, 1), dtype=np.uint32), np.zeros(max(B, 1), dtype=np.uint32)
    cost_out = np.zeros(max(B, 1))
    _check(ctx.lib.rkh_diag_shortcut_dp(ctx.h, T.u32ptr(path_ptr), B, int(max_span), ok.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        T.dptr(w), T.u32ptr(keep), T.u32ptr(n_keep), T.dptr(cost_out), T.u32ptr(n_blocked)))
    return _keep_lists(keep, n_keep[:B], path_ptr), cost_out[:B], n_blocked[:B]


def path_points(pos, indices, start=None, goal=None):
    """The points of a planner's solution as rkh_shortcut_paths takes them: the rows of `pos` (a planner's vertex
    positions) picked by the solution's vertex indices, with an off-roadmap start point in front and goal point behind
    (the query points of PrmPlanner.query_paths)."""
    pos = np.asarray(pos, dtype=np.float64)
    rows = [pos[np.asarray(indices, dtype=np.int64)].reshape(-1, pos.shape[1])]
    if start is not None:
        rows.insert(0, np.asarray(start, dtype=np.float64).reshape(1, -1))
    if goal is not None:
        rows.append(np.asarray(goal, dtype=np.float64).reshape(1, -1))
    return np.ascontiguousarray(np.concatenate(rows))


class Context:
    def __init__(self, device=0):
        self.lib = load()
        self.h = C.c_void_p()
        _check(self.lib.rkh_ctx_create(device, C.byref(self.h)))
        self.device = device

    def synchronize(self):
        _check(self.lib.rkh_ctx_synchronize(self.h))

    @property
    def stream(self):
        return self.lib.rkh_ctx_stream(self.h)

    def release_cached_memory(self):
        """Free the device memory of closed batch planners that the context keeps for the next one."""
        _check(self.lib.rkh_ctx_release_cached_memory(self.h))

    def close(self):
        if self.h:
            self.lib.rkh_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipNeighborSearch:
    """Exact brute-force NN over a growing vertex set kept in HBM (NNFinder + KNN synchro)."""

    def __init__(self, ctx, dims, capacity):
        self.ctx, self.lib, self.D = ctx, ctx.lib, dims
        self.h = C.c_void_p()
        _check(self.lib.rkh_nn_create(ctx.h, dims, capacity, C.byref(self.h)))

    def __len__(self):
        return int(self.lib.rkh_nn_size(self.h))

    def added_vertices(self, pts):
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, self.D)
        _check(self.lib.rkh_nn_append(self.h, T.dptr(pts), pts.shape[0]))

    def removed_vertex(self, index):
        _check(self.lib.rkh_nn_remove(self.h, int(index)))

    def live_size(self):
        return int(self.lib.rkh_nn_live_size(self.h))

    def clear(self):
        _check(self.lib.rkh_nn_clear(self.h))

    def set_coord_bound(self, bound):
        _check(self.lib.rkh_nn_set_coord_bound(self.h, float(bound)))

    def kernel_name(self):
        return self.lib.rkh_nn_kernel_name().decode()

    def fill_uniform(self, n, seed=1):
        _check(self.lib.rkh_nn_fill_uniform(self.h, n, seed))

    def nearest(self, q):
        q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, self.D)
        B = q.shape[0]
        idx = np.zeros(B, dtype=np.uint32)
        dist = np.zeros(B)
        _check(self.lib.rkh_nn_query1(self.h, T.dptr(q), B, T.u32ptr(idx), T.dptr(dist)))
        return idx, dist

    def nearest_async(self, d_q, B, d_idx, d_dist, events=None):
        if events is not None:
            _check(self.lib.rkh_nn_set_events(self.h, events[0], events[1]))
        _check(self.lib.rkh_nn_query1_async(self.h, d_q, B, d_idx, d_dist))

    def k_nearest(self, q, k, radius=np.inf):
        q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, self.D)
        B = q.shape[0]
        idx = np.zeros((B, k), dtype=np.uint32)
        dist = np.zeros((B, k))
        cnt = np.zeros(B, dtype=np.uint32)
        _check(self.lib.rkh_nn_queryk(self.h, T.dptr(q), B, k, float(radius), T.u32ptr(idx), T.dptr(dist), T.u32ptr(cnt)))
        return idx, dist, cnt

    def close(self):
        if self.h:
            self.lib.rkh_nn_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def steer_mapping_name():
    """The mapping the steer plan chose at this thread's last Scene.steer_position_toward or RrtPlanner over a dynamic
    space (rkh_steer_mapping_name): auto, duo, wave, wave16, pair, planar or prismatic."""
    return load().rkh_steer_mapping_name().decode()


def gjk_distance(ctx, a, b, mesh_vertices=None):
    """GJK distance of the world-anchored shape pairs (a[i], b[i]) (rkh_diag_gjk_distance)."""
    n = len(a)
    aa, bb = T.as_array(list(a), T.Shape), T.as_array(list(b), T.Shape)
    verts = np.zeros((0, 3)) if mesh_vertices is None else np.ascontiguousarray(mesh_vertices, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(n)
    _check(ctx.lib.rkh_diag_gjk_distance(ctx.h, aa, bb, n, T.dptr(verts) if len(verts) else None, len(verts), T.dptr(out)))
    return out


def gjk_records(ctx, a, b, mesh_vertices=None):
    """The records of the same searches (rkh_diag_gjk_records): dist [n] (gjk_distance's values), point1 [n][3] on a[i],
    point2 [n][3] on b[i]."""
    n = len(a)
    aa, bb = T.as_array(list(a), T.Shape), T.as_array(list(b), T.Shape)
    verts = np.zeros((0, 3)) if mesh_vertices is None else np.ascontiguousarray(mesh_vertices, dtype=np.float64).reshape(-1, 3)
    d, p1, p2 = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3))
    _check(ctx.lib.rkh_diag_gjk_records(ctx.h, aa, bb, n, T.dptr(verts) if len(verts) else None, len(verts), T.dptr(d),
                                        T.dptr(p1), T.dptr(p2)))
    return {"dist": d, "point1": p1, "point2": p2}


def gjk_depth_records(ctx, a, b, mesh_vertices=None):
    """The same pairs with a penetration depth and a contact normal (rkh_diag_gjk_depth_records): where the cores are
    apart, gjk_records' values and normal [n][3] = the unit vector from a[i]'s closest point towards b[i]'s; where they
    cross, dist = -(r1 + r2 + depth) - 1e-9, the normal of the least separating translation (from a[i] towards b[i]),
    point1 on a[i] and point2 = point1 - (depth + r1 + r2) normal on b[i]."""
    n = len(a)
    aa, bb = T.as_array(list(a), T.Shape), T.as_array(list(b), T.Shape)
    verts = np.zeros((0, 3)) if mesh_vertices is None else np.ascontiguousarray(mesh_vertices, dtype=np.float64).reshape(-1, 3)
    d, p1, p2, nr = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    _check(ctx.lib.rkh_diag_gjk_depth_records(ctx.h, aa, bb, n, T.dptr(verts) if len(verts) else None, len(verts), T.dptr(d),
                                              T.dptr(p1), T.dptr(p2), T.dptr(nr)))
    return {"dist": d, "point1": p1, "point2": p2, "normal": nr}


def nn_mirror_query(ctx, pts, q, coord_bound):
    """1-NN of every query through the planner-regime sweep (half-precision mirror + exact resolution,
    rkh_diag_nn_mirror_query): (index, distance) arrays."""
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    q = np.ascontiguousarray(q, dtype=np.float64)
    n, D = pts.shape
    B = q.shape[0]
    idx = np.zeros(B, dtype=np.uint32)
    dist = np.zeros(B)
    _check(ctx.lib.rkh_diag_nn_mirror_query(ctx.h, T.dptr(pts), n, D, T.dptr(q), B, float(coord_bound), T.u32ptr(idx),
                                            T.dptr(dist)))
    return idx, dist


class Scene:
    def __init__(self, ctx, scn):
        self.ctx, self.lib, self.scn = ctx, ctx.lib, scn
        self.n, self.D = scn.n_dof, 2 * scn.n_dof
        self._ops = scn.ops_array()
        self._shapes = scn.shapes_array() if scn.shapes else (T.Shape * 1)()
        self.h = C.c_void_p()
        verts = getattr(scn, "mesh_vertices", None)
        if verts is not None and len(verts):  # convex vertex sets among the shapes (RKH_SHAPE_MESH)
            self._verts = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
            _check(self.lib.rkh_scene_create_with_meshes(ctx.h, self._ops, len(scn.ops), C.byref(scn.base), self._shapes,
                                                         len(scn.shapes), T.dptr(self._verts), len(self._verts),
                                                         C.byref(self.h)))
        else:
            _check(self.lib.rkh_scene_create(ctx.h, self._ops, len(scn.ops), C.byref(scn.base), self._shapes,
                                             len(scn.shapes), C.byref(self.h)))

    @property
    def num_pairs(self):
        return self.lib.rkh_scene_num_pairs(self.h)

    def state_derivative(self, x, u):
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.D)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1, self.n)
        B = x.shape[0]
        pd, M, f = np.zeros((B, self.D)), np.zeros((B, self.n, self.n)), np.zeros((B, self.n))
        _check(self.lib.rkh_state_derivative(self.h, T.dptr(x), T.dptr(u), B, T.dptr(pd), T.dptr(M), T.dptr(f)))
        return pd, M, f

    def proximity_counts(self, x):
        """Stage counts of the two-lanes steer kernels' proximity test on the states x (rkh_diag_proximity_counts)."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.D)
        c = (C.c_uint64 * 8)()
        _check(self.lib.rkh_diag_proximity_counts(self.h, T.dptr(x), x.shape[0], c))
        return {"states": int(c[0]), "pairs_past_cull": int(c[1]), "closed_forms": int(c[2]), "golden_section": int(c[3]),
                "states_in_collision": int(c[4]), "pairs_per_state": int(c[5]), "pairs_in_static_reach": int(c[6])}

    def proximity_clearance(self, x):
        """The clearance bound the two-lanes steer kernels carry, per state (rkh_diag_proximity_clearance)."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.D)
        out = np.zeros(x.shape[0], dtype=np.float32)
        _check(self.lib.rkh_diag_proximity_clearance(self.h, T.dptr(x), x.shape[0], out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def steer_clearance_counts(self):
        """(edge-steps the carried bound settled, wave-steps that ran the proximity test) of the two-lanes steer launches
        on this scene so far (rkh_diag_steer_clearance_counts)."""
        c = (C.c_uint64 * 2)()
        _check(self.lib.rkh_diag_steer_clearance_counts(self.h, c))
        return int(c[0]), int(c[1])

    def diag_feval_cycles(self, x, u, iters=100):
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.D)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1, self.n)
        out = np.zeros((x.shape[0], 8), dtype=np.uint64)
        _check(self.lib.rkh_diag_feval_cycles(self.h, T.dptr(x), T.dptr(u), x.shape[0], iters,
                                              out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def min_distance(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.D)
        d = np.zeros(x.shape[0])
        _check(self.lib.rkh_min_distance(self.h, T.dptr(x), x.shape[0], T.dptr(d)))
        return d

    def min_distance_records(self, x):
        """proxy_query_pair_3D::findMinimumDistance()->getLastResult() per state (rkh_min_distance_records): dist [B],
        point1 / point2 [B][3] (world frame, on the finder's shape1 / shape2), shape1 / shape2 [B] (indices into the
        scenario's shapes, in the finder's order; 0xFFFFFFFF without finders)."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.D)
        B = x.shape[0]
        d, p1, p2 = np.zeros(B), np.zeros((B, 3)), np.zeros((B, 3))
        s1, s2 = np.zeros(B, dtype=np.uint32), np.zeros(B, dtype=np.uint32)
        _check(self.lib.rkh_min_distance_records(self.h, T.dptr(x), B, T.dptr(d), T.dptr(p1), T.dptr(p2), T.u32ptr(s1),
                                                 T.u32ptr(s2)))
        return {"dist": d, "point1": p1, "point2": p2, "shape1": s1, "shape2": s2}

    def distance_query_ms(self, x, records, runs):
        """Kernel times [runs] in ms of the distance query (records=False), the record query (True) or the depth record
        query (records="depth"; 3D scenes) on the states x, events around each launch (rkh_diag_distance_query_ms)."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.D)
        ms = np.zeros(int(runs), dtype=np.float32)
        _check(self.lib.rkh_diag_distance_query_ms(self.h, T.dptr(x), x.shape[0], 2 if records == "depth" else (1 if records else 0), int(runs),
                                                   ms.ctypes.data_as(C.POINTER(C.c_float))))
        return ms

    def collision_records(self, x, cap):
        """proxy_query_pair_3D::gatherCollisionPoints per state (rkh_collision_records): n_found [B] (all colliding
        finders, may exceed cap) and the first cap records in finder order: dist [B][cap], point1 / point2 [B][cap][3],
        shape1 / shape2 [B][cap]; unused slots hold +inf, zeros and 0xFFFFFFFF."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.D)
        B, cap = x.shape[0], int(cap)
        n = np.zeros(B, dtype=np.uint32)
        d, p1, p2 = np.zeros((B, cap)), np.zeros((B, cap, 3)), np.zeros((B, cap, 3))
        s1, s2 = np.zeros((B, cap), dtype=np.uint32), np.zeros((B, cap), dtype=np.uint32)
        _check(self.lib.rkh_collision_records(self.h, T.dptr(x), B, cap, T.u32ptr(n), T.dptr(d), T.dptr(p1), T.dptr(p2),
                                              T.u32ptr(s1), T.u32ptr(s2)))
        return {"n_found": n, "dist": d, "point1": p1, "point2": p2, "shape1": s1, "shape2": s2}

    def min_distance_records_meshes(self, x):
        """min_distance_records for every non-planar scene, mesh shapes included (rkh_min_distance_records_meshes): the
        same keys.  A pair with a mesh in it reports the witnesses of its support-map search: a closest pair of points
        while the cores are apart, one common point of the cores (no penetration depth) when they cross."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.D)
        B = x.shape[0]
        d, p1, p2 = np.zeros(B), np.zeros((B, 3)), np.zeros((B, 3))
        s1, s2 = np.zeros(B, dtype=np.uint32), np.zeros(B, dtype=np.uint32)
        _check(self.lib.rkh_min_distance_records_meshes(self.h, T.dptr(x), B, T.dptr(d), T.dptr(p1), T.dptr(p2),
                                                        T.u32ptr(s1), T.u32ptr(s2)))
        return {"dist": d, "point1": p1, "point2": p2, "shape1": s1, "shape2": s2}

    def collision_records_meshes(self, x, cap):
        """collision_records for every non-planar scene, mesh shapes included (rkh_collision_records_meshes)."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.D)
        B, cap = x.shape[0], int(cap)
        n = np.zeros(B, dtype=np.uint32)
        d, p1, p2 = np.zeros((B, cap)), np.zeros((B, cap, 3)), np.zeros((B, cap, 3))
        s1, s2 = np.zeros((B, cap), dtype=np.uint32), np.zeros((B, cap), dtype=np.uint32)
        _check(self.lib.rkh_collision_records_meshes(self.h, T.dptr(x), B, cap, T.u32ptr(n), T.dptr(d), T.dptr(p1),
                                                     T.dptr(p2), T.u32ptr(s1), T.u32ptr(s2)))
        return {"n_found": n, "dist": d, "point1": p1, "point2": p2, "shape1": s1, "shape2": s2}

    def min_distance_records_depth(self, x):
        """min_distance_records_meshes with a penetration depth and a contact normal (rkh_min_distance_records_depth): the
        same keys and "normal" [B][3].  A pair with a mesh in it whose cores cross reports dist = -(r1 + r2 + depth) - 1e-9,
        the unit normal of the least separating translation (from shape1 towards shape2) and the two contact points; the
        minimum is taken over these distances, so among crossing mesh pairs the deepest wins.  Every other record is the
        _meshes entry's, with normal = the unit vector of the closest pair (closed forms: (point2 - point1) / dist)."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.D)
        B = x.shape[0]
        d, p1, p2, nr = np.zeros(B), np.zeros((B, 3)), np.zeros((B, 3)), np.zeros((B, 3))
        s1, s2 = np.zeros(B, dtype=np.uint32), np.zeros(B, dtype=np.uint32)
        _check(self.lib.rkh_min_distance_records_depth(self.h, T.dptr(x), B, T.dptr(d), T.dptr(p1), T.dptr(p2), T.dptr(nr),
                                                       T.u32ptr(s1), T.u32ptr(s2)))
        return {"dist": d, "point1": p1, "point2": p2, "normal": nr, "shape1": s1, "shape2": s2}

    def collision_records_depth(self, x, cap):
        """collision_records_meshes with depths and normals (rkh_collision_records_depth): the same finders in the same
        order with the same n_found, and "normal" [B][cap][3] (zeros in unused slots)."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.D)
        B, cap = x.shape[0], int(cap)
        n = np.zeros(B, dtype=np.uint32)
        d, p1, p2, nr = np.zeros((B, cap)), np.zeros((B, cap, 3)), np.zeros((B, cap, 3)), np.zeros((B, cap, 3))
        s1, s2 = np.zeros((B, cap), dtype=np.uint32), np.zeros((B, cap), dtype=np.uint32)
        _check(self.lib.rkh_collision_records_depth(self.h, T.dptr(x), B, cap, T.u32ptr(n), T.dptr(d), T.dptr(p1),
                                                    T.dptr(p2), T.dptr(nr), T.u32ptr(s1), T.u32ptr(s2)))
        return {"n_found": n, "dist": d, "point1": p1, "point2": p2, "normal": nr, "shape1": s1, "shape2": s2}

    def min_distance_records_2d(self, x):
        """proxy_query_pair_2D::findMinimumDistance()->getLastResult() per state of a planar scene
        (rkh_min_distance_records_2d): the keys of min_distance_records with point1 / point2 [B][2].  The winner is what
        the reference's culled loop leaves in min_i, which depends on the finder order."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.D)
        B = x.shape[0]
        d, p1, p2 = np.zeros(B), np.zeros((B, 2)), np.zeros((B, 2))
        s1, s2 = np.zeros(B, dtype=np.uint32), np.zeros(B, dtype=np.uint32)
        _check(self.lib.rkh_min_distance_records_2d(self.h, T.dptr(x), B, T.dptr(d), T.dptr(p1), T.dptr(p2), T.u32ptr(s1),
                                                    T.u32ptr(s2)))
        return {"dist": d, "point1": p1, "point2": p2, "shape1": s1, "shape2": s2}

    def collision_records_2d(self, x, cap):
        """proxy_query_pair_2D::gatherCollisionPoints per state of a planar scene (rkh_collision_records_2d): the keys of
        collision_records with point1 / point2 [B][cap][2]."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.D)
        B, cap = x.shape[0], int(cap)
        n = np.zeros(B, dtype=np.uint32)
        d, p1, p2 = np.zeros((B, cap)), np.zeros((B, cap, 2)), np.zeros((B, cap, 2))
        s1, s2 = np.zeros((B, cap), dtype=np.uint32), np.zeros((B, cap), dtype=np.uint32)
        _check(self.lib.rkh_collision_records_2d(self.h, T.dptr(x), B, cap, T.u32ptr(n), T.dptr(d), T.dptr(p1), T.dptr(p2),
                                                 T.u32ptr(s1), T.u32ptr(s2)))
        return {"n_found": n, "dist": d, "point1": p1, "point2": p2, "shape1": s1, "shape2": s2}

    def move_position_toward(self, lower, upper, min_interval, a, b, fraction=1.0):
        """manip_quasi_static_env::move_position_toward for B (a,b) joint-position pairs (rkh_edge_check)."""
        lower = np.ascontiguousarray(lower, dtype=np.float64)
        upper = np.ascontiguousarray(upper, dtype=np.float64)
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, self.n)
        b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1, self.n)
        out = np.zeros_like(a)
        nchk = np.zeros(a.shape[0], dtype=np.uint32)
        _check(self.lib.rkh_edge_check(self.h, T.dptr(lower), T.dptr(upper), float(min_interval), T.dptr(a), T.dptr(b),
                                       a.shape[0], float(fraction), T.dptr(out), T.u32ptr(nchk)))
        return out, nchk

    def shortcut_paths(self, space, paths, max_span=0):
        """rkh_shortcut_paths over the quasi-static space `space` (make_qs_space): `paths` is a list of [L][n] arrays of
        points, start first.  Returns (keep: one array of path-local indices per path, cost_in [B], cost_out [B],
        n_blocked [B]); the shortcut path b is paths[b][keep[b]].  max_span: the longest hop tried, in vertices (0: all)."""
        pts, path_ptr = _path_table(paths, self.n)
        B = len(path_ptr) - 1
        keep = np.zeros(max(int(path_ptr[B]), 1), dtype=np.uint32)
        n_keep, n_blocked = np.zeros(max(B, 1), dtype=np.uint32), np.zeros(max(B, 1), dtype=np.uint32)
        cost_in, cost_out = np.zeros(max(B, 1)), np.zeros(max(B, 1))
        _check(self.lib.rkh_shortcut_paths(self.h, C.byref(space), T.dptr(pts), T.u32ptr(path_ptr), B, int(max_span),
                                           T.u32ptr(keep), T.u32ptr(n_keep), T.dptr(cost_in), T.dptr(cost_out),
                                           T.u32ptr(n_blocked)))
        return _keep_lists(keep, n_keep[:B], path_ptr), cost_in[:B], cost_out[:B], n_blocked[:B]

    def shortcut_ms(self, space, paths, max_span=0, runs=5):
        """rkh_diag_shortcut_ms: ms [runs][3] of the pair kernel, the walk launch and the search, events around each."""
        pts, path_ptr = _path_table(paths, self.n)
        ms = np.zeros((int(runs), 3), dtype=np.float32)
        _check(self.lib.rkh_diag_shortcut_ms(self.h, C.byref(space), T.dptr(pts), T.u32ptr(path_ptr), len(path_ptr) - 1,
                                             int(max_span), int(runs), ms.ctypes.data_as(C.POINTER(C.c_float))))
        return ms

    # ---- direct kinematics, Jacobians, pose IK (rkh_direct_kinematics[_2d], rkh_jacobians[_2d], rkh_inverse_kinematics) ----
    @property
    def planar(self):
        return any(o.kind in (T.KTE_REVOLUTE_JOINT_2D, T.KTE_PRISMATIC_JOINT_2D) for o in self.scn.ops)

    def _kin_args(self, q, qd, frames):
        q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, self.n)
        qd = None if qd is None else np.ascontiguousarray(qd, dtype=np.float64).reshape(-1, self.n)
        frames = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
        return q, qd, frames, frames.ctypes.data_as(C.POINTER(C.c_int32))

    def direct_kinematics(self, q, frames, qd=None, want=("pos", "rot", "vel", "ang_vel"), planar=None):
        """Frames of the chain for B joint points q [B][n] (rates qd or None): a dict of the arrays named in `want`.
        3D scenes (rkh_direct_kinematics): pos [B][F][3], rot = quat [B][F][4] (w, x, y, z), vel [B][F][3] (world),
        ang_vel [B][F][3] (the frame's own coordinates).  Planar scenes (rkh_direct_kinematics_2d): pos [B][F][2], rot
        [B][F][2] = (cos, sin), vel [B][F][2], ang_vel [B][F].  `planar` forces the entry (to see it refuse)."""
        planar = self.planar if planar is None else planar
        q, qd, frames, fp = self._kin_args(q, qd, frames)
        B, F = q.shape[0], len(frames)
        shapes = {"pos": (B, F, 2), "rot": (B, F, 2), "vel": (B, F, 2), "ang_vel": (B, F)} if planar else \
            {"pos": (B, F, 3), "rot": (B, F, 4), "vel": (B, F, 3), "ang_vel": (B, F, 3)}
        out = {k: np.zeros(shapes[k]) for k in want}
        ptr = [T.dptr(out[k]) if k in out else None for k in ("pos", "rot", "vel", "ang_vel")]
        fn = self.lib.rkh_direct_kinematics_2d if planar else self.lib.rkh_direct_kinematics
        _check(fn(self.h, T.dptr(q), None if qd is None else T.dptr(qd), B, fp, F, *ptr))
        return out

    def jacobians(self, q, frames, qd=None, want=("jac", "jac_dot"), planar=None):
        """getJacobianMatrix[AndDerivative] per (point, frame): jac / jac_dot [B][F][6][n] (planar: [B][F][3][n]), rows
        (velocity, angular velocity) in the frame's own coordinates (rkh_jacobians / rkh_jacobians_2d)."""
        planar = self.planar if planar is None else planar
        q, qd, frames, fp = self._kin_args(q, qd, frames)
        B, F = q.shape[0], len(frames)
        out = {k: np.zeros((B, F, 3 if planar else 6, self.n)) for k in want}
        ptr = [T.dptr(out[k]) if k in out else None for k in ("jac", "jac_dot")]
        fn = self.lib.rkh_jacobians_2d if planar else self.lib.rkh_jacobians
        _check(fn(self.h, T.dptr(q), None if qd is None else T.dptr(qd), B, fp, F, *ptr))
        return out

    def _ik_args(self, targets, seeds, lower, upper):
        tg = T.as_array(list(targets), T.Pose) if len(targets) else (T.Pose * 1)()
        seeds = np.ascontiguousarray(seeds, dtype=np.float64)
        seeds = seeds.reshape(len(targets), -1, self.n) if len(targets) else seeds.reshape(0, 0, self.n)
        lower = np.ascontiguousarray(lower, dtype=np.float64).reshape(-1)
        upper = np.ascontiguousarray(upper, dtype=np.float64).reshape(-1)
        assert len(lower) >= self.n and len(upper) >= self.n
        return tg, seeds, lower, upper

    def inverse_kinematics(self, frame, targets, seeds, lower, upper, params=None):
        """rkh_inverse_kinematics: `targets` a list of T.Pose, seeds [T][S][n], joint box lower / upper [n], params =
        T.make_ik_params(...).  Returns a dict: q [T][S][n], res_pos, res_rot, iters [T][S], converged, free [T][S]
        (bool), best [T] (seed index, or -1 if no seed is converged and free)."""
        params = params if params is not None else T.make_ik_params()
        tg, seeds, lower, upper = self._ik_args(targets, seeds, lower, upper)
        Tn, S = seeds.shape[0], seeds.shape[1]
        q = np.zeros((Tn, S, self.n))
        rp, rr = np.zeros((Tn, S)), np.zeros((Tn, S))
        it, fl = np.zeros((Tn, S), dtype=np.uint32), np.zeros((Tn, S), dtype=np.uint32)
        best = np.zeros(max(Tn, 1), dtype=np.uint32)
        _check(self.lib.rkh_inverse_kinematics(self.h, int(frame), tg, Tn, T.dptr(seeds), S, T.dptr(lower), T.dptr(upper),
                                               C.byref(params), T.dptr(q), T.dptr(rp), T.dptr(rr), T.u32ptr(it), T.u32ptr(fl),
                                               T.u32ptr(best)))
        return {"q": q, "res_pos": rp, "res_rot": rr, "iters": it, "converged": (fl & 1) != 0, "free": (fl & 2) != 0,
                "best": np.where(best[:Tn] == 0xFFFFFFFF, -1, best[:Tn].astype(np.int64))}

    def kinematics_ms(self, q, frames, qd=None, runs=5):
        """rkh_diag_kinematics_ms: ms [runs] of the launch that answers direct_kinematics and jacobians together."""
        q, qd, frames, fp = self._kin_args(q, qd, frames)
        ms = np.zeros(int(runs), dtype=np.float32)
        _check(self.lib.rkh_diag_kinematics_ms(self.h, T.dptr(q), None if qd is None else T.dptr(qd), q.shape[0], fp, len(frames),
                                               int(runs), ms.ctypes.data_as(C.POINTER(C.c_float))))
        return ms

    def ik_ms(self, frame, targets, seeds, lower, upper, params=None, runs=5):
        """rkh_diag_ik_ms: ms [runs][2] of the solve launch and the distance launch of inverse_kinematics."""
        params = params if params is not None else T.make_ik_params()
        tg, seeds, lower, upper = self._ik_args(targets, seeds, lower, upper)
        ms = np.zeros((int(runs), 2), dtype=np.float32)
        _check(self.lib.rkh_diag_ik_ms(self.h, int(frame), tg, seeds.shape[0], T.dptr(seeds), seeds.shape[1], T.dptr(lower),
                                       T.dptr(upper), C.byref(params), int(runs), ms.ctypes.data_as(C.POINTER(C.c_float))))
        return ms

    def steer_position_toward(self, a, b, fraction=1.0, record=False, dyn=None):
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, self.D)
        b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1, self.D)
        dyn = dyn if dyn is not None else self.scn.dyn
        B = a.shape[0]
        out = np.zeros_like(a)
        steps = np.zeros(B, dtype=np.uint32)
        rec = np.zeros((B, dyn.steps_per_edge + 1, self.D)) if record else None
        _check(self.lib.rkh_propagate(self.h, C.byref(dyn), T.dptr(a), T.dptr(b), B, float(fraction), T.dptr(out),
                                      T.u32ptr(steps), T.dptr(rec) if record else None))
        return out, steps, rec

    def close(self):
        if self.h:
            self.lib.rkh_scene_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SvpSpace:
    """The order-1 rate-limited joint space with SVP profiles (rkh_svp_*): points are [2 n] rows (p0, v0, p1, v1, ...) in
    space coordinates.  `space` is a T.SvpSpace (T.make_svp_space); `ctx` serves reach_time, nearest and interpolate,
    `scene` (optional) the edge walk; in_bounds needs neither."""

    def __init__(self, space, ctx=None, scene=None):
        self.lib = load()
        self.space, self.ctx, self.scene = space, ctx if ctx is not None else (scene.ctx if scene is not None else None), scene
        self.n = int(space.n_dof)

    def _rows(self, x):
        return np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, 2 * self.n))

    def in_bounds(self, pts):
        pts = self._rows(pts)
        ok = np.zeros(max(len(pts), 1), dtype=np.uint8)
        _check(self.lib.rkh_svp_in_bounds(C.byref(self.space), T.dptr(pts), len(pts), ok.ctypes.data_as(C.POINTER(C.c_uint8))))
        return ok[:len(pts)].astype(bool)

    def reach_time(self, a, b, peaks=True):
        """(time [B], peak [B][n]) of d(a_e -> b_e); +inf and a row of zeros where the pair is infeasible."""
        a, b = self._rows(a), self._rows(b)
        B = len(a)
        time, peak = np.zeros(max(B, 1)), np.zeros((max(B, 1), self.n))
        _check(self.lib.rkh_svp_reach_time(self.ctx.h, C.byref(self.space), T.dptr(a), T.dptr(b), B, T.dptr(time),
                                           T.dptr(peak) if peaks else None))
        return (time[:B], peak[:B]) if peaks else time[:B]

    def nearest(self, points, queries, k, direction=0):
        """(idx [B][k], dist [B][k]) by d(point -> query) (direction 0) or d(query -> point) (1), ascending by (distance,
        index); padded with 0xFFFFFFFF / +inf."""
        points, queries = self._rows(points), self._rows(queries)
        B = len(queries)
        idx, dist = np.zeros((max(B, 1), k), dtype=np.uint32), np.zeros((max(B, 1), k))
        _check(self.lib.rkh_svp_nearest(self.ctx.h, C.byref(self.space), T.dptr(points), len(points), T.dptr(queries), B, int(k),
                                        int(direction), T.u32ptr(idx), T.dptr(dist)))
        return idx[:B], dist[:B]

    def nearest_async(self, d_points, n_pts, d_queries, B, k, direction, d_idx, d_dist):
        """Device pointers (integers), enqueued on the context's stream."""
        _check(self.lib.rkh_svp_nearest_async(self.ctx.h, C.byref(self.space), d_points, int(n_pts), d_queries, int(B), int(k),
                                              int(direction), d_idx, d_dist))

    def edge_check(self, a, b, fraction=None):
        """The collision-tested walk: (out [B][2n], reach_time [B], n_checked [B], reached [B])."""
        a, b = self._rows(a), self._rows(b)
        B = len(a)
        out, rt = np.zeros((max(B, 1), 2 * self.n)), np.zeros(max(B, 1))
        nc, re = np.zeros(max(B, 1), dtype=np.uint32), np.zeros(max(B, 1), dtype=np.uint8)
        fr = None
        if fraction is not None:
            fr = np.ascontiguousarray(np.broadcast_to(np.asarray(fraction, dtype=np.float64), (B,)))
        _check(self.lib.rkh_svp_edge_check(self.scene.h, C.byref(self.space), T.dptr(a), T.dptr(b), B,
                                           T.dptr(fr) if fr is not None else None, T.dptr(out), T.dptr(rt), T.u32ptr(nc),
                                           re.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out[:B], rt[:B], nc[:B], re[:B]

    def edge_check_back(self, a, b, fraction=None):
        """rkh_svp_edge_check_back: the profile a -> b walked from b backwards; outputs as edge_check."""
        return self._edge_check_dir(a, b, fraction, True)

    def edge_check_dir(self, a, b, back, fraction=None):
        """rkh_diag_svp_edge_check_dir: row e backward where back[e] != 0, forward where 0, in one launch."""
        return self._edge_check_dir(a, b, fraction, np.ascontiguousarray(np.asarray(back, dtype=np.uint8)))

    def _edge_check_dir(self, a, b, fraction, back):
        a, b = self._rows(a), self._rows(b)
        B = len(a)
        out, rt = np.zeros((max(B, 1), 2 * self.n)), np.zeros(max(B, 1))
        nc, re = np.zeros(max(B, 1), dtype=np.uint32), np.zeros(max(B, 1), dtype=np.uint8)
        u8 = C.POINTER(C.c_uint8)
        fr = None
        if fraction is not None:
            fr = np.ascontiguousarray(np.broadcast_to(np.asarray(fraction, dtype=np.float64), (B,)))
        head = (self.scene.h, C.byref(self.space), T.dptr(a), T.dptr(b), B, T.dptr(fr) if fr is not None else None)
        tail = (T.dptr(out), T.dptr(rt), T.u32ptr(nc), re.ctypes.data_as(u8))
        if back is True:
            _check(self.lib.rkh_svp_edge_check_back(*head, *tail))
        else:
            assert len(back) == B
            _check(self.lib.rkh_diag_svp_edge_check_dir(*head, back.ctypes.data_as(u8), *tail))
        return out[:B], rt[:B], nc[:B], re[:B]

    def interpolate(self, a, b, t):
        """(out [B][M][2n], reach_time [B]): the profile of each pair at the times t [B][M]."""
        a, b = self._rows(a), self._rows(b)
        B = len(a)
        t = np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(B, -1))
        M = t.shape[1]
        out, rt = np.zeros((max(B, 1), max(M, 1), 2 * self.n)), np.zeros(max(B, 1))
        _check(self.lib.rkh_svp_interpolate(self.ctx.h, C.byref(self.space), T.dptr(a), T.dptr(b), B, T.dptr(t) if M else None, M,
                                            T.dptr(out), T.dptr(rt)))
        return out[:B, :M], rt[:B]

    def shortcut_paths(self, paths, max_span=0, chunk_pairs=None):
        """rkh_svp_shortcut_paths: `paths` is a list of [L][2n] arrays of points, start first.  Returns (keep: one array of
        path-local indices per path, time_in [B], time_out [B], n_blocked [B]); the shortcut trajectory b is
        paths[b][keep[b]], empty where time_out[b] is +inf (the points are not a trajectory).  max_span: the longest hop
        tried, in vertices (0: all).  chunk_pairs: rkh_diag_svp_shortcut_chunked with that many pairs per walk."""
        pts, path_ptr = _path_table(paths, 2 * self.n)
        B = len(path_ptr) - 1
        keep = np.zeros(max(int(path_ptr[B]), 1), dtype=np.uint32)
        n_keep, n_blocked = np.zeros(max(B, 1), dtype=np.uint32), np.zeros(max(B, 1), dtype=np.uint32)
        time_in, time_out = np.zeros(max(B, 1)), np.zeros(max(B, 1))
        head = (self.scene.h, C.byref(self.space), T.dptr(pts), T.u32ptr(path_ptr), B, int(max_span))
        tail = (T.u32ptr(keep), T.u32ptr(n_keep), T.dptr(time_in), T.dptr(time_out), T.u32ptr(n_blocked))
        if chunk_pairs is None:
            _check(self.lib.rkh_svp_shortcut_paths(*head, *tail))
        else:
            _check(self.lib.rkh_diag_svp_shortcut_chunked(*head, int(chunk_pairs), *tail))
        return _keep_lists(keep, n_keep[:B], path_ptr), time_in[:B], time_out[:B], n_blocked[:B]

    def shortcut_ms(self, paths, max_span=0, runs=5):
        """rkh_diag_svp_shortcut_ms: ms [runs][3] of the pair kernel, the walks and the search, summed over the chunks."""
        pts, path_ptr = _path_table(paths, 2 * self.n)
        ms = np.zeros((int(runs), 3), dtype=np.float32)
        _check(self.lib.rkh_diag_svp_shortcut_ms(self.scene.h, C.byref(self.space), T.dptr(pts), T.u32ptr(path_ptr),
                                                 len(path_ptr) - 1, int(max_span), int(runs),
                                                 ms.ctypes.data_as(C.POINTER(C.c_float))))
        return ms


class SvpRrt:
    """Batch RRT over the SVP space (rkh_svp_rrt_*): `params` is one T.SvpRrtParams (T.make_svp_rrt_params) or a list of
    them, independent problems on one scene that share every launch; trees and sample streams stay on the device."""
    NO_INDEX = 0xFFFFFFFF
    PHASES = ("sample", "nearest", "extend_walk", "commit", "probe_walk", "finish")

    def __init__(self, scene, space, params):
        self.lib = load()
        self.scene, self.space = scene, space
        plist = list(params) if isinstance(params, (list, tuple)) else [params]
        self.P, self.n = len(plist), int(space.n_dof)
        arr = (T.SvpRrtParams * max(self.P, 1))(*plist)
        self.max_vertices = [int(p.max_vertices) for p in plist]
        self.h = C.c_void_p()
        _check(self.lib.rkh_svp_rrt_create_batch(scene.h, C.byref(self.space), arr, self.P, C.byref(self.h)))
        self.stats = SvpRrtStats()

    def solve(self, max_rounds=-1):
        """Rounds until every problem has ended or max_rounds have run (< 0: no limit); resumes where it stopped."""
        _check(self.lib.rkh_svp_rrt_solve(self.h, int(max_rounds), C.byref(self.stats)))
        return self.stats

    @property
    def finished(self):
        return self.stats.problems_finished == self.P

    def status(self):
        """(n_vertices [P], iterations [P], goal_parent [P]); goal_parent 0xFFFFFFFF: not reached"""
        nv, it, gp = (np.zeros(self.P, dtype=np.uint32) for _ in range(3))
        _check(self.lib.rkh_svp_rrt_get_status(self.h, T.u32ptr(nv), T.u32ptr(it), T.u32ptr(gp)))
        return nv, it, gp

    def tree(self, problem=0):
        """{"vertices" [V][2n], "parent" [V], "edge_time" [V]} of one problem"""
        cap = self.max_vertices[problem]
        verts, parent, et = np.zeros((cap, 2 * self.n)), np.zeros(cap, dtype=np.uint32), np.zeros(cap)
        V = C.c_uint32(0)
        _check(self.lib.rkh_svp_rrt_get_tree(self.h, int(problem), T.dptr(verts), T.u32ptr(parent), T.dptr(et), cap, C.byref(V)))
        return {"vertices": verts[:V.value], "parent": parent[:V.value], "edge_time": et[:V.value]}

    def solution(self, problem=0):
        """(points [n_points][2n] start ... goal, duration); (empty, 0.0) when the goal has not been reached"""
        cap = self.max_vertices[problem] + 1
        pts = np.zeros((cap, 2 * self.n))
        n_pts, dur = C.c_uint32(0), C.c_double(0.0)
        _check(self.lib.rkh_svp_rrt_get_solution(self.h, int(problem), T.dptr(pts), cap, C.byref(n_pts), C.byref(dur)))
        return pts[:n_pts.value], dur.value

    def shortcut_solutions(self, max_span=0):
        """The solutions of all problems that reached their goal, shortcut in ONE rkh_svp_shortcut_paths call.  Returns
        {problem: {"points" [L][2n], "duration", "keep", "time_in", "time_out", "n_blocked"}}; the shortcut trajectory is
        points[keep]."""
        _, _, gp = self.status()
        solved = [i for i in range(self.P) if gp[i] != self.NO_INDEX]
        sols = [self.solution(i) for i in solved]
        if not solved:
            return {}
        keep, t_in, t_out, blocked = SvpSpace(self.space, scene=self.scene).shortcut_paths([p for p, _ in sols], max_span)
        return {i: {"points": sols[k][0], "duration": sols[k][1], "keep": keep[k], "time_in": float(t_in[k]),
                    "time_out": float(t_out[k]), "n_blocked": int(blocked[k])} for k, i in enumerate(solved)}

    def profile(self, enable=True):
        """Brackets the phases of later rounds with stream events; returns {phase: ms so far}."""
        ms = np.zeros(len(self.PHASES))
        _check(self.lib.rkh_diag_svp_rrt_profile(self.h, 1 if enable else 0, T.dptr(ms)))
        return dict(zip(self.PHASES, ms.tolist()))

    def close(self):
        if self.h:
            self.lib.rkh_svp_rrt_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SvpBiRrt:
    """Batch bidirectional RRT over the SVP space (rkh_svp_birrt_*): `params` is one T.SvpRrtParams with a goal
    (T.make_svp_rrt_params) or a list of them, independent problems on one scene that share every launch.  Tree 0 grows
    forward from the start, tree 1 backward from the goal (the edge of its vertex v is the profile v -> parent(v))."""
    NO_INDEX = 0xFFFFFFFF
    PHASES = ("sample", "nearest", "steer", "walk", "commit")

    def __init__(self, scene, space, params):
        self.lib = load()
        self.scene, self.space = scene, space
        plist = list(params) if isinstance(params, (list, tuple)) else [params]
        self.P, self.n = len(plist), int(space.n_dof)
        arr = (T.SvpRrtParams * max(self.P, 1))(*plist)
        self.max_vertices = [int(p.max_vertices) for p in plist]
        self.h = C.c_void_p()
        _check(self.lib.rkh_svp_birrt_create_batch(scene.h, C.byref(self.space), arr, self.P, C.byref(self.h)))
        self.stats = SvpRrtStats()
        _check(self.lib.rkh_svp_birrt_solve(self.h, 0, C.byref(self.stats)))   # no round: the totals after create

    def solve(self, max_rounds=-1):
        """Rounds (one half step of every unfinished problem) until every problem has ended or max_rounds have run (< 0: no
        limit); resumes where it stopped."""
        _check(self.lib.rkh_svp_birrt_solve(self.h, int(max_rounds), C.byref(self.stats)))
        return self.stats

    @property
    def finished(self):
        return self.stats.problems_finished == self.P

    def status(self):
        """(n_vertices0 [P], n_vertices1 [P], iterations [P], join0 [P], join1 [P]); a join of 0xFFFFFFFF: none"""
        out = tuple(np.zeros(self.P, dtype=np.uint32) for _ in range(5))
        _check(self.lib.rkh_svp_birrt_get_status(self.h, *(T.u32ptr(x) for x in out)))
        return out

    def tree(self, problem=0, which=0):
        """{"vertices" [V][2n], "parent" [V], "edge_time" [V]} of tree `which` (0: from the start, 1: from the goal)"""
        cap = self.max_vertices[problem]
        verts, parent, et = np.zeros((cap, 2 * self.n)), np.zeros(cap, dtype=np.uint32), np.zeros(cap)
        V = C.c_uint32(0)
        _check(self.lib.rkh_svp_birrt_get_tree(self.h, int(problem), int(which), T.dptr(verts), T.u32ptr(parent), T.dptr(et),
                                               cap, C.byref(V)))
        return {"vertices": verts[:V.value], "parent": parent[:V.value], "edge_time": et[:V.value]}

    def solution(self, problem=0):
        """(points [n_points][2n] start ... join0, join1 ... goal, duration); (empty, 0.0) without a join"""
        cap = 2 * self.max_vertices[problem]
        pts = np.zeros((cap, 2 * self.n))
        n_pts, dur = C.c_uint32(0), C.c_double(0.0)
        _check(self.lib.rkh_svp_birrt_get_solution(self.h, int(problem), T.dptr(pts), cap, C.byref(n_pts), C.byref(dur)))
        return pts[:n_pts.value], dur.value

    def profile(self, enable=True):
        """Brackets the phases of later rounds with stream events; returns {phase: ms so far}."""
        ms = np.zeros(len(self.PHASES))
        _check(self.lib.rkh_diag_svp_birrt_profile(self.h, 1 if enable else 0, T.dptr(ms)))
        return dict(zip(self.PHASES, ms.tolist()))

    def close(self):
        if self.h:
            self.lib.rkh_svp_birrt_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_qs_space(n_dof, lower, upper, min_interval, speed_limits=None):
    """rkh_qs_space; speed_limits makes it the rate-limited joint space (points = joint / speed limit)."""
    q = T.QsSpace()
    q.n_dof = n_dof
    q.min_interval = float(min_interval)
    for i in range(n_dof):
        q.lower[i] = float(lower[i])
        q.upper[i] = float(upper[i])
        q.speed_limits[i] = 0.0 if speed_limits is None else float(speed_limits[i])
    return q


class RrtPlanner:
    """rrt_planner over the steerable dynamic space.  `prm` is one rkh_rrt_params or a list of them (a batch of
    independent problems sharing every kernel launch); `stats` is the first problem's, `all_stats` the array."""

    def __init__(self, scene, prm, dyn=None, qs=None):
        self.scene, self.lib = scene, scene.lib
        self.dyn = dyn if dyn is not None else scene.scn.dyn
        self.prms = list(prm) if isinstance(prm, (list, tuple)) else [prm]
        self.P = len(self.prms)
        self._prm_arr = T.as_array(self.prms, T.RrtParams)
        self.h = C.c_void_p()
        self.qs = qs
        if qs is not None:  # quasi-static free space (points = joint positions)
            self.D = qs.n_dof
            _check(self.lib.rkh_planner_create_qs_batch(scene.h, C.byref(qs), self._prm_arr, self.P, C.byref(self.h)))
        else:
            self.D = scene.D
            _check(self.lib.rkh_planner_create_batch(scene.h, C.byref(self.dyn), self._prm_arr, self.P, C.byref(self.h)))
        self.all_stats = (PlannerStats * self.P)()

    @property
    def stats(self):
        return self.all_stats[0]

    @property
    def done(self):
        return all(s.done for s in self.all_stats)

    @property
    def stream(self):
        return self.lib.rkh_planner_stream(self.h)

    def enqueue(self, rounds):
        _check(self.lib.rkh_planner_enqueue(self.h, rounds))

    def sync(self):
        _check(self.lib.rkh_planner_sync(self.h, self.all_stats))
        return self.all_stats[0]

    def solve_planning_query(self):
        _check(self.lib.rkh_planner_solve(self.h, self.all_stats))
        return self.all_stats[0]

    def nn_profile(self):
        ms, by, ln = C.c_double(), C.c_uint64(), C.c_uint64()
        _check(self.lib.rkh_planner_nn_profile(self.h, C.byref(ms), C.byref(by), C.byref(ln)))
        return ms.value, by.value, ln.value

    def nn_pairs(self):
        pairs = C.c_uint64()
        _check(self.lib.rkh_planner_nn_pairs(self.h, C.byref(pairs)))
        return pairs.value

    def solution(self, problem=0):
        n, cost = C.c_uint32(), C.c_double()
        _check(self.lib.rkh_planner_get_solution(self.h, problem, None, 0, C.byref(n), C.byref(cost)))
        path = np.zeros(max(n.value, 1), dtype=np.uint32)
        _check(self.lib.rkh_planner_get_solution(self.h, problem, T.u32ptr(path), len(path), C.byref(n), C.byref(cost)))
        return path[: n.value], cost.value

    def steer_profile(self):
        ms, ln = C.c_double(), C.c_uint64()
        _check(self.lib.rkh_planner_steer_profile(self.h, C.byref(ms), C.byref(ln)))
        return ms.value, ln.value

    def steer_steps(self):
        """RK4 steps the steer kernels integrated so far (executed work, not n_steps per launched edge)."""
        n = C.c_uint64()
        _check(self.lib.rkh_planner_steer_steps(self.h, C.byref(n)))
        return n.value

    def carry_counts(self):
        """(candidates the rounds discarded, candidates that reused a discarded candidate's steered edge) so far, summed
        over the planner's problems (rkh_diag_planner_carry_counts)."""
        c = (C.c_uint64 * 2)()
        _check(self.lib.rkh_diag_planner_carry_counts(self.h, c))
        return int(c[0]), int(c[1])

    def probe_counts(self, problem=0):
        """Goal probes of one problem (rkh_diag_planner_probe_counts): a dict with the probes settled at commit
        (certified), the probes a steer launch ran (run), probed_n, the open probes (open), the first vertex whose probe
        is open (first_open) and the travel bound reach_q (inf: no certificate)."""
        c, r = (C.c_uint64 * 5)(), C.c_double()
        _check(self.lib.rkh_diag_planner_probe_counts(self.h, problem, c, C.byref(r)))
        return {"certified": int(c[0]), "run": int(c[1]), "probed_n": int(c[2]), "open": int(c[3]),
                "first_open": int(c[4]), "reach_q": r.value}

    def sample_cap(self, problem=0):
        """Samples the problem's stream buffers hold at present (they grow at a sync)."""
        n = C.c_uint64()
        _check(self.lib.rkh_diag_planner_sample_cap(self.h, problem, C.byref(n)))
        return n.value

    def tree(self, problem=0):
        st = self.all_stats[problem]
        nv, it, D = int(st.num_vertices), int(st.iterations), self.D
        pos = np.zeros((nv, D))
        parent = np.zeros(nv, dtype=np.uint32)
        nn_seq = np.zeros(max(it, 1), dtype=np.uint32)
        accept = np.zeros(max(it, 1), dtype=np.uint8)
        gd = np.zeros(max(nv - 1, 1))
        _check(self.lib.rkh_planner_get_tree(self.h, problem, T.dptr(pos), T.u32ptr(parent), T.u32ptr(nn_seq),
                                             accept.ctypes.data_as(C.POINTER(C.c_uint8)), T.dptr(gd)))
        return {"pos": pos, "parent": parent, "nn_seq": nn_seq[:it], "accept": accept[:it], "goal_dist": gd[: nv - 1]}

    def close(self):
        if self.h:
            self.lib.rkh_planner_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RrtPlannerPool:
    """A batch of RRT problems split over `groups` rkh_planner handles, each with its own HIP stream, driven round-robin
    from one host thread: enqueue is asynchronous, so while one group's steer kernel drains its last waves the other
    group's NN sweep and bookkeeping kernels fill the machine (measured +13-15 % with two groups of 128 problems over one
    group of 256; four groups: no further gain).  Same interface as RrtPlanner; problem indices are global."""

    def __init__(self, scene, prms, groups=2, dyn=None, qs=None):
        prms = list(prms)
        groups = max(1, min(groups, len(prms)))
        cut = [len(prms) * g // groups for g in range(groups + 1)]
        self.planners = [RrtPlanner(scene, prms[cut[g]:cut[g + 1]], dyn=dyn, qs=qs) for g in range(groups)]
        self.offsets = cut
        self.P, self.D = len(prms), self.planners[0].D

    @property
    def all_stats(self):
        return [s for pl in self.planners for s in pl.all_stats]

    @property
    def stats(self):
        return self.planners[0].all_stats[0]

    @property
    def done(self):
        return all(pl.done for pl in self.planners)

    def enqueue(self, rounds):
        for pl in self.planners:
            if rounds == 0 or not pl.done:
                pl.enqueue(rounds)

    def sync(self):
        for pl in self.planners:
            pl.sync()
        return self.stats

    def solve_planning_query(self, rounds_per_sync=16):
        self.enqueue(0)
        while True:
            self.enqueue(rounds_per_sync)
            self.sync()
            if self.done:
                return self.stats

    def _local(self, problem):
        for g, pl in enumerate(self.planners):
            if problem < self.offsets[g + 1]:
                return pl, problem - self.offsets[g]
        raise IndexError(problem)

    def tree(self, problem=0):
        pl, i = self._local(problem)
        return pl.tree(i)

    def solution(self, problem=0):
        pl, i = self._local(problem)
        return pl.solution(i)

    def nn_profile(self):
        prof = [pl.nn_profile() for pl in self.planners]
        return sum(p[0] for p in prof), sum(p[1] for p in prof), sum(p[2] for p in prof)

    def nn_pairs(self):
        return sum(pl.nn_pairs() for pl in self.planners)

    def steer_profile(self):
        prof = [pl.steer_profile() for pl in self.planners]
        return sum(p[0] for p in prof), sum(p[1] for p in prof)

    def steer_steps(self):
        return sum(pl.steer_steps() for pl in self.planners)

    def carry_counts(self):
        counts = [pl.carry_counts() for pl in self.planners]
        return sum(c[0] for c in counts), sum(c[1] for c in counts)

    def probe_counts(self):
        """(goal probes settled at commit, goal probes a steer launch ran), summed over all problems."""
        counts = [pl.probe_counts(i) for pl in self.planners for i in range(pl.P)]
        return sum(c["certified"] for c in counts), sum(c["run"] for c in counts)

    def close(self):
        for pl in self.planners:
            pl.close()


class RrtStarPlanner:
    """rrtstar_planner (unidirectional, linear-search k-NN), batch of problems; `space` is a quasi-static space
    (make_qs_space: vertices = joint positions) or a steerable dynamic space (T.DynSpace: vertices = states (q, qd))."""

    def __init__(self, scene, prm, space):
        self.scene, self.lib, self.qs = scene, scene.lib, space
        self.prms = list(prm) if isinstance(prm, (list, tuple)) else [prm]
        dynamic = isinstance(space, T.DynSpace)
        self.P, self.D = len(self.prms), (2 * space.n_dof if dynamic else space.n_dof)
        self._prm_arr = T.as_array(self.prms, T.RrtParams)
        self.h = C.c_void_p()
        create = self.lib.rkh_rrtstar_create_batch if dynamic else self.lib.rkh_rrtstar_create_qs_batch
        _check(create(scene.h, C.byref(space), self._prm_arr, self.P, C.byref(self.h)))
        self.all_stats = (RrtStarStats * self.P)()

    @property
    def stats(self):
        return self.all_stats[0]

    def solve_planning_query(self, max_loop_iterations=-1):
        _check(self.lib.rkh_rrtstar_solve(self.h, int(max_loop_iterations), self.all_stats))
        return self.all_stats[0]

    def set_branch_and_bound(self, enabled=True):
        """USE_BRANCH_AND_BOUND_PRUNING_FLAG: branch_and_bound_connector instead of lazy_node_connector."""
        _check(self.lib.rkh_rrtstar_set_branch_and_bound(self.h, 1 if enabled else 0))

    def removed(self, problem=0):
        out = np.zeros(int(self.all_stats[problem].num_vertices), dtype=np.uint8)
        _check(self.lib.rkh_rrtstar_get_removed(self.h, problem, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def solution(self, problem=0):
        n, cost = C.c_uint32(), C.c_double()
        _check(self.lib.rkh_rrtstar_get_solution(self.h, problem, None, 0, C.byref(n), C.byref(cost)))
        path = np.zeros(max(n.value, 1), dtype=np.uint32)
        _check(self.lib.rkh_rrtstar_get_solution(self.h, problem, T.u32ptr(path), len(path), C.byref(n), C.byref(cost)))
        return path[: n.value], cost.value

    def graph(self, problem=0):
        st = self.all_stats[problem]
        nv, it = int(st.num_vertices), int(st.loop_iterations)
        pos = np.zeros((nv, self.D))
        pred = np.zeros(nv, dtype=np.uint32)
        dist = np.zeros(nv)
        near = np.zeros(max(it, 1), dtype=np.uint32)
        _check(self.lib.rkh_rrtstar_get_graph(self.h, problem, T.dptr(pos), T.u32ptr(pred), T.dptr(dist), T.u32ptr(near)))
        return {"pos": pos, "pred": pred, "dist": dist, "near_seq": near[:it]}

    def close(self):
        if self.h:
            self.lib.rkh_rrtstar_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BiRrtStarStats(C.Structure):
    _fields_ = [("num_vertices", C.c_uint64), ("samples", C.c_uint64), ("loop_iterations", C.c_uint64),
                ("rewires", C.c_uint64), ("fwd_rewires", C.c_uint64), ("joins", C.c_uint64), ("edges_checked", C.c_uint64),
                ("best_join_cost", C.c_double)]


class BiRrtStarPlanner:
    """rrtstar_planner with BIDIRECTIONAL_PLANNING over the quasi-static free space, batch of problems."""

    def __init__(self, scene, prm, qs):
        self.scene, self.lib, self.qs = scene, scene.lib, qs
        self.prms = list(prm) if isinstance(prm, (list, tuple)) else [prm]
        self.P, self.D = len(self.prms), qs.n_dof
        self._prm_arr = T.as_array(self.prms, T.RrtParams)
        self.h = C.c_void_p()
        _check(self.lib.rkh_birrtstar_create_qs_batch(scene.h, C.byref(qs), self._prm_arr, self.P, C.byref(self.h)))
        self.all_stats = (BiRrtStarStats * self.P)()

    @property
    def stats(self):
        return self.all_stats[0]

    def solve_planning_query(self, max_loop_iterations=-1):
        _check(self.lib.rkh_birrtstar_solve(self.h, int(max_loop_iterations), self.all_stats))
        return self.all_stats[0]

    def graph(self, problem=0):
        st = self.all_stats[problem]
        nv, it = int(st.num_vertices), max(int(st.loop_iterations), 1)
        pos = np.zeros((nv, self.D))
        pred = np.zeros(nv, dtype=np.uint32); succ = np.zeros(nv, dtype=np.uint32)
        dist = np.zeros(nv); fwd = np.zeros(nv)
        npred = np.zeros(it, dtype=np.uint32); nsucc = np.zeros(it, dtype=np.uint32)
        _check(self.lib.rkh_birrtstar_get_graph(self.h, problem, T.dptr(pos), T.u32ptr(pred), T.dptr(dist), T.u32ptr(succ),
                                                T.dptr(fwd), T.u32ptr(npred), T.u32ptr(nsucc)))
        n = int(st.loop_iterations)
        return {"pos": pos, "pred": pred, "dist": dist, "succ": succ, "fwd_dist": fwd, "near_pred": npred[:n],
                "near_succ": nsucc[:n]}

    def close(self):
        if self.h:
            self.lib.rkh_rrtstar_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PrmPlanner:
    """prm_planner (linear-search k-NN, adjacency-list motion graph), batch of problems; `space` is a quasi-static space
    (make_qs_space) or a steerable dynamic space (T.DynSpace: vertices = states (q, qd))."""

    def __init__(self, scene, prm, space):
        self.scene, self.lib, self.qs = scene, scene.lib, space
        self.prms = list(prm) if isinstance(prm, (list, tuple)) else [prm]
        dynamic = isinstance(space, T.DynSpace)
        self.P, self.D = len(self.prms), (2 * space.n_dof if dynamic else space.n_dof)
        self._prm_arr = T.as_array(self.prms, T.PrmParams)
        self.h = C.c_void_p()
        create = self.lib.rkh_prm_create_batch if dynamic else self.lib.rkh_prm_create_qs_batch
        _check(create(scene.h, C.byref(space), self._prm_arr, self.P, C.byref(self.h)))
        self.all_stats = (PrmStats * self.P)()

    @property
    def stats(self):
        return self.all_stats[0]

    def solve_planning_query(self, max_loop_iterations=-1):
        _check(self.lib.rkh_prm_solve(self.h, int(max_loop_iterations), self.all_stats))
        return self.all_stats[0]

    def graph(self, problem=0):
        st = self.all_stats[problem]
        nv, ne, it = int(st.num_vertices), int(st.num_edges), int(st.loop_iterations)
        pos = np.zeros((nv, self.D))
        eu = np.zeros(max(ne, 1), dtype=np.uint32)
        ev = np.zeros(max(ne, 1), dtype=np.uint32)
        ew = np.zeros(max(ne, 1))
        dens = np.zeros(nv)
        cc = np.zeros(nv, dtype=np.uint32)
        kind = np.zeros(max(it, 1), dtype=np.uint8)
        exp = np.zeros(max(it, 1), dtype=np.uint32)
        _check(self.lib.rkh_prm_get_graph(self.h, problem, T.dptr(pos), T.u32ptr(eu), T.u32ptr(ev), T.dptr(ew), T.dptr(dens),
                                          T.u32ptr(cc), kind.ctypes.data_as(C.POINTER(C.c_uint8)), T.u32ptr(exp)))
        return {"pos": pos, "edge_u": eu[:ne], "edge_v": ev[:ne], "edge_w": ew[:ne], "density": dens, "cc_root": cc,
                "kind": kind[:it], "expanded": exp[:it]}

    # ---- roadmap queries (prm_planner_visitor::publish_path's search, on the roadmap as it stands)
    def shortest_paths(self, sources, problem=0):
        """(dist [S][num_vertices], pred [S][num_vertices]) from each source vertex; pred: 0xFFFFFFFF = none."""
        src = np.ascontiguousarray(sources, dtype=np.uint32).reshape(-1)
        nv = int(self.all_stats[problem].num_vertices)
        dist = np.zeros((len(src), nv))
        pred = np.zeros((len(src), nv), dtype=np.uint32)
        _check(self.lib.rkh_prm_shortest_paths(self.h, problem, T.u32ptr(src), len(src), T.dptr(dist), T.u32ptr(pred)))
        return dist, pred

    def solution(self, problem=0):
        """(path, cost): start (vertex 0) -> goal (vertex 1) through the roadmap; path is empty and cost +inf if they are
        not connected."""
        n, cost = C.c_uint32(0), C.c_double(0.0)
        _check(self.lib.rkh_prm_get_solution(self.h, problem, None, 0, C.byref(n), C.byref(cost)))
        path = np.zeros(max(n.value, 1), dtype=np.uint32)
        _check(self.lib.rkh_prm_get_solution(self.h, problem, T.u32ptr(path), len(path), C.byref(n), C.byref(cost)))
        return path[:n.value], cost.value

    def query_paths(self, starts, goals, k, radius, problem=0, capacity=None):
        """Multi-query over a quasi-static roadmap: (cost [B], paths: list of B arrays of roadmap vertex ids in travel
        order; empty and +inf where no path exists).  capacity: path slots per query (default: the vertex count)."""
        a = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, self.D)
        b = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, self.D)
        assert len(a) == len(b)
        B = len(a)
        cap = int(self.all_stats[problem].num_vertices) if capacity is None else int(capacity)
        cost = np.zeros(max(B, 1))
        path = np.zeros((max(B, 1), max(cap, 1)), dtype=np.uint32)
        n_path = np.zeros(max(B, 1), dtype=np.uint32)
        _check(self.lib.rkh_prm_query_paths(self.h, problem, T.dptr(a), T.dptr(b), B, int(k), float(radius), cap,
                                            T.dptr(cost), T.u32ptr(path), T.u32ptr(n_path)))
        return cost[:B], [path[i, :min(int(n_path[i]), cap)].copy() for i in range(B)]

    def search_ms(self, sources=None, problem=0, runs=5):
        """rkh_diag_prm_search_ms: (ms [runs], max_rounds, host_dijkstra_ms); sources None: vertex 0 of every problem."""
        ms = np.zeros(runs, dtype=np.float32)
        rounds, host = C.c_uint32(0), C.c_double(0.0)
        if sources is None:
            _check(self.lib.rkh_diag_prm_search_ms(self.h, 0xFFFFFFFF, None, 0, runs, ms.ctypes.data_as(C.POINTER(C.c_float)),
                                                   C.byref(rounds), C.byref(host)))
        else:
            src = np.ascontiguousarray(sources, dtype=np.uint32).reshape(-1)
            _check(self.lib.rkh_diag_prm_search_ms(self.h, problem, T.u32ptr(src), len(src), runs,
                                                   ms.ctypes.data_as(C.POINTER(C.c_float)), C.byref(rounds), C.byref(host)))
        return ms, rounds.value, host.value

    def close(self):
        if self.h:
            self.lib.rkh_prm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BiRrtPlanner:
    """rrt_planner with BIDIRECTIONAL_PLANNING over the quasi-static free space, batch of problems."""

    def __init__(self, scene, prm, qs):
        self.scene, self.lib, self.qs = scene, scene.lib, qs
        self.prms = list(prm) if isinstance(prm, (list, tuple)) else [prm]
        self.P, self.D = len(self.prms), qs.n_dof
        self._prm_arr = T.as_array(self.prms, T.RrtParams)
        self.h = C.c_void_p()
        _check(self.lib.rkh_birrt_create_qs_batch(scene.h, C.byref(qs), self._prm_arr, self.P, C.byref(self.h)))
        self.all_stats = (BiRrtStats * self.P)()

    @property
    def stats(self):
        return self.all_stats[0]

    def solve_planning_query(self, max_loop_iterations=-1):
        _check(self.lib.rkh_birrt_solve(self.h, int(max_loop_iterations), self.all_stats))
        return self.all_stats[0]

    def solution(self, problem=0):
        n1, n2, cost = C.c_uint32(), C.c_uint32(), C.c_double()
        _check(self.lib.rkh_birrt_get_solution(self.h, problem, None, C.byref(n1), None, C.byref(n2), 0, C.byref(cost)))
        cap = max(n1.value, n2.value, 1)
        p1 = np.zeros(cap, dtype=np.uint32); p2 = np.zeros(cap, dtype=np.uint32)
        _check(self.lib.rkh_birrt_get_solution(self.h, problem, T.u32ptr(p1), C.byref(n1), T.u32ptr(p2), C.byref(n2), cap,
                                               C.byref(cost)))
        return p1[: n1.value], p2[: n2.value], cost.value

    def trees(self, problem=0):
        st = self.all_stats[problem]
        n1, n2, it = int(st.num_vertices_1), int(st.num_vertices_2), int(st.loop_iterations)
        p1 = np.zeros((n1, self.D)); q1 = np.zeros(n1, dtype=np.uint32)
        p2 = np.zeros((n2, self.D)); q2 = np.zeros(n2, dtype=np.uint32)
        nn = np.zeros(max(2 * it, 1), dtype=np.uint32); acc = np.zeros(max(2 * it, 1), dtype=np.uint8)
        _check(self.lib.rkh_birrt_get_trees(self.h, problem, T.dptr(p1), T.u32ptr(q1), T.dptr(p2), T.u32ptr(q2), T.u32ptr(nn),
                                            acc.ctypes.data_as(C.POINTER(C.c_uint8))))
        return {"pos1": p1, "parent1": q1, "pos2": p2, "parent2": q2, "nn_seq": nn[: 2 * it], "accept": acc[: 2 * it]}

    def close(self):
        if self.h:
            self.lib.rkh_birrt_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
