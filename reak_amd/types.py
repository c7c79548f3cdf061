"""ctypes mirrors of include/rkh_types.h (the POD scene description that crosses the C-ABI)."""
import ctypes as C
import math

import numpy as np

RKH_MAX_DOF = 16
RKH_MAX_STATE = 2 * RKH_MAX_DOF

# rkh_kte_kind
KTE_DRIVING_ACTUATOR_GEN = 1
KTE_INERTIA_GEN = 2
KTE_REVOLUTE_JOINT_3D = 3
KTE_RIGID_LINK_3D = 4
KTE_INERTIA_3D = 5
KTE_FLEXIBLE_BEAM_3D = 6
KTE_REVOLUTE_JOINT_2D = 7
KTE_RIGID_LINK_2D = 8
KTE_INERTIA_2D = 9
KTE_PRISMATIC_JOINT_3D = 10  # mAxis as given (prismatic_joint_3D does not normalise it)
KTE_PRISMATIC_JOINT_2D = 11  # planar chains: axis[0..1] = mAxis as given, axis[2] ignored

# rkh_shape_kind
SHAPE_SPHERE = 1
SHAPE_BOX = 2
SHAPE_CCYLINDER = 3
SHAPE_CIRCLE = 4
SHAPE_RECTANGLE = 5
SHAPE_CRECT = 6
SHAPE_PLANE = 7      # dims = (x extent, y extent); normal = local z
SHAPE_CYLINDER = 8   # dims = (length, radius); flat ends, axis = local z
SHAPE_MESH = 9       # convex vertex set: dims = (first vertex in the scene's pool, vertex count)


class Pose(C.Structure):
    _fields_ = [("pos", C.c_double * 3), ("quat", C.c_double * 4)]


class KteOp(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("coord", C.c_int32),
        ("base_frame", C.c_int32),
        ("end_frame", C.c_int32),
        ("joint_op", C.c_int32),
        ("upstream", C.c_uint32),
        ("axis", C.c_double * 3),
        ("offset", Pose),
        ("mass", C.c_double),
        ("inertia", C.c_double * 6),
    ]


class ChainBase(C.Structure):
    _fields_ = [("pose", Pose), ("acceleration", C.c_double * 3)]


class Shape(C.Structure):
    _fields_ = [("kind", C.c_int32), ("anchor", C.c_int32), ("pose", Pose), ("dims", C.c_double * 3)]


class DynSpace(C.Structure):
    _fields_ = [
        ("n_dof", C.c_int32),
        ("steps_per_edge", C.c_int32),
        ("dt", C.c_double),
        ("kp", C.c_double),
        ("kd", C.c_double),
        ("u_max", C.c_double),
        ("goal_tol", C.c_double),
        ("lower", C.c_double * RKH_MAX_STATE),
        ("upper", C.c_double * RKH_MAX_STATE),
    ]


class QsSpace(C.Structure):
    _fields_ = [("n_dof", C.c_int32), ("pad", C.c_int32), ("min_interval", C.c_double),
                ("lower", C.c_double * RKH_MAX_DOF), ("upper", C.c_double * RKH_MAX_DOF),
                ("speed_limits", C.c_double * RKH_MAX_DOF)]


class RrtParams(C.Structure):
    _fields_ = [
        ("seed", C.c_uint32),
        ("max_vertices", C.c_uint32),
        ("max_results", C.c_uint32),
        ("steer_tol", C.c_double),
        ("conn_tol", C.c_double),
        ("start", C.c_double * RKH_MAX_STATE),
        ("goal", C.c_double * RKH_MAX_STATE),
    ]


class PrmParams(C.Structure):
    _fields_ = [("base", RrtParams), ("sampling_radius", C.c_double), ("expand_probability", C.c_double)]


class IkParams(C.Structure):
    """rkh_ik_params (include/rkh.h): the damped least-squares pose iteration of rkh_inverse_kinematics."""
    _fields_ = [("struct_size", C.c_uint32), ("max_iters", C.c_uint32), ("damping", C.c_double), ("max_step", C.c_double),
                ("tol_pos", C.c_double), ("tol_rot", C.c_double)]


def make_ik_params(max_iters=100, damping=0.02, max_step=0.5, tol_pos=1e-6, tol_rot=1e-6):
    return IkParams(struct_size=C.sizeof(IkParams), max_iters=int(max_iters), damping=float(damping),
                    max_step=float(max_step), tol_pos=float(tol_pos), tol_rot=float(tol_rot))


class SvpSpace(C.Structure):
    """rkh_svp_space (include/rkh_types.h): the order-1 rate-limited joint space with SVP profiles."""
    _fields_ = [("struct_size", C.c_uint32), ("n_dof", C.c_int32), ("min_interval", C.c_double),
                ("lower", C.c_double * RKH_MAX_DOF), ("upper", C.c_double * RKH_MAX_DOF),
                ("speed_limits", C.c_double * RKH_MAX_DOF), ("accel_limits", C.c_double * RKH_MAX_DOF)]


def make_svp_space(n_dof, lower, upper, min_interval, speed_limits=None, accel_limits=None):
    """lower / upper: the position box in space coordinates; limits None or 0: unit limits."""
    sp = SvpSpace(struct_size=C.sizeof(SvpSpace), n_dof=int(n_dof), min_interval=float(min_interval))
    for i in range(int(n_dof)):
        sp.lower[i], sp.upper[i] = float(lower[i]), float(upper[i])
        sp.speed_limits[i] = 0.0 if speed_limits is None else float(speed_limits[i])
        sp.accel_limits[i] = 0.0 if accel_limits is None else float(accel_limits[i])
    return sp


class SvpRrtParams(C.Structure):
    """rkh_svp_rrt_params (include/rkh_types.h): one problem of the batch RRT over the SVP space."""
    _fields_ = [("struct_size", C.c_uint32), ("seed", C.c_uint32), ("max_vertices", C.c_uint32), ("max_iterations", C.c_uint32),
                ("max_edge_time", C.c_double), ("steer_tol", C.c_double), ("has_goal", C.c_uint32), ("pad", C.c_uint32),
                ("start", C.c_double * RKH_MAX_STATE), ("goal", C.c_double * RKH_MAX_STATE)]


def make_svp_rrt_params(start, goal=None, seed=1, max_vertices=200, max_iterations=20000, max_edge_time=1.0, steer_tol=0.1):
    """start / goal: points (p0, v0, p1, v1, ...) in space coordinates; goal None: no goal probes"""
    pr = SvpRrtParams(struct_size=C.sizeof(SvpRrtParams), seed=int(seed), max_vertices=int(max_vertices),
                      max_iterations=int(max_iterations), max_edge_time=float(max_edge_time), steer_tol=float(steer_tol),
                      has_goal=0 if goal is None else 1)
    for i, v in enumerate(start):
        pr.start[i] = float(v)
    if goal is not None:
        for i, v in enumerate(goal):
            pr.goal[i] = float(v)
    return pr


def make_pose(pos=(0.0, 0.0, 0.0), quat=(1.0, 0.0, 0.0, 0.0)):
    p = Pose()
    p.pos[:] = [float(v) for v in pos]
    p.quat[:] = [float(v) for v in quat]
    return p


def make_pose_2d(pos=(0.0, 0.0), angle=0.0):
    """pose_2D carried in rkh_pose: pos[0..1] = Position, quat[0..1] = rot_mat_2D::q = (cos, sin)."""
    p = Pose()
    p.pos[:] = [float(pos[0]), float(pos[1]), 0.0]
    if angle == 0.0:
        p.quat[:] = [1.0, 0.0, 0.0, 0.0]  # rot_mat_2D() default: identity
    else:
        p.quat[:] = [math.cos(angle), math.sin(angle), 0.0, 0.0]
    return p


def as_array(items, ctype):
    arr = (ctype * len(items))()
    for i, it in enumerate(items):
        arr[i] = it
    return arr


def dptr(a):
    """double* view of a C-contiguous float64 numpy array."""
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_double))


def u32ptr(a):
    assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_uint32))
