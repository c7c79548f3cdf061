"""The kinematics entries without a GPU: the device header under sanitizers, the Python twin's own pins, the boundary.

The twin (tests/ik_ref.py) is what the GPU tests compare the device with, so it is pinned first, against things it shares
no code with: the twist Chain.do_motion leaves in a frame, the 50-digit forward kinematics of tests/lagrange_ref.py with its
geometric Jacobians, and a 50-digit central difference of those along the joint rates."""
import os
import re
import subprocess

import numpy as np
import pytest

import ik_ref
import kte_ref as K
import lagrange_ref as LR
from reak_amd import scenarios

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAMILIES = {
    "c2": lambda: scenarios.make_c2(world_seed=1),
    "track": scenarios.make_crs_a465_track,
    "mixed4_p12": lambda: LR.mixed_chain(4, (1, 2)),   # two prismatic joints along scaled, non-unit axes
    "c1_planar": scenarios.make_c1_planar,
    "planar_mixed4": lambda: scenarios.make_planar_mixed(n=4),
}


def _states(scn, count, seed):
    rng = np.random.default_rng(seed)
    n = scn.n_dof
    lo = np.array([scn.dyn.lower[2 * j] for j in range(n)])
    hi = np.array([scn.dyn.upper[2 * j] for j in range(n)])
    lo, hi = np.maximum(lo, -np.pi), np.minimum(hi, np.pi)
    return rng.uniform(lo, hi, size=(count, n)), rng.uniform(-1.0, 1.0, size=(count, n))


def test_device_header_on_the_host_under_sanitizers(tmp_path):
    """reak_amd/csrc/kinematics_device.h through the host stand-in, against hand-worked frames, twists, columns, column
    rates, the pose error and the 6 x 6 solve; a program of its own, AddressSanitizer + UBSan linked in."""
    exe = str(tmp_path / "kinematics_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tests", "cpp", "hip_host"),
                    os.path.join(ROOT, "tests", "cpp", "kinematics_host.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "kinematics host ok:" in out.stdout


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_jacobian_times_rates_is_the_frames_twist(family):
    """J qd = (velocity rotated into the frame, angular velocity) of doMotion, every frame of the chain, to 1e-12."""
    scn = FAMILIES[family]()
    kin = ik_ref.kin(scn)
    worst = 0.0
    for q, qd in zip(*_states(scn, 3, 5)):
        for f in ik_ref.all_frames(scn):
            J, _ = kin.jacobians(q, qd, f, dot=False)
            fa = kin.frame_arrays(q, qd, [f])
            if ik_ref.is_planar(scn):
                R = fa["rot"][0]
                want = np.array([fa["vel"][0][0] * R[0] + fa["vel"][0][1] * R[1], fa["vel"][0][1] * R[0] - fa["vel"][0][0] * R[1],
                                 fa["ang_vel"][0]])
            else:
                want = np.concatenate([K.vmul(tuple(fa["vel"][0]), K.q_rotmat(tuple(fa["rot"][0]))), fa["ang_vel"][0]])
            worst = max(worst, np.abs(J @ qd - want).max())
    print(family, "worst |J qd - twist|", worst)
    assert worst <= 1e-12


def _mp_jacobian(model, q, frame):
    """Geometric Jacobian of `frame` from lagrange_ref's 50-digit forward kinematics, rotated into the frame: rows
    (v [3], w [3]) as lists of mpf, columns of the joints on the frame's own path through the frame tree."""
    fr, joints = model.fk(q)
    p, R = fr[frame]
    Rt = LR._mt(R)
    js, f = [], frame
    while f is not None:
        f, c = model.parent[f]
        if c is not None:
            js.append(c)
    J = [[LR._ZERO] * model.n for _ in range(6)]
    for c in js:
        a, pc = joints[c]
        if model.kind[c] == "R":
            v, w = LR._mv(Rt, LR._cross(a, LR._sub(p, pc))), LR._mv(Rt, a)
        else:
            v, w = LR._mv(Rt, a), [LR._ZERO] * 3
        for r in range(3):
            J[r][c], J[3 + r][c] = v[r], w[r]
    return J


def _rows(J6, planar):
    """The twin's row set from the six spatial rows: planar chains keep (vx, vy, omega_z)."""
    rows = (0, 1, 5) if planar else range(6)
    return np.array([[float(J6[r][c]) for c in range(len(J6[0]))] for r in rows])


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_jacobians_against_the_50_digit_kinematics(family):
    """Jac = the geometric Jacobian of tests/lagrange_ref.py rotated into the frame, to 1e-11 max(1, reach); JacDot = its
    central difference along the rates (step 1e-20 at 50 digits), to 1e-11 max(1, reach |qd|)."""
    scn = FAMILIES[family]()
    kin, model, planar = ik_ref.kin(scn), LR.Model(scn), ik_ref.is_planar(scn)
    reach = ik_ref.reach(scn)
    frames = ik_ref.all_frames(scn)
    frames = frames if len(frames) <= 9 else frames[:3] + frames[-6:]   # the base, the first joint, the far end
    wj = wd = 0.0
    for q, qd in zip(*_states(scn, 2, 9)):
        qm, qdm = [LR.mpf(float(v)) for v in q], [LR.mpf(float(v)) for v in qd]
        bar_d = 1e-11 * max(1.0, reach * float(np.linalg.norm(qd)))
        for f in frames:
            J, Jd = kin.jacobians(q, qd, f)
            ref = _rows(_mp_jacobian(model, qm, f), planar)
            hi = _mp_jacobian(model, [a + LR.STEP * b for a, b in zip(qm, qdm)], f)
            lo = _mp_jacobian(model, [a - LR.STEP * b for a, b in zip(qm, qdm)], f)
            ref_d = _rows([[(h - l) / (2 * LR.STEP) for h, l in zip(hr, lr)] for hr, lr in zip(hi, lo)], planar)
            ej, ed = np.abs(J - ref).max(), np.abs(Jd - ref_d).max()
            wj, wd = max(wj, ej), max(wd, ed / bar_d)
            assert ej <= 1e-11 * max(1.0, reach), (family, f, ej)
            assert ed <= bar_d, (family, f, ed, bar_d)
            up = ik_ref.upstream(scn)[f]
            for i in range(scn.n_dof):   # the columns of joints that are not upstream are exact zeros
                if not (up >> i) & 1:
                    assert not J[:, i].any() and not Jd[:, i].any()
    print(family, "reach", reach, "worst |J - ref|", wj, "worst |Jdot - ref| / bar", wd)


def test_twin_ik_converges_and_certifies_itself():
    """The iteration of include/rkh.h on the twin: from seeds within 0.3 per joint of a target's own configuration it
    converges, and what it returns meets the target within the tolerances."""
    scn = scenarios.make_c2(world_seed=1)
    kin = ik_ref.Kin3(scn)
    frame = max(ik_ref.all_frames(scn))
    from reak_amd import types as T
    prm = T.make_ik_params()
    rng = np.random.default_rng(3)
    lower, upper = [-np.pi] * 6, [np.pi] * 6
    for _ in range(3):
        qt = rng.uniform(-2.5, 2.5, size=6)
        tg = ik_ref.fk_pose(kin, frame, qt)
        r = ik_ref.ik_solve(kin, frame, tg, qt + rng.uniform(-0.3, 0.3, size=6), lower, upper, prm)
        assert r["converged"] and 0 < r["iters"] <= 100
        fr, _ = kin.motion(r["q"])
        _, rp, rr = ik_ref.pose_error(fr[frame], tuple(tg.pos), tuple(tg.quat))
        assert rp <= prm.tol_pos and rr <= prm.tol_rot and rp == r["res_pos"] and rr == r["res_rot"]


def test_boundary_declares_the_entries_and_keeps_its_abi_number():
    from reak_amd import lib as L

    hdr = open(os.path.join(ROOT, "include", "rkh.h")).read()
    lib_py = open(os.path.join(ROOT, "reak_amd", "lib.py")).read()
    for name in ("rkh_direct_kinematics", "rkh_direct_kinematics_2d", "rkh_jacobians", "rkh_jacobians_2d",
                 "rkh_inverse_kinematics"):
        assert re.search(r"rkh_status " + name + r"\(", hdr), name
        assert name in L.EXPORTS and ("lib." + name + ".argtypes") in lib_py, name
    assert "typedef struct rkh_ik_params" in hdr
    assert re.search(r"#define RKH_ABI_VERSION 3u\b", hdr) and L.ABI_VERSION == 3
    # the handshake's argument list is what it was: the IK parameters carry their own struct_size
    assert "sizeof_ik" not in hdr and len(L.abi_sizes()) == 10
    import ctypes as C

    from reak_amd import types as T
    assert C.sizeof(T.IkParams) == 40 and T.make_ik_params().struct_size == 40
