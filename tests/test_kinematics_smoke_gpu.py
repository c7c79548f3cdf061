"""The C++ adaptors over the kinematics entries (include/rkh_adaptors.hpp: hip_direct_kin_map with map_to_space's call
shape, hip_manip_kinematics_model's getJacobianMatrix / getJacobianMatrixAndDerivative, hip_pose_ik): tests/cpp/
kinematics_smoke.cpp, g++ against librkh.so, gives the Python binding's answers for the same inputs, bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

import ik_ref
from reak_amd import scenarios
from reak_amd import types as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_cpp_adaptors_answer_as_the_binding_does(tmp_path):
    from reak_amd import lib as L

    scn = scenarios.make_c2(world_seed=1)
    n, frame = scn.n_dof, 12
    src, exe = os.path.join(ROOT, "tests", "cpp", "kinematics_smoke.cpp"), os.path.join(ROOT, "tests", "cpp", "kinematics_smoke")
    newer = [src, os.path.join(ROOT, "include", "rkh_adaptors.hpp"), os.path.join(ROOT, "include", "rkh.h")]
    if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(f) for f in newer)):
        lib_dir = os.path.join(ROOT, "reak_amd")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                        "-L", lib_dir, "-lrkh", "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    rng = np.random.default_rng(7)
    states = rng.uniform(-1.5, 1.5, size=(5, 2 * n))
    q, qd = states[:, 0::2].copy(), states[:, 1::2].copy()
    kin = ik_ref.Kin3(scn)
    qt = rng.uniform(-2.0, 2.0, size=n)
    target = ik_ref.fk_pose(kin, frame, qt)
    seeds = qt + rng.uniform(-0.2, 0.2, size=(4, n))
    lo, hi = np.full(n, -np.pi), np.full(n, np.pi)
    blob = tmp_path / "kinematics_scene.bin"
    with open(blob, "wb") as f:
        f.write(np.int32(len(scn.ops)).tobytes())
        f.write(bytes(scn.ops_array()))
        f.write(bytes(scn.base))
        f.write(np.int32(len(scn.shapes)).tobytes())
        f.write(bytes(scn.shapes_array()))
        f.write(np.int32([n, frame, len(states)]).tobytes())
        f.write(np.ascontiguousarray(states).tobytes())
        f.write(bytes(target))
        f.write(np.int32(len(seeds)).tobytes())
        f.write(np.ascontiguousarray(seeds).tobytes())
        f.write(lo.tobytes())
        f.write(hi.tobytes())
    run = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    out = json.loads(run.stdout.strip().splitlines()[-1])
    ctx = L.Context(0)
    sc = L.Scene(ctx, scn)
    fk = sc.direct_kinematics(q, [frame], qd)
    for key, name in (("pos", "pos"), ("quat", "rot"), ("vel", "vel"), ("ang_vel", "ang_vel")):
        assert out[key] == list(fk[name][0, 0]), key
    assert out["last_pos"] == list(fk["pos"][-1, 0]) and out["last_vel"] == list(fk["vel"][-1, 0])
    assert out["still_pos"] == out["pos"] and out["still_vel"] == [0.0, 0.0, 0.0]
    jj = sc.jacobians(q[:1], [frame, 0], qd[:1])
    assert out["jac"] == list(jj["jac"].reshape(-1)) and out["jac_dot"] == list(jj["jac_dot"].reshape(-1))
    assert not any(out["jac"][6 * n:]) and any(out["jac_dot"][:6 * n])   # the base frame's rows: zeros
    assert out["getters_agree"] and out["bad_point_throws"]
    ik = sc.inverse_kinematics(frame, [target], seeds[None], lo, hi, T.make_ik_params())
    good = np.flatnonzero(ik["converged"][0] & ik["free"][0])
    assert out["n_solutions"] == len(good)
    if len(good):
        assert out["first_solution"] == list(ik["q"][0, good[0]]) and ik["best"][0] == good[0]
    assert ik["converged"].all()
