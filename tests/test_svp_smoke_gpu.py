"""The rkh_svp_* entries through the C header: tests/cpp/svp_smoke.cpp, g++ against librkh.so, gives the Python binding's
answers for the same inputs, bit for bit, and a struct of another size is refused."""
import json
import os
import subprocess

import numpy as np
import pytest

import svp_ref as R
from reak_amd import scenarios

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _floats(v):
    return np.array([float(x) for x in v])


def test_the_c_entries_answer_as_the_binding_does(tmp_path):
    from reak_amd import lib as L

    scn = scenarios.make_c2(world_seed=1)
    n = scn.n_dof
    src, exe = os.path.join(ROOT, "tests", "cpp", "svp_smoke.cpp"), str(tmp_path / "svp_smoke")
    lib_dir = os.path.join(ROOT, "reak_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                    "-L", lib_dir, "-lrkh", "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    sp = R.Space(n, [-2.0] * n, [2.0] * n, 0.06, [1.0, 0.0, 1.5, 2.0, 0.5, 1.0], [2.0, 4.0, 0.0, 3.0, 2.0, 4.0])
    a, b, _ = R.random_pairs(sp, 34, seed=9)
    a[:30, 1::2] = 0.0
    B = len(a)
    fraction = np.array([(1.0, 0.37, 0.0)[e % 3] for e in range(B)])
    cs = sp.c_space()
    blob = tmp_path / "svp_scene.bin"
    with open(blob, "wb") as f:
        f.write(np.int32(len(scn.ops)).tobytes())
        f.write(bytes(scn.ops_array()))
        f.write(bytes(scn.base))
        f.write(np.int32(len(scn.shapes)).tobytes())
        f.write(bytes(scn.shapes_array()))
        f.write(bytes(cs))
        f.write(np.int32(B).tobytes())
        f.write(a.tobytes())
        f.write(b.tobytes())
        f.write(fraction.tobytes())
    run = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    out = json.loads(run.stdout.strip().splitlines()[-1])
    ctx = L.Context(0)
    space = L.SvpSpace(cs, scene=L.Scene(ctx, scn))
    same = lambda key, want: np.array_equal(_floats(out[key]).view(np.uint64), np.ascontiguousarray(want, dtype=np.float64).reshape(-1).view(np.uint64))
    assert out["in_bounds"] == space.in_bounds(a).astype(int).tolist()
    time, peak = space.reach_time(a, b)
    assert same("time", time) and same("peak", peak) and np.isinf(time).any() and np.isfinite(time).sum() > 20
    idx, dist = space.nearest(a, b[:3], 4, 0)
    assert out["knn_idx"] == idx.reshape(-1).tolist() and same("knn_dist", dist)
    o, rt, nc, re = space.edge_check(a, b, fraction)
    assert same("out", o) and same("walk_time", rt) and out["n_checked"] == nc.tolist() and out["reached"] == re.tolist()
    assert max(out["n_checked"]) > 32 and 0 < sum(out["reached"]) < B
    t = np.where(np.isfinite(time), time, 1.0)[:, None] * np.array([0.25, 0.5, 0.75])[None, :]
    assert same("traj", space.interpolate(a, b, t)[0])
    assert out["wrong_size_refused"] is True
