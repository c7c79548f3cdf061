"""The rkh_svp_rrt_* entries through the C header: tests/cpp/svp_rrt_smoke.cpp, g++ against librkh.so, grows the trees the
Python binding grows for the same problems, bit for bit; it solves in two calls (two rounds, then the rest), and a struct
of another size is refused."""
import json
import os
import subprocess

import numpy as np
import pytest

import test_svp_rrt_gpu as G
from reak_amd import types as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_c_entries_grow_the_bindings_trees(tmp_path):
    from reak_amd import lib as L

    scn, sp, probs = G.c2_problems()
    probs = probs[:4]   # a goal reached from a later vertex, max_vertices, max_iterations, a goal again
    src, exe = os.path.join(ROOT, "tests", "cpp", "svp_rrt_smoke.cpp"), str(tmp_path / "svp_rrt_smoke")
    lib_dir = os.path.join(ROOT, "reak_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                    "-L", lib_dir, "-lrkh", "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    cs, params = sp.c_space(), G.c_params(probs)
    blob = tmp_path / "svp_rrt_scene.bin"
    with open(blob, "wb") as f:
        f.write(np.int32(len(scn.ops)).tobytes())
        f.write(bytes(scn.ops_array()))
        f.write(bytes(scn.base))
        f.write(np.int32(len(scn.shapes)).tobytes())
        f.write(bytes(scn.shapes_array()))
        f.write(bytes(cs))
        f.write(np.int32(len(params)).tobytes())
        for p in params:
            f.write(bytes(p))
    run = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    out = json.loads(run.stdout.strip().splitlines()[-1])
    ctx = L.Context(0)
    pl = L.SvpRrt(L.Scene(ctx, scn), cs, params)
    st = pl.solve()
    nv, it, gp = pl.status()
    assert out["n_vertices"] == nv.tolist() and out["iterations"] == it.tolist() and out["goal_parent"] == gp.tolist()
    assert (gp != 0xFFFFFFFF).any() and (gp == 0xFFFFFFFF).any() and nv.max() >= 7
    same = lambda key, want: np.array_equal(np.array(out[key], dtype=np.float64).view(np.uint64),
                                            np.ascontiguousarray(want, dtype=np.float64).reshape(-1).view(np.uint64))
    for i in range(len(params)):
        tree = pl.tree(i)
        pts, dur = pl.solution(i)
        assert same("vertices_%d" % i, tree["vertices"]) and same("edge_time_%d" % i, tree["edge_time"]), i
        assert out["parent_%d" % i] == tree["parent"].tolist(), i
        assert same("solution_%d" % i, pts) and out["duration_%d" % i] == dur, i
        assert (len(pts) == 0) == (gp[i] == 0xFFFFFFFF)
    assert out["first_rounds"] == 2 and out["rounds"] == st.rounds > 2 and out["finished"] == len(params)
    assert out["total_iterations"] == st.iterations and out["total_vertices"] == st.vertices
    assert out["wrong_size_refused"] is True
    pl.close()
