"""The goal-probe certificate (reak_amd/csrc/probe_reach.h) and the probe list's granule rule (round_plan.h) are plain host
code: tests/cpp/probe_reach_test.cpp pins the travel bound on a one-joint chain worked by hand, +inf for every refusal
condition, the predicate one ulp either side of equality, and the list through append / drop / leftover / probed_n.  The
program is compiled by the host compiler with AddressSanitizer and UBSan and run directly.

The same program prints the bound of a chain it is given; it is compared with the oracle here, on C2 and on a 3-joint
chain: the acceleration bound A(W4) against the f-eval at 20 000 box states with rates scaled up to W4 and inputs at
+-u_max, the per-joint travel bound against steered edges from the vertices of an oracle tree, and the certificate
against the oracle's goal-probe results.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from reak_amd import scenarios

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("probe_reach") / "probe_reach_test")
    src = os.path.join(ROOT, "tests", "cpp", "probe_reach_test.cpp")
    subprocess.run(["g++", *FLAGS, "-I", os.path.join(ROOT, "reak_amd", "csrc"), src, "-o", exe], check=True)
    return exe


def test_probe_reach_rules_under_sanitizers(program):
    out = subprocess.run([program], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "probe reach ok:" in out.stdout


def chain_bound(program, scn, tmp_path):
    """T[n], reach_q, W4[n], A(W4) of the scenario's serial revolute chain and dynamic space, from probe_reach.h."""
    n, dyn = scn.n_dof, scn.dyn
    assert len(scn.ops) == 5 * n  # serial_chain_ops: actuator, rotor inertia, joint, link, link inertia per joint
    lines = [f"{n} {dyn.steps_per_edge} {dyn.dt!r} {dyn.u_max!r} " + " ".join(repr(float(v)) for v in scn.base.acceleration)]
    for j in range(n):
        rotor, joint, link, inertia = scn.ops[5 * j + 1], scn.ops[5 * j + 2], scn.ops[5 * j + 3], scn.ops[5 * j + 4]
        vals = list(joint.axis) + list(link.offset.pos) + [rotor.mass, inertia.mass] + list(inertia.inertia)
        vals += [dyn.lower[2 * j + 1], dyn.upper[2 * j + 1]]
        lines.append(" ".join(repr(float(v)) for v in vals))
    path = tmp_path / f"{scn.name}.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([program, "bound", str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in out.stdout.splitlines()}
    assert set(rows) == {"T", "reach_q", "W4", "A4"}, out.stdout
    return rows["T"], float(rows["reach_q"][0]), rows["W4"], float(rows["A4"][0])


SCENES = {"c2": lambda: scenarios.make_c2(world_seed=1), "chain3": lambda: scenarios.make_random_chain(3)}


@pytest.fixture(scope="module", params=sorted(SCENES))
def case(request, program, oracle, tmp_path_factory):
    scn = SCENES[request.param]()
    T, reach_q, W4, A4 = chain_bound(program, scn, tmp_path_factory.mktemp("bound"))
    return {"scn": scn, "osc": oracle.OracleScene(scn), "T": T, "reach_q": reach_q, "W4": W4, "A4": A4}


def test_acceleration_bound_against_the_oracle(case):
    scn, osc, W4, A4 = case["scn"], case["osc"], case["W4"], case["A4"]
    n = scn.n_dof
    V = np.array([max(abs(scn.dyn.lower[2 * j + 1]), abs(scn.dyn.upper[2 * j + 1])) for j in range(n)])
    assert np.all(W4 > V)  # the stage rates grow by dt A
    rng = np.random.default_rng(18)
    B = 20000
    x = np.zeros((B, 2 * n))
    x[:, 0::2] = rng.uniform(-np.pi, np.pi, size=(B, n))
    # rates up to W4, half of them on the corners of that box; inputs on the corners of the input box
    x[:, 1::2] = rng.uniform(-1.0, 1.0, size=(B, n)) * W4
    x[: B // 2, 1::2] = np.sign(x[: B // 2, 1::2]) * W4
    u = np.where(rng.uniform(size=(B, n)) < 0.5, -1.0, 1.0) * scn.dyn.u_max
    rc, pd, _, _ = osc.state_derivative(x, u)
    assert rc == 0
    worst = float(np.linalg.norm(pd[:, 1::2], axis=1).max())
    print(f"{scn.name}: max |qdd| = {worst:.6g} over {B} states, A(W4) = {A4:.6g}")
    assert worst <= A4


@pytest.fixture(scope="module")
def tree(case):
    scn, osc = case["scn"], case["osc"]
    rc, out, t = osc.rrt_dyn(scn.rrt_params(seed=3, max_vertices=3000))
    assert rc == 0 and out.num_vertices == 3001
    return t


def test_travel_bound_against_steered_edges(case, tree):
    scn, osc, T = case["scn"], case["osc"], case["T"]
    pos = tree["pos"]
    rng = np.random.default_rng(3)
    lo = np.array([scn.dyn.lower[d] for d in range(scn.D)])
    hi = np.array([scn.dyn.upper[d] for d in range(scn.D)])
    targets = {"goal": np.tile(np.asarray(scn.goal, dtype=np.float64), (len(pos), 1)),
               "random sample": rng.uniform(lo, hi, size=pos.shape)}
    for name, tgt in targets.items():
        rc, end, steps, _ = osc.steer(pos, tgt)
        assert rc == 0
        travel = np.abs(end[:, 0::2] - pos[:, 0::2]).max(axis=0)
        print(f"{scn.name}, steer(vertex, {name}): max travel per joint {travel}, T {T}, mean steps {steps.mean():.2f}")
        assert np.all(travel <= T)


def test_certified_vertices_against_the_oracle(case, tree):
    scn, reach_q = case["scn"], case["reach_q"]
    pos, goal_dist = tree["pos"][1:], tree["goal_dist"]
    goal = np.asarray(scn.goal, dtype=np.float64)
    n_ab = np.sqrt(((pos - goal) ** 2).sum(axis=1))
    dq = np.sqrt(((pos[:, 0::2] - goal[0::2]) ** 2).sum(axis=1))
    in_box = np.all((pos[:, 1::2] >= [scn.dyn.lower[2 * j + 1] for j in range(scn.n_dof)])
                    & (pos[:, 1::2] <= [scn.dyn.upper[2 * j + 1] for j in range(scn.n_dof)]), axis=1)
    certified = in_box & (dq - reach_q >= 0.05 * n_ab * (1.0 + 1e-9))
    share = certified.mean()
    print(f"{scn.name}: reach_q = {reach_q:.4f}, certified {certified.sum()} of {len(pos)}, smallest angle distance "
          f"{dq.min():.3f}, median n_ab {np.median(n_ab):.3f}")
    assert np.all(np.isinf(goal_dist[certified]))
    if scn.name == "C2":  # far from the goal almost everywhere: a bound loosened until nothing is certified must not pass
        assert share >= 0.99
