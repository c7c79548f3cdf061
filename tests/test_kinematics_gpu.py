"""rkh_direct_kinematics[_2d] / rkh_jacobians[_2d] on the GPU against the twin of tests/ik_ref.py (pinned to 50-digit
kinematics by tests/test_kinematics_cpu.py).

Bars, the project's own for posed geometry (reach = ik_ref.reach: how far a frame can be from the world origin):
  positions and Jacobian entries   1e-12 max(1, reach)
  quaternion / (cos, sin) parts    1e-12
  velocities and JacDot            1e-11 max(1, reach |qd|)
Chains: the pendulum (1 joint), C2 (6 revolute), the track robot (prismatic root, 7), a mixed chain with non-unit prismatic
axes, C4 (12 joints in two branches on mount links), the planar 3R arm and a planar mixed chain of 4.  B at the wave edges
(1, 63, 64, 65, 130); F = 1, every frame of the chain, and a list with a repeated frame and the base."""
import numpy as np
import pytest

import ik_ref
import kte_ref as K
import lagrange_ref as LR
from reak_amd import scenarios
from reak_amd import types as T

pytestmark = pytest.mark.gpu

BATCHES = (1, 63, 64, 65, 130)
CHAINS = {
    "pendulum": scenarios.make_pendulum,
    "c2": lambda: scenarios.make_c2(world_seed=1),
    "track": scenarios.make_crs_a465_track,
    "mixed4_p12": lambda: LR.mixed_chain(4, (1, 2)),
    "c4": lambda: scenarios.make_c4(world_seed=1, n_obstacles=8),
    "c1_planar": scenarios.make_c1_planar,
    "planar_mixed4": lambda: scenarios.make_planar_mixed(n=4),
}


@pytest.fixture(scope="module")
def L():
    from reak_amd import lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(0)


def _states(scn, count, seed):
    rng = np.random.default_rng(seed)
    n = scn.n_dof
    lo = np.maximum(np.array([scn.dyn.lower[2 * j] for j in range(n)]), -np.pi)
    hi = np.minimum(np.array([scn.dyn.upper[2 * j] for j in range(n)]), np.pi)
    return rng.uniform(lo, hi, size=(count, n)), rng.uniform(-1.0, 1.0, size=(count, n))


_cache = {}


def _case(name):
    """(scenario, q, qd, frames, twin arrays over all 130 states and all frames): computed once per chain, never changed."""
    if name not in _cache:
        scn = CHAINS[name]()
        kin = ik_ref.kin(scn)
        q, qd = _states(scn, max(BATCHES), 17)
        frames = ik_ref.all_frames(scn)
        ref = {k: [] for k in ("pos", "rot", "vel", "ang_vel", "jac", "jac_dot")}
        for b in range(len(q)):
            fa = kin.frame_arrays(q[b], qd[b], frames)
            for k in ("pos", "rot", "vel", "ang_vel"):
                ref[k].append(fa[k])
            JJ = [kin.jacobians(q[b], qd[b], f) for f in frames]
            ref["jac"].append(np.array([j for j, _ in JJ]))
            ref["jac_dot"].append(np.array([jd for _, jd in JJ]))
        ref = {k: np.array(v) for k, v in ref.items()}
        for v in ref.values():
            v.setflags(write=False)
        _cache[name] = (scn, q, qd, frames, ref)
    return _cache[name]


def _bars(scn, qd):
    reach = ik_ref.reach(scn)
    rate = 1e-11 * np.maximum(1.0, reach * np.linalg.norm(qd, axis=1))
    return 1e-12 * max(1.0, reach), 1e-12, rate


def _compare(scn, dev, ref, qd, sel, worst):
    """dev arrays [B][F]... against the twin's rows `sel` of the frame axis."""
    bar_p, bar_r, bar_v = _bars(scn, qd)
    B = len(qd)
    for k, bar in (("pos", bar_p), ("rot", bar_r), ("jac", bar_p)):
        if k in dev:
            e = np.abs(dev[k] - ref[k][:B][:, sel]).max()
            worst[k] = max(worst.get(k, 0.0), e / bar)
            assert e <= bar, (k, e, bar)
    for k in ("vel", "ang_vel", "jac_dot"):
        if k in dev:
            d = np.abs(dev[k] - ref[k][:B][:, sel]).reshape(B, -1).max(axis=1)
            worst[k] = max(worst.get(k, 0.0), (d / bar_v).max())
            assert (d <= bar_v).all(), (k, d.max(), bar_v.min())


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_frames_and_jacobians_match_the_twin(L, ctx, name):
    scn, q, qd, frames, ref = _case(name)
    sc = L.Scene(ctx, scn)
    worst = {}
    everything = list(range(len(frames)))
    for B in BATCHES:   # every frame of the chain, at the wave edges
        dev = sc.direct_kinematics(q[:B], frames, qd[:B])
        dev.update(sc.jacobians(q[:B], frames, qd[:B]))
        _compare(scn, dev, ref, qd[:B], everything, worst)
    B = 65
    # one frame: the far end of the chain; and a list with a repeated frame and the base
    for sel in ([len(frames) - 1], [len(frames) - 1, 0, 1, len(frames) - 1]):
        fl = [frames[i] for i in sel]
        dev = sc.direct_kinematics(q[:B], fl, qd[:B])
        dev.update(sc.jacobians(q[:B], fl, qd[:B]))
        _compare(scn, dev, ref, qd[:B], sel, worst)
        if 0 in sel:   # the base frame: no upstream joint, both matrices exact zeros, and it does not move
            k = sel.index(0)
            assert not dev["jac"][:, k].any() and not dev["jac_dot"][:, k].any()
            assert not dev["vel"][:, k].any() and not dev["ang_vel"][:, k].any()
            assert np.array_equal(dev["jac"][:, 0], dev["jac"][:, 3]) and np.array_equal(dev["pos"][:, 0], dev["pos"][:, 3])
    # columns of joints that are not upstream are exact zeros (the twin's are: test_kinematics_cpu.py)
    dev = sc.jacobians(q[:B], frames, qd[:B])
    up = ik_ref.upstream(scn)
    for k, f in enumerate(frames):
        for i in range(scn.n_dof):
            if not (up[f] >> i) & 1:
                assert not dev["jac"][:, k, :, i].any() and not dev["jac_dot"][:, k, :, i].any(), (f, i)
    print(name, "reach", ik_ref.reach(scn), "worst error / bar:", {k: float("%.3g" % v) for k, v in worst.items()})


def test_the_two_arms_of_c4_do_not_move_each_other(L, ctx):
    """12 joints in two branches: a frame of one arm has exactly-zero columns for the other arm's joints, and the mount
    link end frames are addressable (no upstream joint)."""
    scn, q, qd, frames, ref = _case("c4")
    up = ik_ref.upstream(scn)
    mounts = [o.end_frame for o in scn.ops if o.kind == T.KTE_RIGID_LINK_3D and o.base_frame == 0]
    assert len(mounts) == 2 and all(up[m] == 0 for m in mounts)
    tips = [f for f in frames if bin(up[f]).count("1") == 6]
    masks = sorted({up[f] for f in tips})
    assert masks == [0b111111, 0b111111000000]
    sc = L.Scene(ctx, scn)
    B = 64
    dev = sc.jacobians(q[:B], tips + mounts, qd[:B])
    for k, f in enumerate(tips):
        other = [i for i in range(12) if not (up[f] >> i) & 1]
        assert not dev["jac"][:, k][:, :, other].any() and not dev["jac_dot"][:, k][:, :, other].any()
        mine = [i for i in range(12) if (up[f] >> i) & 1]
        assert dev["jac"][:, k][:, :, mine].any()
    assert not dev["jac"][:, len(tips):].any()
    pose = sc.direct_kinematics(q[:B], mounts, want=("pos", "rot"))
    idx = [frames.index(m) for m in mounts]
    assert np.abs(pose["pos"] - ref["pos"][:B][:, idx]).max() <= 1e-12 * max(1.0, ik_ref.reach(scn))
    assert np.ptp(pose["pos"], axis=0).max() == 0.0   # a mount does not move with the joints


@pytest.mark.parametrize("name", ["c2", "planar_mixed4"])
def test_null_rates_and_null_outputs(L, ctx, name):
    scn, q, qd, frames, ref = _case(name)
    sc = L.Scene(ctx, scn)
    B = 65
    full = sc.direct_kinematics(q[:B], frames, qd[:B])
    full.update(sc.jacobians(q[:B], frames, qd[:B]))
    # NULL qd: zero rates -- the pose and Jac are what they were, the rates and JacDot exact zeros
    z = sc.direct_kinematics(q[:B], frames, None)
    z.update(sc.jacobians(q[:B], frames, None))
    for k in ("pos", "rot", "jac"):
        assert np.array_equal(z[k], full[k]), k
    for k in ("vel", "ang_vel", "jac_dot"):
        assert not z[k].any(), k
    # each output NULL in turn: the others are the same bits
    for drop in ("pos", "rot", "vel", "ang_vel"):
        want = tuple(k for k in ("pos", "rot", "vel", "ang_vel") if k != drop)
        got = sc.direct_kinematics(q[:B], frames, qd[:B], want=want)
        assert sorted(got) == sorted(want) and all(np.array_equal(got[k], full[k]) for k in want), drop
    for keep in ("jac", "jac_dot"):
        got = sc.jacobians(q[:B], frames, qd[:B], want=(keep,))
        assert np.array_equal(got[keep], full[keep]), keep
    for keep in ("pos", "ang_vel"):
        got = sc.direct_kinematics(q[:B], frames, qd[:B], want=(keep,))
        assert np.array_equal(got[keep], full[keep]), keep


def test_refusals(L, ctx):
    import ctypes as C

    c2, planar = L.Scene(ctx, _case("c2")[0]), L.Scene(ctx, _case("c1_planar")[0])
    q6, q3 = np.zeros((2, 6)), np.zeros((2, 3))
    for sc, q in ((c2, q6), (planar, q3)):
        for bad in (-1, 13 if sc is c2 else 7, 100000):
            with pytest.raises(L.RkhError) as e:
                sc.direct_kinematics(q, [0, bad])
            assert e.value.status == -1 and "frame" in str(e.value)
            with pytest.raises(L.RkhError) as e:
                sc.jacobians(q, [bad])
            assert e.value.status == -1
        # B == 0 or F == 0 is fine, and writes nothing
        assert sc.direct_kinematics(q[:0], [0])["pos"].shape[0] == 0
        assert sc.direct_kinematics(q, [])["pos"].shape[1] == 0
        with pytest.raises(L.RkhError) as e:   # every output NULL
            sc.direct_kinematics(q, [0], want=())
        assert e.value.status == -1
        with pytest.raises(L.RkhError) as e:
            sc.jacobians(q, [0], want=())
        assert e.value.status == -1
    # NULL q with B > 0
    fr = (C.c_int32 * 1)(0)
    out = np.zeros(3)
    assert c2.lib.rkh_direct_kinematics(c2.h, None, None, 1, fr, 1, T.dptr(out), None, None, None) == -1
    assert c2.lib.rkh_jacobians(c2.h, None, None, 1, fr, 1, T.dptr(np.zeros(36)), None) == -1
    # the 3D entries on a planar scene and the planar entries on a 3D scene, the way the record entries refuse
    for sc, q, wrong in ((c2, q6, True), (planar, q3, False)):
        with pytest.raises(L.RkhError) as e:
            sc.direct_kinematics(q, [0], planar=wrong)
        assert e.value.status == -5 and ("planar" in str(e.value) or "3D" in str(e.value))
        with pytest.raises(L.RkhError) as e:
            sc.jacobians(q, [0], planar=wrong)
        assert e.value.status == -5


def test_a_pose_is_the_pose_the_distance_query_gives_its_shapes(L, ctx):
    """C2's chain carrying one sphere on its last joint's end frame (local offset and all), one sphere in the world out of
    reach.  The finder is sphere-sphere with the robot's sphere as shape1, so point1 = centre + r u with u the unit vector
    towards point2: the centre the distance query posed is point1 - r u.  rkh_direct_kinematics' pose of the anchor frame
    composed with the shape's local position gives that centre to 1e-12."""
    scn = scenarios.make_c2(world_seed=1)
    anchor, r, local = 2 * 5 + 1, 0.07, (0.03, -0.02, 0.05)
    rob = T.Shape(kind=T.SHAPE_SPHERE, anchor=anchor)
    rob.pose = T.make_pose(local)
    rob.dims[:] = [r, 0.0, 0.0]
    env = T.Shape(kind=T.SHAPE_SPHERE, anchor=-1)
    env.pose = T.make_pose((3.0, -2.0, 4.0))
    env.dims[:] = [0.2, 0.0, 0.0]
    scn.shapes = [rob, env]
    sc = L.Scene(ctx, scn)
    q, _ = _states(scn, 65, 23)
    x = np.zeros((len(q), 12))
    x[:, 0::2] = q
    rec = sc.min_distance_records(x)
    assert (rec["shape1"] == 0).all() and (rec["shape2"] == 1).all() and (rec["dist"] > 0).all()
    u = rec["point2"] - rec["point1"]
    u /= np.linalg.norm(u, axis=1)[:, None]
    centre = rec["point1"] - r * u
    pose = sc.direct_kinematics(q, [anchor], want=("pos", "rot"))
    mine = np.array([K.add(tuple(p), K.q_rot(tuple(Q), local)) for p, Q in zip(pose["pos"][:, 0], pose["rot"][:, 0])])
    err = np.abs(mine - centre).max()
    print("worst |pose o local - centre of the posed sphere|", err)
    assert err <= 1e-12
