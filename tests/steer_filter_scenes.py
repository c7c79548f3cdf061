"""Scenes that put the collision filters of the two-lanes steer kernels (propagate_pair.hip: pair_proximity_free) at their
edges.  The kernels do not run the reference's proximity loop: a static reach prefix, an fp32 bounding cull, two LDS
queues of fixed size and a separating-axis screen stand in front of the closed forms, and each of them can only fail one
way -- a collision goes unnoticed.  Every builder returns plain Scenarios (and states); the expected verdicts always
come from the oracle, which has none of the filters.

  far_world         C2, or any scene, moved away from the origin (the cull once rounded absolute coordinates to fp32)
  grazing_spheres   spheres whose surface is 0.1 .. 5 mm inside / outside a robot capsule: contacts inside the cull's margin
  crowded           144 thin obstacles around the arm: hundreds of pairs per state pass the cull (first queue overflows)
  box_cage          cubes set diagonally beside every capsule: every pair passes the screen (second queue overflows)
  reach_boundary    a sphere on either side of the static reach of robot shape k

Not a conftest and not a test module: tests/test_steer_filters_cpu.py asserts the premises on the oracle alone,
tests/test_steer_filters_gpu.py runs the kernels on the scenes."""
import dataclasses
import functools
import os

import numpy as np

from reak_amd import scenarios
from reak_amd import types as T

OFFSET_DIRECTION = np.array([1.0, 0.75, 0.1])  # a world offset M moves everything by M * this
FAR_OFFSETS = (0.0, 1e3, 1e5)
Q0_CAGE = np.array([0.4, 0.7, -0.9, 0.5, 0.8, -0.3])
PENETRATIONS = (1e-4, 1e-3, 5e-3)


# ---------------------------------------------------------------------------------------------- small helpers
def _shape(kind, pos, quat, dims, anchor=-1):
    s = T.Shape(kind=kind, anchor=anchor)
    s.pose = T.make_pose(tuple(pos), tuple(quat))
    s.dims[:] = [float(v) for v in dims]
    return s


def _copy_shape(s, offset=(0.0, 0.0, 0.0)):
    return _shape(s.kind, [s.pose.pos[k] + offset[k] for k in range(3)], s.pose.quat, s.dims, s.anchor)


def q_rot(q, v):
    """v rotated by the unit quaternion q = (w, x, y, z)."""
    w, u = q[0], np.asarray(q[1:4])
    v = np.asarray(v, dtype=np.float64)
    return v + 2.0 * np.cross(u, np.cross(u, v) + w * v)


def quat_of_frame(e1, e2, e3):
    """Unit quaternion (w, x, y, z) of the rotation whose matrix has the columns e1, e2, e3 (right-handed, orthonormal)."""
    m = np.column_stack([e1, e2, e3])
    # the eigenvector of the largest eigenvalue of Shepperd's symmetric 4x4 matrix: no branch on the trace
    k = np.array([[m[0, 0] + m[1, 1] + m[2, 2], m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]],
                  [0.0, m[0, 0] - m[1, 1] - m[2, 2], m[0, 1] + m[1, 0], m[0, 2] + m[2, 0]],
                  [0.0, 0.0, m[1, 1] - m[0, 0] - m[2, 2], m[1, 2] + m[2, 1]],
                  [0.0, 0.0, 0.0, m[2, 2] - m[0, 0] - m[1, 1]]])
    k = (k + k.T - np.diag(np.diag(k))) / 3.0
    w, v = np.linalg.eigh(k)
    q = v[:, np.argmax(w)]
    return q if q[0] >= 0 else -q


def quat_z_to(axis):
    """A unit quaternion that turns local z into `axis` (unit)."""
    axis = np.asarray(axis, dtype=np.float64)
    e1 = np.cross(axis, [1.0, 0.0, 0.0] if abs(axis[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    return quat_of_frame(e1, np.cross(axis, e1), axis)


def perpendiculars(axis):
    n1 = np.cross(axis, [1.0, 0.0, 0.0] if abs(axis[0]) < 0.9 else [0.0, 1.0, 0.0])
    n1 /= np.linalg.norm(n1)
    return n1, np.cross(axis, n1)


def state_box(scn):
    return (np.array([scn.dyn.lower[i] for i in range(scn.D)]), np.array([scn.dyn.upper[i] for i in range(scn.D)]))


def random_states(scn, count, seed):
    lo, hi = state_box(scn)
    return np.random.default_rng(seed).uniform(lo, hi, size=(count, scn.D))


def near_states(count, seed, q0, dq, rate):
    """States with joint angles q0 +- dq and rates +- rate (6 joints)."""
    rng = np.random.default_rng(seed)
    x = np.zeros((count, 12))
    x[:, 0::2] = np.asarray(q0) + rng.uniform(-dq, dq, size=(count, 6))
    x[:, 1::2] = rng.uniform(-rate, rate, size=(count, 6))
    return x


def robot_shapes(scn):
    return [s for s in scn.shapes if s.anchor >= 0]


def with_shapes(scn, shapes, name):
    return dataclasses.replace(scn, shapes=list(shapes), name=name, meta=dict(scn.meta))


def capsule_poses(osc, scn, x):
    """(centre, unit axis, length, radius) in the world of every robot capsule of scn at the state x, from the oracle's
    frames: robot shape k sits on joint k's end frame (frame 2k + 1 of serial_chain_ops)."""
    fr = osc.fk(np.asarray(x, dtype=np.float64).reshape(1, -1))[0]
    out = []
    for s in robot_shapes(scn):
        assert s.kind == T.SHAPE_CCYLINDER
        p, q = fr[s.anchor][:3], fr[s.anchor][3:]
        centre = p + q_rot(q, list(s.pose.pos))
        axis = q_rot(q, q_rot(list(s.pose.quat), [0.0, 0.0, 1.0]))
        out.append((centre, axis / np.linalg.norm(axis), s.dims[0], s.dims[1]))
    return out


# ---------------------------------------------------------------------------------------------- the band
def scene_scale(scn):
    """The largest absolute coordinate in the scene: the chain base and the environment shapes' centres."""
    m = max(abs(v) for v in scn.base.pose.pos)
    for s in scn.shapes:
        if s.anchor < 0:
            m = max(m, max(abs(v) for v in s.pose.pos))
    return float(m)


def verdict_band(scn):
    """Distances within this band of contact are excluded from a verdict comparison: 1e-12, the project's bar at the
    origin, or 64 ulp of the largest coordinate of the scene (1.4e-9 at 1e5 m, about 20 times what the oracle itself
    moves by when the same world is shifted there)."""
    return max(1e-12, 64.0 * 2.0 ** -52 * scene_scale(scn))


def split_by_band(osc, x, band):
    """(states in collision, free states, number excluded) by the oracle's distance: d < -band, d > band, the rest."""
    d = osc.min_distance(x)
    hit, free = d < -band, d > band
    return x[hit], x[free], int(len(x) - hit.sum() - free.sum())


# ---------------------------------------------------------------------------------------------- 1. far world
def far_world(scn, M):
    """scn with its base pose and every environment shape moved by M * (1, 0.75, 0.1); joint states keep their meaning."""
    off = float(M) * OFFSET_DIRECTION
    base = T.ChainBase()
    base.pose = T.make_pose([scn.base.pose.pos[k] + off[k] for k in range(3)], tuple(scn.base.pose.quat))
    base.acceleration[:] = list(scn.base.acceleration)
    shapes = [_copy_shape(s, off if s.anchor < 0 else (0.0, 0.0, 0.0)) for s in scn.shapes]
    return dataclasses.replace(scn, base=base, shapes=shapes, name="%s+%g" % (scn.name, M), meta=dict(scn.meta))


def near_contact_sets(osc, x, d_origin, band, width=5e-3):
    """(near-hits, near-misses) of the scene osc among the states x: -width < d < -band and band < d < width.  d_origin
    holds the distances of the same states in the unshifted world; only the states it puts within 1.2 width of contact
    are evaluated again (the oracle moves by 1e-10 under a shift, the pre-selection has 1 mm to spare)."""
    cand = x[np.abs(d_origin) < 1.2 * width]
    d = osc.min_distance(cand)
    return cand[(d > -width) & (d < -band)], cand[(d > band) & (d < width)]


# ---------------------------------------------------------------------------------------------- 2. grazing spheres
def grazing_spheres(oracle, gap=False, count=64, seed=11):
    """The C2 arm without obstacles, `count` random states and one sphere per state: state i's sphere (radius 0.05 .. 0.2)
    sits beside capsule i mod 6, at a random point of its axis segment in a random perpendicular direction, its surface
    PENETRATIONS[(i // 6) mod 3] inside the capsule (gap=True: that far outside).  The point of the axis segment nearest
    to the sphere's centre is then the foot of the perpendicular, so the cull's lower bound IS the pair's distance: the
    contact lies inside the cull's 1 mm margin, or just beyond it.  Returns (scenario with all spheres, states)."""
    arm = scenarios.make_c2(world_seed=1, n_obstacles=0)
    osc = oracle.OracleScene(arm)
    rng = np.random.default_rng(seed)
    x = near_states(count, seed + 1, np.zeros(6), 1.2, 1.0)  # the arm does not fold back onto itself
    x[:, 0] = rng.uniform(-np.pi, np.pi, size=count)  # ... and the states spread around the base
    poses = [capsule_poses(osc, arm, x[i]) for i in range(count)]
    seg_c = np.array([[p[0] for p in ps] for ps in poses])  # [state][capsule][3]
    seg_a = np.array([[p[1] for p in ps] for ps in poses])
    seg_h = np.array([0.5 * p[2] for p in poses[0]])
    seg_r = np.array([p[3] for p in poses[0]])

    def clearance(c, r, i, k, own):
        """Of the sphere (c, r), its own pair (state i, capsule k) left out: (a hard measure, to be >= 2 cm: the gap to the
        base capsule, and 1.9 cm + what the gap to the rest of state i's arm has beyond `own`, the own pair's gap; the
        number of other states whose arm it touches; the gap to every other capsule of every state).  The base capsule
        (0) has the same pose in every state: a sphere that touches it settles all states at once, so a sphere beside
        it is every state's own, and no other sphere may come near it."""
        v = c - seg_c
        t = np.clip(np.einsum("skd,skd->sk", v, seg_a), -seg_h, seg_h)
        gap = np.linalg.norm(v - t[..., None] * seg_a, axis=2) - seg_r - r
        gap[i, k] = np.inf
        g0 = np.inf if k == 0 else gap[:, 0].min()
        gap[:, 0] = np.inf
        return min(g0, gap[i].min() + 0.019 - own), int((gap.min(axis=1) < 0.0).sum()), gap.min()

    spheres = []
    for i in range(count):
        k = i % 6
        centre, axis, length, radius = poses[i][k]
        n1, n2 = perpendiculars(axis)
        p = PENETRATIONS[(i // 6) % 3]
        best = None
        # Always: 2 cm clear of the base capsule, and the rest of its own state's arm 1 mm further away than its own
        # capsule (so that, alone with the arm, the sphere's contact at state i is its own pair's).  Where there is such a
        # place, 2 cm clear of the arm in every other state too; beside capsule 1 there is not (64 arms share its pivot),
        # and the place that touches the fewest other states is taken.
        for _ in range(400):
            phi, t, r = rng.uniform(0.0, 2.0 * np.pi), rng.uniform(-0.5, 0.5) * length, rng.uniform(0.05, 0.2)
            c = centre + t * axis + (radius + r + (p if gap else -p)) * (np.cos(phi) * n1 + np.sin(phi) * n2)
            hard, touched, g = clearance(c, r, i, k, p if gap else 0.0)
            if hard < 0.02:
                continue
            if best is None or (touched, -g) < best[0]:
                best = ((touched, -g), c, r)
            if g >= 0.02:
                break
        assert best is not None, "no placement for state %d that stays clear of the base capsule and of its own arm" % i
        spheres.append(_shape(T.SHAPE_SPHERE, best[1], (1.0, 0.0, 0.0, 0.0), [best[2], 0.0, 0.0]))
    return with_shapes(arm, robot_shapes(arm) + spheres, "grazing_gap" if gap else "grazing_hit"), x


# ---------------------------------------------------------------------------------------------- 3. crowded
def crowded(seed=77):
    """The C2 arm among 60 rods (capped cylinder 1.6 x 0.01), 24 plates (box 0.7 x 0.7 x 0.006) and 60 spheres (r = 0.03):
    144 obstacles, three chunks of 64.  Centres at radius 0.3 .. 0.9 around the z axis, any angle, height -0.2 .. 1.4; rod
    axes in the plane of the tangent and z, plate normals radial, so nothing crosses the base column.  The bounding
    spheres are large and the bodies thin: most states are free although hundreds of pairs pass the bounding cull."""
    rng = np.random.default_rng(seed)
    arm = scenarios.make_c2(world_seed=1, n_obstacles=0)
    shapes = []
    for kind in ["rod"] * 60 + ["plate"] * 24 + ["sphere"] * 60:
        rho, ang, z = rng.uniform(0.3, 0.9), rng.uniform(0.0, 2.0 * np.pi), rng.uniform(-0.2, 1.4)
        radial = np.array([np.cos(ang), np.sin(ang), 0.0])
        tangent = np.array([-np.sin(ang), np.cos(ang), 0.0])
        up = np.array([0.0, 0.0, 1.0])
        c = rho * radial + z * up
        tilt = rng.uniform(0.0, np.pi)
        if kind == "rod":
            e3 = np.cos(tilt) * tangent + np.sin(tilt) * up
            shapes.append(_shape(T.SHAPE_CCYLINDER, c, quat_of_frame(np.cross(radial, e3), radial, e3), [1.6, 0.01, 0.0]))
        elif kind == "plate":
            e1 = np.cos(tilt) * tangent + np.sin(tilt) * up
            shapes.append(_shape(T.SHAPE_BOX, c, quat_of_frame(e1, np.cross(radial, e1), radial), [0.7, 0.7, 0.006]))
        else:
            shapes.append(_shape(T.SHAPE_SPHERE, c, (1.0, 0.0, 0.0, 0.0), [0.03, 0.0, 0.0]))
    return with_shapes(arm, robot_shapes(arm) + shapes, "crowded")


def crowded_states(count, seed=5):
    return near_states(count, seed, np.zeros(6), 1.2, 1.0)


# ---------------------------------------------------------------------------------------------- 4. box cage
def box_cage(oracle, side=0.06, inset=0.004, clear=0.004):
    """The C2 arm at Q0_CAGE with four cubes of side 0.06 beside each capsule: centred at the capsule's centre +-
    (radius + 0.06 sqrt(3)/2 - inset) n for two perpendicular n, and turned so that the capsule's axis runs along the
    cube's (1, 1, 0) face diagonal and n along (1, -1, 0) -- an edge of the cube faces the capsule, and no axis of the
    cube separates the two: every (capsule, cube) pair that passes the bounding cull also passes the separating-axis
    screen and needs the golden-section search.  The cube's bounding sphere (radius 0.052) reaches `inset` into the
    capsule, so the pair passes the bounding cull although the edge (0.042 from the cube's centre) stays 5.6 mm clear.
    (With the bounding spheres 2 cm clear of the capsules the cull drops all but 0.13 pairs per state and the second
    queue never fills.)  A cube is kept if the oracle finds arm + cube at least `clear` apart at
    Q0_CAGE.  Returns (scenario, cubes kept)."""
    arm = scenarios.make_c2(world_seed=1, n_obstacles=0)
    osc = oracle.OracleScene(arm)
    x0 = np.zeros(12)
    x0[0::2] = Q0_CAGE
    cubes = []
    for centre, axis, length, radius in capsule_poses(osc, arm, x0):
        for n in perpendiculars(axis):
            for sign in (1.0, -1.0):
                e1, e2 = (axis + sign * n) / np.sqrt(2.0), (axis - sign * n) / np.sqrt(2.0)
                c = centre + sign * (radius + side * np.sqrt(3.0) / 2.0 - inset) * n
                cube = _shape(T.SHAPE_BOX, c, quat_of_frame(e1, e2, np.cross(e1, e2)), [side, side, side])
                alone = oracle.OracleScene(with_shapes(arm, robot_shapes(arm) + [cube], "cage_probe"))
                if alone.min_distance(x0)[0] >= clear:
                    cubes.append(cube)
    return with_shapes(arm, robot_shapes(arm) + cubes, "box_cage"), len(cubes)


def cage_states(osc, count=1024, seed=9, draws=32768):
    """`count` states with joint angles Q0_CAGE +- 0.03 and rates +- 1 that the oracle scene osc calls free: the first
    `count` free ones of `draws` (the steered edges need free starts, and with the cubes 5.6 mm from the arm at Q0_CAGE
    a state within 0.03 rad of it is more often in collision than not)."""
    x = near_states(draws, seed, Q0_CAGE, 0.03, 1.0)
    return x[osc.min_distance(x) > 1e-12][:count]


def cage_draws(count=2048, seed=9):
    """The first `count` of the draws cage_states selects from, as they come: most of them have the arm inside a cube, by
    a capsule-against-box contact that only the golden-section search finds."""
    return near_states(count, seed, Q0_CAGE, 0.03, 1.0)


# ---------------------------------------------------------------------------------------------- 5. reach boundary
REACH_LINKS = (2, 3, 4, 5)
REACH_DELTAS = (1e-4, 1e-7)


def static_reach(arm, k):
    """What scene.hip computes for robot shape k of the C2 arm: the link offsets below joint k, the shape's local
    position and its bounding radius -- the height of capsule k's top when the arm stands straight up (q = 0)."""
    lengths = [s.dims[0] for s in robot_shapes(arm)]
    return sum(lengths[: k + 1]) + robot_shapes(arm)[k].dims[1]


def reach_boundary(k, delta, inside, radius=0.08):
    """The C2 arm with robot shapes 0 .. k only (shape k is the outermost), one sphere of radius 0.08 on the z axis whose
    lowest point is `delta` below (inside=True: the sphere touches capsule k at q = 0) or above the static reach of
    shape k, and three spheres far beyond every reach."""
    arm = scenarios.make_c2(world_seed=1, n_obstacles=0)
    z = static_reach(arm, k) + radius + (-delta if inside else delta)
    spheres = [_shape(T.SHAPE_SPHERE, (0.0, 0.0, z), (1.0, 0.0, 0.0, 0.0), [radius, 0.0, 0.0])]
    for c in ((2.5, 0.0, 0.5), (0.0, -3.0, 1.0), (1.5, 1.5, 2.5)):
        spheres.append(_shape(T.SHAPE_SPHERE, c, (1.0, 0.0, 0.0, 0.0), [0.1, 0.0, 0.0]))
    return with_shapes(arm, robot_shapes(arm)[: k + 1] + spheres, "reach_k%d_%g_%s" % (k, delta, "in" if inside else "out"))


def reach_states(count=64, seed=13):
    """q = 0 at rest, then count - 1 states with joint angles within 0.02 rad of it and rates within 0.5."""
    x = near_states(count, seed, np.zeros(6), 0.02, 0.5)
    x[0] = 0.0
    return x


# ---------------------------------------------------------------------------------------------- shared samples and edges
# Computed once per process and handed out unchanged (the arrays are read-only).
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def far_sample(oracle, count=60000):
    """(C2, `count` random states, their distances in the world at the origin): the one large sample, from which the
    near-contact sets of every offset are picked."""
    c2 = scenarios.make_c2(world_seed=1)
    x = random_states(c2, count, 101)
    d = oracle.OracleScene(c2).min_distance(x)
    return (c2,) + _frozen(x, d)


@functools.lru_cache(maxsize=None)
def far_edges(oracle, count=640):
    """Steered edges of the far world: starts = states of the sample the world at the origin calls free, half of them
    within 5 mm of an obstacle; random targets."""
    c2, x, d = far_sample(oracle)
    a = np.concatenate([x[(d > 1e-6) & (d < 5e-3)][: count // 2], x[d > 5e-3][: count - count // 2]])[:count]
    return _frozen(a.copy(), random_states(c2, len(a), 102))


@functools.lru_cache(maxsize=None)
def crowded_edges(oracle, count=333):
    """(scenario, states, free starts, targets): 1024 states of the crowded scene and `count` edges (ten whole waves of
    32 and a ragged one) from the first free states to random targets of the same box."""
    scn = crowded()
    x = crowded_states(1024)
    free = x[oracle.OracleScene(scn).min_distance(x) > 1e-12][:count]
    return (scn,) + _frozen(x, free.copy(), crowded_states(len(free), seed=6))


@functools.lru_cache(maxsize=None)
def cage_edges(oracle, count=512):
    """(scenario, cubes kept, 1024 free states, targets of the first `count`)."""
    scn, kept = box_cage(oracle)
    x = cage_states(oracle.OracleScene(scn))
    return (scn, kept) + _frozen(x, random_states(scn, count, 10))


# ---------------------------------------------------------------------------------------------- the track robot
TRACK_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "steer_filters_track.npz")
TRACK_OFFSET = 1e5


class RestatedScene:
    """What OracleScene is for revolute chains, for a chain with prismatic joints (the oracle's KteChain does not know
    prismatic_joint_3D and poses such a chain wrongly): the test-side restatement tests/kte_ref.py with the oracle's
    closed-form pair distances -- the reference of tests/test_prismatic_*.py.  Python: 0.7 ms per distance query, 70 ms
    per steered edge, which is why the steered edges of the track robot are recorded (TRACK_GOLDEN)."""

    def __init__(self, scn, oracle):
        import kte_ref

        self.scn, self.ref = scn, kte_ref
        self.chain = kte_ref.Chain(scn)
        self.dist = kte_ref.Distances(self.chain, oracle)

    def min_distance(self, x):
        return np.array([self.dist.min_distance(s) for s in np.asarray(x).reshape(-1, self.scn.D)])

    def steer(self, a, b):
        res = [self.ref.steer(self.chain, self.dist, self.scn.dyn, a[i], b[i]) for i in range(len(a))]
        return 0, np.array([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.uint32), None


class RecordedSteer:
    """steer() of a reference whose results were recorded."""

    def __init__(self, out, steps):
        self.out, self.steps = out, steps

    def steer(self, a, b):
        assert len(a) == len(self.out)
        return 0, self.out, self.steps, None


def prismatic_chain6():
    """scenarios.make_random_chain(6) with its 12 obstacles, joints 0 and 3 turned prismatic (travel +- 0.5): a second
    chain for the rkh::prismatic two-lanes forms, with a prismatic joint in the middle (the track robot's is its
    root)."""
    scn = scenarios.make_random_chain(6, seed=4, n_obstacles=12)
    for j, op in enumerate([o for o in scn.ops if o.kind == T.KTE_REVOLUTE_JOINT_3D]):
        if j in (0, 3):
            op.kind = T.KTE_PRISMATIC_JOINT_3D
            scn.dyn.lower[2 * j], scn.dyn.upper[2 * j] = -0.5, 0.5
    scn.name = "prismatic6"
    return scn


def track_scene(M):
    return far_world(scenarios.make_crs_a465_track(), M)


def track_edges(count=512):
    scn = scenarios.make_crs_a465_track()
    return random_states(scn, count, 31), random_states(scn, count, 32)


TRACK_STATES = os.path.join(os.path.dirname(TRACK_GOLDEN), "steer_filters_track_states.npz")


@functools.lru_cache(maxsize=None)
def track_states(oracle):
    """(the track robot's scenario at TRACK_OFFSET, its RestatedScene, states): 384 random states, of which 1 in 100 is
    in collision, and the recorded states of make_track_contacts.  They are inputs only: what each of them is, is
    the restatement's to say when the test runs."""
    scn = track_scene(TRACK_OFFSET)
    x = np.concatenate([random_states(scn, 384, 35), np.load(TRACK_STATES)["x"]])
    return (scn, RestatedScene(scn, oracle)) + _frozen(x)


def make_track_contacts(oracle, count=96, width=5e-3):
    """3 `count` states of the track robot at TRACK_OFFSET in `count` triples (in collision; in collision by less than
    `width`; free by less than `width`).  From a random free state the joint positions descend on the restatement's
    distance, one joint at a time by 0.2, until the arm is inside an obstacle; the last step is then bisected (the
    distance is a minimum of continuous functions) until both ends are within `width` of contact.  The restatement
    takes 1 ms per state and a triple some hundred states: too long for a test, so the states are recorded."""
    scn = track_scene(TRACK_OFFSET)
    ref = RestatedScene(scn, oracle)
    lo_box, hi_box = state_box(scn)
    dist = lambda s: ref.min_distance(s)[0]
    out = []
    for start in random_states(scn, 4 * count, 36):
        hi, dhi = start, dist(start)
        deep = None
        for _ in range(12):
            if dhi < 0:
                break
            trials = []
            for j in range(0, scn.D, 2):
                for step in (-0.2, 0.2):
                    t = hi.copy()
                    t[j] = min(max(t[j] + step, lo_box[j]), hi_box[j])
                    trials.append((dist(t), t))
            dbest, best = min(trials, key=lambda p: p[0])
            if dbest < 0:
                deep = best
                break
            if dbest >= dhi:
                break
            hi, dhi = best, dbest
        if deep is None:
            continue
        lo, dlo = deep, dbest
        for _ in range(40):
            if -width < dlo and dhi < width:
                break
            mid = 0.5 * (lo + hi)
            dm = dist(mid)
            if dm < 0:
                lo, dlo = mid, dm
            else:
                hi, dhi = mid, dm
        out += [deep, lo, hi]
        if len(out) == 3 * count:
            break
    assert len(out) == 3 * count
    np.savez_compressed(TRACK_STATES, x=np.array(out))


def track_recorded():
    """{offset: RecordedSteer} of track_edges() at the origin and at TRACK_OFFSET, as tests/make_steer_filter_golden.py left them."""
    g = np.load(TRACK_GOLDEN)
    return {0.0: RecordedSteer(g["out_origin"], g["steps_origin"]), TRACK_OFFSET: RecordedSteer(g["out_far"], g["steps_far"])}


def write_track_golden(oracle):
    a, b = track_edges()
    res = {}
    for key, M in (("origin", 0.0), ("far", TRACK_OFFSET)):
        _, out, steps, _ = RestatedScene(track_scene(M), oracle).steer(a, b)
        res["out_" + key], res["steps_" + key] = out, steps
    np.savez_compressed(TRACK_GOLDEN, **res)

