"""Plain-Python twin of reak_amd/csrc/svp_device.h: the order-1 rate-limited joint space with sustained-velocity-pulse
profiles, every expression grouped as the header groups it (Python floats are IEEE doubles, math.sqrt rounds correctly,
nothing contracts), so that the device is held to it bit for bit.

The five rules: minimum time of one joint (joint_min_time), the peak velocity that takes a given time (joint_peak), the
point of a profile (joint_point), the bounds rule (in_bounds) and the walk (edge_walk).  tests/test_svp_space_cpu.py pins
them against things they share no code with."""
import math

INF = math.inf


class Space:
    """rkh_svp_space as the entries read it: limits of 0 are 1, vm = speed / accel."""

    def __init__(self, n, lower, upper, min_interval, speed_limits=None, accel_limits=None):
        self.n = int(n)
        self.lower = [float(v) for v in lower[:n]]
        self.upper = [float(v) for v in upper[:n]]
        self.min_interval = float(min_interval)
        sl = [0.0] * n if speed_limits is None else [float(v) for v in speed_limits[:n]]
        al = [0.0] * n if accel_limits is None else [float(v) for v in accel_limits[:n]]
        self.speed = [v if v != 0.0 else 1.0 for v in sl]
        self.accel = [v if v != 0.0 else 1.0 for v in al]
        self.vm = [s / a for s, a in zip(self.speed, self.accel)]

    def c_space(self):
        from reak_amd import types as T
        return T.make_svp_space(self.n, self.lower, self.upper, self.min_interval, self.speed, self.accel)


def _sqrt(x):
    """sqrt as the device takes it: a negative or NaN argument gives NaN instead of raising"""
    return math.sqrt(x) if x >= 0.0 else math.nan


def hyperbox_out(lo, hi, x):
    if lo < hi:
        return (x < lo) or (x > hi)
    return (x > lo) or (x < hi)


def cruise_time(vp, v0, v1, T):
    return (T - abs(vp - v0)) - abs(v1 - vp)


def same_point(p0, p1, v0, v1, vm):
    return (abs(p1 - p0) < 1e-6 * vm) and (abs(v1 - v0) < 1e-6 * vm)


def joint_min_time(p0, p1, v0, v1, vm):
    """(feasible, time, peak)"""
    if same_point(p0, p1, v0, v1, vm):
        return True, 0.0, v0
    if (abs(v0) > vm) or (abs(v1) > vm):
        return False, 0.0, 0.0
    s = -1.0 if p0 > p1 else 1.0
    vp = s * vm
    vpd = vp / vm
    rest = ((p1 - p0) - (0.5 * abs(vp - v1)) * (vpd + v1 / vm)) - (0.5 * abs(vp - v0)) * (vpd + v0 / vm)
    if rest * vp > 0.0:
        return True, (abs(rest) + abs(vp - v1)) + abs(vp - v0), vp
    dist = vm * abs(p1 - p0)
    rad = (dist + (0.5 * v0) * v0) + (0.5 * v1) * v1
    vp = _sqrt(rad)
    if (vp > s * v0) and (vp > s * v1):
        vp = vp * s
        return True, abs(vp - v1) + abs(vp - v0), vp
    if dist < 0.5 * (v0 * v0 + v1 * v1):
        vp = _sqrt(((0.5 * v0) * v0 + (0.5 * v1) * v1) - dist)
        if (vp < s * v0) and (vp < s * v1):
            vp = vp * s
        else:
            vp = vp * -s
        return True, abs(vp - v1) + abs(vp - v0), vp
    return False, 0.0, 0.0


def _guard(r, vp, v0, v1, vm, T):
    return (abs(r) < 1.001 * vm) and (cruise_time(vp, v0, v1, T) >= -1e-3 * vm)


def joint_peak(p0, p1, v0, v1, vm, T):
    """(feasible, peak)"""
    if same_point(p0, p1, v0, v1, vm):
        return True, v0
    if (abs(v0) > vm) or (abs(v1) > vm):
        return False, 0.0
    s = -1.0 if p0 > p1 else 1.0
    sv0, sv1 = v0 * s, v1 * s
    a = (v0 + v1) + T * s
    c = vm * abs(p1 - p0)
    q = 0.5 * (v0 * v0 + v1 * v1)
    aa, cq = a * a, 4.0 * (c + q)
    if aa >= cq:
        root = math.sqrt(aa - cq)
        r = (0.5 * (a + root)) * s
        if _guard(r, s * r, v0, v1, vm, T) and r >= sv0 and r >= sv1:
            return True, s * r
        r = (0.5 * (a - root)) * s
        if _guard(r, s * r, v0, v1, vm, T) and r >= sv0 and r >= sv1:
            return True, s * r
    elif abs(aa - cq) < 1e-5 * vm:
        r = (0.5 * a) * s
        if _guard(r, s * r, v0, v1, vm, T) and r >= sv0 and r >= sv1:
            return True, s * r
    c = vm * (p1 - p0)
    if v1 > v0:
        a = (v0 - v1) + T
        q = 0.5 * (v0 * v0 - v1 * v1)
        if abs(a) > 1e-6 * vm:
            vp = (c + q) / a
            if _guard(vp, vp, v0, v1, vm, T) and vp >= v0 and vp <= v1:
                return True, vp
    else:
        a = (v1 - v0) + T
        q = 0.5 * (v1 * v1 - v0 * v0)
        if abs(a) > 1e-6 * vm:
            vp = (c + q) / a
            if _guard(vp, vp, v0, v1, vm, T) and vp >= v1 and vp <= v0:
                return True, vp
    a = (v0 + v1) - T * s
    c = vm * abs(p1 - p0)
    q = 0.5 * (v0 * v0 + v1 * v1)
    aa, qc = a * a, 4.0 * (q - c)
    if aa > qc:
        root = math.sqrt(aa - qc)
        r = (0.5 * (a + root)) * s
        if _guard(r, s * r, v0, v1, vm, T) and r <= sv0 and r <= sv1:
            return True, s * r
        r = (0.5 * (a - root)) * s
        if _guard(r, s * r, v0, v1, vm, T) and r <= sv0 and r <= sv1:
            return True, s * r
    elif abs(aa - qc) < 1e-5 * vm:
        r = (0.5 * a) * s
        if _guard(r, s * r, v0, v1, vm, T) and r <= sv0 and r <= sv1:
            return True, s * r
    return False, 0.0


def profile_segments(v0, v1, vp, T):
    """(first ramp time, cruise time, second ramp time) of a profile, as joint_point cuts it"""
    d1, d2 = abs(vp - v0), abs(v1 - vp)
    return d1, T - (d2 + d1), d2


def joint_point(p0, p1, v0, v1, vp, vm, dt, T):
    """(position, velocity) at time dt"""
    d1, s1 = vp - v0, 1.0
    if vp < v0:
        s1, d1 = -1.0, -d1
    d2, s2 = v1 - vp, 1.0
    if v1 < vp:
        s2, d2 = -1.0, -d2
    cruise = T - (d2 + d1)
    if dt <= 0.0:
        return p0, v0
    if dt < d1:
        return p0 + ((v0 + (0.5 * dt) * s1) * dt) / vm, v0 + dt * s1
    if dt < d1 + cruise:
        w = (dt - d1) / cruise
        ps = p0 + ((0.5 * (v0 + vp)) * d1) / vm
        pe = p1 - ((0.5 * (vp + v1)) * d2) / vm
        return w * pe + (1.0 - w) * ps, vp
    if dt < (d1 + cruise) + d2:
        m = ((d2 + d1) + cruise) - dt
        return p1 - ((v1 - (0.5 * m) * s2) * m) / vm, v1 - m * s2
    return p1, v1


def reach(sp, a, b):
    """(T, peak [n]): d(a -> b) and the peaks of the common-time solve; (inf, zeros) if infeasible"""
    n = sp.n
    T, ok = 0.0, True
    for i in range(n):
        f, t, _ = joint_min_time(a[2 * i], b[2 * i], a[2 * i + 1], b[2 * i + 1], sp.vm[i])
        ok = f and ok
        if T < t:
            T = t
    ok = ok and (T < INF)
    peak = [0.0] * n
    if ok:
        for i in range(n):
            f, peak[i] = joint_peak(a[2 * i], b[2 * i], a[2 * i + 1], b[2 * i + 1], sp.vm[i], T)
            ok = f and ok
    if not ok:
        return INF, [0.0] * n
    return T, peak


def point(sp, a, b, peak, T, dt):
    x = []
    for i in range(sp.n):
        x.extend(joint_point(a[2 * i], b[2 * i], a[2 * i + 1], b[2 * i + 1], peak[i], sp.vm[i], dt, T))
    return x


def model_units(sp, x):
    """(q0, qd0, ...) the model is posed at"""
    out = []
    for i in range(sp.n):
        out.extend((x[2 * i] * sp.speed[i], x[2 * i + 1] * sp.accel[i]))
    return out


def in_bounds(sp, x):
    for i in range(sp.n):
        p, v, vm, lo, hi = x[2 * i], x[2 * i + 1], sp.vm[i], sp.lower[i], sp.upper[i]
        h = ((0.5 * v) * abs(v)) / vm
        if hyperbox_out(lo, hi, p) or hyperbox_out(-vm, vm, v) or hyperbox_out(lo, hi, p + h) or hyperbox_out(lo, hi, p - h):
            return False
    return True


def interpolate(sp, a, b, times):
    """(rows at the given times, T) as rkh_svp_interpolate answers"""
    T, peak = reach(sp, a, b)
    rows = []
    for t in times:
        if not (T < INF) or not (t > 0.0):
            rows.append(list(a))
        elif t >= T:
            rows.append(list(b))
        else:
            rows.append(point(sp, a, b, peak, T, t))
    return rows, T


def walk_times(sp, dt):
    """the travel times the walk tests: min_interval, + min_interval, ... below dt, by repeated addition"""
    out, d = [], sp.min_interval
    while d < dt:
        out.append(d)
        d += sp.min_interval
    return out


def edge_walk(sp, a, b, fraction, is_free):
    """move_pt_toward with a predicate: (out, T, n_checked, reached, why) -- why in {"infeasible", "zero", "completed",
    "bounds", "collision"} for the tests' census; is_free(x) is only the collision part (bounds are tested first here)."""
    T, peak = reach(sp, a, b)
    if not (T < INF):
        return list(a), T, 0, 0, "infeasible"
    dt = T * fraction
    last, n_checked = list(a), 0
    times = walk_times(sp, dt)
    for d in times:
        x = point(sp, a, b, peak, T, d)
        n_checked += 1
        if not in_bounds(sp, x):
            return last, T, n_checked, 0, "bounds"
        if not is_free(x):
            return last, T, n_checked, 0, "collision"
        last = x
    why = "completed" if times else "zero"
    if fraction == 1.0:
        return list(b), T, n_checked, 1, why
    if fraction == 0.0:
        return list(a), T, n_checked, 1, why
    return point(sp, a, b, peak, T, dt), T, n_checked, 1, why


def nearest(sp, points, query, k, direction):
    """(idx [k], dist [k]): the full sort by (distance, index), infinite distances left out, padded"""
    cand = []
    for i, p in enumerate(points):
        d = reach(sp, p, query)[0] if direction == 0 else reach(sp, query, p)[0]
        if d < INF:
            cand.append((d, i))
    cand.sort()
    cand = cand[:k]
    idx = [i for _, i in cand] + [0xFFFFFFFF] * (k - len(cand))
    dist = [d for d, _ in cand] + [INF] * (k - len(cand))
    return idx, dist


# ---- the seeded inputs the CPU and the GPU tests share ---------------------------------------------------------------------
def test_space(n, min_interval=0.05, half_width=2.0):
    """A space of n joints with mixed limits, some 0 (= 1): box [-half_width, half_width]^n in space coordinates."""
    speed = [(0.0, 2.0, 0.5, 1.0, 3.0)[i % 5] for i in range(n)]
    accel = [(0.0, 1.0, 2.0, 4.0)[i % 4] for i in range(n)]
    return Space(n, [-half_width] * n, [half_width] * n, min_interval, speed, accel)


test_space.__test__ = False  # (a helper, not a test)


def random_pairs(sp, count, seed, special=True):
    """(a [count + extra][2n], b, n_random): positions uniform in the box, velocities uniform within +-vm, every fifth pair
    with |dp| < 0.05; with `special`, behind them a == b, pairs inside the 1e-6 same-point shortcut (one of them with
    velocities beyond the limit: the shortcut comes first), and pairs with a velocity beyond the limit."""
    import numpy as np
    rng = np.random.default_rng(seed)
    n = sp.n
    lo, hi, vm = np.array(sp.lower), np.array(sp.upper), np.array(sp.vm)

    def pts(m):
        x = np.zeros((m, 2 * n))
        x[:, 0::2] = rng.uniform(lo, hi, size=(m, n))
        x[:, 1::2] = rng.uniform(-vm, vm, size=(m, n))
        return x

    a, b = pts(count), pts(count)
    near = np.arange(count) % 5 == 0
    b[near, 0::2] = a[near, 0::2] + rng.uniform(-0.05, 0.05, size=(int(near.sum()), n))
    if special:
        sa, sb = pts(6), pts(6)
        sb[0] = sa[0]                                                # a == b
        sb[1] = sa[1] + 4e-7 * np.tile(vm, 2).reshape(2, n).T.reshape(-1) * rng.uniform(-1, 1, size=2 * n)  # inside the shortcut
        sa[2, 1::2] = 1.5 * vm                                       # beyond the limit, but the same point: 0
        sb[2] = sa[2]
        sb[3, 1] = 1.25 * vm[0]                                      # end velocity beyond the limit
        sa[4, 2 * (n - 1) + 1] = -1.0625 * vm[n - 1]                 # start velocity beyond the limit
        sa[5, 0] = math.nan                                          # not finite: infeasible, no fault
        a, b = np.concatenate([a, sa]), np.concatenate([b, sb])
    return np.ascontiguousarray(a), np.ascontiguousarray(b), count
