"""Plain-Python twin of the backward walk over the SVP space (rkh_svp_edge_check_back, the loop include/rkh.h states; the
per-row rules are reak_amd/csrc/svp_walk_rules.h's): move_pt_back_to with a predicate, on the twin of the space
(tests/svp_ref.py).  The profile a -> b is walked from b backwards and the last free point is kept."""
import svp_ref as R

INF = R.INF
PASS = 32   # points per live row and pass of the staged walk (kSvpWalkPass)


def back_times(sp, T, dt):
    """the travel times the backward walk tests: T - min_interval, - min_interval, ... above dt, by repeated subtraction"""
    out, d = [], T - sp.min_interval
    while d > dt:
        out.append(d)
        d -= sp.min_interval
    return out


def edge_walk_back(sp, a, b, fraction, is_free):
    """(out, T, n_checked, reached, why) -- why as svp_ref.edge_walk names it; is_free(x) is only the collision part"""
    T, peak = R.reach(sp, a, b)
    if not (T < INF):
        return list(b), T, 0, 0, "infeasible"
    dt = T * (1.0 - fraction)
    last, n_checked = list(b), 0
    times = back_times(sp, T, dt)
    for d in times:
        x = R.point(sp, a, b, peak, T, d)
        n_checked += 1
        if not R.in_bounds(sp, x):
            return last, T, n_checked, 0, "bounds"
        if not is_free(x):
            return last, T, n_checked, 0, "collision"
        last = x
    why = "completed" if times else "zero"
    if fraction == 1.0:
        return list(a), T, n_checked, 1, why
    if fraction == 0.0:
        return list(b), T, n_checked, 1, why
    return R.point(sp, a, b, peak, T, dt), T, n_checked, 1, why


def walk_dir(sp, a, b, fraction, back, is_free):
    return edge_walk_back(sp, a, b, fraction, is_free) if back else R.edge_walk(sp, a, b, fraction, is_free)


def times_dir(sp, T, fraction, back):
    return back_times(sp, T, T * (1.0 - fraction)) if back else R.walk_times(sp, T * fraction)
