"""A numpy model of the mirror sweep's DOCUMENTED operand format (reak_amd/csrc/nn_mirror.h) and the clouds the bounds
tests share (tests/test_nn_mirror_bounds_gpu.py asks the GPU, tests/test_nn_mirror_band_cpu.py checks the band on the
model).  The halves live in numpy (IEEE binary16, gradual underflow): the format itself stores none below the normal
range.

Everything is in the mirror's prescaled units: p = prescale(bound) is the power of two with 16 <= p * bound < 32,
x_h = half(float(p x)) with a half below 2^-14 stored as 0, |x_h|^2 a float accumulated by fused multiply-adds and split
into three halves, each the half nearest to what the pieces before it left, a piece below 2^-14 and those after it 0."""
import numpy as np

MIN_BOUND, MAX_BOUND = 1e-3, 32.0   # kMirrorMinBound, kMirrorMaxBound
CAND_CAP = 32                       # kMirCandCap (nn_mirror.hip): rows a query's candidate list holds
HALF_MIN_NORMAL = 2.0 ** -14
ACCUMULATE_ROUNDINGS = 15           # of 2^-24 each on partial sums below S (nn_mirror.hip, error bound)


def prescale(bound):
    """mirror_prescale: the power of two p with 16 <= p * bound < 32."""
    _, e = np.frexp(float(bound))
    return float(np.ldexp(1.0, 5 - int(e)))


def operand_half(v):
    """half(float(v)) of a float64 array, round to nearest even twice as the device converts; below the normal range: +0."""
    h = np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float16)
    h[np.abs(h) < np.float16(HALF_MIN_NORMAL)] = np.float16(0.0)
    return h


def float_up(v):
    """float64 -> float32, rounded up."""
    f = np.asarray(v, dtype=np.float64).astype(np.float32)
    low = f.astype(np.float64) < v
    f[low] = np.nextafter(f[low], np.float32(np.inf))
    return f


def float_down(v):
    f = np.asarray(v, dtype=np.float64).astype(np.float32)
    high = f.astype(np.float64) > v
    f[high] = np.nextafter(f[high], np.float32(-np.inf))
    return f


def row_operands(x, scale):
    """The A operands of the rows x [n][D]: (x_h [n][D] float64, the three pieces [n][3] float64, dx).  dx is the tree's
    error word: the maximum over the rows of |p x - x_h|, each rounded up to float as mirror_row_fragments leaves it."""
    xs = np.asarray(x, dtype=np.float64) * scale
    xh = operand_half(xs).astype(np.float64)
    nrm = np.zeros(len(xs), dtype=np.float32)
    for d in range(xs.shape[1]):
        # fmaf(x_h, x_h, nrm): the product is exact in float64 and the float64 sum correctly rounded, so the float of it
        # is the fused result but for half-way cases of relative weight 2^-53 (far inside the band's 12 roundings)
        nrm = (xh[:, d] * xh[:, d] + nrm.astype(np.float64)).astype(np.float32)
    n0 = operand_half(nrm)
    r1 = nrm - n0.astype(np.float32)          # exact
    n1 = np.where(n0 != 0, operand_half(r1), np.float16(0.0))
    r2 = r1 - n1.astype(np.float32)           # exact
    n2 = np.where(n1 != 0, operand_half(r2), np.float16(0.0))
    pieces = np.stack([n0, n1, n2], axis=1).astype(np.float64)
    err = np.sqrt(((xs - xh) ** 2).sum(axis=1)) * (1.0 + 1e-12)
    return xh, pieces, float(float_up(err).max())


def query_operands(q, scale):
    """The B operands of the queries q [B][D] and their qinfo (nn1_mirror_prep_kernel): (q_h [B][D] float64 -- the
    operand holds -2 q_h, exact -- and |q_h|^2, dq = |p q - q_h|, |p q|, rounded up as the kernel does)."""
    qs = np.asarray(q, dtype=np.float64) * scale
    qh = operand_half(qs).astype(np.float64)
    qh2 = (qh * qh).sum(axis=1) * (1.0 + 1e-12) + 1e-300
    dq = np.sqrt(((qs - qh) ** 2).sum(axis=1)) * (1.0 + 1e-12)
    qn = np.sqrt((qs * qs).sum(axis=1)) * (1.0 + 1e-12)
    return qh, qh2, dq, qn


def estimates(xh, pieces, qh):
    """c [n][B] = (n0 + n1 + n2) - 2 x_h.q_h with exact products and a float64 sum: what the matrix instruction
    approximates with its float accumulate."""
    return pieces.sum(axis=1)[:, None] - 2.0 * (xh @ qh.T)


def accumulate_share(D, bound, scale, qn):
    """What the instruction's own float accumulate may add to or take from an estimate, per query: 15 roundings of 2^-24
    on partial sums below S = X^2 + 2 X |q|, X the norm bound as mirror_threshold widens it."""
    X = np.sqrt(float(D)) * bound * scale * (1.0 + 1e-3)
    return ACCUMULATE_ROUNDINGS * 2.0 ** -24 * (X * X + 2.0 * X * qn)


# ---- the clouds of the bounds tests: name -> (D, n, B, bound, kind, spread)
# uniform: rows and queries uniform in [-bound, bound]^D; cluster: in [-spread, spread]^D under the promised bound;
# tiny: uniform in the box, a third of the rows with an exact 0.0 in coordinate 0 (the first two coordinates at D = 12), a
# third with |x| <= 6e-5 -- below the smallest normal half -- in the last coordinate (the last two at D = 12), and every
# seventh query on such a row.
CASES = {
    # dense uniform clouds at small bounds
    "uniform-1d-1e-3": (1, 4096, 64, 1e-3, "uniform", None),
    "uniform-2d-2e-3": (2, 4096, 64, 2e-3, "uniform", None),
    "uniform-2d-0.01": (2, 8192, 64, 0.01, "uniform", None),
    "uniform-3d-5e-3": (3, 8192, 64, 5e-3, "uniform", None),
    "uniform-6d-1e-3": (6, 8192, 64, 1e-3, "uniform", None),
    "uniform-12d-1e-3": (12, 8192, 64, 1e-3, "uniform", None),   # also the lower end of the gate
    "uniform-2d-0.02": (2, 8192, 64, 0.02, "uniform", None),
    # clouds much smaller than the promised bound, around sqrt(D) * bound = 0.125
    "cluster-2d-0.05": (2, 4096, 64, 0.05, "cluster", 0.002),
    "cluster-3d-0.05": (3, 4096, 64, 0.05, "cluster", 0.001),
    "cluster-2d-0.08": (2, 4096, 64, 0.08, "cluster", 0.002),
    # controls: the band swallows hundreds to thousands of rows, far beyond a candidate list
    "control-2d-0.25": (2, 4096, 64, 0.25, "cluster", 0.002),
    "control-2d-1.0": (2, 4096, 64, 1.0, "cluster", 0.002),
    # coordinates that are zero or below the normal range of a half
    "tiny-2d-1.0": (2, 20000, 192, 1.0, "tiny", None),
    "tiny-2d-pi": (2, 20000, 192, np.pi, "tiny", None),
    "tiny-12d-pi": (12, 8192, 64, np.pi, "tiny", None),
    # the ends of the gate (odd sizes at the lower one; at the upper one |x_h|^2 reaches 12288 and a pad row's 60000
    # must still lose)
    "gate-12d-1e-3": (12, 4097, 40, MIN_BOUND, "uniform", None),
    "gate-12d-32": (12, 8192, 64, MAX_BOUND, "uniform", None),
}
CONTROLS = ("control-2d-0.25", "control-2d-1.0")


def cloud(name, seed=0):
    """(pts [n][D], q [B][D], bound) of a case."""
    D, n, B, bound, kind, spread = CASES[name]
    rng = np.random.default_rng(seed)
    sp = bound if spread is None else spread
    pts = rng.uniform(-sp, sp, size=(n, D))
    q = rng.uniform(-sp, sp, size=(B, D))
    if kind == "tiny":
        k = 1 if D < 12 else 2
        pts[0::3, :k] = 0.0
        pts[1::3, D - k:] = rng.uniform(-6e-5, 6e-5, size=(len(pts[1::3]), k))
        treated = np.flatnonzero(np.arange(n) % 3 != 2)
        q[::7] = pts[rng.choice(treated, size=len(q[::7]), replace=False)]
    return pts, q, bound


def exact_sq(pts, q):
    """[n][B] squared distances in plain float64."""
    out = np.zeros((len(pts), len(q)))
    for d in range(pts.shape[1]):
        out += (pts[:, d][:, None] - q[:, d][None, :]) ** 2
    return out


def assert_tie_free(d2):
    """The best and the second-best row of every query differ by more than 1e-12 relative: np.argmin of d2 is THE
    nearest row, whatever the order of a sum's last bits."""
    part = np.partition(d2, 1, axis=0)
    best, second = part[0], part[1]
    assert np.all(second - best > 1e-12 * second), "the cloud has a near-tie: choose another seed"
