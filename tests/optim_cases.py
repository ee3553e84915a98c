"""Inputs and references shared by the tests of the lane-parallel L-BFGS-B optimisers (csrc/dsq_lbfgsb_wave.h,
dsq_lbfgsb.h, dsq_lbfgsb_par.h): the 64-lane device unit (tests/test_devunit_optim.py) and the host comparison with scipy
above 16 variables (tests/test_hostsim.py).

Every reference is a plain restatement in exact (fractions.Fraction), 50-digit (mpmath) or sequential fp64 arithmetic -
never a run of the code under test."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53  # unit roundoff of fp64
M = 10          # pairs kept

# ------------------------------------------------------------------------------------------------ 1. group sums
# (R, rowsum's group of a lane, colsum's group of a lane)
GROUPS = {8: (lambda lane: lane >> 3, lambda lane: lane & 7),
          16: (lambda lane: lane >> 2, lambda lane: lane & 3),
          32: (lambda lane: lane >> 1, lambda lane: lane & 1)}


def group_members(R, which, lane):
    """the lanes of the wavefront whose values lane `lane` must hold the sum of"""
    key = GROUPS[R][["rowsum", "colsum"].index(which)]
    return [k for k in range(64) if key(k) == key(lane)]


def spread_doubles(rng, n, binades=40):
    """mixed signs, exponents spread over `binades` binades"""
    return rng.choice([-1.0, 1.0], n) * rng.uniform(1, 2, n) * 2.0 ** rng.integers(-binades // 2, binades // 2, n)


# ------------------------------------------------------------------------------------------------ 2. the direction
# (P, R, run-time p): the product's instantiations; P = R runs with p <= P and zero padding
DIR_SHAPES = [(5, 8, 5), (7, 8, 7), (8, 8, 8), (9, 16, 9), (12, 16, 12), (16, 16, 13), (16, 16, 16), (32, 32, 17),
              (32, 32, 24), (32, 32, 32)]
DIR_COLS = (0, 1, 2, 10)
DIR_HEADS = (0, 3, 9)
EXACT_COLS = (0, 1, 2, 3)  # the exact test keeps col <= 3


def ring(col, head):
    return [(head + q) % M for q in range(col)]


def _lay_out(R, p, col, head, s, y, rho, g, x):
    """the workspace as the product leaves it: zero padding components, NaN in the slots outside the ring"""
    S, Y, RHO = np.full((M, R), np.nan), np.full((M, R), np.nan), np.full(M, np.nan)
    for q, slot in enumerate(ring(col, head)):
        S[slot], Y[slot] = 0.0, 0.0
        S[slot, :p], Y[slot, :p], RHO[slot] = s[q], y[q], rho[q]
    G, X = np.zeros(R), np.zeros(R)
    G[:p], X[:p] = g, x
    return dict(S=S, Y=Y, RHO=RHO, g=G, x=X)


def exact_direction_case(rng, R, p, col, head):
    """small integers, theta and every rho a power of two: every intermediate of the recurrence is exact in fp64 in any
    summation order, fused or not (direction_exact checks that)"""
    s = rng.integers(-2, 3, (col, p)).astype(float)
    y = rng.integers(-2, 3, (col, p)).astype(float)
    rho = 2.0 ** rng.integers(-4, -1, col)
    case = _lay_out(R, p, col, head, s, y, rho, rng.integers(-3, 4, p).astype(float), rng.integers(-8, 9, p).astype(float))
    case.update(R=R, p=p, col=col, head=head, theta=float(2.0 ** rng.integers(-1, 3)))
    return case


def random_direction_case(rng, R, p, col, head):
    """well-scaled pairs of a convex quadratic (y = A s, A SPD: y's > 0), rho = 1 / y's, theta = y'y / y's of the last"""
    B = rng.normal(size=(p + 2, p))
    A = B.T @ B / p + 0.5 * np.eye(p)
    s = rng.normal(size=(col, p))
    y = s @ A
    ys = np.einsum("qi,qi->q", y, s)
    assert (ys > 0).all()
    theta = float(y[-1] @ y[-1] / ys[-1]) if col else 1.0
    case = _lay_out(R, p, col, head, s, y, 1.0 / ys, rng.normal(size=p), rng.normal(size=p))
    case.update(R=R, p=p, col=col, head=head, theta=theta)
    return case


def _replay(case, num, guard=None):
    """H_k = the pairs replayed on I / theta in the arithmetic `num` (a constructor of numbers); (d, z, H) over the p
    live components.  guard(terms): called with the terms of every sum"""
    R, col, head = case["p"], case["col"], case["head"]  # (the padding components are zero: they decouple exactly)
    one, zero = num(1), num(0)

    def tot(terms):
        if guard is not None:
            guard(terms)
        s = zero
        for t in terms:
            s = s + t
        return s

    ith = one / num(case["theta"])
    H = [[ith if i == j else zero for j in range(R)] for i in range(R)]
    for slot in ring(col, head):
        s, y, rho = [num(v) for v in case["S"][slot, :R]], [num(v) for v in case["Y"][slot, :R]], num(case["RHO"][slot])
        Hy = [tot([H[i][j] * y[j] for j in range(R)]) for i in range(R)]
        yhy = tot([y[i] * Hy[i] for i in range(R)])
        cc = rho * yhy + one
        for i in range(R):
            for j in range(R):
                terms = [cc * (s[i] * s[j]), -(s[i] * Hy[j] + Hy[i] * s[j])]
                if guard is not None:
                    guard([cc * (s[i] * s[j]), s[i] * Hy[j], Hy[i] * s[j], H[i][j] / rho if rho else zero])
                H[i][j] = H[i][j] + rho * (terms[0] + terms[1])
    g, x = [num(v) for v in case["g"][:R]], [num(v) for v in case["x"][:R]]
    Hg = [tot([H[i][j] * g[j] for j in range(R)]) for i in range(R)]
    if guard is not None:
        guard([x[i] for i in range(R)] + Hg)
    return [-v for v in Hg], [x[i] - Hg[i] for i in range(R)], H


def _padded(case, v):
    out = np.zeros(case["R"])
    out[:case["p"]] = v
    return out


def direction_exact(case):
    """(d, z) as floats from the recurrence in exact rationals.  Raises unless every sum of the recurrence is exact in
    fp64 whatever its order: all terms are multiples of one power of two q and sum |terms| < 2^53 q."""
    def guard(terms):
        den = 1
        for t in terms:
            den = max(den, Fraction(t).denominator)
        if den & (den - 1) or sum(abs(Fraction(t)) for t in terms) * den >= 2 ** 53:
            raise AssertionError("the exact case leaves the exactly representable numbers")

    d, z, _ = _replay(case, Fraction, guard)
    return _padded(case, [float(v) for v in d]), _padded(case, [float(v) for v in z])


def direction_mp(case):
    """(d, z, max |H|) from a 50-digit replay (mpmath numbers)"""
    import mpmath

    with mpmath.workdps(50):
        d, z, H = _replay(case, lambda v: mpmath.mpf(float(v)))
        return d, z, float(max(abs(v) for row in H for v in row))


def direction_fp64(case):
    """(d, z) from the same recurrence in plain fp64, sequential sums, nothing fused"""
    d, z, _ = _replay(case, lambda v: float(v))
    return _padded(case, d), _padded(case, z)


def direction_error(dz, ref):
    """max |dz - ref| over the live components of d and z (ref: mpmath numbers)"""
    import mpmath

    with mpmath.workdps(50):
        return float(max(abs(mpmath.mpf(float(a)) - b) for got, want in zip(dz, ref) for a, b in zip(got, want)))


# ------------------------------------------------------------------------------------------------ 3 / 4. test objectives
def make_problem(seed, n, cond, bounds="none"):
    """f = 1/2 d'Qd + sum exp(clip(w d, -50, 50)), d = x - c (the family of test_hostsim's scipy comparisons), Q symmetric
    with eigenvalues log-spaced over [1, cond].  bounds: "none", "box" (a box that cuts the unconstrained minimiser
    off in some variables), "half" (lower bounds on the even variables only)."""
    rng = np.random.default_rng([seed, n, int(cond)])
    V, _ = np.linalg.qr(rng.normal(size=(n, n)))
    lam = np.logspace(0, np.log10(cond), n) if n > 1 else np.ones(1)
    Q = (V * lam) @ V.T
    Q = 0.5 * (Q + Q.T)
    c, w = rng.normal(0, 1, n), rng.uniform(0.2, 1.0, n)
    x0 = c + rng.normal(0, 1, n)
    b = None
    if bounds == "box":
        b = [(ci + 0.1, ci + 2.0) if i % 3 == 0 else (ci - 3.0, ci + 3.0) for i, ci in enumerate(c)]
    elif bounds == "half":
        b = [(ci - 0.1 * (1 + i % 4), None) if i % 2 == 0 else (None, None) for i, ci in enumerate(c)]
    elif bounds != "none":
        raise ValueError(bounds)
    return dict(Q=Q, c=c, w=w, x0=x0, bounds=b, n=n, cond=cond, seed=seed, kind=bounds)


def objective(q, ulp=0):
    """fg(x) -> (f, g) of a problem in numpy; ulp = k: every gradient component moved by k ulp, up in the even
    components and down in the odd ones (k < 0: the other way round)"""
    Q, c, w = q["Q"], q["c"], q["w"]
    sign = np.where(np.arange(len(c)) % 2 == 0, 1.0, -1.0) * ulp

    def fg(x):
        d = x - c
        e = np.exp(np.clip(w * d, -50, 50))
        g = Q @ d + w * e
        if ulp:
            g = g + sign * np.spacing(np.abs(g))
        return 0.5 * d @ Q @ d + e.sum(), g

    return fg


def host_trace(q, ulp=0):
    """the compact form on the host (tests/hostsim, LbfgsbWork<48>) -> dict(x, f, g: the evaluations; xfin, success,
    nit, status)"""
    import tests.hostsim as hs

    fg = objective(q, ulp)
    xs, fs, gs = [], [], []

    def rec(x):
        f, g = fg(x)
        xs.append(x.copy()); fs.append(f); gs.append(np.array(g))
        return f, g

    n = q["n"]
    x, f, ok, nfev, nit, st = hs.lbfgsb_nd48(rec, q["x0"], q["bounds"] or [(None, None)] * n)
    return dict(x=np.array(xs), f=np.array(fs), g=np.array(gs), xfin=x, success=ok, nit=nit, nfev=nfev, status=st)


def trace_distance(a, b, n_eval=5):
    """largest relative difference of x, f, g over the first n_eval evaluations of two traces (each number relative to
    max(1, the infinity norm of its vector))"""
    k = min(n_eval, len(a["f"]), len(b["f"]))
    worst = 0.0
    for e in range(k):
        for key in ("x", "g"):
            va, vb = np.atleast_1d(a[key][e]), np.atleast_1d(b[key][e])
            worst = max(worst, float(np.max(np.abs(va - vb)) / max(1.0, np.max(np.abs(va)))))
        worst = max(worst, float(abs(a["f"][e] - b["f"][e]) / max(1.0, abs(a["f"][e]))))
    return worst


# (seed, (P, R, p), condition number): lbfgsb_wave<P, R> against lbfgsb_nd<R, ., 10, OneLane>, both on the device
# every shape of DIR_SHAPES, condition numbers 10 ... 10^4, and per R at least two problems of more than 12 iterations
# (the ring of 10 pairs overwrites its oldest).  Kept: problems whose host run keeps nit, flag and status when every
# gradient component moves by 1, 8 or 64 ulp (test_wave_problems_are_settled) - a problem that stops within rounding
# of a stopping rule cannot tell a wrong optimiser from a right one.
WAVE_PROBLEMS = [
    (1, (5, 8, 5), 10), (2, (5, 8, 5), 10000), (1, (7, 8, 7), 1000), (1, (8, 8, 8), 100), (2, (8, 8, 8), 10000),
    (1, (9, 16, 9), 10000), (2, (9, 16, 9), 10), (1, (12, 16, 12), 100), (1, (16, 16, 13), 1000), (2, (16, 16, 16), 10),
    (1, (16, 16, 16), 100),
    (1, (32, 32, 17), 100), (2, (32, 32, 24), 10), (1, (32, 32, 24), 1000), (1, (32, 32, 32), 100), (2, (32, 32, 32), 10),
]

# (seed, NMAX, n, condition number, bounds): lbfgsb_nd<NMAX, ., 10, DeviceWave> against OneLane, bit for bit
# per n: an unbounded problem of >= 14 iterations (both moves ran), a box with bounds active at the solution, a
# half-bounded one (test_lanes_problems_have_their_properties)
LANES_PROBLEMS = [(1, 16, 5, 1000, "none"), (1, 16, 5, 100, "box"), (1, 16, 5, 100, "half")] + \
                 [(1, nmax, n, 100, kind) for nmax, n in ((16, 16), (48, 33), (48, 40), (48, 48))
                  for kind in ("none", "box", "half")]


def wave_problem(entry):
    seed, (P, R, p), cond = entry
    return make_problem(seed, p, cond)


def lanes_problem(entry):
    seed, nmax, n, cond, kind = entry
    return make_problem(seed, n, cond, kind)
