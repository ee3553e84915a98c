"""The fp64 scalar math of csrc/dsq_math.h (and the count helpers built on it) as the DEVICE computes it.

tests/hostsim compiles the host branch of every `__HIP_DEVICE_COMPILE__` switch with -ffp-contract=off; these tests run
the device branches (v_rcp_f64 / v_rsq_f64 + Newton steps, the LDS log / exp tables, the constant-memory count tables)
under the product's flags through tests/devunit, against mpmath at 120 bits.  Every bound is the header's own claim or
is derived from the arithmetic in a comment; u = 2^-53 is the unit roundoff."""
import math

import mpmath
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mpmath.mp.prec = 120
U = 2.0**-53
TINY = np.finfo(np.float64).tiny  # 2^-1022
SUB = 2.0**-1074  # subnormal spacing


@pytest.fixture(scope="module")
def du():
    from tests import devunit

    devunit.lib()  # builds on first use
    return devunit


def cr(v):
    """The correctly rounded double of an mpmath value (subnormals rounded once, onto the 2^-1074 grid)."""
    v = mpmath.mpf(v)
    if v != 0 and abs(v) < TINY:
        return float(mpmath.nint(v * mpmath.mpf(2) ** 1074)) * SUB
    return float(v)


def cr_all(f, xs):
    return np.array([cr(f(mpmath.mpf(float(x)))) for x in xs])


def ordered(a):
    """doubles -> integers in the same order, consecutive for neighbouring doubles (-0 and +0 both map to 0)."""
    b = np.asarray(a, dtype=np.float64).view(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFFFFFFFFFF), b)


def ulps(got, ref):
    """Distance in representable doubles between got and the correctly rounded ref."""
    return np.abs(ordered(got) - ordered(ref))


def worst(x, got, ref, k=3):
    d = ulps(got, ref)
    i = np.argsort(d)[-k:]
    arg = [tuple(map(float, v)) if isinstance(v, tuple) else float(v) for v in (x[j] for j in i)]
    return [(v, float(got[j]), float(ref[j]), int(d[j])) for v, j in zip(arg, i)]


def nb(x, k=1):
    """x and its k float neighbours on either side."""
    x = np.asarray(x, dtype=np.float64)
    out = [x]
    lo, hi = x.copy(), x.copy()
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


RNG = np.random.default_rng(20261015)


# ------------------------------------------------------------------------------------------------ reciprocals
def normals_loguniform(n, lo=-1022, hi=1023):
    return np.ldexp(RNG.uniform(1.0, 2.0, n), RNG.integers(lo, hi, n))


def mantissa_edges():
    """mantissas next to 1 and next to 2 over a spread of exponents"""
    e = np.arange(-1000, 1000, 37)
    m = np.concatenate([nb(np.ones(1), 4), nb(np.full(1, 2.0), 4)])
    m = m[(m >= 1.0) & (m < 2.0)]
    return np.ldexp(m[None, :], e[:, None]).ravel()


def test_frcp_frcp_g_one_ulp(du):
    # header: v_rcp_f64 + two Newton steps, <= 1 ulp for positive normal x.  Over the whole normal range: from 2^1022 on
    # the reciprocal is subnormal, and "1 ulp" is the subnormal spacing 2^-1074 there (which `ulps` counts alike).
    big = np.ldexp(RNG.uniform(1.0, 2.0, 1000), 1022)
    x = np.concatenate([normals_loguniform(3000), mantissa_edges(), 2.0 ** np.arange(-1022, 1024), big,
                        nb(np.ldexp(1.0, 1022) * np.array([0.75, 1.0, 2.0, 3.0])), [np.finfo(float).max],
                        [1.0, 3.0, 7.0, 1e8, 0.1]])
    x = x[(x >= TINY) & np.isfinite(x)]
    ref = cr_all(lambda v: 1 / v, x)
    for op in ("frcp", "frcp_g"):
        got, _ = du.math(op, x)
        assert np.max(ulps(got, ref)) <= 1, (op, worst(x, got, ref))


def test_frsq_one_ulp(du):
    # header: v_rsq_f64 + two Newton steps, <= 1 ulp, positive normal x (the whole normal range: 1/sqrt stays normal)
    x = np.concatenate([normals_loguniform(3000), mantissa_edges(), 2.0 ** np.arange(-1022, 1024), [TINY, 4.0, 1e300]])
    ref = cr_all(lambda v: 1 / mpmath.sqrt(v), x)
    got, _ = du.math("frsq", x)
    assert np.max(ulps(got, ref)) <= 1, worst(x, got, ref)


def ieee_div(a, b):
    with np.errstate(all="ignore"):
        return np.float64(a) / np.float64(b)


SPECIAL_DIVISORS = [0.0, -0.0, np.inf, -np.inf, np.nan]


def same_ieee(got, ref):
    """bit for bit, except that any NaN matches any NaN (the payload is not specified)"""
    got, ref = np.asarray(got), np.asarray(ref)
    return np.where(np.isnan(ref), np.isnan(got), got.view(np.int64) == ref.view(np.int64))


def test_frcp_g_specials(du):
    # header: 1/0 = inf and 1/inf = 0 survive the Newton steps, as an IEEE division gives them
    x = np.array(SPECIAL_DIVISORS)
    got, _ = du.math("frcp_g", x)
    ref = np.array([ieee_div(1.0, v) for v in x])
    assert same_ieee(got, ref).all(), list(zip(x, got, ref))


def test_fdiv_specials(du):
    # header: b = 0 or inf give what the division gives
    a = np.array([1.5, -3.0, 1e-300, 7e300, 0.0, -0.0, np.inf, np.nan])
    A, B = np.meshgrid(a, np.array(SPECIAL_DIVISORS), indexing="ij")
    A, B = A.ravel(), B.ravel()
    got, _ = du.math("fdiv", A, B)
    ref = np.array([ieee_div(p, q) for p, q in zip(A, B)])
    ok = same_ieee(got, ref)
    assert ok.all(), [(p, q, g, r) for p, q, g, r, o in zip(A, B, got, ref, ok) if not o]


def test_fdiv_one_ulp(du):
    # header: a / b to <= 1 ulp for normal non-zero b; here the quotient is normal as well, and the divisors cover the
    # whole normal range (b > 2^1022 has a subnormal reciprocal)
    n = 4000
    a = normals_loguniform(n) * RNG.choice([-1.0, 1.0], n)
    b = normals_loguniform(n) * RNG.choice([-1.0, 1.0], n)
    edge_b = np.concatenate([nb(np.array([2.0**1022, 2.0**1023, 1.5 * 2.0**1023])), np.full(3, np.finfo(float).max)])
    edge_a = np.concatenate([np.full(9, 2.0**1023), [1e308, 1.0, 2.0**1020]])
    a, b = np.concatenate([a, edge_a]), np.concatenate([b, edge_b])
    q = np.array([abs(ieee_div(p, r)) for p, r in zip(a, b)])
    keep = (q >= TINY) & np.isfinite(q)
    a, b = a[keep], b[keep]
    ref = np.array([cr(mpmath.mpf(float(p)) / mpmath.mpf(float(r))) for p, r in zip(a, b)])
    got, _ = du.math("fdiv", a, b)
    assert np.max(ulps(got, ref)) <= 1, worst(list(zip(a, b)), got, ref)


def test_fdiv_subnormal_operands(du):
    # what the IEEE division gives where the quotient is finite although b is subnormal (b < 2^-1024 has an infinite
    # reciprocal: the Newton / residual path cannot represent it), and subnormal quotients of normal operands
    n = 1500
    b = np.concatenate([np.ldexp(RNG.uniform(1.0, 2.0, n), RNG.integers(-1074, -1022, n)), [SUB, 1e-310, TINY / 2]])
    a = np.ldexp(RNG.uniform(1.0, 2.0, b.size), RNG.integers(-1074, -900, b.size)) * RNG.choice([-1.0, 1.0], b.size)
    a2 = np.ldexp(RNG.uniform(1.0, 2.0, n), RNG.integers(-1022, -900, n))
    b2 = np.ldexp(RNG.uniform(1.0, 2.0, n), RNG.integers(1, 200, n)) * RNG.choice([-1.0, 1.0], n)
    a, b = np.concatenate([a, a2, [0.0, -0.0, 0.0]]), np.concatenate([b, b2, [SUB, SUB, -1e-310]])
    q = np.array([ieee_div(p, r) for p, r in zip(a, b)])
    keep = np.isfinite(q)
    a, b, q = a[keep], b[keep], q[keep]
    ref = np.array([cr(mpmath.mpf(float(p)) / mpmath.mpf(float(r))) for p, r in zip(a, b)])
    got, _ = du.math("fdiv", a, b)
    assert np.max(ulps(got, ref)) <= 1, worst(list(zip(a, b)), got, ref)
    zero = a == 0.0
    assert (got[zero].view(np.int64) == q[zero].view(np.int64)).all()  # signed zeros


# ------------------------------------------------------------------------------------------------ logarithms
def log_inputs():
    j = np.arange(0, 129)
    return np.concatenate([10 ** RNG.uniform(-300, 300, 3000), np.linspace(0.5, 2.0, 3001),
                           nb(1.0 + j / 128.0), nb(0.5 * (1.0 + j / 128.0)), 2.0 ** np.arange(-1022, 1024),
                           [TINY, np.finfo(float).max, 1.0]])


def test_flog_one_ulp(du):
    # header: fdlibm scheme, |error| < 1 ulp
    x = log_inputs()
    ref = cr_all(mpmath.log, x)
    got, _ = du.math("flog", x)
    assert np.max(ulps(got, ref)) <= 1, worst(x, got, ref)


def test_flog_t_one_ulp_and_absolute_below_one(du):
    # header: <= 0.93 ulp measured against binary128, except on [0.5, 1), where the result -ln2 + T + log1p(r)
    # cancels and only an ABSOLUTE error of ~1e-16 is claimed.  Derivation of that bound (k = -1, result in
    # (-ln2, 0]): the table entry T = -log(rc) in [0, ln2) is rounded (<= ulp(T)/2 <= 2^-54); the inner sum
    # T + (r + (p + dk lo)) in [0, ln2) is rounded once more (<= 2^-54); r + p, p + dk lo are O(2^-7) (<= 2^-61 each),
    # the polynomial truncation is < 2^-59 |r| <= 2^-66; the final fma(dk, ln2hi, .) rounds a result of magnitude < 1
    # (<= 2^-54).  Total < 3 * 2^-54 + 2^-59.
    x = log_inputs()
    ref = cr_all(mpmath.log, x)
    got, _ = du.math("flog_t", x)
    below = (x >= 0.5) & (x < 1.0)
    assert np.max(ulps(got[~below], ref[~below])) <= 1, worst(x[~below], got[~below], ref[~below])
    exact = np.array([mpmath.log(mpmath.mpf(float(v))) for v in x[below]])
    err = np.array([float(abs(mpmath.mpf(float(g)) - e)) for g, e in zip(got[below], exact)])
    bound = 3 * 2.0**-54 + 2.0**-59
    assert err.max() < bound, (err.max(), x[below][np.argmax(err)])


def log1p_inputs():
    return np.concatenate([10 ** RNG.uniform(-20, 6, 4000), [0.0, 4.9e-9, 5e-9, 1e-300, TINY, 1.0, 2.0**-53],
                           nb(np.array([4.9e-9, 5e-9, 2.0**-52, 1.0 / 128, np.sqrt(2.0) - 1.0]))])


@pytest.mark.parametrize("op", ["flog1p", "flog1p_t"])
def test_flog1p_one_ulp(du, op):
    # header: log(1 + u) for u >= 0, the rounding of 1 + u corrected; flog1p_t is called as the kernels call it,
    # flog1p_t(u, frcp(1 + u)).  <= 1 ulp (for u = 0: exactly 0)
    u = log1p_inputs()
    ref = cr_all(mpmath.log1p, u)
    got, _ = du.math(op, u)
    assert np.max(ulps(got, ref)) <= 1, worst(u, got, ref)
    assert got[u == 0.0].view(np.int64).tolist() == [0] * int((u == 0.0).sum())


# ------------------------------------------------------------------------------------------------ exponential
def test_fexp_t_one_ulp(du):
    # header: <= 1 ulp over [-745, 710], gradual underflow.  Inputs: hostsim's sets (fewer of them), every reduction
    # point k ln2/128 and every rounding boundary (k + 1/2) ln2/128 of rint over the whole range, each with its two
    # float neighbours (1.6 M arguments); the gradual-underflow range [-745.13, -708.4].
    step = math.log(2) / 128
    k = np.arange(-137450, 131072).astype(np.float64)
    x = np.concatenate([RNG.uniform(-745, 709.7, 4000), RNG.normal(0, 3, 1000), RNG.uniform(-1e-3, 1e-3, 500),
                        nb(k * step), nb((k + 0.5) * step), RNG.uniform(-745.13, -708.4, 2000),
                        [0.0, -0.0, 1.0, -1.0, 709.78, -708.4, -744.0, -745.0, -745.13, 709.782]])
    x = x[(x > -745.14) & (x < 709.78)]
    ref = cr_all(mpmath.exp, x)
    got, _ = du.math("fexp_t", x)
    # <= 1 ulp of the correctly rounded value; in the subnormal range the ulp is the subnormal spacing 2^-1074 (the last
    # multiplication by the scale factor rounds once onto that grid), which `ulps` counts the same way
    assert np.max(ulps(got, ref)) <= 1, worst(x, got, ref)


def test_fexp_t_limits(du):
    # exact limits: exp(+-0) = 1, overflow = inf, underflow = +0, NaN passes through
    x = np.array([0.0, -0.0, 710.0, 1e300, np.inf, -746.0, -1e300, -np.inf, np.nan])
    got, _ = du.math("fexp_t", x)
    assert got[0] == 1.0 and got[1] == 1.0
    assert np.isposinf(got[2:5]).all(), got
    assert (got[5:8].view(np.int64) == 0).all(), got  # +0, not -0
    assert np.isnan(got[8])


# ------------------------------------------------------------------------------------------------ lgamma / digamma
def gamma_inputs():
    return np.concatenate([10 ** RNG.uniform(-6, 9, 3000), np.arange(1, 60) * 0.5,
                           [1e-8, 1.0, 2.0, 9.999999, 10.0, 1e8 + 3],
                           1.0 + np.linspace(-1e-3, 1e-3, 201), 2.0 + np.linspace(-1e-3, 1e-3, 201),
                           nb(np.array([1.0, 2.0, 10.0, 9.0, 11.0]), 3), [10.000001, 1e-300, 1e15]])


@pytest.fixture(scope="module")
def gamma_ref():
    x = gamma_inputs()
    lg = np.array([float(mpmath.loggamma(mpmath.mpf(float(v)))) for v in x])
    dg = np.array([float(mpmath.digamma(mpmath.mpf(float(v)))) for v in x])
    return x, lg, dg


@pytest.mark.parametrize("op,want_dg", [("lgdg00", False), ("lgdg10", True), ("lgdg01", False), ("lgdg11", True),
                                        ("lgamma_pos", False), ("digamma_pos", True)])
def test_lgamma_digamma(du, gamma_ref, op, want_dg):
    # hostsim's bounds: |err| / max(|ref|, 1) < 1e-14 (lgamma) and < 4e-15 (digamma) - absolute for |ref| < 1, which
    # is the case next to the zeros of lgamma at 1 and 2.  All four instantiations <WANT_DG, TAB> and the wrappers.
    x, lg, dg = gamma_ref
    o1, o2 = du.math(op, x)
    if op != "digamma_pos":
        e = np.abs(o1 - lg) / np.maximum(np.abs(lg), 1.0)
        assert e.max() < 1e-14, (op, x[np.argmax(e)], e.max())
    if want_dg:
        d = o1 if op == "digamma_pos" else o2
        e = np.abs(d - dg) / np.maximum(np.abs(dg), 1.0)
        assert e.max() < 4e-15, (op, x[np.argmax(e)], e.max())


# ------------------------------------------------------------------------------------------------ counts
def count_inputs():
    p = 2 ** np.arange(1, 31)
    c = np.concatenate([np.arange(0, 301), p - 1, p, p + 1, [2**31 - 1, 1000, 100000]])
    return np.unique(c)


def test_log_count(du):
    # log_count: the correctly rounded table below 256 (exact), flog above (<= 1 ulp)
    c = count_inputs()
    c = c[c >= 1]
    got, _ = du.math("log_count", c.astype(np.float64))
    ref = cr_all(mpmath.log, c)
    assert (got[c < 256] == ref[c < 256]).all()
    assert np.max(ulps(got, ref)) <= 1, worst(c, got, ref)


def stirling_bound(lg):
    # lg = (z - 0.5) l - z + h + tail: l = flog_t(z) within 1.5 ulp(l) (<= 1 ulp of its correct rounding), so
    # (z - 0.5) l carries 1.5 ulp(l) * (z - 0.5) <= 3 u P relative to the product P, rounded (u P); the three
    # additions round at most u P each (every partial sum is <= P); tail truncation < 1e-15.  P / lg(z) <=
    # log z / (log z - 1) <= 1.23 for z >= 256.  Total <= 7 u P <= 8.7 u lg(z)  ->  bound 9 u |lg| + 1e-15.
    return 9 * U * np.abs(lg) + 1e-15


def test_stirling_big_and_log_factorial(du):
    # stirling_big(z), z >= 256 (the row / mixed-design kernels), and irls_init's log-factorial above the table,
    # (z - 0.5) flog_t(z) - z + h + stirling_tail_big(frcp(z)) at z = y + 1: the same expression
    c = count_inputs()
    z = (c[c >= 255] + 1).astype(np.float64)
    z = np.concatenate([z, z + 0.37, [256.0, 512.0, 1e9]])
    lg, psi = du.math("stirling_big", z)
    rlg = np.array([float(mpmath.loggamma(mpmath.mpf(float(v)))) for v in z])
    rpsi = np.array([float(mpmath.digamma(mpmath.mpf(float(v)))) for v in z])
    e = np.abs(lg - rlg)
    assert (e <= stirling_bound(rlg)).all(), (z[np.argmax(e / rlg)], np.max(e / rlg) / U)
    # psi = l + digamma_tail_big: l within 1.5 ulp(l) (3 u l), one addition (u), tail truncation < 1e-15
    e = np.abs(psi - rpsi)
    assert (e <= 4 * U * np.abs(rpsi) + 1e-15).all(), (z[np.argmax(e)], e.max())


def test_irls_log_factorial_switch(du):
    # irls_init (dsq_irls.h) with one sample of count y:  -cst = (lgamma(a) - lgamma(y + a)) + log(y!)  with log(y!)
    # from kLgammaInt below 256 and from the Stirling expression from 256 on.  The gamma difference carries
    # lgamma_digamma's documented error twice (lga and the Stirling value at y + a: 1e-14 max(|.|, 1) each); log(y!)
    # the table's 0.5 ulp or stirling_bound; the final sum one rounding.  A table/Stirling mix-up at the switch would
    # be off by about log(256) = 5.5.
    y = np.concatenate([np.arange(0, 12), [63, 64, 65, 200, 254, 255, 256, 257, 258, 300, 511, 512, 1000, 100000,
                                            2**20 + 1, 2**31 - 1]])
    for a in (0.37, 3.0, 1e4):
        got = -du.irls_cst(y, a)
        A = mpmath.mpf(a)
        lga = float(mpmath.loggamma(A))
        for yi, g in zip(y, got):
            lgy = mpmath.loggamma(A + int(yi))
            lf = mpmath.loggamma(int(yi) + 1)
            ref = mpmath.loggamma(A) - lgy + lf
            tol = (1e-14 * (max(abs(lga), 1.0) + max(abs(float(lgy)), 1.0)) + stirling_bound(float(lf))
                   + 4 * U * abs(float(ref)) + 1e-300)
            assert abs(g - float(ref)) <= tol, (a, int(yi), g, float(ref), tol)


# ------------------------------------------------------------------------------------------------ gamma differences
YS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 63, 64, 65, 255, 256, 257, 1000, 100000, 2**31 - 1]
YS_BIG = [256, 257, 1000, 100000, 2**31 - 1]

# bound in ulps of max(|lgamma(a)|, |lgamma(y + a)|, 1): for y >= 10 dl = lga - S(y + a), both carrying
# lgamma_digamma's documented 1e-14 max(|.|, 1) (= 45.04 ulp of max(|.|, 1)), plus the final subtraction (<= 1 ulp of
# the larger): c = 92.
# For y <= 9, dl = -flog_t(prod of y <= 9 rounded factors): <= 17 u relative on the product, i.e. 17 u absolute on the
# log, plus the log's own error - far inside the same bound.  The BIG (truncated-tail) path adds < 1e-15 absolute.
C_DL = 92
# digamma: 4e-15 max(|.|, 1) twice (18.02 ulp each) plus one subtraction: c = 37
C_DD = 37


def ulp(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)))


def lgdiff_case(wave, big):
    """[genes][wave] counts and one a per gene: genes of small counts only, of table / large counts only, and mixed
    (small, memo-sized and large counts in one wave, so that the Wv::any branches run together)."""
    ys = np.array(YS_BIG if big else YS)
    G = 48
    alpha = 10 ** RNG.uniform(-8, 2, G)
    alpha[:4] = [1e-8, 1e2, 1.0, 0.05]
    a = 1.0 / alpha
    y = np.empty((G, wave), np.int64)
    for g in range(G):
        if big:
            y[g] = RNG.choice(ys, wave)
        elif g % 3 == 0:
            y[g] = RNG.choice(ys[ys <= 9], wave)
        elif g % 3 == 1:
            y[g] = RNG.choice(ys[ys >= 10], wave)
        else:
            y[g] = np.resize(np.roll(ys, g), wave)
    return y, a


@pytest.mark.parametrize("wave", [64, 16])
@pytest.mark.parametrize("big", [False, True])
def test_lgamma_digamma_diff(du, wave, big):
    y, a = lgdiff_case(wave, big)
    dl, dd = du.lgdiff(wave, y, a, grad=True, big=big)
    dl0, dd0 = du.lgdiff(wave, y, a, grad=False, big=big)
    assert (dd0 == 0.0).all()
    worst_c = 0.0
    for g in range(y.shape[0]):
        A = mpmath.mpf(float(a[g]))
        lga, dga = mpmath.loggamma(A), mpmath.digamma(A)
        cache = {}
        for lane in range(wave):
            yi = int(y[g, lane])
            if yi not in cache:
                lgy, dgy = mpmath.loggamma(A + yi), mpmath.digamma(A + yi)
                cache[yi] = (float(lga - lgy), float(dga - dgy), max(abs(float(lga)), abs(float(lgy)), 1.0),
                             max(abs(float(dga)), abs(float(dgy)), 1.0))
            rl, rd, ml, md = cache[yi]
            tl = C_DL * ulp(ml) + (1e-15 if big else 0.0)
            td = C_DD * ulp(md) + (1e-15 if big else 0.0)
            for d_l in (dl, dl0):  # GRAD = true and false
                assert abs(d_l[g, lane] - rl) <= tl, (wave, big, float(a[g]), yi, d_l[g, lane], rl, tl)
            assert abs(dd[g, lane] - rd) <= td, (wave, big, float(a[g]), yi, dd[g, lane], rd, td)
            worst_c = max(worst_c, abs(dl[g, lane] - rl) / ulp(ml))
            if yi == 0:
                assert dl[g, lane] == 0.0 and dd[g, lane] == 0.0
    print(f"lgamma_digamma_diff wave={wave} big={big}: worst |dl error| = {worst_c:.2f} ulp of max(|lgamma|, 1)")


# ------------------------------------------------------------------------------------------------ normal tail
def test_norm_sf(du):
    # norm_sf mirrors scipy's ndtr arithmetic: a = z * fl(1/sqrt2) rounded, then 0.5 erfc(a), flushed to 0 where cephes
    # flushes (a^2 > MAXLOG, z > 37.6767...).  Checked: the zero / non-zero pattern of scipy.stats.norm.sf, including
    # both sides of the flush; <= 1e-13 relative to mpmath's 0.5 erfc of that same a (the library erfc and the halving;
    # plus one subnormal spacing where the result is subnormal: both round onto the 2^-1074 grid there); and against
    # mpmath's exact sf(z) the argument rounding on top: a = (z / sqrt2)(1 + t), |t| <= 2u, moves log erfc by
    # |t a| * |erfc'(a) / erfc(a)| <= 2u |a| (2|a| + 1.13)  (the ratio is < a + sqrt(a^2 + 4/pi) for a > 0,
    # <= 2/sqrt(pi) for a <= 0) - up to 1.8e-13 at z = 37, shared with scipy, whose ndtr rounds the same product.
    from scipy.stats import norm

    zc = math.sqrt(2 * 7.09782712893383996843e2)
    z = np.concatenate([np.linspace(-8, 37.6, 2001), nb(np.array([zc]), 8), [37.67, 37.676, 37.677, 37.678, 37.68,
                                                                            37.7, 38.0, 50.0, 0.0, -0.0, -40.0]])
    got, _ = du.math("norm_sf", z)
    sp = norm.sf(z)
    assert ((got == 0) == (sp == 0)).all(), [(v, g, s) for v, g, s in zip(z, got, sp) if (g == 0) != (s == 0)]
    nz = sp != 0
    zn, gn = z[nz], got[nz]
    a = zn * 0.70710678118654752440
    sub = np.where(gn < TINY, SUB, 0.0)
    ref_a = np.array([float(mpmath.erfc(mpmath.mpf(float(v)))) / 2 for v in a])
    err = np.abs(gn - ref_a)
    assert (err <= 1e-13 * ref_a + sub).all(), [(v, g, r) for v, g, r, e, s in zip(zn, gn, ref_a, err, sub)
                                                 if e > 1e-13 * r + s][:5]
    ref = np.array([float(mpmath.erfc(mpmath.mpf(float(v)) / mpmath.sqrt(2)) / 2) for v in zn])
    err = np.abs(gn - ref)
    tol = (1e-13 + 2 * U * np.abs(a) * (2 * np.abs(a) + 1.13)) * ref + sub
    assert (err <= tol).all(), [(v, g, r) for v, g, r, e, t in zip(zn, gn, ref, err, tol) if e > t][:5]
    rel = err / np.maximum(ref, TINY)
    print(f"norm_sf: worst relative error {rel.max():.3g} at z = {zn[np.argmax(rel)]} (exact sf), "
          f"{np.max(np.abs(gn - ref_a) / np.maximum(ref_a, TINY)):.3g} against 0.5 erfc(rounded a)")


# ------------------------------------------------------------------------------------------------ tables
def test_tables_as_the_device_reads_them(du):
    """kLgammaInt, kLogInt (constant memory) and the LDS copies of kLogTab, kExpTab: bitwise the correctly rounded
    values."""
    t = du.tables()
    lgi = np.array([cr(mpmath.loggamma(k + 1)) for k in range(256)])
    assert (t["lgamma_int"].view(np.int64) == lgi.view(np.int64)).all()
    li = np.array([0.0] + [cr(mpmath.log(k)) for k in range(1, 256)])  # entry 0 unused (0.0)
    assert (t["log_int"].view(np.int64) == li.view(np.int64)).all()
    rc = np.array([cr(mpmath.mpf(128) / (128 + j)) for j in range(128)])
    T = np.array([cr(-mpmath.log(mpmath.mpf(float(r)))) for r in rc])
    lt = np.empty(256)
    lt[0::2], lt[1::2] = rc, T
    assert (t["log_tab"].view(np.int64) == lt.view(np.int64)).all()
    et = np.array([cr(mpmath.mpf(2) ** (mpmath.mpf(j) / 128)) for j in range(128)])
    assert (t["exp_tab"].view(np.int64) == et.view(np.int64)).all()
