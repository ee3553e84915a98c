"""The lane-parallel p x p algebra of csrc/dsq_wide.h, the rpart / rpart2 right-hand side of irls_sweep_wide and
row_chol_solve (csrc/dsq_linalg.h) as the DEVICE runs them: 64 (16) lanes, real barriers, stride loops with a second
pass beyond lane 63, matrices in LDS (MP = 48, DeviceWave) or in a slot of device memory behind SlotWave's fence
(MP = 128).  tests/hostwide runs the same templates with one lane and empty barriers.

Every tolerance is a componentwise backward-error bound (Higham, Accuracy and Stability of Numerical Algorithms, 2nd
ed., Thms 10.3 / 10.4 and the inner-product bound (3.5)); gamma_k = k u / (1 - k u), u = 2^-53; nothing is measured.
The references act on the device's own fp64 outputs (tests/devunit/ref.py: double-double over the full arrays, sampled
entries in mpmath at 120 bits).  Genes 0..3 of a launch have kappa_2 = 1e2, genes 4..7 kappa_2 = 1e8.

wide_inverse has no clean componentwise bound: the device may err 4 x as much as the same algorithm in host float64
loops does on the same factors (test_wide_inverse_against_host; DESIGN.md holds the figures of both), and what needs no
tolerance is asserted besides (bit symmetry, the diagonal of L^-1, placement)."""
from operator import mul

import mpmath
import numpy as np
import pytest

from tests.devunit import ref

pytestmark = pytest.mark.gpu

P48 = (1, 5, 8, 9, 12, 13, 15, 16, 17, 31, 32, 33, 47, 48)
P128 = (49, 63, 64, 65, 80, 81, 96, 97, 112, 113, 127, 128)
SHAPES = [(48, p) for p in P48] + [(128, p) for p in P128]
MOVED = [(48, p) for p in P48 if p >= 33] + [(128, p) for p in P128 if p >= 65]  # several lanes / a second stride pass
G = 8
BLOCKS = 3  # MP = 128: three workgroups (slots) take the eight genes
ORDER = np.array([3, 1, 2, 6, 5, 4, 7, 0])  # gene 0 to the last place, every gene moves
K_LOG = 1  # ulp bound of a logarithm (tests/test_devunit_math.py::test_flog_one_ulp)
K_FRSQ = 1  # ulp bound of frsq (tests/test_devunit_math.py::test_frsq_one_ulp)


@pytest.fixture(scope="module")
def du():
    from tests import devunit

    devunit.lib()  # builds on first use
    return devunit


def spd(P, seed):
    """A = B^T B + delta I with eigenvalues log-spaced from 1 down to 1 / kappa (so kappa_2 = kappa up to rounding),
    kappa = 1e2 (genes 0..3) and 1e8 (genes 4..7), each gene scaled by another power of two"""
    rng = np.random.default_rng([seed, P])
    A = np.empty((G, P, P))
    for g in range(G):
        kappa = 1e2 if g < 4 else 1e8
        Q, _ = np.linalg.qr(rng.standard_normal((P, P)))
        lam = np.logspace(0.0, -np.log10(kappa), P) if P > 1 else np.ones(1)
        delta = 0.5 / kappa
        B = np.sqrt(lam - delta)[:, None] * Q.T
        a = B.T @ B + delta * np.eye(P)
        A[g] = 0.5 * (a + a.T) * 2.0 ** (g - 3)
    return A


def lower(Lfull, P):
    """the lower triangle of a [G][P][ld] factor (the strict upper triangle is never read)"""
    return np.tril(Lfull.reshape(G, P, -1)[:, :, :P])


def device_chol(du, mp, P, A, diag_add=0.0):
    L = lower(du.wide_linalg(mp, "chol", P, A, diag_add=diag_add, blocks=BLOCKS), P)
    assert np.isfinite(L).all()
    return L


def abs_llt(L):
    return np.abs(L) @ np.swapaxes(np.abs(L), 1, 2)


# ------------------------------------------------------------------------------------------------ Cholesky, solve
@pytest.mark.parametrize("mp,P", SHAPES)
def test_wide_chol_backward_error(du, mp, P):
    # Thm 10.3 is about the matrix the factorisation is handed.  wide_chol forms a_jj + diag_add in fp64 first, and where
    # that sum rounds the diagonal takes one more rounding than the theorem counts: j + 2 on l_jj^2, which at j = P is
    # above gamma_{P+1} (at P = 1, sqrt(fl(a + d)) squared is off by up to 3 u against the bound's 2 u).  So the data
    # make the sum exact: the diagonal (below 2^5) on the grid of 2^-44, diag_add = 2^-20 (about 1e-6, the size of the
    # product's ridge, 1e10 times the bound on a diagonal entry).  Then fl(A + diag_add I) = A + diag_add I and the bound
    # holds as stated.
    A = spd(P, 11)
    dg = np.arange(P)
    A[:, dg, dg] = np.round(A[:, dg, dg] * 2.0**44) * 2.0**-44
    d = 2.0**-20
    L = device_chol(du, mp, P, A, d)
    Lk = np.swapaxes(L, 1, 2)  # [g][k][i]
    hi, lo, ab = ref.dd_dot(Lk, Lk)
    eye = np.eye(P, dtype=bool)[None]
    th, tl = ref._two_sum(A, np.where(eye, d, 0.0))  # A + diag_add I, exactly
    assert not tl.any()  # the sum is a double
    err = np.abs((th - hi) + (tl - lo))
    tol = ref.gamma(P + 1) * ab
    low = np.tril(np.ones((P, P), dtype=bool))[None]
    bad = low & ~(err <= tol)
    assert not bad.any(), (np.argwhere(bad)[:5], err[bad][:5], tol[bad][:5])
    rng = np.random.default_rng([12, P])
    with mpmath.workprec(ref.MP_PREC):
        for _ in range(12):  # sampled entries against mpmath itself
            g, i = int(rng.integers(0, G)), int(rng.integers(0, P))
            j = int(rng.integers(0, i + 1))
            s, a = ref.mp_dot(L[g, i, : j + 1], L[g, j, : j + 1])
            t = mpmath.mpf(float(A[g, i, j])) + (mpmath.mpf(d) if i == j else 0)
            assert abs(t - s) <= ref.gamma(P + 1) * a, (g, i, j)


@pytest.mark.parametrize("mp,P", SHAPES)
def test_wide_chol_solve_backward_error(du, mp, P):
    A = spd(P, 13)
    rng = np.random.default_rng([14, P])
    b = rng.standard_normal((G, P)) * 10.0 ** rng.uniform(-2, 2, (G, P))
    L = device_chol(du, mp, P, A)
    x = du.wide_linalg(mp, "solve", P, L, b, blocks=BLOCKS)
    assert np.isfinite(x).all()
    hi, lo, _ = ref.dd_dot(A, x[:, :, None])  # A symmetric: [g][k][i] = A[g][i][k]
    err = np.abs((b - hi[:, :, 0]) - lo[:, :, 0])
    tol = ref.gamma(3 * P + 1) * np.einsum("gij,gj->gi", abs_llt(L), np.abs(x))
    assert (err <= tol).all(), (np.argwhere(~(err <= tol))[:5], err.max(), tol.min())
    with mpmath.workprec(ref.MP_PREC):
        for g in (0, G - 1):
            i = int(rng.integers(0, P))
            s, _ = ref.mp_dot(A[g, i], x[g])
            assert abs(mpmath.mpf(float(b[g, i])) - s) <= tol[g, i], (g, i)


@pytest.mark.parametrize("mp,P", SHAPES)
def test_wide_logdet(du, mp, P):
    # 2 sum_j log L_jj: P logarithms (<= K_LOG ulp each: sum_j ulp(t_j) <= 2 u sum |t_j| < 2 ulp(S)), P - 1 additions
    # (<= (P - 1) u sum |t_j| < P ulp(S)) and an exact doubling, S = 2 sum |log L_jj|
    L = device_chol(du, mp, P, spd(P, 15))
    out = du.wide_linalg(mp, "logdet", P, L, blocks=BLOCKS)
    for g in range(G):
        assert ref.same_bits(out[g], np.full(64, out[g, 0]))  # every lane holds the value
        with mpmath.workprec(ref.MP_PREC):
            t = [2 * mpmath.log(mpmath.mpf(float(L[g, j, j]))) for j in range(P)]
            s, sa = mpmath.fsum(t), float(mpmath.fsum(abs(v) for v in t))
            tol = (P + 2 * K_LOG) * np.spacing(sa)
            assert ref.mp_err(out[g, 0], s) <= tol, (g, out[g, 0], float(s), tol)


# ------------------------------------------------------------------------------------------------ inner products
@pytest.mark.parametrize("mp,P", SHAPES)
def test_wide_frob(du, mp, P):
    # sum_ij A_ij B_ij: P^2 terms
    rng = np.random.default_rng([16, P])
    A, B = spd(P, 17), rng.standard_normal((G, P, P)) * 10.0 ** rng.uniform(-3, 3, (G, P, P))
    B = np.tril(B) + np.swapaxes(np.tril(B, -1), 1, 2)
    out = du.wide_linalg(mp, "frob", P, A, B, blocks=BLOCKS)
    hi, lo, ab = ref.dd_dot(A.reshape(G, P * P, 1), B.reshape(G, P * P, 1))
    for g in range(G):
        assert ref.same_bits(out[g], np.full(64, out[g, 0]))
    err = ref.err_vs_dd(out[:, 0], hi[:, 0, 0], lo[:, 0, 0])
    tol = ref.gamma(P * P) * ab[:, 0, 0]
    assert (err <= tol).all(), (err, tol)
    s, a = ref.mp_dot(A[G - 1].ravel(), B[G - 1].ravel())
    assert ref.dd_agrees_with_mp(hi[G - 1, 0, 0], lo[G - 1, 0, 0], s, a)
    assert ref.mp_err(out[G - 1, 0], s) <= ref.gamma(P * P) * float(a)


@pytest.mark.parametrize("mp,P", SHAPES)
def test_wide_quad_xs(du, mp, P):
    # x^T A x for each of the 64 staged columns: P^2 + P terms
    rng = np.random.default_rng([18, P])
    A = spd(P, 19)
    xs = rng.standard_normal((G, P, 64)) * 10.0 ** rng.uniform(-2, 2, (G, P, 64))
    out = du.wide_linalg(mp, "quad_xs", P, A, xs, blocks=BLOCKS)
    for g in range(G):  # columns as dd_dot's leading axis: r_i = sum_j A_ij x_j, then q = sum_i r_i x_i
        xc = xs[g].T  # [col][j]
        At = np.broadcast_to(A[g].T[None], (64, P, P))  # [col][k = j][i]
        hi, lo, ab = ref.dd_dot(At, np.ones((64, P, 1)), xc)
        qh, ql = ref.dd_weighted_sum(hi[:, :, 0], lo[:, :, 0], xc)
        err = ref.err_vs_dd(out[g], qh, ql)
        tol = ref.gamma(P * P + P) * np.einsum("ci,ci->c", ab[:, :, 0], np.abs(xc))
        assert (err <= tol).all(), (g, err.max(), tol.min())
    col = int(rng.integers(0, 64))
    s, a = ref.mp_dot(np.repeat(xs[0, :, col], P), np.tile(xs[0, :, col], P), A[0].ravel())
    assert ref.mp_err(out[0, col], s) <= ref.gamma(P * P + P) * float(a)


@pytest.mark.parametrize("mp,P", SHAPES)
def test_wide_gram_from_cells(du, mp, P):
    # sum_c (Xc_ci Xc_cj) s_c: 2 C roundings
    rng = np.random.default_rng([20, P])
    for C in (1, 5, 64):
        Xc = rng.standard_normal((G, C, P)) * 10.0 ** rng.uniform(-2, 2, (G, C, P))
        s = 10.0 ** rng.uniform(-6, 6, (G, C)) * rng.choice([-1.0, 1.0], (G, C))
        M = du.wide_linalg(mp, "cells", P, Xc, s, cells=C, blocks=BLOCKS).reshape(G, P, -1)[:, :, :P]
        assert ref.same_bits(M, np.swapaxes(M, 1, 2))
        hi, lo, ab = ref.dd_dot(Xc, Xc, s)
        err = ref.err_vs_dd(M, hi, lo)
        assert (err <= ref.gamma(2 * C) * ab).all(), (C, np.argwhere(~(err <= ref.gamma(2 * C) * ab))[:5])
        g, i = int(rng.integers(0, G)), int(rng.integers(0, P))
        j = int(rng.integers(0, i + 1))
        sm, a = ref.mp_dot(Xc[g, :, i], Xc[g, :, j], s[g])
        assert ref.dd_agrees_with_mp(hi[g, i, j], lo[g, i, j], sm, a)
        assert ref.mp_err(M[g, i, j], sm) <= ref.gamma(2 * C) * float(a)


# ------------------------------------------------------------------------------------------------ inverse
@pytest.mark.parametrize("mp,P", SHAPES)
def test_wide_inverse_structure(du, mp, P):
    L = device_chol(du, mp, P, spd(P, 21))
    out = du.wide_linalg(mp, "inverse", P, L, blocks=BLOCKS).reshape(G, 2, P, -1)
    Li, inv = np.tril(out[:, 0, :, :P]), out[:, 1, :, :P]
    assert np.isfinite(Li).all() and np.isfinite(inv).all()
    assert ref.same_bits(inv, np.swapaxes(inv, 1, 2))
    d = np.arange(P)
    assert ref.same_bits(Li[:, d, d], 1.0 / L[:, d, d])
    # first-order sanity of the product, far from a tolerance on the inverse: |L Li - I| <= gamma_P |L||Li| by rows
    # (each column of Li is a forward substitution, Higham Thm 8.5)
    hi, lo, ab = ref.dd_dot(np.swapaxes(L, 1, 2), Li)
    err = np.abs((hi - np.eye(P)[None]) + lo)
    assert (err <= ref.gamma(P) * ab).all(), np.argwhere(~(err <= ref.gamma(P) * ab))[:5]


def host_inverse(L):
    """wide_inverse's algorithm (L^-1 by columns, then L^-T L^-1) in plain float64 loops, unfused, k ascending.  Python
    floats are IEEE doubles; lists of them index ten times faster than numpy scalars."""
    P = len(L)
    Li = [[0.0] * P for _ in range(P)]
    inv = [[0.0] * P for _ in range(P)]
    for j in range(P):
        Li[j][j] = 1.0 / L[j][j]
        for i in range(j + 1, P):
            s = 0.0
            for k in range(j, i):
                s -= L[i][k] * Li[k][j]
            Li[i][j] = s / L[i][i]
    for i in range(P):
        for j in range(i + 1):
            s = 0.0
            for k in range(i, P):
                s += Li[k][i] * Li[k][j]
            inv[i][j] = inv[j][i] = s
    return np.array(inv)


FX = 320  # fraction bits of the fixed-point reference


def _fx(x, bits=FX):
    n, d = float(x).as_integer_ratio()  # d is a power of two: exact for every entry above 2^(52 - bits)
    return (n << bits) // d


def fixed_inverse(L):
    """(L L^T)^-1 in Python integers scaled by 2^FX (L^-1) and 2^(2 FX) (the inverse): every product and sum is
    exact, each division truncates at 2^-FX.  mpmath's mpf is the same integers with an exponent; this form costs
    0.1 s at P = 128 where mpf takes several.  -> (columns of L^-1, lower triangle of the inverse)"""
    P = len(L)
    Lx = [[_fx(v) for v in row] for row in L]
    cols = []
    for j in range(P):
        c = [0] * P
        c[j] = (1 << 2 * FX) // Lx[j][j]
        for i in range(j + 1, P):
            c[i] = -sum(map(mul, Lx[i][j:i], c[j:i])) // Lx[i][i]
        cols.append(c)
    return cols, [[sum(map(mul, cols[i][i:], cols[j][i:])) for j in range(i + 1)] for i in range(P)]


def max_err_vs_fixed(X, inv_fx):
    """max_ij |X_ij - inverse_ij| over the lower triangle, correctly rounded to a double"""
    P = len(inv_fx)
    worst = max(abs(_fx(X[i][j], 2 * FX) - inv_fx[i][j]) for i in range(P) for j in range(i + 1))
    return worst / (1 << 2 * FX)


@pytest.mark.parametrize("mp,P", SHAPES)
def test_wide_inverse_against_host(du, mp, P):
    # No tolerance is fixed in advance.  The max-norm error of host_inverse against the 320-bit reference is measured on
    # the device's own factors, relative to max |inverse| of the gene (the genes are scaled by different powers of
    # two), and pooled over the four genes of a kappa: the device may err 4 x as much, since fusing and the order inside
    # a dot product change roundings, not their number.  Sampled entries of the reference are certified in mpmath.
    L = device_chol(du, mp, P, spd(P, 21))
    inv = du.wide_linalg(mp, "inverse", P, L, blocks=BLOCKS).reshape(G, 2, P, -1)[:, 1, :, :P]
    assert np.isfinite(inv).all()
    rng = np.random.default_rng([26, P])
    host, dev = np.empty(G), np.empty(G)
    for g in range(G):
        Lg = L[g].tolist()
        cols, inv_fx = fixed_inverse(Lg)
        top = max(abs(v) for row in inv_fx for v in row) / (1 << 2 * FX)
        host[g] = max_err_vs_fixed(host_inverse(Lg).tolist(), inv_fx) / top
        dev[g] = max_err_vs_fixed(inv[g].tolist(), inv_fx) / top
        if g in (0, G - 1):
            i = int(rng.integers(0, P))
            j = int(rng.integers(0, i + 1))
            with mpmath.workprec(FX + 128):  # holds every entry of L^-1 and every product with a double exactly
                li, lj = ([mpmath.ldexp(mpmath.mpf(v), -FX) for v in cols[c]] for c in (i, j))
                row = [u * mpmath.mpf(v) for u, v in zip(lj, Lg[i])]  # row i of L times column j of L^-1
                assert abs(mpmath.fsum(row) - (i == j)) <= mpmath.ldexp(mpmath.fsum(row, absolute=True), -FX + 8)
            with mpmath.workprec(ref.MP_PREC):
                t = [u * v for u, v in zip(li, lj)]
                got = mpmath.ldexp(mpmath.mpf(inv_fx[i][j]), -2 * FX)
                assert abs(mpmath.fsum(t) - got) <= mpmath.ldexp(mpmath.fsum(t, absolute=True), -95), (g, i, j)
    for name, sel in (("1e2", slice(0, 4)), ("1e8", slice(4, 8))):
        print(f"wide_inverse P={P} kappa={name} host={host[sel].max():.3e} device={dev[sel].max():.3e}")
        assert dev[sel].max() <= 4.0 * host[sel].max(), (name, host[sel], dev[sel])


# ------------------------------------------------------------------------------------------------ placement
@pytest.mark.parametrize("mp,P", MOVED)
def test_same_bits_wherever_the_gene_runs(du, mp, P):
    # a missing sync() shows as a dependence on timing, hence on the neighbours and the place of a gene
    rng = np.random.default_rng([22, P])
    A = spd(P, 23)
    b = rng.standard_normal((G, P))
    xs = rng.standard_normal((G, P, 64))
    Xc, s = rng.standard_normal((G, 7, P)), rng.uniform(0.5, 2.0, (G, 7))
    L = device_chol(du, mp, P, A)

    def run(o):
        kw = dict(blocks=BLOCKS)
        return [du.wide_linalg(mp, "chol", P, A[o], diag_add=1e-6, **kw),
                du.wide_linalg(mp, "logdet", P, L[o], **kw),
                du.wide_linalg(mp, "solve", P, L[o], b[o], **kw),
                du.wide_linalg(mp, "inverse", P, L[o], **kw),
                du.wide_linalg(mp, "frob", P, A[o], A[o][:, ::-1, ::-1].copy(), **kw),
                du.wide_linalg(mp, "quad_xs", P, A[o], xs[o], **kw),
                du.wide_linalg(mp, "cells", P, Xc[o], s[o], cells=7, **kw)]

    ld = P | 1
    keep = np.tril(np.ones((P, ld), dtype=bool))  # what an op with a triangular result defines
    for op, r0, r1 in zip(("chol", "logdet", "solve", "inverse", "frob", "quad_xs", "cells"), run(np.arange(G)), run(ORDER)):
        if op == "chol":
            r0, r1 = r0.reshape(G, P, ld)[:, keep], r1.reshape(G, P, ld)[:, keep]
        elif op == "inverse":
            r0, r1 = r0.reshape(G, 2, P, ld)[:, :, :, :P], r1.reshape(G, 2, P, ld)[:, :, :, :P]
            r0[:, 0], r1[:, 0] = np.tril(r0[:, 0]), np.tril(r1[:, 0])
        elif op == "cells":
            r0, r1 = r0.reshape(G, P, ld)[:, :, :P], r1.reshape(G, P, ld)[:, :, :P]
        assert not np.isnan(r0).any(), op
        assert ref.same_bits(r1, r0[ORDER]), op


# ------------------------------------------------------------------------------------------------ IRLS right-hand side
@pytest.mark.parametrize("N", [63, 130])
@pytest.mark.parametrize("mp,P", [(48, 13), (48, 48), (128, 64), (128, 65), (128, 128)])
def test_irls_rhs_exact(du, mp, P, N):
    # one irls_sweep_wide at beta = 0 with dispersion 0 and size factors 2^k: eta = 0, mu = sf, w = mu / (1 + 0) = sf,
    # z = (y - mu) / mu exactly (a power of two divides exactly), w z = y - sf: integers, so X^T (w z) and X^T W X are
    # exact in any order.  W.v(1) comes from rpart (entries below 64) and rpart2 (entries j + 64)
    rng = np.random.default_rng([24, P, N])
    X = rng.integers(-15, 16, (G, N, P))
    X[:, rng.integers(0, N, 5), :] = 0
    y = rng.integers(0, 256, (G, N))
    sf = 2.0 ** rng.integers(0, 8, (G, N))
    Xt = np.full((G, P, N + 3), 7777.0)
    Xt[:, :, :N] = np.swapaxes(X, 1, 2)
    v1, M = du.irls_rhs(mp, Xt, y, sf, np.zeros((G, P)), disp=0.0, min_mu=0.5, a=1.0, blocks=BLOCKS)
    wz = y.astype(np.int64) - sf.astype(np.int64)
    Xi = X.astype(np.int64)
    assert ref.same_bits(v1, np.einsum("gnj,gn->gj", Xi, wz).astype(np.float64)), np.argwhere(
        v1 != np.einsum("gnj,gn->gj", Xi, wz))[:5]
    assert ref.same_bits(M[:, :, :P], np.einsum("gni,gn,gnj->gij", Xi, sf.astype(np.int64), Xi).astype(np.float64))


# ------------------------------------------------------------------------------------------------ row_chol_solve
def row_data(P, seed):
    """64 genes: ent = packed lower triangle of a random SPD matrix (kappa_2 1e2 / 1e6 alternating), then b"""
    rng = np.random.default_rng([seed, P])
    n = 64
    A, b = np.empty((n, P, P)), rng.standard_normal((n, P)) * 10.0 ** rng.uniform(-1, 1, (n, P))
    for g in range(n):
        kappa = 1e2 if (g // 2) % 2 == 0 else 1e6  # both kinds among the even and the odd rows
        Q, _ = np.linalg.qr(rng.standard_normal((P, P)))
        a = (Q * np.logspace(0.0, -np.log10(kappa), P)) @ Q.T
        A[g] = 0.5 * (a + a.T) * 2.0 ** (g % 5)
    il = np.tril_indices(P)
    return A, b, np.concatenate([A[:, il[0], il[1]], b], axis=1)


@pytest.mark.parametrize("P", [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16])
def test_row_chol_solve(du, P):
    # residual bound of the solve (Thm 10.4: gamma_{3P+1} |L||L^T||x|) with frsq (K_FRSQ ulp = 2 K_FRSQ u) times a
    # multiplication (u) in place of each correctly rounded square root / division (u): 2 K_FRSQ more roundings in each
    # of the three stages (factor, forward, backward), so gamma_{3P + 1 + 6 K_FRSQ}.  |L||L^T| from numpy's factor of
    # the same matrix (it differs from the device's to first order in u only).
    ridge = 1e-6
    A, b, ent = row_data(P, 25)
    x = du.row_solve(P, ent, ridge)
    assert np.isfinite(x).all()
    for lane in range(1, 16):  # lanes >= P shadow the last row and must end with the same solution
        assert ref.same_bits(x[:, lane], x[:, 0]), lane
    x0 = x[:, 0]
    Ar = A + ridge * np.eye(P)[None]  # (the rounding of a_ii + ridge is one of the factorisation's counted operations)
    hi, lo, _ = ref.dd_dot(Ar, x0[:, :, None])
    err = np.abs((b - hi[:, :, 0]) - lo[:, :, 0])
    L = np.linalg.cholesky(Ar)
    tol = ref.gamma(3 * P + 1 + 6 * K_FRSQ) * np.einsum("gij,gj->gi", abs_llt(L), np.abs(x0))
    assert (err <= tol).all(), (np.argwhere(~(err <= tol))[:5], (err / tol).max())
    with mpmath.workprec(ref.MP_PREC):
        for g in (0, 2, 63):
            s, _ = ref.mp_dot(A[g, P - 1], x0[g])
            r = mpmath.mpf(float(b[g, P - 1])) - s - mpmath.mpf(ridge) * mpmath.mpf(float(x0[g, P - 1]))
            assert abs(r) <= tol[g, P - 1], g
    xe = du.row_solve(P, ent, ridge, even_only=True)
    assert ref.same_bits(xe[0::2], x[0::2])  # rows 0 and 2 of every wavefront: the same bits without their neighbours
    assert np.isnan(xe[1::2]).all()
