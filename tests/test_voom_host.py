"""limma-voom on the host: lowess_delta against a scalar restatement of R's clowess, the trend's knots and refusals, the
library sizes, the table lookup, and the host build of both row functions (tests/hostvoom) against the float64 reference
and mpmath (tests/voom_ref.py).  No GPU."""
import math

import numpy as np
import pytest

from pydeseq2_amd import voom
from tests import hostvoom as hv
from tests import voom_ref as vr
from tests.voom_cases import (EPS, KAPPA_MAX, KERNEL_P, VOOM_C_E, VOOM_C_FIT1, VOOM_C_HOST, VOOM_C_REL_HOST,
                              check_against_reference, kernel_case, kernel_N, mp_cases, scenario_design, voom_scenario)


def _data(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 10.0, n)
    y = 1.5 + 0.5 * np.sin(x) + rng.normal(0, 0.1, n)
    if kind == "ties":
        x = np.round(x, 2 if n > 100 else 0)
    elif kind == "equal":
        x = np.full(n, 3.25)
    elif kind == "outlier":
        y[n // 3] += 40.0
    elif kind == "linear":
        y = 2.0 + 0.75 * x
    return x, y


def _both(x, y, f, it, delta):
    o = np.argsort(x, kind="stable")
    ys, a = vr.clowess(x[o], y[o], f, it, delta)
    got = voom.lowess_delta(x, y, f=f, iter=it, delta=delta)
    want = np.empty(len(x))
    want[o] = ys
    return got, want, x[o][a], np.asarray(ys)[a]


@pytest.mark.parametrize("kind,n", [("plain", 2), ("plain", 3), ("plain", 10), ("plain", 1000), ("ties", 1000), ("ties", 10),
                                    ("equal", 7), ("outlier", 200), ("linear", 50)])
@pytest.mark.parametrize("delta_frac", [0.0, 0.01, 0.1])
def test_lowess_delta_against_scalar_clowess(kind, n, delta_frac):
    """1e-12 relative at every point and at the anchors, unsorted input; the anchors are strictly increasing in x."""
    x, y = _data(kind, n, seed=n)
    delta = delta_frac * (x.max() - x.min())
    got, want, ax, ay = _both(x, y, 0.5, 3, delta)
    assert np.all(np.abs(got.fitted - want) <= 1e-12 * np.abs(want))
    assert np.array_equal(got.knot_x, ax) and np.all(np.abs(got.knot_y - ay) <= 1e-12 * np.abs(ay))
    assert got.knot_x.shape[0] >= 1 and (np.diff(got.knot_x) > 0).all()
    if kind == "linear":  # exactly linear data: the smooth is the line
        assert np.allclose(got.fitted, y, rtol=1e-12, atol=0)
    if kind == "equal":
        assert got.knot_x.shape[0] == 1 and np.all(got.fitted == got.fitted[0])


def test_lowess_outlier_is_downweighted():
    x, y = _data("outlier", 200, seed=200)
    k = 200 // 3
    rob = voom.lowess_delta(x, y, f=0.5, iter=3, delta=0.0).fitted
    raw = voom.lowess_delta(x, y, f=0.5, iter=0, delta=0.0).fitted
    clean = 1.5 + 0.5 * np.sin(x)
    assert abs(raw[k] - clean[k]) > 0.3 and abs(rob[k] - clean[k]) < 0.1


def test_lowess_delta_agrees_with_delta_zero_at_the_anchors():
    """With delta > 0 the FIRST pass fits the anchors exactly as delta = 0 fits those points (the robustness weights of
    the later passes see interpolated residuals and differ)."""
    x, y = _data("plain", 1000, seed=5)
    d = voom.lowess_delta(x, y, f=0.5, iter=0, delta=0.01 * (x.max() - x.min()))
    z = voom.lowess_delta(x, y, f=0.5, iter=0, delta=0.0)
    at = np.searchsorted(z.knot_x, d.knot_x)
    assert np.array_equal(z.knot_x[at], d.knot_x) and np.array_equal(z.knot_y[at], d.knot_y)
    assert d.knot_x.shape[0] <= 202 < z.knot_x.shape[0]


def test_lowess_anchor_count_on_60000_points():
    rng = np.random.default_rng(60000)
    x = rng.normal(5.0, 3.0, 60000)
    y = 0.4 + 1.0 / (1.0 + np.exp(0.5 * (x - 4.0))) + rng.gamma(4.0, 0.02, 60000)
    lo = voom.lowess_delta(x, y, f=0.5, iter=3)  # delta: 1 % of the range
    assert 2 <= lo.knot_x.shape[0] <= 202 and (np.diff(lo.knot_x) > 0).all()
    kx, ky = voom.check_knots(lo.knot_x, lo.knot_y)
    assert np.array_equal(kx, lo.knot_x)
    o = np.argsort(x, kind="stable")  # the interpolant through the anchors is the smooth (rule = 2 outside)
    assert np.allclose(voom.knot_eval(kx, ky, x), lo.fitted, rtol=1e-9, atol=0)
    assert np.array_equal(voom.knot_eval(kx, ky, [x[o[0]] - 5.0, x[o[-1]] + 5.0]), [ky[0], ky[-1]])


def test_host_refusals_come_before_any_library_call():
    """Every refusal of the host side, with the library unreachable (a pipeline whose launches would raise)."""

    class NoDevice:
        G, N, P = 10, 6, 2
        ctx = None

        class design:
            full_rank = True

        def _k(self, *a):
            raise AssertionError("a launch was attempted")

    pipe = NoDevice()
    with pytest.raises(ValueError, match="1 ... 48 columns"):
        voom.check_design(100, 49)
    with pytest.raises(ValueError, match="residual degrees of freedom"):
        voom.check_design(4, 4)
    with pytest.raises(ValueError, match="full column rank"):
        voom.check_design(10, 3, False)
    for bad in ("libsize", np.ones(5), [1.0, 2.0, 0.0, 1.0, 1.0, 1.0], [1.0, 2.0, np.inf, 1.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match="lib_size"):
            voom.voom_test(pipe, None, [0.0, 1.0], bad)
    with pytest.raises(ValueError, match="column sums"):
        voom.library_sizes("colsums", 6)
    with pytest.raises(ValueError, match="library size of zero"):
        voom.library_sizes("colsums", 3, colsums=[5, 0, 2])
    for bad in ([0.0, 0.0], [1.0, 2.0, 3.0], [np.nan, 1.0], np.zeros((0, 2))):
        with pytest.raises(ValueError, match="contrast"):
            voom.voom_test(pipe, None, bad, np.ones(6))
    pipe.design.full_rank = False
    with pytest.raises(ValueError, match="full column rank"):
        voom.voom_test(pipe, None, [0.0, 1.0], np.ones(6))
    # the trend: fewer than 2 genes with counts, a knot that is not positive and finite, too many knots
    nan = np.nan
    with pytest.raises(ValueError, match="at least 2"):
        voom.voom_trend(np.array([1.0, nan, nan]), np.array([0.5, nan, nan]), np.zeros(4))
    with pytest.raises(ValueError, match="positive finite"):
        voom.voom_trend(np.array([1.0, 2.0, 3.0]), np.array([0.0, 0.0, 0.0]), np.zeros(4))
    with pytest.raises(ValueError, match="positive finite"):
        voom.check_knots([0.0, 1.0], [0.5, -0.1])
    with pytest.raises(ValueError, match="positive finite"):
        voom.check_knots([0.0, 1.0], [0.5, np.inf])
    with pytest.raises(ValueError, match="257 knots"):
        voom.check_knots(np.arange(257.0), np.ones(257))
    with pytest.raises(ValueError, match="strictly increasing"):
        voom.check_knots([0.0, 2.0, 1.0], [1.0, 1.0, 1.0])


def test_facade_refusals_need_no_device():
    """DeseqStats(test='voom') refuses lfc_null, alt_hypothesis, reduced and strata before it looks at the data set; the
    gene-sharded pipeline refuses the call."""
    from pydeseq2_amd.api import DeseqStats
    from pydeseq2_amd.distributed import DistDeseqPipeline

    for kw in (dict(lfc_null=0.5), dict(alt_hypothesis="greater"), dict(reduced="~1"), dict(strata="batch")):
        with pytest.raises(ValueError, match="voom"):
            DeseqStats(None, ["condition", "b", "a"], test="voom", **kw)
    with pytest.raises(ValueError, match="test='voom'"):
        DeseqStats(None, ["condition", "b", "a"], lib_size="colsums")
    with pytest.raises(ValueError, match="gene-sharded"):
        DistDeseqPipeline.voom(None, None, [0.0, 1.0])


def test_effective_library_sizes():
    rng = np.random.default_rng(3)
    cs = rng.integers(10**5, 10**7, 9)
    sf = np.exp(rng.normal(0, 0.4, 9))
    L = voom.library_sizes("size_factors", 9, sf, cs)
    nf = voom.norm_factors(L, cs)
    assert abs(np.exp(np.mean(np.log(nf))) - 1.0) < 1e-14  # geometric mean 1
    assert np.allclose(L / L[0], sf / sf[0], rtol=1e-14)  # proportional to the size factors
    assert np.allclose(L, vr.effective_lib_sizes(sf, cs), rtol=1e-13)
    assert np.array_equal(voom.library_sizes("colsums", 9, sf, cs), cs.astype(float))
    assert np.array_equal(voom.library_sizes(np.arange(1.0, 10.0), 9), np.arange(1.0, 10.0))
    assert np.allclose(voom.sample_offsets(L), np.log2(L + 1.0) - math.log2(1e6), rtol=0, atol=1e-15)


@pytest.mark.parametrize("nk", [2, 17, 256])
def test_table_lookup(nk):
    """Below the first knot, above the last, exactly on every knot, midway, NaN; tables of 2 and of 256 knots."""
    rng = np.random.default_rng(nk)
    kx = np.cumsum(rng.uniform(0.01, 1.0, nk)) - 3.0
    kf = rng.uniform(0.3, 2.0, nk)
    mid = 0.5 * (kx[:-1] + kx[1:])
    lam = np.concatenate([[kx[0] - 1.0, -np.inf, kx[-1] + 1.0, np.inf], kx, mid, rng.uniform(kx[0], kx[-1], 50)])
    got = hv.lookup(kx, kf, lam)
    assert got[0] == kf[0] and got[1] == kf[0] and got[2] == kf[-1] and got[3] == kf[-1]
    assert np.array_equal(got[4:4 + nk], kf)  # exactly on a knot: the knot's value, no rounding
    tol = 4 * EPS * 2 * kf.max()  # t = (lam - x_lo) / (x_hi - x_lo) carries two roundings, times |f_hi - f_lo| <= 2 max f
    assert np.allclose(got, np.interp(lam, kx, kf), rtol=0, atol=tol)
    slack = np.abs(np.diff(kf) / np.diff(kx)) * EPS * np.abs(mid)  # (the midpoint itself is rounded)
    assert (np.abs(got[4 + nk:4 + nk + nk - 1] - 0.5 * (kf[:-1] + kf[1:])) <= tol + slack).all()
    assert np.isnan(hv.lookup(kx, kf, [np.nan]))[0]


def test_test_designs_are_well_conditioned():
    """The condition on the inputs (not a measurement): kappa = cond_2(diag(sqrt w) X)^2 <= 1e6 on every gene of every
    kernel case and of the end-to-end scenario, and the scenario's reference knots are positive - by the reference alone."""
    worst = 0.0
    for P in KERNEL_P:
        for N in kernel_N(P):
            kc = kernel_case(N, P)
            b1 = vr.first_fit(kc["counts"], kc["X"], kc["L"])[0]
            lam = kc["X"] @ np.nan_to_num(b1).T + kc["off"][:, None]
            w = np.interp(lam, kc["kx"], kc["ky"]) ** -4.0
            for g in range(0, w.shape[1], 1 if N < 100 else 16):
                sv = np.linalg.svd(kc["X"] * np.sqrt(w[:, g])[:, None], compute_uv=False)
                worst = max(worst, (sv[0] / sv[-1]) ** 2)
            assert (kc["ky"] > 0).all()
    counts, meta, _ = voom_scenario()
    X = scenario_design(meta)
    ref = vr.voom_reference(counts.to_numpy(), X, counts.to_numpy().sum(1).astype(float), np.eye(4)[1])
    print(f"largest kappa of the kernel cases {worst:.3g}, of the scenario {np.nanmax(ref['kappa']):.3g}")
    assert worst <= KAPPA_MAX and np.nanmax(ref["kappa"]) <= KAPPA_MAX
    assert (ref["knots"][1] > 0).all() and np.isfinite(ref["knots"][1]).all() and len(ref["knots"][0]) <= 202


def _host(kc, G=None, K=None, layers=True):
    c = kc["contrasts"][:K]
    counts = kc["counts"][:, :G]
    b1, am, s1 = hv.fit1(counts, kc["off"], kc["X"], kc["pinv"])
    return (b1, am, s1) + hv.wls(counts, kc["off"], kc["X"], b1, kc["kx"], kc["ky"], c, layers=layers)


@pytest.mark.parametrize("P", KERNEL_P)
def test_host_build_against_reference(P):
    """Both row functions at every row length of the GPU test, all 257 genes and 3 contrasts, at the host bound."""
    for N in kernel_N(P):
        kc = kernel_case(N, P)
        got = _host(kc)
        ref1 = vr.first_fit(kc["counts"], kc["X"], kc["L"])
        live = ~np.isnan(ref1[1])
        assert np.array_equal(live, ~np.isnan(got[1])) and not live[1]
        condX = np.linalg.cond(kc["X"]) ** 2
        nb = np.linalg.norm(ref1[0][live], axis=1)
        assert (np.linalg.norm(got[0][live] - ref1[0][live], axis=1) <= VOOM_C_FIT1 * EPS * condX * nb).all()
        scale = (np.abs(np.log2(kc["counts"] + 0.5)) + np.abs(kc["off"])[:, None]).mean(0)[live]
        # (the reference's own mean - a pairwise sum of N terms and a quotient - is within (log2 N + 1) eps of the truth)
        assert (np.abs(got[1][live] - ref1[1][live]) <= (VOOM_C_E + math.log2(N) + 1) * EPS * scale).all()
        assert (np.abs(got[2][live] - ref1[2][live]) <= VOOM_C_REL_HOST * EPS * ref1[2][live]).all()
        check_against_reference(kc, got, VOOM_C_HOST, VOOM_C_REL_HOST, f"host N={N} P={P}")


def test_host_build_against_mpmath():
    """A handful of genes at 50 digits: the measurement behind VOOM_C_HOST / VOOM_C_REL_HOST (printed), asserted at
    the host bound."""
    import mpmath

    wa = wr = we = 0.0
    for N, P, genes in mp_cases():
        kc = kernel_case(N, P)
        slope = np.max(np.abs(np.diff(kc["ky"]) / np.diff(kc["kx"]))) / kc["ky"].min()
        b1, am, s1, beta, s2, est, u, E, w = _host(kc)
        ref = vr.wls(kc["counts"], kc["X"], kc["L"], b1, kc["kx"], kc["ky"], kc["contrasts"])
        for g in genes:
            if np.isnan(b1[g]).any():
                continue
            y = kc["counts"][:, g]
            with mpmath.workdps(50):
                mp = mpmath.mpf
                T = vr.gene_truth(y, kc["off"], kc["X"], b1[g], kc["kx"], kc["ky"], kc["contrasts"])
                kap = ref["kappa"][g]
                nb = float(mpmath.sqrt(sum(v * v for v in T["beta"])))
                ca = float(mpmath.sqrt(sum((mp(float(a)) - v) ** 2 for a, v in zip(beta[g], T["beta"])))) / (EPS * kap * nb)
                for k in range(3):
                    cn = float(np.linalg.norm(kc["contrasts"][k]))
                    ca = max(ca, float(abs(mp(float(est[g, k])) - T["est"][k])) / (EPS * kap * cn * nb),
                             float(abs(mp(float(u[g, k])) - T["u"][k]) / T["u"][k]) / (EPS * kap))
                cr = float(abs(mp(float(s2[g])) - T["sigma2"]) / T["sigma2"]) / EPS
                cr = max(cr, float(abs(mp(float(s1[g])) - T["sigma1"]) / T["sigma1"]) / EPS)
                for n in range(N):
                    sc = abs(math.log2(y[n] + 0.5)) + abs(kc["off"][n])
                    we = max(we, float(abs(mp(float(E[g, n])) - T["E"][n])) / (EPS * sc))
                    # f^-4 of a lambda that carries the roundings of its P + 1 terms, through the steepest piece of the table
                    dlam = (P + 2) * EPS * (np.abs(kc["X"][n]) @ np.abs(b1[g]) + abs(kc["off"][n]))
                    assert abs(mp(float(w[g, n])) - T["w"][n]) <= (8 * EPS + 4 * slope * dlam) * T["w"][n]
            wa, wr = max(wa, ca), max(wr, cr)
    print(f"host build against mpmath: C = {wa:.3g} (beta, est, u; bound {VOOM_C_HOST}), "
          f"C_rel = {wr:.3g} (sigma2, sigma1; bound {VOOM_C_REL_HOST}), C_E = {we:.3g} (bound {VOOM_C_E})")
    assert wa <= VOOM_C_HOST and wr <= VOOM_C_REL_HOST and we <= VOOM_C_E
