"""The trend fit's cases (tests/trend_cases.py) on the CPU: the references against each other, the host instantiation of
dsq_trend.h's passes (WaveTrendOps<HostWave>) against mpmath, and its fit against the oracle over all sizes x kinds.
The measured worst ratios of the host evaluations fix the bounds of the device unit (tests/test_devunit_trend.py)."""
import warnings

import numpy as np
import pytest

from oracle import nbglm_oracle as orc
from tests import hostsim as hs
from tests import trend_cases as tc


def test_the_restated_loop_is_the_oracles():
    """tc.oracle_fit reports ok, n_outer and the coefficients of orc.fit_parametric_trend, bit for bit"""
    for n in tc.SIZES:
        for kind in tc.KINDS:
            c = tc.case(kind, n)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                co, n_outer = orc.fit_parametric_trend(c["t"], c["means"])
            fit = c["fit"]
            assert fit["ok"] == (co is not None) and fit["n_outer"] == n_outer, (kind, n)
            if co is not None:
                assert np.array_equal(co, fit["coef"]), (kind, n)
            assert fit["n_kept"] == int(fit["kept"].sum()) <= int(tc.init_mask(c["means"]).sum())


@pytest.mark.parametrize("n", [s for s in tc.SIZES if s <= tc.MP_MAX])
def test_the_longdouble_reference_against_mpmath(n):
    """The form used beyond MP_MAX genes agrees with mpmath to 2^-8 of the error unit wherever both can be run: a term
    takes a handful of longdouble operations (2^-63 each, 2^-11 units), the sum is exact."""
    for kind in tc.KINDS:
        c = tc.case(kind, n)
        k0 = tc.init_mask(c["means"])
        for a0, a1 in tc.points(c):
            a = tc.ref_eval(c["t"], c["means"], k0, a0, a1, use_mp=True)
            b = tc.ref_eval(c["t"], c["means"], k0, a0, a1, use_mp=False)
            assert (a["cf"], a["c0"], a["c1"]) == (b["cf"], b["c0"], b["c1"])
            for key, unit in (("f", "uf"), ("g0", "ug0"), ("g1", "ug1")):
                assert tc.ratio(b[key], a[key], a[unit]) <= 2.0 ** -8, (kind, n, a0, a1, key)
                assert tc.ratio(b[unit], a[unit], a[unit]) <= 2.0 ** -8


def test_host_evaluations_against_the_reference():
    """hs.trend_eval within K_h EPS S / count of the reference at every size, kind and point, before and after one
    filter pass, with exact kept counts.  K_h: the smallest power of two over the measured worst ratio, for f and g."""
    worst_f, worst_g = (0.0, None), (0.0, None)
    for n in tc.SIZES:
        for kind in tc.KINDS:
            c = tc.case(kind, n)
            for a0, a1 in tc.points(c):
                ref = tc.ref_point(c, a0, a1)
                k0, e0, k1, e1 = hs.trend_eval(c["gw"], c["means"], tc.MIN_DISP, tc.MAX_DISP, a0, a1)
                assert (k0, k1) == (ref["kept0"], ref["kept1"]), (kind, n, a0, a1)
                for got, want in ((e0, ref["e0"]), (e1, ref["e1"])):
                    rf, rg = tc.worst_ratios(got, want)
                    worst_f = max(worst_f, (rf, (kind, n, a0, a1)))
                    worst_g = max(worst_g, (rg, (kind, n, a0, a1)))
    print("host worst f", worst_f, "worst g", worst_g)
    assert worst_f[0] <= tc.K_H_F, worst_f
    assert worst_g[0] <= tc.K_H_G, worst_g
    assert tc.K_H_F == tc.pow2_ceil(tc.HOST_WORST_F) and tc.K_H_G == tc.pow2_ceil(tc.HOST_WORST_G)
    assert tc.K_D_F == tc.pow2_ceil(4 * tc.HOST_WORST_F) and tc.K_D_G == tc.pow2_ceil(4 * tc.HOST_WORST_G)


def test_host_fit_against_the_oracle():
    """hs.trend_fit reproduces the oracle's ok, n_outer and n_kept in every case - the NaN dispersions included, which
    numpy.clip keeps and nanmean skips - and its coefficients within 1e-9 where both converged; at least 90 % of the
    cases with 63 genes or more are compared as converged in both.
    ("flat", 3) is the case that found lbfgsb_dense's missing memory refresh (csrc/dsq_lbfgsb_dense.h): scipy evaluates
    (1e-12, 1e-12) in mid-run there; the coefficients were 1.28e-6 apart before the refresh was reproduced."""
    big = conv = 0
    worst = (0.0, None)
    over = []
    for n in tc.SIZES:
        for kind in tc.KINDS:
            c = tc.case(kind, n)
            fit = c["fit"]
            ch, ok, no, nk = hs.trend_fit(c["gw"], c["means"], tc.MIN_DISP, tc.MAX_DISP, with_kept=True)
            assert ok == fit["ok"], (kind, n)
            assert (no, nk) == (fit["n_outer"], fit["n_kept"]), (kind, n)
            if ok:
                d = float(np.max(np.abs(ch - fit["coef"]) / np.abs(fit["coef"])))
                worst = max(worst, (d, (kind, n)))
                if not d < tc.COEF_TOL:
                    over.append((kind, n, d))
            if n >= 63:
                big += 1
                conv += int(ok and fit["ok"])
    print("host fit: worst coefficient distance", worst, "converged in both", conv, "of", big)
    assert conv >= 0.9 * big, (conv, big)
    assert not over, over


def test_dense_optimiser_follows_the_compact_form_through_a_memory_refresh():
    """lbfgsb_dense (the trend fit's optimiser) against lbfgsb_nd (the compact form, which follows scipy) on 3000 random
    gamma-GLM fits of 2 to 7 genes - flat, trend-like, pure noise, increasing.  More than 100 of them evaluate
    (1e-12, 1e-12) in mid-run, where the reference skips `formk` and refreshes its memory afterwards: same number of
    evaluations and coefficients within 1e-9 in every one (70 differed, some by more than 1e-2, before lbfgsb_dense reproduced
    the refresh)."""
    rng = np.random.default_rng(0)
    touched, bad = 0, []
    for k in range(3000):
        n = int(rng.integers(2, 8))
        nm = np.exp(rng.normal(4, 2, n))
        kind = rng.integers(0, 4)
        if kind == 0:
            t = np.full(n, 0.2) * np.exp(rng.normal(0, 0.05, n))
        elif kind == 1:
            t = (0.05 + 3 / nm) * np.exp(rng.normal(0, 0.3, n))
        elif kind == 2:
            t = np.exp(rng.normal(-2, 3, n))
        else:
            t = (0.01 + nm * 1e-3) * np.exp(rng.normal(0, 0.2, n))
        cov = 1 / nm
        seen = []

        def fg(x, note=None):
            x = np.asarray(x, float)
            if note is not None and (x <= 1e-12).all():
                note.append(1)
            mu = x[0] + x[1] * cov
            with np.errstate(all="ignore"):
                r = (t / mu - 1) / mu
                return float(np.mean(t / mu + np.log(mu))), np.array([-np.mean(r), -np.mean(r * cov)])

        a = hs.lbfgsb_nd(lambda x: fg(x, seen), [1.0, 1.0], [(1e-12, None)] * 2)
        d = hs.lbfgsb_dense(fg, [1.0, 1.0], [(1e-12, None)] * 2)
        touched += bool(seen)
        rel = float(np.max(np.abs(a[0] - d[0]) / np.abs(a[0])))
        if a[2] != d[2] or a[3] != d[3] or not rel <= 1e-9:
            bad.append((k, bool(seen), rel, a[3], d[3]))
    assert touched > 100, touched
    assert not bad, bad
