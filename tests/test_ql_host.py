"""Quasi-likelihood F-test without a GPU: the F distribution's survival function and the deviances of csrc/dsq_ql.h in their
host instantiation (tests/hostql) against mpmath, the moderation against an independent reference (tests/ql_ref.py), the
whole test end to end from oracle fits, the contrast's reduced design, and the refusals of the façade."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests import hostlrt as hl
from tests import hostql as hq
from tests import ql_ref
from tests.helpers import assert_close
from tests.lrt_cases import CASES, lrt_case
from tests.ql_cases import (DEV_C, EPS, F_D1, F_D2, F_SF_C_HOST, deviance_truth, f_sf_check, f_sf_grid, ql_scenario,
                            unit_deviance_truth)


def test_f_sf_against_400_digits():
    """d1 x d2 x F of the issue's grid, truths by the hypergeometric series at 400 digits (tests/ql_cases.py): relative
    error <= c eps (1 + |ln p|) with c = 75, twice the measured 37.2 (at d1 = 127, d2 = 1e5 + 0.4, F = 1).  scipy.stats.f.sf
    is checked against the same truth and the host build against scipy wherever scipy itself is within the bound (it is
    not at large d2: 4e-8 off at d2 = 2.6e7)."""
    import mpmath
    from scipy.stats import f as f_dist

    f_sf_check(hq.f_sf, "host f_sf", F_SF_C_HOST)
    n_ok = 0
    for d1, d2, Fs, truths in f_sf_grid():
        for F, tv in zip(Fs, truths):
            sp = float(f_dist.sf(F, d1, d2))
            lim = F_SF_C_HOST * EPS * (1.0 + abs(float(mpmath.log(tv))))
            if float(abs(mpmath.mpf(sp) - tv) / tv) <= lim:
                n_ok += 1
                assert abs(hq.f_sf([F], d1, d2)[0] - sp) <= 2 * lim * sp, (d1, d2, F)
    assert n_ok >= 100


def test_f_sf_edges():
    for d1 in (1, 2, 127):
        for d2 in (0.7, 21.0, 3e7):
            out = hq.f_sf([0.0, -3.0, -np.inf, np.inf, 1e308, np.nan, 1e-300], d1, d2)
            assert (out[:3] == 1.0).all() and out[3] == 0.0 and 0.0 <= out[4] < 1e-100 and np.isnan(out[5]) and out[6] == 1.0
    assert np.isnan(hq.f_sf([1.0], 3, np.nan)[0])
    # closed forms: d1 = 2: (1 + 2 F / d2)^(-d2 / 2);  d1 = 1, d2 = 1: 1 - (2 / pi) atan(sqrt F)
    F = np.array([0.01, 0.5, 3.0, 40.0])
    np.testing.assert_allclose(hq.f_sf(F, 2, 7.0), (1 + 2 * F / 7.0) ** -3.5, rtol=1e-14)
    np.testing.assert_allclose(hq.f_sf(F, 1, 1.0), 1 - 2 / np.pi * np.arctan(np.sqrt(F)), rtol=1e-14)
    p = hq.f_sf(np.geomspace(1e-3, 1e3, 200), 5, 33.3)
    assert (np.diff(p) < 0).all() and (p > 0).all() and (p < 1).all()


@pytest.mark.parametrize("case", CASES)
def test_deviance_vs_mpmath_and_numerator_bits(case):
    """The shapes of the likelihood-ratio fixture, both host instantiations: |D_f - truth| <= c_D eps sum(|term1| +
    |term2|) with c_D = 2.3 (measured: 0.25 on these genes, 1.14 on single counts), and num equal to hostlrt's statistic
    bit for bit."""
    import mpmath

    counts, sf, X, Xr, fx = lrt_case(case)
    D, S = deviance_truth(counts, sf, X, fx["disp"], fx["beta_full"])
    worst = 0.0
    for wave64 in (False, True):
        num, dev, s2 = hq.deviance(counts, sf, X, Xr, fx["disp"], fx["beta_full"], fx["beta_reduced"], wave64=wave64)
        stat, _ = hl.lrt(counts, sf, X, Xr, fx["disp"], fx["beta_full"], fx["beta_reduced"], wave64=wave64)
        assert num.tobytes() == stat.tobytes()
        assert np.array_equal(s2, dev / (X.shape[0] - X.shape[1]))
        with mpmath.workdps(50):
            worst = max(worst, max(float(abs(mpmath.mpf(float(d)) - t) / (EPS * s)) for d, t, s in zip(dev, D, S)))
    print(f"{case}: c_D = {worst:.3f}")
    assert worst <= DEV_C


def test_unit_deviance_grid_and_edge_rows():
    """Single counts over y in {0 ... 1e6}, mu in {1e-3 ... 3e7}, r in {1e-8 ... 1e8} against mpmath at c_D; y = mu gives
    exactly 0; a row of y = mu (and of zeros at a vanishing mean) and N = 1."""
    import mpmath

    worst = 0.0
    for y in (0, 1, 5, 1000, 10 ** 6):
        for mu in (1e-3, 0.7, 5.0, 999.5, 1000.0, 1e6, 3e7):
            for r in (1e-8, 1e-3, 0.5, 10.0, 1e4, 1e8):
                d = hq.unit_deviance([y], [mu], [r])[0]
                tv, S = unit_deviance_truth(y, mu, r)
                if S == 0:
                    assert d == 0.0, (y, mu, r)
                    continue
                assert d >= 0.0
                with mpmath.workdps(50):
                    worst = max(worst, float(abs(mpmath.mpf(float(d)) - tv) / (EPS * S)))
    print(f"unit deviance: c_D = {worst:.3f}")
    assert worst <= DEV_C
    # all y = mu: eta = 0, mu = sf = y exactly
    N = 70
    y = (np.arange(N) % 9 + 1).astype(np.int64)
    X = np.column_stack([np.ones(N), np.arange(N) % 2]).astype(float)
    for wave64 in (False, True):
        num, dev, s2 = hq.deviance(y[:, None], y.astype(float), X, X[:, :1], [0.3], [[0.0, 0.0]], [[0.0]], wave64=wave64)
        assert num[0] == 0.0 and dev[0] == 0.0 and s2[0] == 0.0
    # rows with zeros; one sample (df = N - P = -1: s2 is the plain quotient)
    y0 = np.zeros((N, 1), np.int64)
    y0[::7] = 3
    num, dev, s2 = hq.deviance(y0, np.ones(N), X, X[:, :1], [0.5], [[0.2, -0.1]], [[0.1]])
    assert_close(dev, ql_ref.unit_deviance(y0[:, 0], np.exp(X @ [0.2, -0.1]), 2.0).sum()[None], 1e-12, 0, "zeros")
    num, dev, s2 = hq.deviance(y0[:1], np.ones(1), X[:1], X[:1, :1], [0.5], [[0.2, -0.1]], [[0.1]], wave64=True)
    assert_close(dev, ql_ref.unit_deviance([3], [np.exp(0.2)], 2.0), 1e-14, 0, "N = 1")
    assert s2[0] == -dev[0]


def test_polygamma_and_trigamma_inverse():
    from scipy.special import digamma, polygamma

    from pydeseq2_amd import ql

    for x in (0.3, 0.5, 1.0, 2.5, 14.9, 15.0, 400.0, 1e6):
        assert abs(ql.digamma(x) - digamma(x)) <= 4e-15 * max(1.0, abs(digamma(x)))
        assert abs(ql.trigamma(x) / polygamma(1, x) - 1) <= 4e-15
        assert abs(ql._polygamma(2, x) / polygamma(2, x) - 1) <= 4e-15
    for v in (1e-8, 1e-5, 0.01, 0.5, 3.0, 100.0, 1e6):
        y = ql.trigamma_inverse(v)
        assert abs(polygamma(1, y) / v - 1) <= (1e-6 if v < 1e-6 else 1e-12)
        assert abs(y / ql_ref.trigamma_inverse(v) - 1) <= 1e-12


def test_squeeze_var_vs_reference():
    from pydeseq2_amd import ql

    rng = np.random.default_rng(11)
    df = 21
    s2 = 0.8 * rng.chisquare(df, 300) / df * np.exp(rng.normal(0, 0.4, 300))  # spread beyond the sampling error
    a, (post, df0, s02, dft) = ql.squeeze_var(s2, df), ql_ref.squeeze_var(s2, df)
    assert np.isfinite(a.df0) and a.n_used == 300
    assert_close(a.df0, df0, 1e-10, 0, "df0")
    assert_close(a.s02, s02, 1e-12, 0, "s02")
    assert_close(a.s2_post, post, 1e-12, 0, "s2_post")
    assert_close(a.df_total, dft, 1e-10, 0, "df_total")
    assert ql.squeeze_var(s2[::-1], df).df0 == a.df0  # (fsum: no dependence on the order)
    # zero and non-finite entries take no part in the prior; zero gets a posterior, NaN stays NaN
    s2b = s2.copy()
    s2b[[3, 50]], s2b[7], s2b[9] = 0.0, np.nan, np.inf
    b, (post, df0, s02, dft) = ql.squeeze_var(s2b, df), ql_ref.squeeze_var(s2b, df)
    assert b.n_used == 296
    assert_close(b.df0, df0, 1e-10, 0, "df0")
    assert_close(b.s2_post, post, 1e-12, 0, "s2_post")
    assert np.isnan(b.s2_post[7]) and np.isinf(b.s2_post[9]) and b.s2_post[3] == b.df0 * b.s02 / (b.df0 + df)
    # v <= 0: s2 exactly chi2_df / df on 8 genes whose sample variance falls below trigamma(df / 2)
    from scipy.special import polygamma

    s2c = np.random.default_rng(1).chisquare(10, 8) / 10
    assert np.log(s2c).var(ddof=1) < polygamma(1, 5.0)
    c, (post, df0, s02, dft) = ql.squeeze_var(s2c, 10), ql_ref.squeeze_var(s2c, 10)
    assert np.isinf(c.df0) and np.isinf(df0) and c.df_total == 80.0 == dft
    assert_close(c.s02, s02, 1e-13, 0, "s02")
    assert (c.s2_post == c.s02).all()
    with pytest.raises(ValueError, match="at least 1"):
        ql.squeeze_var(s2, 0)
    with pytest.raises(ValueError, match="at least 2"):
        ql.squeeze_var([1.0, np.nan], 3)


def _check_f_sf_on_reference(F, d2, p_scipy):
    """The host f_sf at the reference's own F and degrees of freedom (d1 = 1): within the f_sf bound of the mpmath truth
    everywhere, and within twice the bound of scipy.stats.f.sf wherever scipy itself is within the bound of the truth, as
    for the grid (scipy reaches c = 450 at F ~ 1e-3, d2 ~ 60: p = 0.99)."""
    import mpmath
    from tests.ql_cases import f_sf_truth

    mine, n_scipy = hq.f_sf(F, 1, d2), 0
    for m, s, Fg in zip(mine, p_scipy, F):
        if Fg <= 0.0:
            assert m == 1.0 == s
            continue
        tv = f_sf_truth(float(Fg), 1, float(d2), dps=60)
        lim = F_SF_C_HOST * EPS * (1.0 + abs(float(mpmath.log(tv))))
        assert float(abs(mpmath.mpf(float(m)) - tv) / tv) <= lim, (Fg, d2, m)
        if float(abs(mpmath.mpf(float(s)) - tv) / tv) <= lim:
            n_scipy += 1
            assert abs(m - s) <= 2 * lim * s, (Fg, d2, m, s)
    return n_scipy


def _host_path(y, sf, X, Xr, trend, ref):
    """The host-build path on the reference's coefficients: hostql deviances in the device's order,
    pydeseq2_amd.ql.squeeze_var and score_df, hostql score -> (num, dev, sq, F, p)."""
    from pydeseq2_amd import ql

    num, dev, s2 = hq.deviance(y, sf, X, Xr, trend, ref["beta_f"], ref["beta_r"], wave64=True)
    sq = ql.squeeze_var(s2, X.shape[0] - X.shape[1])
    F, p = hq.score(num, sq.s2_post, X.shape[1] - Xr.shape[1], ql.score_df(sq))
    return num, dev, sq, F, p


@pytest.mark.parametrize("N", [6, 64])
def test_end_to_end_reference(N):
    """200 genes, N = 6 (~condition) and 64 (~batch + condition): the reference (oracle IRLS at the trend dispersion,
    numpy deviances, ql_ref.squeeze_var, scipy.stats.f.sf) against the host-build path on the same coefficients.
    F: the reference's deviance is a sum of cancelling terms, S / D <~ 1e4, each good to a few eps: 1e-10 on D_f, 1e-9 on
    F.  p: the reference's OWN F and degrees of freedom go through the host f_sf, so the comparison stands at the pure
    f_sf bound (_check_f_sf_on_reference); the path's own p is f_sf of its own F."""
    from oracle import nbglm_oracle as orc

    counts, meta, X, Xr, c, trend = ql_scenario(N)
    y = counts.to_numpy()
    sf = orc.size_factors_ratio(y)[0]
    ref = ql_ref.ql_reference(y, sf, X, Xr, trend, np.ones(y.shape[1], bool))
    assert np.isfinite(ref["df0"]) and ref["df0"] > 0  # the reference alone finds gene-specific variability (v > 0)
    num, dev, sq, F, p = _host_path(y, sf, X, Xr, trend, ref)
    assert_close(dev, ref["dev"], 1e-10, 0, "deviance")
    assert_close(num, ref["num"], 1e-9, 1e-10, "num")
    assert_close(sq.df0, ref["df0"], 1e-8, 0, "df0")
    assert_close(sq.s02, ref["s02"], 1e-9, 0, "s02")
    assert_close(sq.df_total, ref["df_total"], 1e-8, 0, "df_total")
    assert_close(F, ref["F"], 1e-9, 1e-10, "F")
    assert _check_f_sf_on_reference(ref["F"], ref["df_total"], ref["p"]) >= 100
    assert np.array_equal(p, hq.f_sf(F, 1, sq.df_total))
    assert (ref["p"] < 0.01).sum() >= 5 and (ref["p"] > 0.5).sum() >= 5  # (both tails of the test are exercised)


@pytest.mark.parametrize("seed,df0_inf", [(10, True), (1, False)])
def test_end_to_end_reference_without_gene_specific_variability(seed, df0_inf):
    """10 genes x 12 samples drawn AT the trend.  Seed 10: the sample variance of log s2 falls below trigamma(df / 2), the
    moderation ends with df0 = infinity, and the p-value is the chi-square limit chisq_sf(df_test F, df_test) - NOT F on
    (df_test, n_used df) degrees of freedom, which df_total's cap would give (0.0022 against 0.0016 at F = 10 with 80
    degrees of freedom).  Seed 1: a finite df0 = 112 above the cap, F on (1, 90).  The reference's F through both
    survival functions at the bound of the function used (chisq_sf: tests/lrt_cases.py; f_sf: _check_f_sf_on_reference)."""
    from oracle import nbglm_oracle as orc
    from pydeseq2_amd import ql
    from scipy.stats import chi2, f as f_dist
    from tests.lrt_cases import chisq_grid

    counts, meta, X, Xr, c, trend = ql_scenario(12, G=10, seed=seed, spread=0.0)
    y = counts.to_numpy()
    sf = orc.size_factors_ratio(y)[0]
    ref = ql_ref.ql_reference(y, sf, X, Xr, trend, np.ones(10, bool))
    num, dev, sq, F, p = _host_path(y, sf, X, Xr, trend, ref)
    assert np.isinf(ref["df0"]) == df0_inf == np.isinf(sq.df0) and sq.df_total == 90.0 == ref["df_total"]
    assert_close(sq.s02, ref["s02"], 1e-9, 0, "s02")
    assert_close(F, ref["F"], 1e-9, 1e-10, "F")
    assert F.max() > 20
    if df0_inf:
        assert np.isinf(ql.score_df(sq)) and (sq.s2_post == sq.s02).all()
        assert np.array_equal(ref["p"], chi2.sf(ref["F"], 1))
        assert (np.abs(hl.chisq_sf(ref["F"], 1) - ref["p"]) <= 2 * chisq_grid()["bound"] * ref["p"]).all()
        assert np.array_equal(p, hl.chisq_sf(F, 1))
        assert (np.abs(p / f_dist.sf(F, 1, 90.0) - 1) > 0.05)[F > 10].all()  # (the two behaviours are far apart here)
    else:
        assert ql.score_df(sq) == 90.0 and sq.df0 + 9 > 90.0
        assert _check_f_sf_on_reference(ref["F"], 90.0, ref["p"]) >= 5
        assert np.array_equal(p, hq.f_sf(F, 1, 90.0))


def test_null_space_reduced():
    from pydeseq2_amd.lrt import check_reduced_design
    from pydeseq2_amd.ql import null_space_reduced

    counts, meta, X, Xr, c, trend = ql_scenario(24)
    for cv in (c, np.array([0.0, 1.0, -1.0]), np.array([0.3, -2.0, 1.0])):
        R = null_space_reduced(X, cv)
        assert R.shape == (24, 2) and np.linalg.matrix_rank(R) == 2
        check_reduced_design(X, R)  # nested
        # every model of the reduced design has c . beta = 0: R = X Nc with c^T Nc = 0
        Nc = np.linalg.lstsq(X, R, rcond=None)[0]
        assert np.abs(cv @ Nc).max() < 1e-14
    # a single-coefficient contrast: the column space of X without that column
    R = null_space_reduced(X, c)
    assert np.linalg.matrix_rank(np.hstack([R, X[:, :2]])) == 2
    assert np.array_equal(np.sort(R, axis=1), np.sort(X[:, :2], axis=1))
    with pytest.raises(ValueError, match="not all zero"):
        null_space_reduced(X, np.zeros(3))
    with pytest.raises(ValueError, match="same length"):
        null_space_reduced(X, np.ones(2))


def test_facade_refusals_need_no_gpu():
    from pydeseq2_amd import ql
    from pydeseq2_amd.api import DeseqDataSet, DeseqStats
    from pydeseq2_amd.distributed import DistDeseqPipeline

    counts, meta, X, Xr, c, trend = ql_scenario(24)
    dds = DeseqDataSet(counts=counts, metadata=meta, design="~batch + condition", min_replicates=4)
    con = ["condition", "y", "x"]
    with pytest.raises(ValueError, match="quasi-likelihood F-test has no lfc_null / alt_hypothesis"):
        DeseqStats(dds, con, test="QL", lfc_null=0.5)
    with pytest.raises(ValueError, match="quasi-likelihood F-test has no lfc_null / alt_hypothesis"):
        DeseqStats(dds, con, test="QL", alt_hypothesis="greater")
    with pytest.raises(ValueError, match="not nested"):
        DeseqStats(dds, con, test="QL", reduced=np.column_stack([np.ones(24), np.arange(24.0)]))
    with pytest.raises(ValueError, match="between 1 and 2 columns"):
        DeseqStats(dds, con, test="QL", reduced="~batch + condition")
    with pytest.raises(ValueError, match="'QL' for the"):
        DeseqStats(dds, con, test="score")
    with pytest.raises(ValueError, match="test='QL' fits a reduced design per contrast"):
        DeseqStats.batch(dds, [con], test="QL")
    small = DeseqDataSet(counts=counts.iloc[:3], metadata=meta.iloc[[0, 1, 2]], design="~batch + condition")
    with pytest.raises(ValueError, match="residual degrees of freedom: 3 samples and 3 design columns"):
        DeseqStats(small, con, test="QL")
    assert dds._pipe_obj is None and small._pipe_obj is None  # nothing above has touched the GPU
    # a fit without trend dispersions, and the gene-sharded pipeline: refused before anything is launched
    pipe = SimpleNamespace(design=SimpleNamespace(X=X), G=5, N=24, P=3, ctx=None)
    res = SimpleNamespace(fitted_dispersions=None, non_zero=np.ones(5, bool))
    with pytest.raises(ValueError, match="carries no fitted_dispersions"):
        ql.ql_test(pipe, res, Xr)
    res.fitted_dispersions = np.array([0.1, np.nan, 0.1, 0.1, 0.1])
    with pytest.raises(ValueError, match="not a finite positive number"):
        ql.ql_test(pipe, res, Xr)
    with pytest.raises(ValueError, match="gene-sharded pipeline has no quasi-likelihood test"):
        DistDeseqPipeline.ql(pipe, res, Xr)


def test_ql_entry_points_are_declared_and_the_abi_version_stays():
    from pydeseq2_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "deseq_hip.h")).read()
    names = ("dsq_dev_ql_deviance", "dsq_dev_ql_score", "dsq_dev_f_sf")
    lib = _lib.load()
    for n in names:
        assert re.search(rf"int {n}\(", hdr) and n in _lib.EXPORTS and hasattr(lib, n)
    assert lib.dsq_abi_version() == 5
    assert len(F_D1) * len(F_D2) == 42
