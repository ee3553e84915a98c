"""Likelihood-ratio test without a GPU: the chi-square survival function and the per-gene statistic of csrc/dsq_lrt.h in
their host instantiation (tests/hostlrt) against 50-digit arithmetic and the reference fixture (kat_lrt.npz), the
validation of a reduced design, and the façade's reduced design from a formula."""
import numpy as np
import pandas as pd
import pytest

from tests import hostlrt as hl
from tests.helpers import assert_close
from tests.lrt_cases import CASES, chisq_check, facade_scenario, lrt_case


def test_chisq_sf_against_50_digits():
    """df in {1, 2, 3, 4, 7, 16, 47, 64, 127} x 120 log-spaced x in [1e-8, 1400]: relative error <= 8 x scipy's own worst
    on the grid wherever the truth is >= 1e-300; below that <= 1e-299 and non-negative.  Measured: 4.9e-14 at df = 1,
    x = 1128.4 (scipy: 1.02e-13 at the same point; bound 8.2e-13)."""
    chisq_check(hl.chisq_sf, "host chisq_sf")


def test_chisq_sf_edges():
    for df in (1, 2, 127):
        out = hl.chisq_sf([0.0, -3.0, -np.inf, np.inf, 1e300, np.nan], df)
        assert (out[:3] == 1.0).all() and (out[3:5] == 0.0).all() and np.isnan(out[5])
    # the closed forms of df = 2 and df = 4
    x = np.array([0.5, 3.0, 40.0, 900.0])
    np.testing.assert_allclose(hl.chisq_sf(x, 2), np.exp(-x / 2), rtol=1e-15)
    np.testing.assert_allclose(hl.chisq_sf(x, 4), np.exp(-x / 2) * (1 + x / 2), rtol=1e-15)


@pytest.mark.parametrize("wave64", [False, True], ids=["one_lane", "wave64_order"])
@pytest.mark.parametrize("case", CASES)
def test_lrt_gene_vs_reference_fixture(case, wave64):
    """lrt_gene given the fixture's coefficients: stat to rtol 1e-7 (the Wald-stat tolerance) + 10 x the reference's own
    cancellation error, p to rtol 1e-6 (the Wald-p tolerance) above 1e-300.  Both host instantiations: one lane over all
    samples, and the 64 lane sums in the order of the device's butterfly."""
    counts, sf, X, Xr, fx = lrt_case(case)
    assert 22 <= len(fx["genes"]) <= 24 and int(fx["df"]) == X.shape[1] - Xr.shape[1]
    assert fx["conv_reduced"].all() and fx["conv_full"].all()
    stat, p = hl.lrt(counts, sf, X, Xr, fx["disp"], fx["beta_full"], fx["beta_reduced"], wave64=wave64)
    assert_close(stat, fx["stat"], 1e-7, 10 * float(fx["stat_ref_err"]), f"{case} stat")
    big = fx["p"] > 1e-300
    assert_close(p[big], fx["p"][big], 1e-6, 0, f"{case} p")
    assert (p[~big] <= 1e-299).all() and (p >= 0).all()


def test_lrt_gene_special_values():
    counts, sf, X, Xr, fx = lrt_case("p2")
    bf, br = fx["beta_full"].copy(), fx["beta_reduced"].copy()
    # the same model twice (the dropped coefficient zero): the statistic is exactly 0 and p exactly 1
    bf[:, 0], bf[:, 1] = br[:, 0], 0.0
    stat, p = hl.lrt(counts, sf, X, Xr, fx["disp"], bf, br)
    assert (stat == 0.0).all() and (p == 1.0).all()
    # a "full fit" below the reduced one: negative statistic, p = 1; NaN dispersion (all-zero gene): NaN
    disp = fx["disp"].copy()
    disp[3] = np.nan
    stat, p = hl.lrt(counts, sf, X, Xr, disp, bf + [[1.0, 0.0]], br)  # (any other intercept than the reduced MLE's)
    ok = np.arange(len(disp)) != 3
    assert (stat[ok] < 0).all() and (p[ok] == 1.0).all() and np.isnan(stat[3]) and np.isnan(p[3])


def test_reduced_design_validation():
    from pydeseq2_amd.pipeline import check_reduced_design

    counts, sf, X, Xr, fx = lrt_case("p4")
    assert np.array_equal(check_reduced_design(X, Xr), Xr)
    assert check_reduced_design(X, X @ np.array([[1.0, 0], [1, 1], [0, 2], [0, 0]])).shape == (60, 2)  # nested, re-mixed
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError, match="not nested"):
        check_reduced_design(X, np.column_stack([np.ones(60), rng.normal(size=60)]))
    with pytest.raises(ValueError, match="between 1 and 3 columns"):
        check_reduced_design(X, np.zeros((60, 0)))
    with pytest.raises(ValueError, match="between 1 and 3 columns"):
        check_reduced_design(X, X)
    with pytest.raises(ValueError, match="59 rows"):
        check_reduced_design(X, Xr[:59])
    with pytest.raises(ValueError, match="rank deficient"):
        check_reduced_design(X, np.column_stack([X[:, 0], X[:, 1], X[:, 0] + X[:, 1]]))


def test_facade_reduced_design_and_argument_checks_need_no_gpu():
    from pydeseq2_amd.api import DeseqDataSet, DeseqStats, reduced_design_matrix

    counts, meta, X = facade_scenario()
    dds = DeseqDataSet(counts=counts, metadata=meta, design="~batch + condition", min_replicates=4)
    Xr = reduced_design_matrix(dds, "~batch")
    assert list(Xr.columns) == ["Intercept", "batch[T.b]"] and np.array_equal(Xr.to_numpy(), X[:, :2])
    assert (Xr.index == dds.obs_names).all()
    one = reduced_design_matrix(dds, "~1")
    assert list(one.columns) == ["Intercept"] and (one.to_numpy() == 1.0).all()
    assert np.array_equal(reduced_design_matrix(dds, X[:, [0, 2, 3]]).to_numpy(), X[:, [0, 2, 3]])
    assert np.array_equal(reduced_design_matrix(dds, pd.DataFrame(X[:, :1], index=meta.index)).to_numpy(), X[:, :1])
    with pytest.raises(ValueError, match="not nested"):
        reduced_design_matrix(dds, np.column_stack([np.ones(24), np.arange(24.0)]))
    con = ["condition", "y", "x"]
    with pytest.raises(ValueError, match="between 1 and 3 columns"):
        DeseqStats(dds, con, test="LRT", reduced="~batch + condition")
    with pytest.raises(ValueError, match="needs a reduced design"):
        DeseqStats(dds, con, test="LRT")
    with pytest.raises(ValueError, match="alt_hypothesis"):
        DeseqStats(dds, con, alt_hypothesis="greater", test="LRT", reduced="~batch")
    with pytest.raises(ValueError, match="lfc_null"):
        DeseqStats(dds, con, lfc_null=0.5, test="LRT", reduced="~batch")
    with pytest.raises(ValueError, match="'wald' or 'LRT'"):
        DeseqStats(dds, con, test="score")
    with pytest.raises(ValueError, match="test='LRT'"):
        DeseqStats(dds, con, reduced="~batch")
    assert dds._pipe_obj is None  # nothing above has touched the GPU


def test_lrt_entry_points_are_declared_and_the_abi_version_stays():
    import os
    import re

    from pydeseq2_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "deseq_hip.h")).read()
    assert re.search(r"int dsq_dev_lrt\(", hdr) and re.search(r"int dsq_dev_chisq_sf\(", hdr)
    assert {"dsq_dev_lrt", "dsq_dev_chisq_sf"} <= set(_lib.EXPORTS)
    lib = _lib.load()
    assert hasattr(lib, "dsq_dev_lrt") and hasattr(lib, "dsq_dev_chisq_sf") and lib.dsq_abi_version() == 5
