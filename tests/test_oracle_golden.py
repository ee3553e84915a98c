"""The oracle (oracle/nbglm_oracle.py) against (i) vectors produced by the unmodified
reference kernels (tests/golden/kat_*.npz, see make_golden.py) and (ii) the reference's
own R-DESeq2 fixtures at the reference's own tolerances (tests/test_pydeseq2.py:932-942)."""
import os

import numpy as np
import pytest

from oracle import nbglm_oracle as orc
from tests.helpers import assert_close, load_dataset, load_kat, max_rel_err, r_csv, treatment_design

CASES = ["p1", "p2", "p3", "p4", "p5", "p6", "p7", "p8", "p8m", "p9", "p10", "p11", "p12", "p16", "p24", "p40", "p48"]


@pytest.mark.parametrize("case", CASES)
def test_size_factors_and_mom(case):
    k = load_kat(case)
    sf, normed, lm, filt = orc.size_factors_ratio(k["counts"])
    assert_close(sf, k["sf"], 1e-13, what="sf")
    assert_close(normed, k["normed"], 1e-13, what="normed")
    assert (filt == k["filtered"]).all()
    assert_close(orc.rough_dispersions(k["normed"], k["X"]), k["rough"], 1e-9, 1e-13, "rough")
    assert_close(orc.moments_dispersions(k["normed"], k["sf"]), k["moments"], 1e-12, 1e-15, "mom")
    assert_close(orc.mom_dispersions(k["normed"], k["X"], k["sf"], 1e-8, max(10, len(sf))),
                 k["mom"], 1e-9, 0, "clip(min)")


@pytest.mark.parametrize("case", CASES)
def test_lin_mu_and_irls(case):
    k = load_kat(case)
    assert_close(orc.lin_reg_mu(k["counts"], k["sf"], k["X"], 0.5), k["lin_mu"], 1e-10, 0, "lin_mu")
    b, mu, H, conv = orc.irls(k["counts"], k["sf"], k["X"], k["mom"], 0.5, 1e-8)
    assert (conv == k["irls_conv"]).all()
    assert_close(b, k["irls_beta"], 1e-8, 1e-10, "irls beta")
    assert_close(mu, k["irls_mu"], 1e-8, 1e-10, "irls mu")
    assert_close(H, k["irls_H"], 1e-8, 1e-12, "irls H")


@pytest.mark.parametrize("case", CASES)
def test_alpha_mle(case):
    k = load_kat(case)
    N = k["counts"].shape[0]
    a, c = orc.alpha_mle(k["counts"], k["X"], k["mu_hat"], k["mom"], 1e-8, max(10, N))
    assert (c == k["gw_conv"]).all()
    assert_close(a, k["gw_alpha"], 1e-9, 0, "genewise alpha")
    a, c = orc.alpha_mle(k["counts"], k["X"], k["mu_hat"], k["fitted"], 1e-8, max(10, N),
                         prior_disp_var=float(k["prior_var"]), cr_reg=True, prior_reg=True)
    assert (c == k["map_conv"]).all()
    assert_close(a, k["map_alpha"], 1e-9, 0, "MAP alpha")
    for g in range(len(k["grid_alpha"])):
        la = orc.grid_fit_alpha(k["counts"][:, g], k["X"], k["mu_hat"][:, g], k["mom"][g], 1e-8,
                                max(10, N))
        assert abs(la - k["grid_alpha"][g]) < 1e-12
    nll = [orc.nb_nll(k["counts"][:, g], k["mu_hat"][:, g], np.clip(k["gw_alpha"][g], 1e-8, max(10, N)))
           for g in range(k["counts"].shape[1])]
    assert_close(nll, k["nll"], 1e-14, 0, "nll")


def test_grid_beta():
    k = load_kat("p2")
    disp = np.clip(k["map_alpha"], 1e-8, 40)
    for g in range(len(k["grid_beta"])):
        b = orc.grid_fit_beta(k["counts"][:, g], k["sf"], k["X"], disp[g])
        assert np.abs(b - k["grid_beta"][g]).max() < 1e-12


def test_bfgs_option_of_the_per_gene_kernels():
    """optimizer="BFGS" of fit_alpha_mle / irls_solver: the oracle (scipy's BFGS itself) on the reference's outputs."""
    from tests.helpers import check_bfgs_kats

    check_bfgs_kats(
        load_kat,
        lambda y, X, mu, ah, lo, hi, pv, cr, pr: orc.alpha_mle(y, X, mu, ah, lo, hi, pv, cr, pr, optimizer="BFGS"),
        lambda y, sf, X, d: (lambda r: (r[0], r[3]))(orc.irls(y, sf, X, d, optimizer="BFGS")),
        exact=True)


def test_hard_genes_grid_fallbacks():
    """kat_hard.npz: genes on which the unmodified reference leaves its optimiser for a grid search
    (fit_alpha_mle -> grid_fit_alpha, utils.py:556-564; irls_solver -> grid_fit_beta, utils.py:404-411)."""
    k = load_kat("hard")
    X, sf = k["X"], k["sf"]
    a, c = orc.alpha_mle(k["a_counts"], X, k["a_mu_hat"], k["a_mom"], 1e-8, 40.0)
    assert (c == k["a_conv"]).all() and (~c).sum() >= 10
    assert_close(a, k["a_alpha"], 1e-12, 0, "alpha incl. the grid fallback")
    for g in range(len(k["a_mom"])):
        la = orc.grid_fit_alpha(k["a_counts"][:, g], X, k["a_mu_hat"][:, g], k["a_mom"][g], 1e-8, 40.0)
        assert abs(la - k["a_grid_log_alpha"][g]) < 1e-12
    b, mu, H, conv = orc.irls(k["b_counts"], sf, X, k["b_disp"], 0.5, 1e-8)
    assert (conv == k["b_conv"]).all() and not conv.any()
    assert_close(b, k["b_beta"], 1e-10, 1e-12, "beta after the grid fallback")
    assert_close(b, k["b_grid_beta"], 1e-12, 1e-12, "= grid_fit_beta")
    assert_close(mu, k["b_mu"], 1e-9, 1e-12, "mu")
    assert_close(H, k["b_H"], 1e-8, 1e-12, "H")


@pytest.mark.parametrize("case", CASES)
def test_trend_cooks_wald(case):
    k = load_kat(case)
    N = k["counts"].shape[0]
    gwc = np.clip(k["gw_alpha"], 1e-8, max(10, N))
    means = k["normed"].mean(0)
    coeffs, pred, conv = orc.trend_gamma_glm(1 / means, gwc)
    assert conv == bool(k["trend_conv"])
    assert_close(coeffs, k["trend_coeffs"], 1e-10, 0, "trend coeffs")
    assert_close(orc.robust_mom_disp(k["normed"], k["X"]), k["robust_disp"], 1e-11, 0, "robust")
    assert_close(orc.trimmed_mean(k["normed"], 0.2, axis=0), k["trim_mean_02"], 1e-13, 0, "tm")
    assert abs(orc.mean_absolute_deviation(np.log(gwc) - np.log(k["fitted"])) - k["mad"]) < 1e-13
    disp = np.clip(k["map_alpha"], 1e-8, max(10, N))
    mu_w = np.exp(k["X"] @ k["lfc_beta"].T) * k["sf"][:, None]
    ridge = np.diag(np.repeat(1e-6, k["X"].shape[1]))
    for alt, null in ((None, 0.0), ("greater", 0.5), ("less", -0.5), ("greaterAbs", 0.5),
                      ("lessAbs", 0.5)):
        tag = alt or "none"
        p, s, se = orc.wald_test(k["X"], disp, k["lfc_beta"], mu_w, ridge, k["contrast"],
                                 np.log(2) * null, alt)
        assert_close(se, k[f"wald_se_{tag}"], 1e-11, 0, f"se {tag}")
        assert_close(s, k[f"wald_stat_{tag}"], 1e-10, 1e-14, f"stat {tag}")
        assert_close(p, k[f"wald_p_{tag}"], 1e-9, 1e-300, f"p {tag}")


# ---------------------------------------------------------------- R fixtures, end to end


def _run_r_case(which, factors, continuous=(), with_outliers=False, **kw):
    counts, meta = load_dataset(which)
    if with_outliers:  # tests/test_pydeseq2.py:452-456
        counts.loc["sample1", "gene1"] = 2000
        counts.loc["sample11", "gene7"] = 1000
        meta.loc["sample1", "condition"] = "C"
    X, names = treatment_design(meta, factors, continuous)
    return counts, X, names


def _check_res(res, counts, r_res, contrast_idx, tol):
    l2 = res.LFC[:, contrast_idx] / np.log(2)
    assert max_rel_err(l2, r_res["log2FoldChange"].to_numpy()) < tol
    p = res.pvalue.copy()
    p[res.cooks_outlier] = np.nan
    assert max_rel_err(p, r_res["pvalue"].to_numpy()) < tol


def test_r_single_factor():
    counts, X, names = _run_r_case("synthetic", ["condition"])
    res = orc.deseq2(counts.to_numpy(), X, contrast=[0, 1])
    r_sf = r_csv("single_factor", "r_test_size_factors.csv")["x"].to_numpy()
    np.testing.assert_array_almost_equal(res.size_factors, r_sf, decimal=6)
    _check_res(res, counts, r_csv("single_factor", "r_test_res.csv"), 1, 0.02)
    r_disp = r_csv("single_factor", "r_test_dispersions.csv")["x"].to_numpy()
    assert max_rel_err(res.dispersions, r_disp) < 0.02
    padj = orc.p_value_adjustment(np.where(res.cooks_outlier, np.nan, res.pvalue))
    r_noif = r_csv("single_factor", "r_test_res_no_independent_filtering.csv")
    assert max_rel_err(padj, r_noif["padj"].to_numpy()) < 0.02


@pytest.mark.parametrize("alt,null", [("greater", 0.5), ("less", -0.5), ("greaterAbs", 0.5),
                                      ("lessAbs", 0.5)])
def test_r_alt_hypothesis(alt, null):
    counts, X, _ = _run_r_case("synthetic", ["condition"])
    res = orc.deseq2(counts.to_numpy(), X, contrast=[0, 1], lfc_null=null, alt_hypothesis=alt)
    r_res = r_csv("single_factor", f"r_test_res_{alt}.csv")
    # same comparisons as the reference's test (tests/test_pydeseq2.py:209-226)
    p = np.where(res.cooks_outlier, np.nan, res.pvalue)
    assert (np.isnan(p) == r_res["pvalue"].isna().to_numpy()).all()
    assert max_rel_err(res.LFC[:, 1] / np.log(2), r_res["log2FoldChange"].to_numpy()) < 0.02
    st = np.abs(res.stat) if alt == "lessAbs" else res.stat
    r_st = r_res["stat"].to_numpy()
    nzs = r_st != 0
    assert np.max(np.abs(r_st[nzs] - st[nzs]) / np.abs(r_st[nzs])) < 0.02
    assert ((st != 0) == nzs).all()
    assert max_rel_err(p[nzs], r_res["pvalue"].to_numpy()[nzs]) < 0.02


@pytest.mark.parametrize("with_outliers", [False, True])
def test_r_multi_factor(with_outliers):
    counts, X, names = _run_r_case("synthetic", ["group", "condition"], with_outliers=with_outliers)
    ci = names.index("condition[T.B]")
    c = np.zeros(len(names))
    c[ci] = 1
    res = orc.deseq2(counts.to_numpy(), X, contrast=c)
    fn = "r_test_res_outliers.csv" if with_outliers else "r_test_res.csv"
    _check_res(res, counts, r_csv("multi_factor", fn), ci, 0.04)


@pytest.mark.parametrize("with_outliers", [False, True])
def test_r_continuous(with_outliers):
    counts, X, names = _run_r_case("continuous", ["group", "condition"], ["measurement"],
                                   with_outliers=with_outliers)
    c = np.zeros(len(names))
    c[-1] = 1
    res = orc.deseq2(counts.to_numpy(), X, contrast=c)
    fn = "r_test_res_outliers.csv" if with_outliers else "r_test_res.csv"
    _check_res(res, counts, r_csv("continuous", fn), len(names) - 1, 0.04)


def test_r_wide():
    counts, X, names = _run_r_case("wide", ["group", "condition"])
    ci = names.index("condition[T.B]")
    c = np.zeros(len(names))
    c[ci] = 1
    res = orc.deseq2(counts.to_numpy(), X, contrast=c)
    _check_res(res, counts, r_csv("wide", "r_test_res.csv"), ci, 0.02)


# ---------------------------------------------------------------- summary tail
def test_lowess_and_bh_match_reference():
    """Restated utils.lowess (utils.py:1379-1442) and BH against vectors produced by the unmodified
    reference / scipy (tests/golden/make_golden.py)."""
    k = np.load(os.path.join(os.path.dirname(__file__), "golden", "kat_lowess.npz"))
    for i in range(6):
        out = orc.lowess(k[f"x{i}"], k[f"y{i}"], frac=float(k[f"f{i}"]))
        np.testing.assert_allclose(out, k[f"out{i}"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(orc.bh_adjust(k["bh_in"]), k["bh_out"], rtol=1e-14)


def test_bh_equals_scipy_bit_for_bit_on_ties():
    """scipy.stats.false_discovery_control is what the reference calls (ds.py:486-542); it is installed here.  On
    p-values that tie exactly on the alpha boundary one rounding decides a rejection, so the restatement must keep
    scipy's operation order (`ps *= m / i`): bit-for-bit on tie-heavy vectors, and the rejection counts of the
    independent-filtering passes on the vector that exposed it (seed 354: 208 rejections in pass 47, not 206)."""
    from scipy.stats import false_discovery_control

    for seed in (354, 456, 903, 1, 2):
        rng = np.random.default_rng(seed)
        G = 5000
        bm = 10 ** rng.uniform(-1, 4, G)
        p = rng.uniform(0, 1, G) ** np.where(bm > 50, 6, 1.2)
        p[rng.random(G) < 0.03] = np.nan
        p, bm = np.round(p, 3), np.round(bm, 0)
        ok = ~np.isnan(p)
        assert (orc.bh_adjust(p[ok]) == false_discovery_control(p[ok], method="bh")).all()
        _, info = orc.independent_filtering(bm, p, 0.05)
        for i in (16, 17, 47, 48, 49):
            use = (bm >= info["cutoffs"][i]) & ok
            assert info["num_rej"][i] == int((false_discovery_control(p[use], method="bh") < 0.05).sum())


def test_r_single_factor_summary_padj():
    """DeseqStats.summary() columns incl. independent filtering against R (tests/test_pydeseq2.py:94-118)."""
    counts, X, names = _run_r_case("synthetic", ["condition"])
    res = orc.deseq2(counts.to_numpy(), X, contrast=[0, 1])
    r_res = r_csv("single_factor", "r_test_res.csv")
    s = orc.summary(res, [0, 1])
    assert max_rel_err(s["log2FoldChange"], r_res["log2FoldChange"].to_numpy()) < 0.02
    assert max_rel_err(s["lfcSE"], r_res["lfcSE"].to_numpy()) < 0.02
    assert max_rel_err(s["baseMean"], r_res["baseMean"].to_numpy()) < 0.02
    assert (np.isnan(s["padj"]) == r_res["padj"].isna().to_numpy()).all()
    assert max_rel_err(s["padj"], r_res["padj"].to_numpy()) < 0.02
    s2 = orc.summary(res, [0, 1], independent_filter=False)
    r_noif = r_csv("single_factor", "r_test_res_no_independent_filtering.csv")
    assert max_rel_err(s2["padj"], r_noif["padj"].to_numpy()) < 0.02


# ---------------------------------------------------------------- apeGLM shrinkage
@pytest.mark.parametrize("case", ["p2", "p4"])
def test_nbinom_glm_matches_reference(case):
    """Restated utils.nbinomGLM against outputs of the unmodified reference (kat_shrink.npz)."""
    k = np.load(os.path.join(os.path.dirname(__file__), "golden", "kat_shrink.npz"))
    kk = load_kat(case)
    sidx = int(k[f"{case}_sidx"])
    for tag in "ab":
        for g in range(0, int(k[f"{case}_G"]), 3):
            b, ih, cv = orc.nbinom_glm_gene(kk["X"], kk["counts"][:, g], k[f"{case}_size"][g], np.log(kk["sf"]), 15,
                                            float(k[f"{case}{tag}_scale"]), sidx)
            np.testing.assert_allclose(b, k[f"{case}{tag}_beta"][g], rtol=1e-10, atol=1e-12)
            np.testing.assert_allclose(ih, k[f"{case}{tag}_invh"][g], rtol=1e-8, atol=1e-12)
            assert cv == k[f"{case}{tag}_conv"][g]


@pytest.mark.parametrize("optimizer,tag", [("BFGS", "bfgs"), ("Newton-CG", "ncg")])
def test_nbinom_glm_other_optimizers_match_reference(optimizer, tag):
    """The restated utils.nbinomGLM with optimizer = "BFGS" / "Newton-CG" against the unmodified reference (kat_shrink_opt.npz)."""
    k = np.load(os.path.join(os.path.dirname(__file__), "golden", "kat_shrink_opt.npz"))
    for case in ("p2", "p8"):
        kk = load_kat(case)
        sidx = int(k[f"{case}_sidx"])
        for g in range(0, int(k[f"{case}_G"]), 4):
            b, ih, cv = orc.nbinom_glm_gene(kk["X"], kk["counts"][:, g], k[f"{case}_size"][g], np.log(kk["sf"]), 15,
                                            float(k[f"{case}_scale"]), sidx, optimizer)
            np.testing.assert_allclose(b, k[f"{case}_{tag}_beta"][g], rtol=1e-10, atol=1e-12)
            assert cv == k[f"{case}_{tag}_conv"][g]


@pytest.mark.parametrize("adapt,fn", [(True, "r_test_lfc_shrink_res.csv"),
                                      (False, "r_test_lfc_shrink_no_apeAdapt_res.csv")])
def test_r_lfc_shrink_single_factor(adapt, fn):
    """tests/test_pydeseq2.py:256-341: start from R's size factors, dispersions, LFC and SE."""
    counts, X, names = _run_r_case("synthetic", ["condition"])
    res = orc.deseq2(counts.to_numpy(), X, contrast=[0, 1])
    r_res = r_csv("single_factor", "r_test_res.csv")
    res.size_factors = r_csv("single_factor", "r_test_size_factors.csv")["x"].to_numpy()
    res.dispersions = r_csv("single_factor", "r_test_dispersions.csv")["x"].to_numpy()
    res.LFC[:, 1] = r_res["log2FoldChange"].to_numpy() * np.log(2)
    res.lfcSE = r_res["lfcSE"].to_numpy() * np.log(2)
    lfc, se, conv, scale = orc.lfc_shrink(counts.to_numpy(), X, res, 1, adapt=adapt)
    r_shr = r_csv("single_factor", fn)
    assert max_rel_err(lfc / np.log(2), r_shr["log2FoldChange"].to_numpy()) < 0.02


# ---------------------------------------------------------------- VST
@pytest.mark.parametrize("use_design,fit_type,fn", [(False, "parametric", "r_vst.csv"),
                                                    (True, "parametric", "r_vst_with_design.csv"),
                                                    (False, "mean", "r_mean_vst.csv")])
def test_r_vst(use_design, fit_type, fn):
    """tests/test_pydeseq2.py:761-805."""
    counts, X, _ = _run_r_case("synthetic", ["condition"])
    out, _ = orc.vst(counts.to_numpy(), X, use_design=use_design, fit_type=fit_type)
    r_vst = r_csv("single_factor", fn).T.to_numpy()
    assert np.max(np.abs(r_vst - out) / r_vst) < 0.02


def test_r_size_factors_poscounts_and_control_genes():
    """tests/test_pydeseq2.py:56-91."""
    counts, X, _ = _run_r_case("synthetic", ["condition"])
    c = counts.to_numpy()
    r_sf = r_csv("single_factor", "r_test_size_factors_poscount.csv")["sizeFactor"].to_numpy()
    np.testing.assert_array_almost_equal(orc.size_factors_poscounts(c), r_sf)
    mask = np.zeros(c.shape[1], dtype=bool)
    mask[3] = True  # "gene4"
    expect = c[:, 3] / np.exp(np.log(c[:, 3]).mean())
    np.testing.assert_array_almost_equal(orc.size_factors_control(c, mask), expect)
    np.testing.assert_array_almost_equal(orc.size_factors_poscounts(c, mask), expect)


def test_r_iterative_size_factors():
    """tests/test_pydeseq2.py:344-364."""
    counts, X, _ = _run_r_case("synthetic", ["condition"])
    sf = orc.size_factors_iterative(counts.to_numpy())
    r = r_csv("single_factor", "r_iterative_size_factors.csv").squeeze().to_numpy()
    assert np.max(np.abs(r - sf) / np.abs(r)) < 0.02


@pytest.mark.parametrize("name", ["c3", "c4", "c5"])
def test_oracle_end_to_end_is_the_unmodified_reference_at_benchmark_shapes(name):
    """kat_e2e_*.npz hold the outputs of the reference's own kernels (DefaultInference) end to end at the benchmark
    shapes (8000 x 1000 p=2, 4000 x 500 p=8, 4000 x 5000 p=8 with categorical and continuous covariates).  The oracle's per-gene
    routines repeat the reference's operation sequence (same scipy / numpy / LAPACK calls on the same operands), so on
    the machine that generated the files every output is BIT-IDENTICAL.  Another CPU's BLAS kernels may round a dot
    product differently; a last-bit change of mu_hat moves the stopping point of ~0.1 % of the L-BFGS-B runs
    (tests/tools/flip_floor.py, profiles/r03_flip_floor.json), so the portable assertion is: at most 0.4 % of the genes
    change a success flag, every other gene agrees to 2e-6 (p-values: 2e-6 times 1 + z^2, what 2e-6 on the statistic allows),
    and the cross-gene quantities to 1e-6."""
    import os
    import warnings

    from tests.helpers import flag_flips, load_e2e

    counts, X, ref = load_e2e(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = orc.deseq2(counts, X, n_jobs=max(1, min(16, os.cpu_count() or 1)), keep_layers=False)
    G = counts.shape[1]
    gw, mp, rf = flag_flips(r, ref)
    flips = gw | mp | rf
    assert flips.sum() <= max(2, 0.004 * G), (int(gw.sum()), int(mp.sum()), int(rf.sum()))
    ok = ~flips
    exact = True
    for f in ("size_factors", "normed_means", "mom_dispersions", "genewise_dispersions", "fitted_dispersions",
              "MAP_dispersions", "dispersions", "LFC", "lfcSE", "stat", "pvalue"):
        a, b = np.asarray(getattr(r, f), float), np.asarray(getattr(ref, f), float)
        if f != "size_factors":
            a, b = a[ok], b[ok]
        exact &= np.array_equal(a, b, equal_nan=True)
        tol = 1e-12 if f in ("size_factors", "normed_means", "mom_dispersions") else 2e-6
        if f == "pvalue":
            # p = 2 sf(|z|) multiplies the statistic's relative error by d log p / d log |z| <= 1 + z^2 (Mills' ratio): a
            # statistic that agrees to 2e-6 moves a p-value by up to (1 + z^2) 2e-6, and that is the bound it is held to
            assert (np.isnan(a) == np.isnan(b)).all(), "pvalue: NaN pattern differs"
            z2 = np.nan_to_num(np.asarray(ref.stat, float)[ok]) ** 2
            m = ~np.isnan(b)
            rel = np.abs(a[m] - b[m]) / np.maximum(np.abs(b[m]), 1e-300) / (1.0 + z2[m])
            assert rel.max(initial=0.0) <= tol, f"pvalue: max relative error per (1 + z^2) {rel.max():.3e}"
            continue
        assert_close(a, b, tol, 1e-9 if f in ("LFC", "stat") else 0, f)
    assert_close(r.trend_coeffs, ref.trend_coeffs, 1e-6, 0, "trend")
    assert abs(r.prior_disp_var - ref.prior_disp_var) <= 1e-6 * ref.prior_disp_var
    for f in ("non_zero", "outlier_genes", "replaced", "cooks_outlier", "new_all_zeroes"):
        assert np.array_equal(np.asarray(getattr(r, f))[ok], np.asarray(getattr(ref, f))[ok]), f
    print(f"{name}: {int(flips.sum())} flag flips of {G}; bit-identical on the others: {exact}")
