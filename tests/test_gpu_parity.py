"""GPU parity tests (run with -m gpu on an MI355X): the HIP engine, called through the C ABI
(ctypes -> libdeseq_hip.so), against the reference's kernels (golden KATs), the oracle on seeded
synthetic inputs, and the reference's R fixtures.  Tolerance for floating point results is the
north-star's 1e-5 relative (LFC, dispersions, Wald p-values); genes on which either optimiser's
line search fails at rounding-noise level (reference falls back to a quantised grid search) are
counted and bounded separately."""
import os

import numpy as np
import pytest

from oracle import nbglm_oracle as orc
from tests.helpers import (assert_close, check_hard_dispersion_genes, check_hard_lfc_genes, load_dataset, load_kat,
                           max_rel_err, r_csv, treatment_design)

pytestmark = pytest.mark.gpu

RTOL = 1e-5


@pytest.fixture(scope="module")
def inf():
    from pydeseq2_amd import HipInference

    return HipInference(device=0)


def test_library_is_native(inf):
    info = inf.ctx.device_info()
    assert "gfx950" in info["arch"], info
    assert info["cu_count"] >= 200


@pytest.mark.parametrize("P", list(range(1, 13)))
def test_dispersion_kernel_every_design_width(inf, P):
    """k_alpha<P> (every template instantiation, all memo sizes: genes whose largest count is < 64,
    < 128, < 256 and beyond) against the host instantiation of the same templates, for the MLE and
    the MAP objective.  Guards the register-heavy wide-design variants against miscompiles."""
    from tests import hostsim as hs

    rng = np.random.default_rng(100 + P)
    N, G = 150, 96
    X = np.ones((N, P))
    for j in range(1, P):
        X[:, j] = rng.integers(0, 2, N) if j % 3 else rng.normal(0, 1, N)
    scale = np.repeat([3.0, 30.0, 90.0, 400.0], G // 4)  # one block of genes per memo size
    beta = rng.normal(0, 0.3, (P, G))
    beta[0] = np.log(scale) + rng.normal(0, 0.2, G)
    mu_true = np.exp(np.clip(X @ beta, -20, 9))
    disp = rng.uniform(0.02, 1.0, G)
    counts = rng.negative_binomial(1.0 / disp, 1.0 / (1.0 + mu_true * disp)).astype(np.int64)
    mu = np.maximum(mu_true * np.exp(rng.normal(0, 0.05, (N, G))), 0.5)
    a0 = disp * np.exp(rng.normal(0, 0.3, G))
    for kw in (dict(), dict(prior_disp_var=0.7, cr_reg=True, prior_reg=True)):
        a, c = inf.alpha_mle(counts, X, mu, a0, 1e-8, float(N), **kw)
        ra, rc, _ = hs.alpha_mle(counts, X, mu, a0, 1e-8, float(N),
                                 prior_var=kw.get("prior_disp_var"), cr_reg=True, prior_reg=bool(kw))
        both = c & rc
        assert both.mean() > 0.9, (c.mean(), rc.mean())
        assert (c == rc).mean() > 0.97
        # device and host sum in different orders; a gene whose line search ends inside that rounding
        # noise may stop one step apart (DESIGN.md "parity caveat"): allow a few such genes
        rel = np.abs(a[both] - ra[both]) / np.abs(ra[both])
        assert (rel > 1e-6).mean() <= 0.03 and rel.max() < 5e-3, (P, bool(kw), np.sort(rel)[-5:])


@pytest.mark.parametrize("case", ["p1", "p2", "p3", "p4", "p5", "p6", "p7", "p8", "p8m", "p9", "p10", "p11", "p12", "p16", "p24", "p40", "p48"])
def test_inference_vs_reference_kats(inf, case):
    """Every Inference method on the device against the outputs of the unmodified reference kernels.
    p = 10, 12: the split second sweep of the register path; p = 16, 24: the LDS / MFMA path for designs
    wider than 12 columns."""
    k = load_kat(case)
    N, P = k["X"].shape
    maxd = float(max(10, N))
    atol_a = 1e-6 if P <= 8 else 2e-6  # wide designs: see tests/test_hostsim.py::test_alpha_mle
    assert_close(inf.fit_rough_dispersions(k["normed"], k["X"]), k["rough"], 1e-9, 1e-13, "rough")
    assert_close(inf.fit_moments_dispersions(k["normed"], k["sf"]), k["moments"], 1e-10, 1e-14, "moments")
    assert_close(inf.lin_reg_mu(k["counts"], k["sf"], k["X"], 0.5), k["lin_mu"], 1e-10, 0, "lin_mu")
    if 5 <= P <= 12:
        # batches of < 1024 genes (these KATs; the outlier refit) leave the sixteen-lane IRLS kernel to the one-gene-per-
        # wavefront kernels: pin the sixteen-lane kernel to the same reference outputs as well
        os.environ["DSQ_IRLS_ROW_MIN_G"] = "0"
        try:
            b, mu, H, conv = inf.irls(k["counts"], k["sf"], k["X"], k["mom"], 0.5, 1e-8)
        finally:
            del os.environ["DSQ_IRLS_ROW_MIN_G"]
        assert (conv == k["irls_conv"]).all()
        assert_close(b, k["irls_beta"], 1e-8, 1e-10, "irls beta (sixteen-lane kernel)")
        assert_close(mu, k["irls_mu"], 1e-8, 1e-10, "irls mu (sixteen-lane kernel)")
        assert_close(H, k["irls_H"], 1e-8, 1e-12, "irls H (sixteen-lane kernel)")
    b, mu, H, conv = inf.irls(k["counts"], k["sf"], k["X"], k["mom"], 0.5, 1e-8)
    # p16 holds one low-count gene whose IRLS diverges; the success flag of its L-BFGS-B rescue is decided at
    # rounding-noise level (tests/test_hostsim.py::test_wide_path_vs_reference_kats), its beta agrees
    assert (conv != k["irls_conv"]).sum() <= (1 if case == "p16" else 0)
    assert_close(b, k["irls_beta"], 1e-8, 1e-10, "irls beta")
    assert_close(mu, k["irls_mu"], 1e-8, 1e-10, "irls mu")
    assert_close(H, k["irls_H"], 1e-8, 1e-12, "irls H")
    a, c = inf.alpha_mle(k["counts"], k["X"], k["mu_hat"], k["mom"], 1e-8, maxd)
    assert (c == k["gw_conv"]).all()
    assert_close(a, k["gw_alpha"], atol_a, 0, "genewise alpha")
    a, c = inf.alpha_mle(k["counts"], k["X"], k["mu_hat"], k["fitted"], 1e-8, maxd,
                         prior_disp_var=float(k["prior_var"]), cr_reg=True, prior_reg=True)
    assert (c == k["map_conv"]).all()
    assert_close(a, k["map_alpha"], atol_a, 0, "MAP alpha")
    ng = len(k["grid_alpha"])  # a7: the device grid-search kernels (100 waves per gene and level)
    la = inf.grid_fit_alpha(k["counts"][:, :ng], k["X"], k["mu_hat"][:, :ng], 1e-8, maxd)
    assert np.abs(la - k["grid_alpha"]).max() < 1e-12
    if "grid_beta" in k:  # a11
        gb = inf.grid_fit_beta(k["counts"][:, :ng], k["sf"], k["X"], np.clip(k["map_alpha"], 1e-8, maxd)[:ng])
        assert np.abs(gb - k["grid_beta"]).max() < 1e-12
    disp = np.clip(k["map_alpha"], 1e-8, maxd)
    b, mu, H, conv = inf.irls(k["counts"], k["sf"], k["X"], disp, 0.5, 1e-8)
    assert (conv == k["lfc_conv"]).all()
    assert_close(b, k["lfc_beta"], 1e-8, 1e-10, "lfc beta")
    mu_w = np.exp(k["X"] @ k["lfc_beta"].T) * k["sf"][:, None]
    ridge = np.diag(np.repeat(1e-6, P))
    for alt, null in ((None, 0.0), ("greater", 0.5), ("less", -0.5), ("greaterAbs", 0.5), ("lessAbs", 0.5)):
        tag = alt or "none"
        p, s, se = inf.wald_test(k["X"], disp, k["lfc_beta"], mu_w, ridge, k["contrast"], np.log(2) * null, alt)
        assert_close(se, k[f"wald_se_{tag}"], 1e-10, 0, f"se {tag}")
        assert_close(s, k[f"wald_stat_{tag}"], 1e-9, 1e-13, f"stat {tag}")
        assert_close(p, k[f"wald_p_{tag}"], 1e-8, 1e-300, f"p {tag}")
    coeffs, pred, ok = inf.dispersion_trend_gamma_glm(1 / k["normed"].mean(0), np.clip(k["gw_alpha"], 1e-8, maxd))
    assert ok == bool(k["trend_conv"])
    assert_close(coeffs, k["trend_coeffs"], 1e-10, 0, "trend")


def test_grid_fallbacks_on_genes_where_the_reference_takes_them(inf):
    """a7 / a11 on the device (kat_hard.npz: every gene of a seeded search on which the unmodified reference
    left its optimiser): k_alpha_grid_eval / k_alpha_grid_pick against grid_fit_alpha, k_grid_beta and the
    rescue kernel's fallback against grid_fit_beta, and the full entry points alpha_mle / irls on those genes."""
    k = load_kat("hard")
    X, sf = k["X"], k["sf"]
    la = inf.grid_fit_alpha(k["a_counts"], X, k["a_mu_hat"], 1e-8, 40.0)
    a, c = inf.alpha_mle(k["a_counts"], X, k["a_mu_hat"], k["a_mom"], 1e-8, 40.0)
    check_hard_dispersion_genes(k, a, c, la)
    gb = inf.grid_fit_beta(k["b_counts"], sf, X, k["b_disp"])
    assert np.abs(gb - k["b_grid_beta"]).max() < 1e-12
    b, mu, H, conv = inf.irls(k["b_counts"], sf, X, k["b_disp"], 0.5, 1e-8)
    check_hard_lfc_genes(k, b, mu, H, conv)


def test_bfgs_option_of_alpha_mle_and_irls(inf):
    """optimizer="BFGS" through the plug-in interface (Inference.alpha_mle / Inference.irls, inference.py:46-178):
    scipy's BFGS restated on the device (csrc/dsq_bfgs.h) against the unmodified reference (kat_bfgs.npz)."""
    from tests.helpers import check_bfgs_kats

    check_bfgs_kats(
        load_kat,
        lambda y, X, mu, ah, lo, hi, pv, cr, pr: inf.alpha_mle(y, X, mu, ah, lo, hi, pv, cr, pr, optimizer="BFGS"),
        lambda y, sf, X, d: (lambda r: (r[0], r[3]))(inf.irls(y, sf, X, d, 0.5, 1e-8, optimizer="BFGS")))
    # the default optimiser is back afterwards
    k = load_kat("p2")
    a, c = inf.alpha_mle(k["counts"], k["X"], k["mu_hat"], k["mom"], 1e-8, 40.0)
    assert_close(a, k["gw_alpha"], 1e-6, 0, "genewise alpha (L-BFGS-B after a BFGS call)")


def test_rough_dispersions_n_equals_p_raises(inf):
    X = np.eye(3)
    with pytest.raises(ValueError):
        inf.fit_rough_dispersions(np.ones((3, 5)), X)


def _compare(res, ref, frac_noise=0.002):
    """1e-5 parity on the north-star outputs.  Only genes on which the two L-BFGS-B runs DISAGREE about
    convergence (line search lost in rounding noise: one side returns its last iterate, the other the
    quantised grid value) are excluded, and they must be a tiny fraction.  Genes on which BOTH report
    non-convergence went through the deterministic grid search on both sides (utils.py:556-564) and must
    agree to 1e-10 (the grid objective has no prior term, so this holds for the MAP fit as well)."""
    G = len(ref.dispersions)
    assert_close(res.size_factors, ref.size_factors, 1e-12, 0, "size factors")
    assert (res.non_zero == ref.non_zero).all()
    nz = ref.non_zero
    with np.errstate(invalid="ignore"):
        noisy = (res.genewise_converged != ref.genewise_converged) | (res.MAP_converged != ref.MAP_converged)
    noisy &= nz
    noisy |= res.refitted != ref.refitted
    assert noisy.sum() <= max(2, frac_noise * G), f"{noisy.sum()} noise-limited genes of {G}"
    untouched = nz & ~res.refitted & ~ref.refitted  # refitted genes carry the dispersions of the replaced counts
    both_gw = untouched & (res.genewise_converged == 0) & (ref.genewise_converged == 0)
    assert_close(res.genewise_dispersions[both_gw], ref.genewise_dispersions[both_gw], 1e-10, 0, "grid genewise")
    both_map = untouched & (res.MAP_converged == 0) & (ref.MAP_converged == 0)
    assert_close(res.MAP_dispersions[both_map], ref.MAP_dispersions[both_map], 1e-10, 0, "grid MAP")
    ok = ~noisy
    assert (res.refitted[ok] == ref.refitted[ok]).all()
    assert (res.cooks_outlier[ok] == ref.cooks_outlier[ok]).all()
    assert_close(res.dispersions[ok], ref.dispersions[ok], RTOL, 0, "dispersions")
    assert_close(res.LFC[ok], ref.LFC[ok], RTOL, 1e-8, "LFC")
    # p = 2 sf(|z|): a relative error eps of the statistic is a relative error ~ eps * z^2 of the p-value in the tail
    assert_close(res.stat[ok], ref.stat[ok], RTOL, 1e-8, "stat")
    with np.errstate(invalid="ignore", divide="ignore"):
        perr = np.abs(res.pvalue[ok] - ref.pvalue[ok]) / np.maximum(ref.pvalue[ok], 1e-300)
        perr = np.nan_to_num(perr / np.maximum(1.0, ref.stat[ok] ** 2))
    assert (np.isnan(res.pvalue[ok]) == np.isnan(ref.pvalue[ok])).all() and perr.max() <= RTOL, perr.max()
    # the RAW p-value (north-star wording) next to the per-z^2 one: bounded by the reference's own noise floor (the reference
    # against itself with mu_hat moved by one ulp: up to 0.33 % of the genes beyond 1e-5, worst 6.6e-5; bench.py)
    with np.errstate(invalid="ignore", divide="ignore"):
        praw = np.nan_to_num(np.abs(res.pvalue[ok] - ref.pvalue[ok]) / np.maximum(ref.pvalue[ok], 1e-300))
    # (asserted where the floor was measured - slices of 2000 genes and more - and wherever no flag flipped: ONE flip among
    # G genes moves the trend, and with it every p-value, by ~2e-3 / G times z^2 / 2, which on a 120-gene slice is 1e-5 at |z| = 1)
    if G >= 2000 or noisy.sum() == 0:
        assert (praw > 1e-5).sum() <= max(3, 4e-3 * G), f"{(praw > 1e-5).sum()} genes with a raw p-value difference beyond 1e-5"
        assert praw.max() <= 3e-4, f"raw p-value difference {praw.max():.3e}"
    assert_close(res.lfcSE[ok], ref.lfcSE[ok], RTOL, 0, "lfcSE")
    # the trend is fitted on all genes, so it carries the noise genes' influence: one flip of G genes moves it by ~2e-3 / G
    # (measured: engine vs reference 8e-7 at 20 000 / 60 000 genes, 2.2e-6 at 2000; the reference against itself 1e-6 ... 3.8e-6)
    assert_close(res.trend_coeffs, ref.trend_coeffs, max(2e-5, 0.02 / G), 0, "trend coeffs")
    return int(noisy.sum()), int(both_gw.sum() + both_map.sum())


@pytest.mark.parametrize("G,N,design,seed", [(1000, 100, "2level", 1), (1500, 60, "3factor", 2),
                                              (800, 80, "mixed", 3)])
def test_pipeline_vs_oracle(G, N, design, seed):
    import pydeseq2_amd

    counts, X = orc.synth_counts(G, N, design, seed)
    counts[:, 5] = 0  # an all-zero gene -> NaN outputs (tests/test_edge_cases.py:10-52)
    if design == "2level":  # inject outliers so the Cook's refit path is live
        counts[3, 10] = 200000
        counts[7, 11] = 150000
    res = pydeseq2_amd.deseq2(counts, X, device=0)
    ref = orc.deseq2(counts, X, n_jobs=8)
    assert np.isnan(res.dispersions[5]) and np.isnan(res.pvalue[5]) and np.isnan(res.LFC[5]).all()
    _compare(res, ref)
    if design == "2level":
        assert ref.replaced.sum() >= 2 and (res.replaced == ref.replaced).all()


@pytest.mark.parametrize("levels,N", [(6, 90), (8, 200), (3, 75)])
def test_pipeline_one_factor_many_levels(levels, N):
    """One factor with `levels` levels: as many design cells as columns, so mu_hat is the linear model's (dds.py:747-756)
    and the dispersion fits run four genes per wavefront - per-cell tables in LDS for 5 .. 32 cells (k_alpha_rows_c, linear
    branch: clamped mu_hat from x_c . coef), registers up to 4 cells (k_alpha_rows) - against the oracle."""
    import pydeseq2_amd

    rng = np.random.default_rng(40 + levels)
    lv = np.arange(N) % levels
    rng.shuffle(lv)
    X = np.column_stack([np.ones(N)] + [(lv == k).astype(float) for k in range(1, levels)])
    G = 700
    beta = np.zeros((levels, G))
    beta[0] = rng.normal(4, 2, G)
    beta[1:] = rng.normal(0, 0.5, (levels - 1, G))
    disp = 4 / np.maximum(2.0 ** beta[0], 1e-3) + 0.1
    sf = np.exp(rng.normal(0, 0.2, N))
    mu = sf[:, None] * 2.0 ** (X @ beta)
    counts = rng.negative_binomial(1 / disp[None, :], 1 / (1 + mu * disp[None, :])).astype(np.int64)
    counts[:, 7] = 0
    c = np.zeros(levels)
    c[1] = 1.0
    pipe = pydeseq2_amd.DeseqPipeline(counts, X, device=0)
    assert pipe._row_mode == (1 if levels <= 4 else 2) and pipe.design.linear_mu
    res = pipe.deseq2(contrast=c)
    ref = orc.deseq2(counts, X, contrast=c, n_jobs=_jobs())
    _compare(res, ref, frac_noise=0.006)


def test_pipeline_vs_oracle_many_samples():
    """C5-shaped case (N = 2500, two categorical + three continuous covariates): rows too long for the
    LDS staging, so the dispersion kernel runs its streaming (unstaged, masked) variant, IRLS supplies
    mu_hat, Cook's sorts over the whole gene (no design cells with replicates)."""
    import pydeseq2_amd

    counts, X = orc.synth_counts(160, 2500, "mixed", 5)
    res = pydeseq2_amd.deseq2(counts, X, device=0)
    ref = orc.deseq2(counts, X, n_jobs=8)
    _compare(res, ref)


def _jobs():
    import os

    return max(1, min(64, os.cpu_count() or 1))


@pytest.mark.parametrize("cfg,G,N,design,seed", [
    ("c3", 2000, 1000, "2level", 2),      # BASELINE configs[2]: the benchmark's shape (LDS-staged dispersion kernel)
    ("c4", 2000, 500, "3factor", 3),      # configs[3]: p = 8, 30 design cells, IRLS supplies mu_hat
    ("c5-shard", 2000, 5000, "mixed", 4),  # configs[4] per-GPU shard: p = 8 with continuous covariates, long rows
])
def test_pipeline_vs_oracle_at_benchmark_shapes(cfg, G, N, design, seed):
    """End-to-end 1e-5 parity against the oracle on 2000-gene slices with the benchmark configurations' sample
    counts and designs (the per-gene kernels run the very instantiations the full-size launches use)."""
    import pydeseq2_amd

    counts, X = orc.synth_counts(G, N, design, seed)
    res = pydeseq2_amd.deseq2(counts, X, device=0)
    ref = orc.deseq2(counts, X, n_jobs=_jobs(), keep_layers=False)
    # At N >= 500 about 0.1 % of the fits per launch end with |gradient| between 1e-5 and 1e-3 at a point where
    # the expected decrease of the next step (g^2 / 2h ~ 1e-11) is below the fp64 resolution of the loss itself
    # (ulp(5000) ~ 1e-12): whether scipy's - or this engine's - line search then reports success is decided by
    # the last bit of the loss, in both implementations, on different genes (DESIGN.md par. 7).  Measured on these
    # slices: 6-8 genes of 2000 over the genewise fit, the MAP fit and the refit together.
    n_noise, n_grid = _compare(res, ref, frac_noise=0.005)
    print(f"{cfg}: {n_noise} noise-limited genes, {n_grid} grid-fallback fits compared at 1e-10")


@pytest.mark.parametrize("name", ["c3", "c4", "c5"])
def test_pipeline_vs_unmodified_reference_at_benchmark_shapes(name):
    """The engine against the outputs of the UNMODIFIED reference (tests/golden/kat_e2e_*.npz: DefaultInference end to end,
    8000 x 1000 p=2 / 4000 x 500 p=8 / 4000 x 5000 p=8 categorical + continuous) - no oracle in between.  1e-5 on every gene whose
    success flags agree; the flips are counted per stage and written next to the bench outputs.  The floor of that count
    is what a one-ulp change of mu_hat does to the reference's own fits: 0.09-0.18 % of the genes per fit
    (profiles/r03_flip_floor.json)."""
    import json
    import os

    import pydeseq2_amd
    from tests.helpers import flag_flips, load_e2e

    counts, X, ref = load_e2e(name)
    res = pydeseq2_amd.deseq2(counts, X, device=0)
    gw, mp, rf = flag_flips(res, ref)
    # (c5: 4000 genes since round 4 - measured 3 flips of 4000, profiles/r04_parity_vs_reference_c5.json; the floor of its
    # shape is 1-3 flips per fit per 1000 genes, profiles/r03_flip_floor_c5.json)
    n_noise, n_grid = _compare(res, ref, frac_noise=0.004)
    rec = {"case": name, "genes": int(counts.shape[1]), "samples": int(counts.shape[0]), "p": int(X.shape[1]),
           "flips_genewise": int(gw.sum()), "flips_MAP": int(mp.sum()), "flips_refit": int(rf.sum()),
           "flip_genes": n_noise, "flip_rate": round(n_noise / counts.shape[1], 6), "both_on_grid": n_grid,
           "reference_non_converged": int(np.nansum(ref.genewise_converged == 0) + np.nansum(ref.MAP_converged == 0))}
    ok = ~(gw | mp | rf) & ref.non_zero
    for f in ("dispersions", "lfcSE", "stat"):
        a, b = np.asarray(getattr(res, f))[ok], np.asarray(getattr(ref, f))[ok]
        rec[f"max_rel_{f}"] = float(np.nanmax(np.abs(a - b) / np.maximum(np.abs(b), 1e-3 if f == "stat" else 1e-300)))
    rec["max_rel_LFC"] = float(np.nanmax(np.abs(res.LFC[ok] - ref.LFC[ok]) / np.maximum(np.abs(ref.LFC[ok]), 1e-3)))
    print(rec)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    os.makedirs(out, exist_ok=True)
    json.dump(rec, open(os.path.join(out, f"parity_vs_reference_{name}.json"), "w"), indent=1)


def _wide_case(kind, G, N, seed):
    rng = np.random.default_rng(seed)
    if kind == "factor16":  # one factor with 16 levels: P = 16 = number of cells (linear-model mu_hat, cell path)
        lv = np.arange(N) % 16
        rng.shuffle(lv)
        X = np.column_stack([np.ones(N)] + [(lv == k).astype(float) for k in range(1, 16)])
    elif kind == "factor40":  # one factor with 40 levels (round 6: up to 48 columns): P = 40 = number of cells
        lv = np.arange(N) % 40
        rng.shuffle(lv)
        X = np.column_stack([np.ones(N)] + [(lv == k).astype(float) for k in range(1, 40)])
    else:  # a 2-level and a 4-level factor + 9 (mixed14) or 39 (mixed44) continuous covariates: no cell structure
        a, b = np.arange(N) % 2, (np.arange(N) // 2) % 4
        n_cont = 39 if kind == "mixed44" else 9
        X = np.column_stack([np.ones(N), a == 1] + [(b == k) for k in (1, 2, 3)] + [rng.normal(0, 0.5, N) for _ in range(n_cont)])
        X = X.astype(float)
    P = X.shape[1]
    beta = np.zeros((P, G))
    beta[0] = rng.normal(4, 2, G)
    beta[1:] = rng.normal(0, 0.3, (P - 1, G))
    disp = 4 / np.maximum(2.0 ** beta[0], 1e-3) + 0.1
    sf = np.exp(rng.normal(0, 0.2, N))
    mu = sf[:, None] * 2.0 ** (X @ beta)
    size = 1 / disp
    counts = rng.negative_binomial(size[None, :], size[None, :] / (size[None, :] + mu)).astype(np.int64)
    return counts, X


@pytest.mark.parametrize("kind,G,N", [("factor16", 600, 160), ("mixed14", 500, 120), ("factor40", 300, 480),
                                      ("mixed44", 240, 520)])
def test_pipeline_with_designs_wider_than_12_columns(kind, G, N):
    """The reference has no limit on the design width (utils.py:345-371): designs beyond the 12 columns of the
    register kernels run the LDS / matrix-core path (dsq_wide.h), end to end against the oracle - up to the engine's 48
    columns (round 6: a 40-level factor = 40 design cells, and 44 columns without cell structure: three 16-row tiles of the
    matrix-core Gram accumulation)."""
    import pydeseq2_amd

    counts, X = _wide_case(kind, G, N, 31)
    if X.shape[1] > 32:  # expressed genes only: a low-count gene with 40 coefficients goes through the IRLS rescue, whose
        counts = counts[:, counts.mean(0) >= 30]  # stopping point on a flat likelihood is pinned by kat_hard, not here
    counts[:, 4] = 0
    c = np.zeros(X.shape[1])
    c[1] = 1.0
    res = pydeseq2_amd.deseq2(counts, X, contrast=c, device=0)
    ref = orc.deseq2(counts, X, contrast=c, n_jobs=_jobs())
    _compare(res, ref, frac_noise=0.01)


def test_matrix_core_path_equals_register_path_at_p8():
    """DSQ_WIDE_MIN_P routes narrower designs without cell structure through the LDS / MFMA kernels: same results
    as the register kernels on the c5-shaped design (two categorical + three continuous covariates, p = 8)."""
    import os
    import subprocess
    import sys

    code = ("import numpy as np, pydeseq2_amd; from oracle import nbglm_oracle as orc; "
            "counts, X = orc.synth_counts(400, 300, 'mixed', 6); r = pydeseq2_amd.deseq2(counts, X, device=0); "
            "np.savez(sys.argv[1], d=r.dispersions, l=r.LFC, p=r.pvalue, g=r.genewise_converged, m=r.MAP_converged)")
    import tempfile

    outs = []
    for env in ({}, {"DSQ_WIDE_MIN_P": "5"}):
        f = tempfile.mktemp(suffix=".npz")
        subprocess.run([sys.executable, "-c", "import sys; " + code, f], check=True, env={**os.environ, **env},
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), timeout=400)
        outs.append(dict(np.load(f)))
    a, b = outs
    same = (a["g"] == b["g"]) & (a["m"] == b["m"])
    assert same.mean() > 0.99
    assert_close(b["d"][same], a["d"][same], 1e-6, 0, "dispersions")
    assert_close(b["l"][same], a["l"][same], 1e-6, 1e-9, "LFC")


def test_sixteen_lane_irls_equals_the_wavefront_kernel():
    """Designs with cells and p >= 5 fit their LFCs (and the IRLS mu_hat) with sixteen lanes per gene (k_irls_row,
    RowWave); DSQ_NO_ROW_WAVE=1 keeps the one-gene-per-wavefront kernel: the same results to rounding on the 30-cell
    design, incl. the rescue of diverged genes, the Cook's flags and the refit of an injected outlier (apart from the
    odd gene whose dispersion fit flips its convergence flag on the last bits of mu_hat)."""
    import os
    import subprocess
    import sys
    import tempfile

    code = ("import numpy as np, pydeseq2_amd; from oracle import nbglm_oracle as orc; "
            "counts, X = orc.synth_counts(2400, 90, '3factor', 7); counts[5, :40] = 200000; "
            "r = pydeseq2_amd.deseq2(counts, X, device=0); "
            "np.savez(sys.argv[1], d=r.dispersions, l=r.LFC, p=r.pvalue, se=r.lfcSE, g=r.genewise_converged, "
            "m=r.MAP_converged, c=r.cooks_outlier, f=r.refitted, lc=r.LFC_converged)")
    outs = []
    for env in ({}, {"DSQ_NO_ROW_WAVE": "1"}):
        f = tempfile.mktemp(suffix=".npz")
        subprocess.run([sys.executable, "-c", "import sys; " + code, f], check=True, env={**os.environ, **env},
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), timeout=400)
        outs.append(dict(np.load(f)))
    a, b = outs
    assert (a["f"] == b["f"]).all() and (a["c"] == b["c"]).all() and (a["lc"] == b["lc"]).all()
    with np.errstate(invalid="ignore"):
        same = (a["g"] == b["g"]) & (a["m"] == b["m"]) & \
            ~(np.abs(a["d"] - b["d"]) > 1e-6 * np.abs(b["d"]))  # (a flipped dispersion-outlier decision shows here)
    assert (~same).sum() <= 3
    # the two kernels order their sums differently (four samples per trip, start values from per-cell sums), so mu_hat
    # differs in the last bits and the dispersion optimiser lands within its own resolution (4e-7 for an ulp of mu_hat,
    # profiles/r03_flip_floor.json: max_rel_same_flag)
    assert_close(b["d"][same], a["d"][same], 2e-6, 0, "dispersions")
    assert_close(b["l"][same], a["l"][same], 1e-6, 1e-9, "LFC")
    assert_close(b["se"][same], a["se"][same], 1e-6, 0, "lfcSE")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["2level", "3factor", "mixed", "2level_layers", "continuous"])
def test_lfc_fit_in_two_launches_equals_the_single_launch(kind):
    """In a whole pass the genes whose MAP dispersion is final after the MAP stage's full-size launch start their LFC fit
    from inside that stage, on a stream of their own, and the rest follow in a second launch that joins it
    (pipeline._fork_lfc, csrc dsq_lfc_set_part).  Every gene is fitted exactly once with its final dispersion: the results
    are BIT-identical to the single launch (DSQ_LFC_OVERLAP=0), over the wavefront kernel (two cells), the sixteen-lane
    kernel (30 cells), the mixed-design kernels and the general kernel, with zero genes, injected outliers (the refit)
    and, once, the N x G layers kept."""
    from pydeseq2_amd import DeseqPipeline

    if kind == "mixed":
        counts, X = _mixed_case(8, 3, 1400, 3000, 5, (2, 4))
    elif kind == "3factor":
        counts, X = orc.synth_counts(3200, 120, "3factor", 11)
    elif kind == "continuous":  # four covariates: beyond the mixed-design kernels, no cells - the general kernel
        counts, X = _mixed_case(5, 4, 200, 3000, 12, ())
    else:
        counts, X = orc.synth_counts(6000, 200, "2level", 13)
    counts = counts.copy()
    counts[:, 17] = 0
    counts[3, 40:44] = 150000  # Cook's outliers: replaced, refitted
    keep = kind.endswith("_layers")
    pipe = DeseqPipeline(counts, X, device=0)
    pipe.keep_layers = keep
    pipe._lfc_overlap = True  # (the default depends on the design family: DSQ_LFC_OVERLAP)
    forks = pipe.lfc_forks
    a = pipe.deseq2()
    assert pipe.lfc_forks == forks + 1, "the LFC fit did not fork"
    la = {k: pipe.layer(k).copy() for k in (("mu_LFC", "hat_diagonals", "cooks") if keep else ("cooks",))}
    a2 = pipe.deseq2()  # a second pass on recycled buffers
    pipe._lfc_overlap = False
    b = pipe.deseq2()
    assert pipe.lfc_forks == forks + 2
    lb = {k: pipe.layer(k).copy() for k in la}
    if kind in ("2level", "2level_layers", "3factor"):  # (continuous covariates: no sample is replaceable, dds.py:1301-1330)
        assert a.refitted.sum() >= 1
    for f in ("size_factors", "genewise_dispersions", "MAP_dispersions", "MAP_converged", "dispersions", "outlier_genes", "LFC",
              "LFC_converged", "lfcSE", "stat", "pvalue", "cooks_outlier", "replaced", "refitted"):
        for x in (a, a2):
            va, vb = np.asarray(getattr(x, f)), np.asarray(getattr(b, f))
            assert va.shape == vb.shape and np.array_equal(va, vb, equal_nan=va.dtype.kind == "f"), f
    for k in la:
        assert np.array_equal(la[k], lb[k], equal_nan=True), k


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["2factor", "3factor", "factor16", "mixed14"])
def test_whole_passes_are_bit_reproducible(kind):
    """deseq2() twice on the same pipeline gives the same bits, whatever ran on the device in between (recycled buffers,
    stale LDS): the many-cell kernels (whose sixteen-lane IRLS used to take "any sample" of a design cell for its start
    values - the column of pinv(X) of whichever thread wrote last, equal to rounding only), the LDS / matrix-core kernels
    of designs beyond 12 columns.  (Two cells, mixed and general designs: test_lfc_fit_in_two_launches_equals_the_single_
    launch and test_rescued_gene_is_reproducible_from_pass_to_pass.)"""
    from pydeseq2_amd import DeseqPipeline

    if kind in ("2factor", "3factor"):
        counts, X = orc.synth_counts(2400, 120, kind, 21)
    else:
        counts, X = _wide_case(kind, 800, 160, 9)
    counts = np.array(counts, copy=True)
    counts[:, 5] = 0
    counts[2, 30:33] = 120000
    pipe = DeseqPipeline(counts, X, device=0)
    first = pipe.deseq2()
    ref = {f: np.array(getattr(first, f), copy=True) for f in
           ("genewise_dispersions", "dispersions", "LFC", "lfcSE", "pvalue", "LFC_converged", "refitted", "cooks_outlier")}
    for _ in range(4):
        r = pipe.deseq2()
        for f, v in ref.items():
            assert np.array_equal(np.asarray(getattr(r, f)), v, equal_nan=v.dtype.kind == "f"), f


@pytest.mark.gpu
def test_rescued_gene_is_reproducible_from_pass_to_pass():
    """A gene whose IRLS diverges is rescued by the bounded L-BFGS-B (utils.py:389-399).  scipy hands that routine
    zero-initialised work arrays and the routine reads entries it has not written yet; the device workspace lives in LDS,
    which holds whatever the previous workgroup left: before it was zeroed (dsq_lbfgsb.h) such a gene took 14, 18, 20 or 22
    iterations from one whole pass to the next and its dispersions moved in the sixth digit."""
    from pydeseq2_amd import DeseqPipeline

    counts, X = _mixed_case(5, 4, 200, 3000, 12, ())  # four covariates: the general kernels
    counts = counts.copy()
    counts[3, 40:44] = 150000  # one sample with a count three orders of magnitude beyond the rest, in four genes
    pipe = DeseqPipeline(counts, X, device=0)
    seen = set()
    for _ in range(10):
        r = pipe.deseq2()
        seen.add((r.genewise_dispersions[40:44].tobytes(), r.dispersions[40:44].tobytes(), r.LFC[40:44].tobytes(),
                  r.pvalue[40:44].tobytes()))
    assert len(seen) == 1


@pytest.mark.parametrize("kind", ["two cells of 18000", "17000 + 60", "no cells, 20000 samples"])
def test_design_cells_and_rows_beyond_a_wavefronts_lds(kind):
    """The reference sorts whatever it is given (utils.py:567-650, 914-960; dds.py:1332-1352).  The robust dispersions and the
    outlier replacement used to buffer a design cell / a gene's row in a wavefront's LDS and refused cells of more than
    16 384 samples; the buffer-less kernels (k_robust_disp_lean, k_replace_lean: bucket pass or radix selection over
    recomputed values) take any size.  End to end against the oracle, with injected outliers that are replaced and
    refitted."""
    import pydeseq2_amd

    rng = np.random.default_rng(31)
    G = 40
    if kind == "two cells of 18000":
        N = 36000
        cell = np.arange(N) % 2
        X = np.column_stack([np.ones(N), cell.astype(float)])
    elif kind == "17000 + 60":
        N = 17060
        cell = (np.arange(N) >= 17000).astype(int)
        X = np.column_stack([np.ones(N), cell.astype(float)])
    else:
        N = 20000
        cell = np.arange(N) % 2
        X = np.column_stack([np.ones(N), cell.astype(float), rng.normal(0, 1, N)])
    beta0 = rng.normal(4, 1.5, G)
    lfc = rng.normal(0, 0.4, G)
    sf = np.exp(rng.normal(0, 0.2, N))
    mu = sf[:, None] * np.exp(beta0[None, :] + lfc[None, :] * cell[:, None])
    disp = 4 / np.exp(beta0) + 0.1
    size = 1 / disp
    counts = rng.negative_binomial(size[None, :], size[None, :] / (size[None, :] + mu)).astype(np.int64)
    counts[:, 3] = rng.negative_binomial(1, 0.7, N)  # mostly zeros
    counts[7, 5] = 3000000                           # outliers
    counts[N - 3, 6] = 900000
    res = pydeseq2_amd.deseq2(counts, X, device=0)
    ref = orc.deseq2(counts, X, n_jobs=_jobs(), keep_layers=False)
    if kind != "no cells, 20000 samples":  # (continuous covariate: no replaceable sample, the outliers only flag)
        assert ref.replaced.sum() >= 2 and (res.replaced == ref.replaced).all() and (res.refitted == ref.refitted).all()
    assert (res.cooks_outlier == ref.cooks_outlier).all()
    _compare(res, ref, frac_noise=0.06)


def test_replacement_through_the_buffer_less_kernel_equals_the_buffered_one(monkeypatch):
    """DSQ_REPLACE_LEAN=1 sends rows of ordinary length through k_replace_lean: the same replaced counts (the trimmed mean is
    the same sum in the same order when the bucket pass applies, and agrees to rounding otherwise), hence the same refit."""
    import subprocess
    import sys
    import tempfile

    code = ("import numpy as np, sys, pydeseq2_amd; from oracle import nbglm_oracle as orc; "
            "counts, X = orc.synth_counts(1500, 300, '2level', 17); counts[5, :60] = 400000; counts[40, 70] = 90000; "
            "r = pydeseq2_amd.deseq2(counts, X, device=0); "
            "np.savez(sys.argv[1], d=r.dispersions, l=r.LFC, p=r.pvalue, f=r.refitted, r=r.replaced)")
    outs = []
    for env in ({}, {"DSQ_REPLACE_LEAN": "1"}):
        f = tempfile.mktemp(suffix=".npz")
        subprocess.run([sys.executable, "-c", code, f], check=True, env={**os.environ, **env},
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), timeout=400)
        outs.append(dict(np.load(f)))
    a, b = outs
    assert a["f"].sum() >= 30 and (a["f"] == b["f"]).all() and (a["r"] == b["r"]).all()
    assert_close(b["d"], a["d"], 1e-9, 0, "dispersions")
    assert_close(b["l"], a["l"], 1e-9, 1e-12, "LFC")


def test_hip_inference_under_the_reference_orchestration():
    """All Inference methods of the plug-in driven in DeseqDataSet.deseq2()'s call order with the reference's
    keyword arguments (dds.py:713-984, ds.py:303-360; the orchestration is the oracle's restatement of it, since
    the stock DeseqDataSet needs anndata): same results as the oracle with its own kernels."""
    from pydeseq2_amd import HipInference

    for design, G, N, seed in (("2level", 600, 60, 21), ("3factor", 400, 60, 22)):
        counts, X = orc.synth_counts(G, N, design, seed)
        counts[:, 9] = 0
        if design == "2level":
            counts[3, 10] = 200000  # live Cook's refit: the plug-in is re-entered with a sub-dataset
        ref = orc.deseq2(counts, X, n_jobs=4)
        res = orc.deseq2(counts, X, inference=HipInference(device=0))
        _compare(res, ref)
        if design == "2level":
            assert ref.refitted.sum() >= 1 and (res.refitted == ref.refitted).all()


def test_cooks_layer_vs_oracle():
    import pydeseq2_amd

    counts, X = orc.synth_counts(300, 60, "3factor", 7)
    pipe = pydeseq2_amd.DeseqPipeline(counts, X, device=0)
    res = pipe.deseq2()
    ref = orc.deseq2(counts, X, n_jobs=4)
    assert_close(pipe.layer("cooks"), ref.cooks, 1e-6, 1e-12, "cooks")
    assert_close(pipe.layer("hat_diagonals")[:, ref.non_zero], ref.hat_diagonals, 1e-7, 1e-12, "hat")
    assert_close(pipe.layer("mu_LFC")[:, ref.non_zero], ref.mu_LFC, 1e-7, 1e-10, "mu")


def _r_case(which, factors, continuous=(), with_outliers=False):
    counts, meta = load_dataset(which)
    if with_outliers:
        counts.loc["sample1", "gene1"] = 2000
        counts.loc["sample11", "gene7"] = 1000
        meta.loc["sample1", "condition"] = "C"
    X, names = treatment_design(meta, factors, continuous)
    return counts.to_numpy(), X, names


@pytest.mark.parametrize("which,factors,cont,sub,fn,tol,outl", [
    ("synthetic", ["condition"], (), "single_factor", "r_test_res.csv", 0.02, False),
    ("synthetic", ["group", "condition"], (), "multi_factor", "r_test_res.csv", 0.04, False),
    ("synthetic", ["group", "condition"], (), "multi_factor", "r_test_res_outliers.csv", 0.04, True),
    ("continuous", ["group", "condition"], ("measurement",), "continuous", "r_test_res.csv", 0.04, False),
    ("continuous", ["group", "condition"], ("measurement",), "continuous", "r_test_res_outliers.csv", 0.04, True),
    ("wide", ["group", "condition"], (), "wide", "r_test_res.csv", 0.02, False),
])
def test_r_fixtures(which, factors, cont, sub, fn, tol, outl):
    """The reference's own known-answer tests (tests/test_pydeseq2.py:94-176, 432-560, 625-660)."""
    import pydeseq2_amd

    counts, X, names = _r_case(which, factors, cont, outl)
    ci = names.index("condition[T.B]") if not cont else len(names) - 1
    c = np.zeros(len(names))
    c[ci] = 1
    res = pydeseq2_amd.deseq2(counts, X, contrast=c, device=0)
    r_res = r_csv(sub, fn)
    assert max_rel_err(res.LFC[:, ci] / np.log(2), r_res["log2FoldChange"].to_numpy()) < tol
    p = np.where(res.cooks_outlier, np.nan, res.pvalue)
    assert max_rel_err(p, r_res["pvalue"].to_numpy()) < tol
    if sub == "single_factor":
        np.testing.assert_array_almost_equal(
            res.size_factors, r_csv(sub, "r_test_size_factors.csv")["x"].to_numpy(), decimal=6)


@pytest.mark.parametrize("alt,null", [("greater", 0.5), ("less", -0.5), ("greaterAbs", 0.5), ("lessAbs", 0.5)])
def test_r_alt_hypotheses(alt, null):
    import pydeseq2_amd

    counts, X, _ = _r_case("synthetic", ["condition"])
    res = pydeseq2_amd.deseq2(counts, X, contrast=[0, 1], lfc_null=null, alt_hypothesis=alt, device=0)
    r_res = r_csv("single_factor", f"r_test_res_{alt}.csv")
    st = np.abs(res.stat) if alt == "lessAbs" else res.stat
    r_st = r_res["stat"].to_numpy()
    nzs = r_st != 0
    assert np.max(np.abs(r_st[nzs] - st[nzs]) / np.abs(r_st[nzs])) < 0.02
    p = np.where(res.cooks_outlier, np.nan, res.pvalue)
    assert max_rel_err(p[nzs], r_res["pvalue"].to_numpy()[nzs]) < 0.02


def test_full_size_properties():
    """Config C2-like size (20k x 200): properties that do not need the (slow) oracle."""
    import pydeseq2_amd

    counts, X = orc.synth_counts(20000, 200, "2level", 0)
    res = pydeseq2_amd.deseq2(counts, X, device=0)
    nz = res.non_zero
    assert np.isfinite(res.dispersions[nz]).all() and (res.dispersions[nz] >= 1e-8).all()
    assert (res.dispersions[nz] <= 200).all()
    ok = nz & ~np.isnan(res.pvalue)
    assert ((res.pvalue[ok] >= 0) & (res.pvalue[ok] <= 1)).all()
    # Wald consistency: stat = LFC/SE and p = 2*sf(|stat|)
    from scipy.stats import norm
    z = res.LFC[ok, 1] / res.lfcSE[ok]
    assert np.allclose(z, res.stat[ok], rtol=1e-9, atol=1e-12)
    assert np.allclose(res.pvalue[ok], 2 * norm.sf(np.abs(res.stat[ok])), rtol=1e-9, atol=1e-300)
    # permutation invariance over genes: shuffling genes only permutes per-gene outputs of the
    # stages that do not depend on other genes (size factors are permutation invariant too)
    perm = np.random.default_rng(0).permutation(20000)
    res2 = pydeseq2_amd.deseq2(counts[:, perm], X, device=0)
    assert np.allclose(res2.size_factors, res.size_factors, rtol=1e-13)
    assert np.allclose(res2.genewise_dispersions, res.genewise_dispersions[perm], rtol=1e-9, equal_nan=True)
    # subset check against the oracle's per-gene kernels on 300 random genes
    sel = np.sort(np.random.default_rng(1).choice(np.nonzero(nz)[0], 300, replace=False))
    mu = orc.lin_reg_mu(counts[:, sel], res.size_factors, X, 0.5)
    a, c = orc.alpha_mle(counts[:, sel], X, mu, res.mom_dispersions[sel], 1e-8, 200.0, n_jobs=8)
    same = c == res.genewise_converged[sel].astype(bool)
    assert same.mean() > 0.99
    assert_close(res.genewise_dispersions[sel][same & c], np.clip(a, 1e-8, 200)[same & c], RTOL, 0, "gw subset")


@pytest.mark.parametrize("kind", ["2level", "mixed"])
def test_distributed_pipeline_world1_equals_single(kind):
    """RCCL path with a one-rank communicator: dlopen(librccl), comm init, all-reduce / all-gather
    on device buffers, per-pass size-factor kernels, gathered trend fit == single-GPU pipeline.  "mixed": a shard of the
    size whose LFC fit runs in two launches (the c5 shards of a multi-GPU job), forked from inside the sharded pipeline."""
    import pydeseq2_amd
    from pydeseq2_amd._lib import Context
    from pydeseq2_amd.distributed import DistDeseqPipeline, RcclComm

    if kind == "mixed":
        counts, X = _mixed_case(5, 2, 300, 2600, 3, (3,))
    else:
        counts, X = orc.synth_counts(1200, 40, "2level", 4)
    counts[:, 7] = 0
    ctx = Context(0)
    comm = RcclComm(ctx, RcclComm.unique_id(ctx), 0, 1)
    pipe_d = DistDeseqPipeline(counts, X, comm=comm, ctx=ctx)
    res_d = pipe_d.deseq2()
    assert pipe_d.lfc_forks == (1 if kind == "mixed" else 0)
    res_s = pydeseq2_amd.DeseqPipeline(counts, X, ctx=ctx).deseq2()
    assert_close(res_d.size_factors, res_s.size_factors, 1e-15, 0, "sf")
    assert_close(res_d.trend_coeffs, res_s.trend_coeffs, 1e-12, 0, "trend")
    assert abs(res_d.prior_disp_var - res_s.prior_disp_var) < 1e-12
    assert_close(res_d.dispersions, res_s.dispersions, 1e-10, 0, "disp")
    assert_close(res_d.pvalue, res_s.pvalue, 1e-9, 1e-300, "p")
    comm.close()


@pytest.mark.parametrize("sf_mode", ["ratio", "poscounts+control", "ratio-sample-shard", "iterative"])
def test_distributed_pipeline_two_ranks_threads(sf_mode):
    """Two gene shards run as two ranks (threads, one context each on the same GPU) through
    DistDeseqPipeline with a host-staged communicator: every rank must reproduce its slice of the
    single-GPU result on the whole matrix (size-factor radix protocol, NaN-padded all-gather of the
    trend inputs, trend + prior over the genes of all ranks)."""
    import threading

    import pydeseq2_amd
    from pydeseq2_amd._lib import Context
    from pydeseq2_amd.distributed import DistDeseqPipeline

    G, N, W = 1400, 40, 2
    if sf_mode == "iterative":  # the Powell search over N log size factors: keep it small
        G, N = 420, 10
    counts, X = orc.synth_counts(G, N, "2level", 11)
    counts[:, 3] = 0  # a gene without counts in rank 0's shard: its vectors are NaN padded
    cuts = [0, 600 if G > 1000 else 180, G]  # unequal shards: the gathered vectors are padded to the larger one
    kw_full, kw_rank = {}, [{}, {}]
    n_collectives = [0] * W
    if sf_mode == "iterative":
        # every gene gets a zero: the median-of-ratios factors are NaN on every rank and both the single-GPU and
        # the sharded pipeline switch to the iterative mode by themselves (dds.py:682-690)
        counts[np.arange(G) % N, np.arange(G)] = 0
    elif sf_mode == "ratio-sample-shard":  # the two-collective size-factor protocol (sample blocks of all genes)
        from pydeseq2_amd.distributed import sample_block

        kw_rank = [dict(sample_shard=counts[slice(*sample_block(r, W, N))]) for r in range(W)]
    elif sf_mode != "ratio":  # poscounts log means restricted to control genes, which live on both ranks
        counts[::3, 10:900:7] = 0
        control = np.r_[np.arange(20, 500, 3), np.arange(700, 1300, 2)]
        kw_full = dict(size_factors_fit_type="poscounts", control_genes=control)
        kw_rank = [dict(size_factors_fit_type="poscounts",
                        control_genes=control[(control >= cuts[r]) & (control < cuts[r + 1])] - cuts[r])
                   for r in range(W)]
    res_full = pydeseq2_amd.DeseqPipeline(counts, X, device=0, **kw_full).deseq2()

    barrier = threading.Barrier(W)
    slots = [None] * W

    class ThreadComm:
        def __init__(self, ctx, rank):
            self.ctx, self.rank, self.world = ctx, rank, W

        def _exchange(self, host):
            slots[self.rank] = host
            barrier.wait()
            got = list(slots)
            barrier.wait()
            return got

        def allreduce_sum(self, darr):
            n_collectives[self.rank] += 1
            n = darr.nbytes // darr.dtype.itemsize
            host = np.empty(n, dtype=darr.dtype)
            self.ctx.d2h(host, darr.ptr)
            self.ctx.h2d(darr.ptr, np.sum(self._exchange(host), axis=0).astype(darr.dtype))
            return darr

        def allgather(self, dsend, drecv):
            n_collectives[self.rank] += 1
            host = np.empty(dsend.nbytes // 8, dtype=np.float64)
            self.ctx.d2h(host, dsend.ptr)
            self.ctx.h2d(drecv.ptr, np.concatenate(self._exchange(host)))
            return drecv

    out, errs = [None] * W, []

    def run(rank):
        try:
            ctx = Context(0)
            sl = slice(cuts[rank], cuts[rank + 1])
            pipe = DistDeseqPipeline(np.ascontiguousarray(counts[:, sl]), X, comm=ThreadComm(ctx, rank), ctx=ctx,
                                     **kw_rank[rank])
            out[rank] = pipe.deseq2()
        except Exception as e:  # pragma: no cover
            errs.append(e)
            barrier.abort()

    ts = [threading.Thread(target=run, args=(r,)) for r in range(W)]
    [t.start() for t in ts]
    [t.join(600) for t in ts]
    assert not errs, errs
    # collectives per step + 1 at construction: radix protocol 1 + 8 all-reduces, sample-shard protocol 2 all-gathers;
    # trend inputs ONE all-gather in both (both per-gene vectors packed into one send buffer): 3 per step
    if sf_mode != "iterative":
        assert n_collectives[0] == (1 + 2 + 1 if sf_mode == "ratio-sample-shard" else 1 + 9 + 1), n_collectives
    for rank in range(W):
        sl = slice(cuts[rank], cuts[rank + 1])
        r = out[rank]
        assert_close(r.size_factors, res_full.size_factors, 1e-14, 0, "sf")
        assert_close(r.trend_coeffs, res_full.trend_coeffs, 1e-9, 0, "trend")
        assert abs(r.prior_disp_var - res_full.prior_disp_var) < 1e-10
        assert_close(r.dispersions, res_full.dispersions[sl], 1e-7, 0, "disp")
        assert_close(r.LFC, res_full.LFC[sl], 1e-6, 1e-10, "LFC")
        assert_close(r.pvalue, res_full.pvalue[sl], 1e-6, 1e-300, "p")


@pytest.mark.parametrize("G,N,zero_frac,count_dtype", [(3000, 7, 0.0, np.int64), (32768, 5, 0.0, np.int32),
                                                     (32769, 5, 0.0, np.int64), (50000, 6, 0.0, np.int32),
                                                     (50000, 9, 0.5, np.int64)])
def test_size_factors_register_and_key_matrix_paths(G, N, zero_frac, count_dtype):
    """Median of ratios (preprocessing.py:59-102): up to 32 768 usable genes a sample's keys stay in the registers of
    its workgroup (k_sf_row), above that the key matrix is written and read by the radix passes - both against numpy's
    medians, at the boundary, with ties (small counts) and with genes that contain zeros (left out)."""
    import pydeseq2_amd

    rng = np.random.default_rng(G + N)
    counts = rng.poisson(rng.gamma(2.0, 20.0, G)[None, :] * rng.uniform(0.5, 2.0, N)[:, None]).astype(np.int64) + 1
    zero_genes = rng.random(G) < zero_frac
    counts[rng.integers(0, N, G)[zero_genes], np.nonzero(zero_genes)[0]] = 0
    X = np.column_stack([np.ones(N), np.arange(N) % 2]).astype(np.float64)
    pipe = pydeseq2_amd.DeseqPipeline(counts.astype(count_dtype), X, device=0)
    res = pipe.deseq2(stop_after_size_factors=True)
    sf_o = orc.size_factors_ratio(counts)[0]
    assert_close(res.size_factors, sf_o, 1e-13, 0, "size factors")


@pytest.mark.parametrize("n", [5000, 40000, 300001])
def test_prior_mad_kernel_vs_numpy(n):
    """dsq_dev_prior_mad (one 1024-thread workgroup that narrows in value space, at every n - also for the
    gathered vectors of the multi-GPU layout) against numpy medians, with NaN padding and genes below
    the 100*min_disp threshold; the branches of the selection and exact ties: tests/test_gpu_medians.py."""
    import ctypes as C

    from pydeseq2_amd._lib import Context, DeviceArray

    rng = np.random.default_rng(n)
    gw = 10 ** rng.uniform(-9, 1, n)
    gw[rng.random(n) < 0.1] = np.nan           # NaN padding of ranks with fewer genes
    gw[rng.random(n) < 0.05] = 0.25            # ties
    fit = 10 ** rng.uniform(-2, 0, n)
    fit[np.isnan(gw)] = np.nan
    fit[rng.integers(0, n, 3)] = 0.0            # log residual +inf: counts at the high end of both medians
    fit[rng.integers(0, n, 2)] = np.inf         # -inf
    ctx = Context(0)
    d_gw, d_fit = DeviceArray.from_host(ctx, gw), DeviceArray.from_host(ctx, fit)
    d_work = DeviceArray(ctx, (ctx.lib.dsq_prior_mad_work_doubles(n),), np.float64)
    sq = C.c_double()
    ctx.call("dsq_dev_prior_mad", C.c_void_p(d_gw.ptr), C.c_void_p(d_fit.ptr), n, C.c_double(1e-8), C.c_double(10.0),
             C.c_void_p(d_work.ptr), C.byref(sq))
    g = np.clip(gw, 1e-8, 10.0)
    ok = ~np.isnan(gw) & (g >= 1e-6)
    with np.errstate(divide="ignore"):
        res = np.log(g[ok]) - np.log(fit[ok])
    res = res[~np.isnan(res)]
    mad = np.median(np.abs(res - np.median(res))) / 0.67448975019608171
    assert abs(sq.value - mad**2) <= 1e-12 * mad**2


def test_full_size_c3_properties():
    """The benchmark configuration itself (BASELINE.json configs[2]: 60 000 genes x 1000 samples, p = 2):
    run-to-run determinism (bit-identical results), Wald consistency, and the oracle's per-gene kernels
    (genewise MLE, MAP, IRLS LFC) on a random gene subset with the pipeline's own cross-gene quantities."""
    import pydeseq2_amd
    from scipy.stats import norm

    counts, X = orc.synth_counts(60000, 1000, "2level", 2)
    pipe = pydeseq2_amd.DeseqPipeline(counts, X, device=0)
    res = pipe.deseq2()
    res2 = pipe.deseq2()
    for f in ("size_factors", "genewise_dispersions", "MAP_dispersions", "dispersions", "LFC", "pvalue"):
        a, b = getattr(res, f), getattr(res2, f)
        assert np.array_equal(a, b, equal_nan=True), f  # idempotent and deterministic
    nz = res.non_zero
    ok = nz & ~np.isnan(res.pvalue)
    assert np.isfinite(res.dispersions[nz]).all()
    z = res.LFC[ok, 1] / res.lfcSE[ok]
    assert np.allclose(z, res.stat[ok], rtol=1e-9, atol=1e-12)
    assert np.allclose(res.pvalue[ok], 2 * norm.sf(np.abs(res.stat[ok])), rtol=1e-9, atol=1e-300)
    # ---- the cross-gene steps at the benchmark size, against the oracle on the engine's own per-gene vectors:
    # size factors over all 60 000 genes (preprocessing.py:31-102), the iterated parametric trend on the 60 000
    # genewise dispersions (dds.py:1199-1275) and the MAD prior (dds.py:840-884)
    sf_o = orc.size_factors_ratio(counts)[0]
    assert_close(res.size_factors, sf_o, 1e-12, 0, "size factors, 60 000 genes")
    # (the refit overwrites the refitted genes' genewise dispersions and means with those of the replaced counts, while
    # trend and prior were fitted before it: a second pass without the refit exposes the vectors they were fitted on)
    pipe_nr = pydeseq2_amd.DeseqPipeline(counts, X, device=0, refit_cooks=False)
    r0 = pipe_nr.deseq2()
    pipe_nr.close()
    assert np.array_equal(r0.trend_coeffs, res.trend_coeffs) and r0.prior_disp_var == res.prior_disp_var
    coeffs_o, _ = orc.fit_parametric_trend(r0.genewise_dispersions[nz], r0.normed_means[nz])
    assert_close(res.trend_coeffs, coeffs_o, 1e-9, 0, "trend coefficients, 60 000 genes")
    fitted_o = coeffs_o[0] + coeffs_o[1] / r0.normed_means[nz]
    assert_close(r0.fitted_dispersions[nz], fitted_o, 1e-9, 0, "fitted dispersions")
    sq_o, pv_o = orc.dispersion_prior(r0.genewise_dispersions[nz], r0.fitted_dispersions[nz], 1000, 2, 1e-8)
    assert abs(res.squared_logres - sq_o) <= 1e-10 * sq_o and abs(res.prior_disp_var - pv_o) <= 1e-10 * pv_o
    sel = np.sort(np.random.default_rng(3).choice(np.nonzero(nz & ~res.replaced)[0], 2000, replace=False))
    c = counts[:, sel]
    mu = orc.lin_reg_mu(c, res.size_factors, X, 0.5)
    a, cv = orc.alpha_mle(c, X, mu, res.mom_dispersions[sel], 1e-8, 1000.0, n_jobs=_jobs())
    gc = res.genewise_converged[sel] == 1
    assert (cv == gc).mean() >= 0.995
    same = cv & gc
    assert_close(res.genewise_dispersions[sel][same], np.clip(a, 1e-8, 1000.0)[same], RTOL, 0, "genewise")
    both = ~cv & ~gc  # grid search on both sides: deterministic
    assert_close(res.genewise_dispersions[sel][both], np.clip(a, 1e-8, 1000.0)[both], 1e-10, 0, "genewise grid")
    m, mc = orc.alpha_mle(c, X, mu, res.fitted_dispersions[sel], 1e-8, 1000.0, prior_disp_var=res.prior_disp_var,
                          cr_reg=True, prior_reg=True, n_jobs=_jobs())
    gm = res.MAP_converged[sel] == 1
    assert (mc == gm).mean() >= 0.995
    same = mc & gm
    assert_close(res.MAP_dispersions[sel][same], np.clip(m, 1e-8, 1000.0)[same], RTOL, 0, "MAP")
    beta, _, _, bc = orc.irls(c, res.size_factors, X, res.dispersions[sel], 0.5, 1e-8)
    assert_close(res.LFC[sel][bc], beta[bc], RTOL, 1e-8, "LFC")


def test_bench_two_ranks_strong_scaling_on_one_gpu():
    """bench.py's multi-GPU path end to end on a one-GPU box: two ranks started by its own launcher share device 0
    (DSQ_BENCH_SHARE_GPU; RCCL refuses two ranks per device, so the collectives take the host-staged transport), strong
    scaling (the named matrix split by genes, sample blocks for the two-collective size factors), one JSON line with
    the collective timings, and the in-run parity of rank 0's shard against the oracle (both measured with `--full` only)."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DSQ_BENCH_SHARE_GPU="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--config", "c2", "--genes",
                          "3000", "--steps", "2", "--warmup", "2", "--full", "--cpu-sample", "600", "--no-extras"],
                         env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["genes_total"] == 3000
    assert d["config"]["genes_per_gpu"] == 1500 and "host-staged" in d["config"]["collectives"]
    assert d["collectives_per_step"] == 3 and d["collective_ms_per_step"] > 0
    assert d["parity"]["ok"], d["parity"]


def test_bench_plain_run_measures_the_headline_figure_only(tmp_path):
    """Without `--full` bench.py times its steps and nothing else: the line carries the headline figure, the workload and the
    roofline of the dispersion launches timed inside those steps; every figure that takes a run of its own (upload time,
    profiled step, CPU baseline, parity, extras, other configurations) is null or absent, and `--no-cpu-baseline` /
    `--no-extras` change nothing.  `--dump-outputs` still writes the last timed step's arrays."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    lines = []
    for extra in ([], ["--no-cpu-baseline", "--no-extras"]):
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--config", "c2", "--genes", "3000", "--steps", "3",
               "--warmup", "1", "--dump-outputs", str(tmp_path / f"dump{len(lines)}")] + extra
        out = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        lines.append(json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]))
    for d in lines:
        assert d["full"] is False and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
        assert d["unit"] == "genes/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(3000 / (d["ms_per_step"] * 1e-3), rel=1e-3)
        assert d["roofline"]["full_launch_ms"] > 0 and d["roofline"]["full_launches_timed"] == 2 * 3
        for k in ("h2d_ms", "value_with_h2d", "cpu_baseline", "parity", "speedup_vs_cpu_baseline",
                  "stage_wall_ms_profiled_step", "collective_ms_per_step"):
            assert d[k] is None, k
        assert d["roofline"]["kernel_ms_per_step"] is None
        assert not {"summary_tail", "lfc_shrink", "plugin_path", "other_configs", "parity_c4"} & set(d)
        assert "pvalue" in d["dumped_outputs"]["arrays"]
        assert np.load(os.path.join(d["dumped_outputs"]["dir"], "pvalue.npy")).shape == (3000,)
    assert sorted(lines[0]) == sorted(lines[1])


@pytest.mark.parametrize("config,genes,per_rank,block", [("c3", 0, 15000, 250), ("c5", 6000, 1500, 1250)])
def test_bench_four_ranks_on_one_gpu(config, genes, per_rank, block):
    """The driver's multi-rank launch on a one-GPU box: four ranks of bench.py share device 0 over the host-staged
    transport - strong scaling of BASELINE configs[2] (60 000 x 1000: 15 000 genes and a block of 250 samples per rank)
    and of a slice of configs[4] (5000 samples: blocks of 1250; the tiled generator builds only the rank's blocks) -
    three collectives per step and the single-GPU step's host synchronisations.  Four ranks and this process keep the
    number of processes holding the device at five; the `--gpus 8` data plan itself is checked on the host
    (tests/test_distributed_cpu.py::test_bench_eight_rank_data_plan)."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DSQ_BENCH_SHARE_GPU="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "4", "--config", config, "--steps", "2", "--warmup", "1",
           "--no-cpu-baseline", "--no-extras"] + (["--genes", str(genes)] if genes else [])
    out = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 4 and d["scaling"] == "strong"
    assert d["config"]["genes_per_gpu"] == per_rank and d["config"]["genes_total"] == 4 * per_rank
    assert d["config"]["sample_block_rows"] == block
    assert d["collectives_per_step"] == 3, d["collectives_per_step"]
    assert d["value"] > 0 and d["ms_per_step"] > 0


# ---------------------------------------------------------------------------------------------------------------
# Mixed designs (csrc/dsq_mix.h, dsq_k_alpha_mix.hip): categorical columns + up to three continuous covariates
def _mix_launches(ctx):
    return int(ctx.lib.dsq_mix_launch_count())


@pytest.mark.parametrize("case", ["p4", "p6", "p8m"])
def test_mixed_design_dispersion_kernel_vs_reference_kats(inf, case, monkeypatch):
    """k_alpha_mix against the outputs of the unmodified utils.fit_alpha_mle (utils.py:441-564) on the KAT designs with
    continuous covariates: p = 4 (2 x 2 levels + 1 covariate), p = 6 (2 x 3 levels + 2), p = 8 (2 x 4 levels + 3, the
    benchmark's design shape).  Through the plug-in entry point, which hands mu over as a matrix (gathered into slot
    order by the kernel).  DSQ_MIX_FORCE lifts the padding limit: the KATs have 15 - 20 samples per cell."""
    monkeypatch.setenv("DSQ_MIX_FORCE", "1")
    k = load_kat(case)
    N, P = k["X"].shape
    maxd = float(max(10, N))
    before = _mix_launches(inf.ctx)
    a, c = inf.alpha_mle(k["counts"], k["X"], k["mu_hat"], k["mom"], 1e-8, maxd)
    assert _mix_launches(inf.ctx) > before, "the design did not take the mixed-design kernel"
    assert (c == k["gw_conv"]).all()
    assert_close(a, k["gw_alpha"], 1e-6, 0, "genewise alpha")
    a, c = inf.alpha_mle(k["counts"], k["X"], k["mu_hat"], k["fitted"], 1e-8, maxd,
                         prior_disp_var=float(k["prior_var"]), cr_reg=True, prior_reg=True)
    assert (c == k["map_conv"]).all()
    assert_close(a, k["map_alpha"], 1e-6, 0, "MAP alpha")
    # a gene with a count beyond the kernel's 16-bit staging stays on the general kernel, the others on this one
    counts = k["counts"].copy()
    counts[3, 1] = 70000
    mu = k["mu_hat"].copy()
    a2, c2 = inf.alpha_mle(counts, k["X"], mu, k["mom"], 1e-8, maxd)
    keep = np.arange(counts.shape[1]) != 1
    assert_close(a2[keep], k["gw_alpha"][keep], 1e-6, 0, "genewise alpha beside a 17-bit gene")
    monkeypatch.delenv("DSQ_MIX_FORCE")
    a3, c3 = inf.alpha_mle(counts, k["X"], mu, k["mom"], 1e-8, maxd)  # all genes on the general kernel
    assert c2[1] == c3[1] and abs(a2[1] - a3[1]) <= 1e-9 * abs(a3[1])


def _mixed_case(P, Q, N, G, seed, cells_levels):
    """Counts and design with `cells_levels` categorical factors (levels) + Q continuous covariates, P columns."""
    rng = np.random.default_rng(seed)
    cols = [np.ones(N)]
    for lv in cells_levels:
        v = np.arange(N) % lv
        rng.shuffle(v)
        cols += [(v == kk).astype(float) for kk in range(1, lv)]
    cols += [rng.normal(0, 1.0, N) for _ in range(Q)]
    X = np.column_stack(cols)
    assert X.shape[1] == P, X.shape
    beta = np.zeros((P, G))
    beta[0] = rng.normal(4, 2, G)
    beta[1:] = rng.normal(0, 0.3, (P - 1, G))
    disp = 4 / np.maximum(2.0 ** beta[0], 1e-3) + 0.1
    sf = np.exp(rng.normal(0, 0.2, N))
    mu = sf[:, None] * 2.0 ** (X @ beta)
    size = 1 / disp
    counts = rng.negative_binomial(size[None, :], size[None, :] / (size[None, :] + mu)).astype(np.int64)
    return counts, X


@pytest.mark.parametrize("P,Q,levels,N", [(3, 1, (2,), 300), (5, 2, (3,), 750), (8, 3, (2, 4), 1400), (4, 3, (), 260),
                                          (7, 1, (2, 5), 900), (6, 2, (4,), 640)])
def test_mixed_design_pipeline_every_shape(P, Q, levels, N, monkeypatch):
    """Every (columns, covariates) shape of the mixed-design kernels end to end: mu_hat rebuilt from the IRLS coefficients
    inside the dispersion kernel (no N x G matrix), against the same pipeline on the general kernels (HIP vs HIP, all
    genes at 1e-8 apart from success-flag flips) and against the oracle at 1e-5."""
    import pydeseq2_amd
    from pydeseq2_amd import DeseqPipeline

    G = 360
    counts, X = _mixed_case(P, Q, N, G, 100 + P * 10 + Q, levels)
    counts[:, 7] = 0
    counts[5, 11] = 66000  # one gene beyond the 16-bit staging: the matrix route of the kernel + the general kernel
    pipe = DeseqPipeline(counts, X, device=0)
    assert pipe._row_mode == 3, "not routed to the mixed-design kernels"
    before = _mix_launches(pipe.ctx)
    res = pipe.deseq2()
    assert _mix_launches(pipe.ctx) >= before + 2
    c2 = counts.copy()
    c2[5, 11] = 60000  # every gene fits: mu_hat from the coefficients
    pipe2 = DeseqPipeline(c2, X, device=0)
    res2 = pipe2.deseq2()
    monkeypatch.setenv("DSQ_NO_ALPHA_MIX", "1")
    gen = DeseqPipeline(c2, X, device=0)
    assert gen._row_mode == 0
    ref_hip = gen.deseq2()
    monkeypatch.delenv("DSQ_NO_ALPHA_MIX")
    nz = ref_hip.non_zero
    same = nz & (res2.genewise_converged == ref_hip.genewise_converged) & (res2.MAP_converged == ref_hip.MAP_converged)
    # (two kernel families with different summation orders, two fits per gene: a handful of the 360 genes end their line
    # search in rounding noise on one side only - 0-3 observed over the six shapes)
    assert (nz & ~same).sum() <= 4
    assert_close(res2.genewise_dispersions[same], ref_hip.genewise_dispersions[same], 2e-6, 0, "genewise, mix vs general")
    assert_close(res2.dispersions[same], ref_hip.dispersions[same], 2e-6, 0, "dispersions, mix vs general")
    ref = orc.deseq2(c2[:, :120], X, n_jobs=_jobs(), keep_layers=False)
    sub = pydeseq2_amd.deseq2(c2[:, :120], X, device=0)
    _compare(sub, ref, frac_noise=0.02)
    # the run with the 17-bit gene (mu_hat gathered from the matrix, that gene on the general kernel) against the general
    # kernels on the same counts
    monkeypatch.setenv("DSQ_NO_ALPHA_MIX", "1")
    ref17 = DeseqPipeline(counts, X, device=0).deseq2()
    monkeypatch.delenv("DSQ_NO_ALPHA_MIX")
    ok = nz & (res.genewise_converged == ref17.genewise_converged) & (res.MAP_converged == ref17.MAP_converged)
    assert (nz & ~ok).sum() <= 4
    assert_close(res.genewise_dispersions[ok], ref17.genewise_dispersions[ok], 2e-6, 0, "matrix route vs general")
    assert_close(res.dispersions[ok], ref17.dispersions[ok], 2e-6, 0, "matrix route vs general, final")


def test_mixed_design_counts_at_the_sixteen_bit_boundary(monkeypatch):
    """The slot-ordered uint16 copies of the mixed-design kernels keep 0xFFFF for padding and 0xFFFE for "saturated": a gene
    whose largest count is 65 534 or 65 535 must NOT be fitted from that copy (it would silently be fitted with 65 534).
    Genes with a largest count of 65 533 / 65 534 / 65 535 / 65 536 against the general kernels on the same counts (HIP vs
    HIP, 1e-8 scale) and against the oracle; a one-count error of such a sample moves the genewise dispersion by ~3e-5."""
    import pydeseq2_amd
    from pydeseq2_amd import DeseqPipeline

    P, Q, N, G = 5, 2, 420, 240
    counts, X = _mixed_case(P, Q, N, G, 977, (3,))
    edge = {20: 65533, 21: 65534, 22: 65535, 23: 65536}
    for g, v in edge.items():
        counts[:, g] = np.minimum(counts[:, g], 40000)
        counts[3 + g, g] = v
        counts[100 + g, g] = v - 7
    pipe = DeseqPipeline(counts, X, device=0)
    assert pipe._row_mode == 3
    res = pipe.deseq2()
    monkeypatch.setenv("DSQ_NO_ALPHA_MIX", "1")
    gen = DeseqPipeline(counts, X, device=0)
    assert gen._row_mode == 0
    ref_hip = gen.deseq2()
    monkeypatch.delenv("DSQ_NO_ALPHA_MIX")
    ref = orc.deseq2(counts[:, :60], X, n_jobs=_jobs(), keep_layers=False)
    sub = pydeseq2_amd.deseq2(counts[:, :60], X, device=0)
    for g in edge:
        assert res.genewise_converged[g] == ref_hip.genewise_converged[g]
        assert_close(res.genewise_dispersions[[g]], ref_hip.genewise_dispersions[[g]], 2e-7, 0, f"count {edge[g]}, mix vs general")
        assert_close(res.LFC[[g]], ref_hip.LFC[[g]], 2e-7, 1e-9, f"count {edge[g]}, LFC mix vs general")
        if sub.genewise_converged[g] == ref.genewise_converged[g]:
            assert_close(sub.genewise_dispersions[[g]], ref.genewise_dispersions[[g]], 2e-6, 0, f"count {edge[g]} vs oracle")


@pytest.mark.parametrize("design,N", [("2level", 600), ("mixed", 700), ("2factor", 1200)])
def test_robust_dispersions_without_the_lds_buffer(design, N, monkeypatch):
    """Designs whose cells all hold >= 129 samples (or that have no cells: continuous covariates) take
    k_robust_disp_lean - the trimmed sums recompute the normalised counts from the gene's row instead of buffering the
    cell in LDS.  Same values up to the contraction of a multiply-add (the recomputed value is not rounded through
    memory): the Cook's layer (which the robust dispersion scales) agrees to 1e-12 with the buffered kernel's; genes with
    heavy ties / huge counts exercise the hand-back to the buffered kernel."""
    from pydeseq2_amd import DeseqPipeline

    monkeypatch.setenv("DSQ_ROBUST_LEAN_MIN", "0")  # (the default leaves cells below 2048 samples to the buffered kernel)
    counts, X = orc.synth_counts(500, N, design, 21)
    counts[:, 3] = 0
    counts[:, 4] = 1            # one value: every boundary bucket holds all samples
    counts[::2, 5] = 7          # two values
    counts[:, 6] = np.where(np.arange(N) % 50 == 0, 10 ** 9, 3)  # huge range
    counts[7, 8] = 300000       # an outlier (refit path)
    pipe = DeseqPipeline(counts, X, device=0)
    res = pipe.deseq2()
    cooks = pipe.layer("cooks")
    monkeypatch.setenv("DSQ_NO_ROBUST_LEAN", "1")
    pipe2 = DeseqPipeline(counts, X, device=0)
    res2 = pipe2.deseq2()
    cooks2 = pipe2.layer("cooks")
    assert np.array_equal(np.isnan(cooks), np.isnan(cooks2))
    ok = ~np.isnan(cooks)
    assert_close(cooks[ok], cooks2[ok], 1e-12, 0, "Cook's distances, lean vs buffered robust dispersions")
    assert np.array_equal(res.cooks_outlier, res2.cooks_outlier) and np.array_equal(res.refitted, res2.refitted)


@pytest.mark.parametrize("case", ["p4", "p6", "p8m"])
def test_mixed_design_irls_kernel_vs_reference_kats(inf, case, monkeypatch):
    """k_irls_mix against the unmodified utils.irls_solver (utils.py:273-438) on the KAT designs with continuous
    covariates: coefficients, the unclamped mu, hat diagonals, convergence flags - for the mu_hat fit (method-of-moments
    dispersions) and for the LFC fit; then the Wald statistics of the fused epilogue through the pipeline are covered by
    test_mixed_design_pipeline_every_shape."""
    monkeypatch.setenv("DSQ_MIX_FORCE", "1")
    k = load_kat(case)
    N, P = k["X"].shape
    b, mu, H, conv = inf.irls(k["counts"], k["sf"], k["X"], k["mom"], 0.5, 1e-8)
    assert (conv == k["irls_conv"]).all()
    assert_close(b, k["irls_beta"], 1e-8, 1e-10, "irls beta")
    assert_close(mu, k["irls_mu"], 1e-8, 1e-10, "irls mu")
    assert_close(H, k["irls_H"], 1e-8, 1e-12, "irls H")
    disp = np.clip(k["map_alpha"], 1e-8, float(max(10, N)))
    b, mu, H, conv = inf.irls(k["counts"], k["sf"], k["X"], disp, 0.5, 1e-8)
    assert (conv == k["lfc_conv"]).all()
    assert_close(b, k["lfc_beta"], 1e-8, 1e-10, "lfc beta")
    assert_close(mu, k["lfc_mu"], 1e-8, 1e-10, "lfc mu")
    assert_close(H, k["lfc_H"], 1e-8, 1e-12, "lfc H")
    # a gene with a count beyond the 16-bit staging: gathered from its row inside the same kernel
    counts = k["counts"].copy()
    counts[2, 1] = 70001
    monkeypatch.delenv("DSQ_MIX_FORCE")
    b0, mu0, H0, c0 = inf.irls(counts, k["sf"], k["X"], disp, 0.5, 1e-8)   # general kernel
    monkeypatch.setenv("DSQ_MIX_FORCE", "1")
    b1, mu1, H1, c1 = inf.irls(counts, k["sf"], k["X"], disp, 0.5, 1e-8)   # mixed-design kernel
    assert (c0 == c1).all()
    assert_close(b1, b0, 1e-8, 1e-10, "beta, 17-bit gene")
    assert_close(H1, H0, 1e-8, 1e-12, "hat, 17-bit gene")


def test_mixed_design_cooks_layer_of_rescued_genes():
    """for mixed designs the Cook's layer is slot-ordered, and genes that leave the mixed IRLS kernel for the
    general rescue kernel (utils.py:374-413) get their row written in sample order.  The rescued rows must land in their own
    slot-ordered row (and nobody else's).  `irls_maxiter=5` (the `maxiter` of Inference.irls) pushes a quarter of the genes through the
    rescue on both sides: layer('cooks') of EVERY gene against the oracle."""
    import pydeseq2_amd

    G = 96
    counts, X = _mixed_case(8, 3, 1400, G, 4242, (2, 4))
    pipe = pydeseq2_amd.DeseqPipeline(counts, X, device=0, irls_maxiter=5)
    assert pipe._row_mode == 3 and pipe._cooks_ld() > 0, "not on the slot-ordered mixed-design path"
    res = pipe.deseq2()
    ref = orc.deseq2(counts, X, n_jobs=_jobs(), inference=orc._OracleInference(_jobs(), irls_maxiter=5))
    sweeps = orc.irls(counts, ref.size_factors, X, ref.dispersions, maxiter=250, return_iters=True, n_jobs=_jobs())[-1]
    rescued = sweeps >= 4  # (>= 5 sweeps: rescued, utils.py:374; one sweep of margin for the looser tolerance)
    assert (sweeps >= 5).sum() >= 10, "maxiter=5 did not push genes through the rescue: the test tests nothing"
    ck = pipe.layer("cooks")
    # rescued fits end where a loosely-toleranced L-BFGS-B stops (two implementations: 1e-6 on beta): 1e-4 on their rows;
    # a misplaced row (the bug) is off by orders of magnitude
    assert_close(ck[:, ~rescued], ref.cooks[:, ~rescued], 1e-6, 1e-12, "cooks layer, ordinary genes")
    assert_close(ck[:, rescued], ref.cooks[:, rescued], 1e-4, 1e-10, "cooks layer, rescued genes (slot-ordered layer)")
    assert_close(res.LFC, ref.LFC, 1e-4, 1e-6, "LFC incl. rescued genes")
    assert (res.cooks_outlier == ref.cooks_outlier).all()


def test_mixed_design_refit_with_rescued_genes():
    """The same with a design whose rows repeat (a dose covariate with few distinct values next to a two-level factor):
    cells of >= 7 replicates exist, so the outlier replacement READS the slot-ordered Cook's layer (dds.py:1301-1367) -
    injected outliers in rescued and ordinary genes, replaced / refitted flags and the layer against the oracle."""
    import pydeseq2_amd

    rng = np.random.default_rng(99)
    N, G = 960, 120
    grp = (np.arange(N) % 2).astype(float)
    dose = rng.permutation(np.arange(N) % 40).astype(float) / 10.0  # 40 distinct values -> "continuous" for the design analysis
    X = np.column_stack([np.ones(N), grp, dose])
    beta = np.vstack([rng.normal(5, 1, G), rng.normal(0, 0.3, G), rng.normal(0, 0.1, G)])
    sf = np.exp(rng.normal(0, 0.2, N))
    mu = sf[:, None] * 2.0 ** (X @ beta)
    size = 1 / (0.05 + 4 / mu.mean(0))
    counts = rng.negative_binomial(size[None, :], size[None, :] / (size[None, :] + mu)).astype(np.int64)
    for g in (5, 9, 50, 70):  # gross outliers: Cook's distance far beyond the cutoff
        n = int(np.nonzero(grp == 0)[0][g % 7])
        counts[n, g] = counts[:, g].max() * 400 + 10000
    pipe = pydeseq2_amd.DeseqPipeline(counts, X, device=0, irls_maxiter=4)
    if pipe._row_mode != 3 or pipe._cooks_ld() == 0:
        pytest.skip("design not taken by the mixed-design IRLS kernel")
    res = pipe.deseq2()
    ref = orc.deseq2(counts, X, n_jobs=_jobs(), inference=orc._OracleInference(_jobs(), irls_maxiter=4))
    assert ref.replaced.sum() >= 3, "the injected outliers were not replaced on the reference side"
    assert (res.replaced == ref.replaced).all()
    assert (res.refitted == ref.refitted).all()
    assert_close(pipe.layer("cooks"), ref.cooks, 1e-4, 1e-10, "cooks layer")
    assert_close(res.LFC, ref.LFC, 1e-4, 1e-6, "LFC")
    assert_close(res.dispersions, ref.dispersions, 1e-4, 0, "dispersions")
    assert (res.cooks_outlier == ref.cooks_outlier).all()


def test_plugin_cache_hits_adoption_and_invalidation():
    """The device cache behind HipInference (csrc/dsq_plugin_cache.h): a second call with a fresh host COPY of the same
    matrices uploads nothing; the mu_hat lin_reg_mu returned is recognised when it comes back into alpha_mle; a matrix
    mutated IN PLACE (same pointer, one element changed) is a different matrix - the result follows the new content; the
    results with the cache on equal those with it off, bit for bit."""
    from pydeseq2_amd import HipInference

    k = load_kat("p2")
    counts, X, sf = k["counts"].astype(np.int64), k["X"], k["sf"]
    N, G = counts.shape
    maxd = float(max(10.0, N))
    inf = HipInference(device=0)
    inf.cache_clear()
    s0 = inf.cache_stats()
    mu = inf.lin_reg_mu(counts, sf, X, 0.5)
    s1 = inf.cache_stats()
    assert s1["misses"] == s0["misses"] + 1 and s1["adopted_outputs"] == s0["adopted_outputs"] + 1
    mu_copy = np.ascontiguousarray(np.array(mu))  # what `layers["_mu_hat"][:, idx]` hands back: a fresh C-order copy
    a1, c1 = inf.alpha_mle(counts.copy(), X, mu_copy, k["mom"], 1e-8, maxd)
    s2 = inf.cache_stats()
    assert s2["misses"] == s1["misses"], "the count matrix or the returned mu_hat was uploaded again"
    assert s2["h2d_bytes"] == s1["h2d_bytes"] and s2["hits"] == s1["hits"] + 2
    assert_close(a1, k["gw_alpha"], 1e-6, 0, "genewise alpha through the cache")
    # F-order copy, int32 counts: the same matrices
    a1f, _ = inf.alpha_mle(np.asfortranarray(counts.astype(np.int32)), X, np.asfortranarray(mu_copy), k["mom"], 1e-8, maxd)
    assert inf.cache_stats()["misses"] == s2["misses"] and (a1f == a1).all()
    # in-place mutation: same buffer, one count of gene 3 changed -> that gene's fit changes, nobody else's
    y = counts.copy()
    a_y, _ = inf.alpha_mle(y, X, mu_copy, k["mom"], 1e-8, maxd)
    n_hit = int(np.argmax(y[:, 3]))
    y[n_hit, 3] = y[n_hit, 3] * 3 + 50
    s3 = inf.cache_stats()
    a_y2, _ = inf.alpha_mle(y, X, mu_copy, k["mom"], 1e-8, maxd)
    s4 = inf.cache_stats()
    assert s4["misses"] == s3["misses"] + 1, "a mutated count matrix was served from the cache"
    assert a_y2[3] != a_y[3] and (np.delete(a_y2, 3) == np.delete(a_y, 3)).all()
    # ... and one element of mu changed by one ulp
    m2 = mu_copy.copy()
    m2[5, 9] = np.nextafter(m2[5, 9], np.inf)
    inf.alpha_mle(counts, X, m2, k["mom"], 1e-8, maxd)
    assert inf.cache_stats()["misses"] == s4["misses"] + 1
    # cache off: every call uploads; identical results
    inf.cache_config(enabled=False)
    s5 = inf.cache_stats()
    b1, d1 = inf.alpha_mle(counts, X, mu_copy, k["mom"], 1e-8, maxd)
    b2, d2 = inf.alpha_mle(counts, X, mu_copy, k["mom"], 1e-8, maxd)
    s6 = inf.cache_stats()
    assert s6["misses"] == s5["misses"] + 4 and s6["hits"] == s5["hits"]
    assert (b1 == a1).all() and (b2 == a1).all() and (d1 == c1).all()
    inf.cache_config(enabled=True)
    # a budget smaller than one matrix: still correct (entries of the running call are kept until it ends)
    inf.cache_config(budget_bytes=1024)
    e1, _ = inf.alpha_mle(counts, X, mu_copy, k["mom"], 1e-8, maxd)
    assert (e1 == a1).all()
    inf.cache_config(budget_bytes=8 << 30)
    # a non-positive mu is still refused (checked on the device, once per resident matrix)
    bad = mu_copy.copy()
    bad[0, 0] = 0.0
    with pytest.raises(ValueError):
        inf.alpha_mle(counts, X, bad, k["mom"], 1e-8, maxd)
    # the cache shares its context with a device-resident pipeline (bench.py does exactly this): a pipeline run in between -
    # larger than anything the context has seen, so its grow-only workspaces are reallocated - leaves the cache intact
    import pydeseq2_amd

    s7 = inf.cache_stats()
    c_big, X_big = orc.synth_counts(5000, 40, "2level", 3)
    pydeseq2_amd.DeseqPipeline(c_big, X_big, ctx=inf.ctx).deseq2()
    a_again, _ = inf.alpha_mle(counts, X, mu_copy, k["mom"], 1e-8, maxd)
    s8 = inf.cache_stats()
    assert (a_again == a1).all() and s8["hits"] == s7["hits"] + 2 and s8["misses"] == s7["misses"]
    # all-zero genes are dropped by fit_moments_dispersions as utils.py:878 does
    normed = counts / sf[:, None]
    normed[:, 4] = 0.0
    mde = inf.fit_moments_dispersions(normed, sf)
    assert len(mde) == G - 1
    assert_close(mde, orc.moments_dispersions(normed, sf), 1e-10, 1e-14, "moments with a zero gene")


def test_plugin_cache_verify_mode_and_hits_of_a_whole_fit(monkeypatch):
    """DSQ_PLUGIN_CACHE_VERIFY: every cache hit is re-uploaded and compared with the resident device copy word for word (a
    digest collision would fail the call) - through one whole deseq2() + Wald under the reference's orchestration, with
    the hit / miss / verified counters of that fit checked: the count matrix is uploaded once, the two mu matrices the
    engine produced are recognised when they come back, and the results equal those of a run without the mode."""
    from pydeseq2_amd import HipInference
    from pydeseq2_amd._lib import Context

    counts, X = orc.synth_counts(600, 80, "2level", 17)
    plain = orc.deseq2(counts, X, n_jobs=1, keep_layers=False, inference=HipInference(device=0))
    monkeypatch.setenv("DSQ_PLUGIN_CACHE_VERIFY", "1")
    inf = HipInference(ctx=Context(0))  # (a context of its own: the mode is read when the context's cache is created)
    s0 = inf.cache_stats()
    res = orc.deseq2(counts, X, n_jobs=1, keep_layers=False, inference=inf)
    s1 = inf.cache_stats()
    assert s1["verified_hits"] > 0 and s1["verified_hits"] == s1["hits"] - s0["hits"]
    # misses: the normed counts (fp64), the counts (int64) and the sub-matrices of the outlier refit - the two N x G
    # matrices the engine produced (mu_hat, mu) come back as hits of their adopted device copies
    assert s1["misses"] - s0["misses"] <= 8 and s1["adopted_outputs"] - s0["adopted_outputs"] >= 2
    for f in ("dispersions", "LFC", "pvalue", "genewise_dispersions"):
        np.testing.assert_array_equal(getattr(res, f), getattr(plain, f), err_msg=f)
