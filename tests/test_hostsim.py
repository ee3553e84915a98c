"""The per-gene device templates (pydeseq2_amd/csrc/dsq_*.h), instantiated on the host
(tests/hostsim), against the reference's own kernels (golden KATs) and against scipy."""
import os

import warnings

import numpy as np
import pytest
from scipy.optimize import minimize
from scipy.special import digamma, gammaln
from scipy.stats import f as f_dist
from scipy.stats import norm

from oracle import nbglm_oracle as orc
from tests import hostsim as hs
from tests import stats_cases as sc
from tests.helpers import assert_close, check_hard_dispersion_genes, check_hard_lfc_genes, load_kat

CASES = ["p1", "p2", "p3", "p4", "p5", "p6", "p7", "p8", "p8m", "p9", "p10", "p11", "p12"]


def test_special_functions():
    x = np.concatenate([10 ** np.random.default_rng(0).uniform(-6, 9, 4000), np.arange(1, 60) * 0.5,
                        [1e-8, 1.0, 2.0, 9.999999, 10.0, 1e8 + 3]])
    lg, dg = hs.lgamma_digamma(x)
    ref = gammaln(x)
    assert np.max(np.abs(lg - ref) / np.maximum(np.abs(ref), 1.0)) < 1e-14
    rd = digamma(x)
    assert np.max(np.abs(dg - rd) / np.maximum(np.abs(rd), 1.0)) < 4e-15
    z = np.linspace(-8, 37.6, 2001)
    assert np.max(np.abs(hs.norm_sf(z) - norm.sf(z)) / norm.sf(z)) < 1e-13
    assert (hs.norm_sf(np.array([37.7, 38.0, 50.0])) == 0).all() and (norm.sf([37.7, 38.0, 50.0]) == 0).all()


def test_lbfgsb1d_matches_scipy():
    rng = np.random.default_rng(7)
    bad = 0
    for t in range(400):
        c, a, b, k = rng.normal(0, 3), 10 ** rng.uniform(-2, 3), 10 ** rng.uniform(-3, 2), rng.uniform(-2, 2)

        def fg(x):
            return a * (x - c) ** 2 + b * np.exp(k * (x - c)), 2 * a * (x - c) + b * k * np.exp(k * (x - c))

        lo = c + rng.normal(0, 4) - abs(rng.normal(0, 3))
        hi = lo + 10 ** rng.uniform(-1, 1.3)
        x0 = rng.uniform(lo - 1, hi + 1)
        res = minimize(lambda x: fg(x[0])[0], [x0], jac=lambda x: np.array([fg(x[0])[1]]), method="L-BFGS-B",
                       bounds=[(lo, hi)])
        x, f, ok, nfev, nit, st = hs.lbfgsb1d(fg, x0, lo, hi)
        if ok != res.success or abs(x - res.x[0]) > 1e-9 * max(1, abs(x)) or nfev != res.nfev:
            bad += 1
    assert bad <= 1  # searches that are pure rounding noise may differ in evaluation count


@pytest.mark.parametrize("case", CASES)
def test_sizefactor_mom_linmu(case):
    k = load_kat(case)
    N = k["counts"].shape[0]
    lm, nz = hs.logmeans(k["counts"])
    assert_close(lm, k["logmeans"], 1e-14, 0, "logmeans")
    assert nz.all()
    m = hs.mom(k["counts"], k["sf"], k["X"], 1e-8, max(10, N))
    assert_close(m["rough"], k["rough"], 1e-9, 1e-13, "rough")
    assert_close(m["moments"], k["moments"], 1e-11, 1e-14, "moments")
    assert_close(m["mom"], k["mom"], 1e-9, 0, "mom")
    assert_close(m["normed_mean"], k["normed"].mean(0), 1e-13, 0, "normed mean")
    lin = hs.lin_mu(k["counts"], k["sf"], k["X"], 0.5)
    assert_close(lin, k["lin_mu"], 1e-10, 0, "lin mu")
    # the fused MoM + linear mu_hat template does the same arithmetic in the same order
    f = hs.mom_lin_mu(k["counts"], k["sf"], k["X"], 1e-8, max(10, N), 0.5)
    assert np.array_equal(f["mom"], m["mom"]) and np.array_equal(f["normed_mean"], m["normed_mean"])
    assert np.array_equal(f["mu"], lin)


@pytest.mark.parametrize("case", CASES)
def test_alpha_mle(case):
    k = load_kat(case)
    N = k["counts"].shape[0]
    a, c, nfev = hs.alpha_mle(k["counts"], k["X"], k["mu_hat"], k["mom"], 1e-8, max(10, N))
    assert (c == k["gw_conv"]).all()
    # L-BFGS-B stops on scipy's loose defaults (ftol 2.2e-9): the last bits of the loss (logarithms, summation
    # order) move the stopping point by up to a few 1e-7 relative on individual genes (wide designs, whose
    # p x p log-det / trace terms carry more rounding: 2e-6) - an order of magnitude inside the 1e-5 parity bar;
    # the same 1e-6 as the GPU run of these vectors
    tol = 1e-6 if k["X"].shape[1] <= 8 else 2e-6
    assert_close(a, k["gw_alpha"], tol, 0, "genewise alpha")
    a, c, _ = hs.alpha_mle(k["counts"], k["X"], k["mu_hat"], k["fitted"], 1e-8, max(10, N),
                           prior_var=float(k["prior_var"]), cr_reg=True, prior_reg=True)
    assert (c == k["map_conv"]).all()
    assert_close(a, k["map_alpha"], tol, 0, "MAP alpha")
    ng = len(k["grid_alpha"])
    la = hs.grid_alpha(k["counts"][:, :ng], k["X"], k["mu_hat"][:, :ng], 1e-8, max(10, N))
    assert np.abs(la - k["grid_alpha"]).max() < 1e-12


@pytest.mark.parametrize("case", CASES)
def test_irls(case):
    k = load_kat(case)
    b, mu, H, conv, it, fb = hs.irls(k["counts"], k["sf"], k["X"], k["mom"])
    assert not fb[k["irls_conv"]].any()  # wide cases hold a few low-count genes that go through the rescue
    assert (conv == k["irls_conv"]).all()
    assert_close(b, k["irls_beta"], 1e-8, 1e-10, "beta")
    assert_close(mu, k["irls_mu"], 1e-8, 1e-10, "mu")
    assert_close(H, k["irls_H"], 1e-8, 1e-12, "H")
    N = k["counts"].shape[0]
    disp = np.clip(k["map_alpha"], 1e-8, max(10, N))
    b, mu, H, conv, it, fb = hs.irls(k["counts"], k["sf"], k["X"], disp)
    assert_close(b, k["lfc_beta"], 1e-8, 1e-10, "lfc beta")
    assert_close(H, k["lfc_H"], 1e-8, 1e-12, "lfc H")
    # same iteration counts as the reference algorithm (oracle restatement)
    _, _, _, _, it_o = orc.irls(k["counts"], k["sf"], k["X"], disp, return_iters=True)
    assert (it == it_o)[~fb.astype(bool)].all()
    assert (conv == k["lfc_conv"]).all()


def test_grid_fallbacks_on_genes_where_the_reference_takes_them():
    """Host instantiation of the device templates on kat_hard.npz (same assertions as the GPU test)."""
    k = load_kat("hard")
    a, c, _ = hs.alpha_mle(k["a_counts"], k["X"], k["a_mu_hat"], k["a_mom"], 1e-8, 40.0)
    la = hs.grid_alpha(k["a_counts"], k["X"], k["a_mu_hat"], 1e-8, 40.0)
    check_hard_dispersion_genes(k, a, c, la)
    b, mu, H, conv, it, fb = hs.irls(k["b_counts"], k["sf"], k["X"], k["b_disp"])
    assert fb.all()
    check_hard_lfc_genes(k, b, mu, H, conv)


@pytest.mark.parametrize("case", CASES)
def test_wald(case):
    k = load_kat(case)
    N, P = k["X"].shape
    disp = np.clip(k["map_alpha"], 1e-8, max(10, N))
    ridge = np.diag(np.repeat(1e-6, P))
    mu_w = np.exp(k["X"] @ k["lfc_beta"].T) * k["sf"][:, None]
    for alt, null in ((None, 0.0), ("greater", 0.5), ("less", -0.5), ("greaterAbs", 0.5), ("lessAbs", 0.5)):
        tag = alt or "none"
        for mu in (None, mu_w):
            p, s, se = hs.wald(k["X"], disp, k["lfc_beta"], k["sf"], ridge, k["contrast"], np.log(2) * null, alt, mu)
            assert_close(se, k[f"wald_se_{tag}"], 1e-10, 0, f"se {tag}")
            assert_close(s, k[f"wald_stat_{tag}"], 1e-9, 1e-13, f"stat {tag}")
            assert_close(p, k[f"wald_p_{tag}"], 1e-8, 1e-300, f"p {tag}")


@pytest.mark.parametrize("case", CASES)
def test_cooks(case):
    k = load_kat(case)
    N, P = k["X"].shape
    cutoff = f_dist.ppf(0.99, P, N - P)
    ck, rd, (g_all, g_use, g_use_nr, few) = hs.cooks(k["counts"], k["sf"], k["X"], k["lfc_mu"], k["lfc_H"], cutoff)
    assert_close(rd, k["robust_disp"], 1e-11, 0, "robust disp")
    ref = orc.cooks_distance(k["counts"], k["normed"], k["X"], k["lfc_mu"], k["lfc_H"])
    assert_close(ck, ref, 1e-10, 1e-300, "cooks")
    assert (g_all == (ref > cutoff).any(0)).all()
    cid, cnt = orc.design_cells(k["X"])
    use = cnt[cid] >= 3
    assert (g_use == (ref[use] > cutoff).any(0)).all()
    pos = ref.argmax(0)
    few_ref = (k["counts"] > k["counts"][pos, np.arange(ck.shape[1])]).sum(0) < 3
    assert (few == few_ref).all()
    assert_close(hs.trimmed_base_mean(k["counts"], k["sf"], 0.2), k["trim_mean_02"], 1e-13, 0, "tbm")


def test_lbfgsb_nd_matches_scipy():
    """The n-dimensional L-BFGS-B restatement against scipy on random bounded problems
    (smooth and kinked objectives).  Iterates agree to rounding; evaluation counts may differ by
    a few in line searches that are resolved at rounding level (BLAS summation order)."""
    rng = np.random.default_rng(3)
    bad = 0
    for t in range(120):
        n = int(rng.integers(1, 9))
        A = rng.normal(size=(n + 3, n))
        Q = A.T @ A * 10 ** rng.uniform(-1, 2) + np.eye(n) * 10 ** rng.uniform(-3, 0)
        c, b, w = rng.normal(0, 3, n), rng.normal(0, 2, n), rng.uniform(0.2, 2, n)
        kinked = t % 2 == 1

        def fg(x):
            d = x - c
            e = np.exp(np.clip(w * d, -50, 50))
            if kinked:
                ge = np.where(e > 0.5, w * e, 0.0)
                e = np.maximum(e, 0.5)
                return 0.05 * d @ Q @ d + e.sum() - (b * d).sum(), 0.1 * Q @ d + ge - b
            return 0.5 * d @ Q @ d + e.sum(), Q @ d + w * e

        bounds = [(-30, 30)] * n if t % 3 else [(ci - abs(rng.normal(0, 2)), None) for ci in c]
        x0 = c + rng.normal(0, 3, n)
        res = minimize(lambda x: fg(x)[0], x0, jac=lambda x: fg(x)[1], method="L-BFGS-B", bounds=bounds)
        x, f, ok, nfev, nit, st = hs.lbfgsb_nd(fg, x0, bounds)
        if ok != res.success or nit != res.nit or np.max(np.abs(x - res.x)) > 1e-8 * max(1, np.max(np.abs(res.x))):
            bad += 1
    assert bad <= 1


def test_lbfgsb_nd_matches_scipy_above_16_variables():
    """The compact form on LbfgsbWork<48> - the workspace of the 33 ... 48-coefficient shrinkage kernel, whose 64-lane
    build tests/test_devunit_optim.py holds to this one-lane build bit for bit - against scipy on the unbounded, boxed
    and half-bounded problems of tests/optim_cases.py with more than 16 variables: same flag, same number of
    iterations, the same point."""
    from tests import optim_cases as oc

    cases = [e for e in oc.LANES_PROBLEMS if e[2] > 16]
    assert {e[2] for e in cases} == {33, 40, 48} and {e[4] for e in cases} == {"none", "box", "half"}
    for entry in cases:
        q = oc.lanes_problem(entry)
        fg = oc.objective(q)
        bounds = q["bounds"] or [(None, None)] * q["n"]
        res = minimize(lambda x: fg(x)[0], q["x0"], jac=lambda x: fg(x)[1], method="L-BFGS-B", bounds=bounds)
        x, f, ok, nfev, nit, st = hs.lbfgsb_nd48(fg, q["x0"], bounds)
        assert ok == res.success and nit == res.nit, (entry, ok, nit, res.success, res.nit)
        assert np.max(np.abs(x - res.x)) <= 1e-7 * max(1, np.max(np.abs(res.x))), entry


def test_bfgs_matches_scipy():
    """The restatement of scipy's BFGS (line_search_wolfe1 = MINPACK-2 dcsrch, line_search_wolfe2 / zoom as the
    fall-back, dense inverse-Hessian update; dsq_bfgs.h) against scipy itself on random smooth and kinked problems,
    incl. ones whose line search fails ("precision loss")."""
    rng = np.random.default_rng(5)
    bad, failures = 0, 0
    for t in range(160):
        n = int(rng.integers(1, 9))
        A = rng.normal(size=(n + 3, n))
        Q = A.T @ A * 10 ** rng.uniform(-1, 2) + np.eye(n) * 10 ** rng.uniform(-3, 0)
        c, b, w = rng.normal(0, 3, n), rng.normal(0, 2, n), rng.uniform(0.2, 2, n)
        kinked = t % 4 == 3

        def fg(x):
            d = x - c
            e = np.exp(np.clip(w * d, -50, 50))
            if kinked:
                ge = np.where(e > 0.5, w * e, 0.0)
                e = np.maximum(e, 0.5)
                return 0.05 * d @ Q @ d + e.sum() - (b * d).sum(), 0.1 * Q @ d + ge - b
            return 0.5 * d @ Q @ d + e.sum(), Q @ d + w * e

        x0 = c + rng.normal(0, 3, n)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = minimize(lambda x: fg(x)[0], x0, jac=lambda x: fg(x)[1], method="BFGS")
        x, ok, nfev, nit, st = hs.bfgs(fg, x0)
        failures += not res.success
        if ok != res.success or nit != res.nit or st != res.status or \
                np.max(np.abs(x - res.x)) > 1e-8 * max(1, np.max(np.abs(res.x))):
            bad += 1
    assert failures >= 3  # the fall-back search and the failure exit are exercised
    assert bad <= 2


def test_bfgs_option_matches_the_reference():
    """optimizer="BFGS" of the dispersion fit and of the IRLS rescue (host instantiation of dsq_bfgs.h inside the
    per-gene templates) against the unmodified reference (kat_bfgs.npz)."""
    from tests.helpers import check_bfgs_kats

    check_bfgs_kats(
        load_kat,
        lambda y, X, mu, ah, lo, hi, pv, cr, pr: hs.alpha_mle(y, X, mu, ah, lo, hi, pv, cr, pr, optimizer="BFGS")[:2],
        lambda y, sf, X, d: (lambda r: (r[0], r[3]))(hs.irls(y, sf, X, d, optimizer="BFGS")))


def test_irls_rescue_matches_reference_fallback():
    """Low-count genes on a 30-cell design: IRLS diverges and the reference falls back to scipy's
    p-dimensional L-BFGS-B (utils.py:374-403), keeping whatever iterate it stops at."""
    counts, X = orc.synth_counts(1500, 60, "3factor", 2)
    sf, normed, _, _ = orc.size_factors_ratio(counts)
    nz = ~(counts == 0).all(0)
    c, nrm = counts[:, nz], normed[:, nz]
    mom = orc.mom_dispersions(nrm, X, sf, 1e-8, 60)
    b_h, mu_h, H_h, conv_h, it_h, fb_h = hs.irls(c, sf, X, mom)
    assert fb_h.sum() >= 2
    sel = np.nonzero(fb_h)[0]
    b_o, mu_o, H_o, conv_o = orc.irls(c[:, sel], sf, X, mom[sel])
    assert (conv_o == conv_h[sel]).all()
    assert_close(b_h[sel], b_o, 1e-7, 1e-9, "fallback beta")
    assert_close(H_h[:, sel], H_o, 1e-6, 1e-12, "fallback H")


def test_trend_fit_matches_reference_loop():
    """Device trend-fit template (n-dim L-BFGS-B, n = 2) vs the oracle's restatement of
    dds.py:1199-1275 / default_inference.py:200-230 (scipy L-BFGS-B on numpy sums)."""
    for G, N, design, seed in [(3000, 60, "2level", 1), (2500, 60, "3factor", 2)]:
        counts, X = orc.synth_counts(G, N, design, seed)
        sf, normed, _, _ = orc.size_factors_ratio(counts)
        nz = ~(counts == 0).all(0)
        c, nrm = counts[:, nz], normed[:, nz]
        mom = orc.mom_dispersions(nrm, X, sf, 1e-8, N)
        mu = orc.lin_reg_mu(c, sf, X, 0.5) if design == "2level" else orc.irls(c, sf, X, mom)[1]
        gw, _, _ = hs.alpha_mle(c, X, mu, mom, 1e-8, N)
        nm = nrm.mean(0)
        co, n_outer = orc.fit_parametric_trend(np.clip(gw, 1e-8, N), nm)
        ch, ok, no = hs.trend_fit(gw, nm, 1e-8, N)
        assert ok and no == n_outer
        assert_close(ch, co, 1e-10, 0, "trend coefficients")


def test_lean_log_matches_libm():
    x = np.concatenate([10 ** np.random.default_rng(1).uniform(-12, 80, 50000), np.linspace(0.5, 2, 20001)])
    lg, _, rc = hs.flog(x)
    assert np.max(np.abs(lg - np.log(x)) / np.spacing(np.abs(np.log(x)) + 1e-300)) <= 1.0
    u = np.concatenate([10 ** np.random.default_rng(2).uniform(-20, 6, 50000), [0.0, 4.9e-9, 5e-9]])
    _, l1, _ = hs.flog(u)
    assert np.max(np.abs(l1 - np.log1p(u)) / (np.spacing(np.log1p(u)) + 1e-320)) <= 1.0


def test_table_exponential_matches_libm():
    """fexp_t (dsq_math.h): the exponential of the mixed-design kernels' per-sample loops, <= 1 ulp against the C
    library over the whole range, exact limits, gradual underflow, NaN."""
    import math

    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-745, 709.7, 200000), rng.normal(0, 3, 200000), rng.uniform(-1e-3, 1e-3, 20000),
                        np.arange(-100, 100) * (math.log(2) / 128), [0.0, -0.0, 1.0, -1.0, 709.78, -708.4, -744.0]])
    e = hs.fexp(x)
    ref = np.exp(x)
    ulp = np.spacing(ref)
    assert np.max(np.abs(e - ref) / ulp) <= 1.0, np.max(np.abs(e - ref) / ulp)
    assert hs.fexp([0.0])[0] == 1.0
    with np.errstate(over="ignore"):
        assert np.isinf(hs.fexp([710.0, 1e300, np.inf])).all()
    assert (hs.fexp([-746.0, -1e300, -np.inf]) == 0.0).all()
    assert np.isnan(hs.fexp([np.nan])[0])


def test_lbfgsb_dense_matches_scipy():
    """Dense-matrix L-BFGS-B (n <= 4) used by the trend fit: same iterates as scipy."""
    rng = np.random.default_rng(8)
    for t in range(150):
        n = int(rng.integers(1, 5))
        A = rng.normal(size=(n + 3, n))
        Q = A.T @ A * 10 ** rng.uniform(-1, 2) + np.eye(n) * 10 ** rng.uniform(-3, 0)
        c, w = rng.normal(0, 3, n), rng.uniform(0.2, 2, n)

        def fg(x):
            d = x - c
            e = np.exp(np.clip(w * d, -50, 50))
            return 0.5 * d @ Q @ d + e.sum(), Q @ d + w * e

        bounds = [(-30, 30)] * n if t % 2 else [(ci - abs(rng.normal(0, 2)), None) for ci in c]
        x0 = c + rng.normal(0, 3, n)
        res = minimize(lambda x: fg(x)[0], x0, jac=lambda x: fg(x)[1], method="L-BFGS-B", bounds=bounds)
        x, f, ok, nfev, nit, st = hs.lbfgsb_dense(fg, x0, bounds)
        assert ok == res.success and nit == res.nit
        assert np.max(np.abs(x - res.x)) <= 1e-7 * max(1, np.max(np.abs(res.x)))


def test_trimmed_sum_by_selection_matches_sort():
    """Radix-select trimmed sums (Cook's robust variance) == sum of the sorted slice, incl. heavy ties,
    negative values, tiny ranges that share all leading bytes, and every trim count."""
    rng = np.random.default_rng(12)
    cases = []
    for n in (1, 2, 3, 7, 24, 100, 500, 1000):
        cases.append(sc.heavy_ties(rng, n))
        cases.append(sc.mixed_signs(rng, n))
        cases.append(sc.shared_leading_bytes(rng, n))
        cases.append(sc.all_equal(n))
        cases.append(sc.nb_over_size_factors(rng, n))
    for v in cases:
        n = len(v)
        for nt in sorted({0, n // 8, n // 4, n // 3, (n - 1) // 2}):
            if n - 2 * nt < 1:
                continue
            ref = np.sort(v)[nt:n - nt].sum()
            got = hs.trimmed_sum(v, nt)
            assert abs(got - ref) <= 1e-12 * max(1.0, np.abs(v).sum()), (n, nt, got, ref)


def test_results_do_not_depend_on_what_the_workspaces_held():
    """The optimisers' workspaces are wave-private LDS on the device - whatever the previous workgroup left there.  Every
    routine that takes one must give the same bits on a workspace of zeros, of 0xFF (NaNs) and of 0x5A: the IRLS rescue
    (bounded L-BFGS-B), its BFGS variant, the wide rescue, the three shrinkage optimisers (narrow, dense and wide work
    structs), the trend fit.  (The entry points here used to zero the workspaces themselves - the device did not, and one
    rescued gene's iterates varied from launch to launch with the LDS contents until lbfgsb_nd zeroed its workspace as scipy
    does.  That case needs the device's arithmetic: 9 400 random rescues on the host instantiation built with
    -DDSQ_LBFGSB_NO_ZERO read no unwritten entry, so the test with detection power for it is the GPU one,
    test_rescued_gene_is_reproducible_from_pass_to_pass; this one guards every host-visible dependence.)"""
    k = load_kat("hard")    # genes whose IRLS diverges: all of them take the rescue
    kw = load_kat("p16")    # the LDS / matrix-core templates
    k4, k8 = load_kat("p4"), load_kat("p8")

    def run_all():
        out = []
        b, mu, H, conv, it, fb = hs.irls(k["b_counts"], k["sf"], k["X"], k["b_disp"])
        assert fb.all()
        out += [b, mu, conv, it]
        b2 = hs.irls(k["b_counts"], k["sf"], k["X"], k["b_disp"], optimizer="BFGS")
        out += [b2[0], b2[3]]
        # the same hard genes padded to a wide design (columns of noise): the wide kernels' rescue
        rng = np.random.default_rng(3)
        Xw = np.column_stack([k["X"]] + [rng.normal(0, 0.1, k["X"].shape[0]) for _ in range(14 - k["X"].shape[1])])
        res = hs.lfc_fit(k["b_counts"], k["sf"], Xw, k["b_disp"], entry="hs_lfc_fit_wide")
        out += [res["beta"], res["conv"]]
        res = hs.lfc_fit(kw["counts"], kw["sf"], kw["X"], kw["map_alpha"], entry="hs_lfc_fit_wide")
        out += [res["beta"], res["conv"]]
        sh = hs.shrink(kw["counts"], kw["X"], 1.0 / kw["map_alpha"], np.log(kw["sf"]), 15.0, 0.3, 1)
        out += [sh[0], sh[2]]
        for opt in ("L-BFGS-B", "BFGS", "Newton-CG"):
            sh = hs.shrink(k4["counts"], k4["X"], 1.0 / k4["map_alpha"], np.log(k4["sf"]), 15.0, 0.3, 1, optimizer=opt)
            out += [sh[0], sh[1], sh[2]]
        sh = hs.shrink(k8["counts"], k8["X"], 1.0 / k8["map_alpha"], np.log(k8["sf"]), 15.0, 0.3, 2)
        out += [sh[0], sh[2]]
        out += [np.asarray(hs.trend_fit(k8["gw_alpha"], k8["normed"].mean(0), 1e-8, 10.0)[0], float)]
        return out

    try:
        hs.set_workspace_fill(0x00)
        ref = run_all()
        for fill in (0xFF, 0x5A):
            hs.set_workspace_fill(fill)
            got = run_all()
            for i, (a, b) in enumerate(zip(ref, got)):
                a, b = np.asarray(a), np.asarray(b)
                assert a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (hex(fill), i)
    finally:
        hs.set_workspace_fill(0x00)


def test_rank_sums_by_selection_over_an_accessor():
    """select_rank_sum (the buffer-less fallback of the bucket pass: cells of any size): sum of the ranks j_lo .. j_hi among
    the active (>= 0) entries == the sorted slice, with inactive markers (zero counts) scattered in, heavy ties, ranges that
    share their leading bytes, single ranks and empty ranges."""
    rng = np.random.default_rng(21)
    for n in (1, 2, 5, 64, 129, 1000, 20000):
        for kind in range(4):
            if kind == 0:
                v = sc.heavy_ties(rng, n, 1, 7)
            elif kind == 1:
                v = sc.nb_over_size_factors(rng, n, 1e-3)
            elif kind == 2:
                v = sc.shared_leading_bytes(rng, n)
            else:
                v = sc.all_equal(n)
            v = sc.with_inactive(rng, v)
            act = np.sort(v[v >= 0])
            m = len(act)
            for (a, b) in {(0, m - 1), (m // 8, m - m // 8 - 1), (m // 3, m // 3), (m // 2, m // 2 - 1), (0, 0)}:
                if m == 0 or a < 0 or b >= m:
                    continue
                ref = act[a:b + 1].sum() if b >= a else 0.0
                got = hs.select_rank_sum(v, a, b)
                assert abs(got - ref) <= 1e-12 * max(1.0, act.sum()), (n, kind, a, b, got, ref)


def test_buffer_less_robust_dispersions_and_trimmed_means():
    """robust_disp_gene_lean / trimmed_base_mean_lean (kernels of cells and rows beyond a wavefront's LDS) against the
    reference's utils.robust_method_of_moments_disp / trimmed_mean restated in the oracle: small cells (selection), cells at
    the bucket threshold, cells of 9000 samples whose boundary buckets overflow (selection again), unbalanced designs,
    rows with many zeros."""
    rng = np.random.default_rng(8)
    for N, levels, G in ((60, 3, 12), (300, 2, 10), (1290, 10, 8), (18000, 2, 6), (4000, 1, 6)):
        cell = np.arange(N) % levels
        if levels == 2 and N == 300:
            cell = (np.arange(N) < 40).astype(int)  # 40 / 260
        X = np.column_stack([np.ones(N)] + [(cell == k).astype(float) for k in range(1, levels)])
        if levels == 1:
            X = np.column_stack([np.ones(N), rng.normal(0, 1, N)])  # no cells: one trimmed variance over every sample
        sf = np.exp(rng.normal(0, 0.3, N))
        mu = np.exp(rng.normal(3, 2, G))
        counts = rng.negative_binomial(3, 3 / (3 + mu[None, :] * sf[:, None])).astype(np.int64)
        counts[:, 0] = rng.negative_binomial(1, 0.6, N)  # mostly zeros
        counts[5, 1] = 500000
        rd, failed = hs.robust_disp_lean(counts, sf, X)
        assert not failed.any()
        normed = counts / sf[:, None]
        ref = orc.robust_mom_disp(normed, X)
        assert_close(rd, ref, 1e-10, 0, f"robust disp N={N}")
        tbm = hs.trimmed_base_mean_lean(counts, sf, 0.2)
        assert_close(tbm, orc.trimmed_mean(normed, 0.2), 1e-12, 0, f"trimmed mean N={N}")


@pytest.mark.parametrize("case", ["p2", "p4", "p8"])
def test_apeglm_shrinkage_templates_match_reference(case):
    """shrink_gene (unbounded n-dim L-BFGS-B with ftol = gtol = 1e-8, apeGLM objective, the reference's
    Hessian incl. its broadcasting quirk) against outputs of the unmodified utils.nbinomGLM."""
    k = np.load(os.path.join(os.path.dirname(__file__), "golden", "kat_shrink.npz"))
    kk = load_kat(case)
    G, sidx = int(k[f"{case}_G"]), int(k[f"{case}_sidx"])
    for tag in "ab":
        b, ih, cv = hs.shrink(kk["counts"][:, :G], kk["X"], k[f"{case}_size"], np.log(kk["sf"]), 15.0,
                              float(k[f"{case}{tag}_scale"]), sidx)
        assert (cv == k[f"{case}{tag}_conv"]).all()
        np.testing.assert_allclose(b, k[f"{case}{tag}_beta"], rtol=1e-6, atol=1e-9)
        scale = np.abs(k[f"{case}{tag}_invh"]).max(axis=(1, 2), keepdims=True)
        assert np.max(np.abs(ih - k[f"{case}{tag}_invh"]) / scale) < 1e-8


@pytest.mark.parametrize("case", ["p5", "p6", "p7", "p9", "p10", "p11", "p12"])
def test_apeglm_shrinkage_templates_match_reference_at_the_widths_between(case):
    """The same at the design widths between the three above (kat_shrink_mid.npz): the host instantiation runs scipy's
    compact-form L-BFGS-B at these widths; the device runs the wavefront-resident inverse form (dsq_lbfgsb_wave.h), which
    tests/test_gpu_summary.py holds to the same file."""
    k = np.load(os.path.join(os.path.dirname(__file__), "golden", "kat_shrink_mid.npz"))
    kk = load_kat(case)
    G, sidx = int(k[f"{case}_G"]), int(k[f"{case}_sidx"])
    for tag in "ab":
        b, ih, cv = hs.shrink(kk["counts"][:, :G], kk["X"], k[f"{case}_size"], np.log(kk["sf"]), 15.0,
                              float(k[f"{case}{tag}_scale"]), sidx)
        assert (cv == k[f"{case}{tag}_conv"]).all()
        np.testing.assert_allclose(b, k[f"{case}{tag}_beta"], rtol=1e-6, atol=1e-9)
        scale = np.abs(k[f"{case}{tag}_invh"]).max(axis=(1, 2), keepdims=True)
        assert np.max(np.abs(ih - k[f"{case}{tag}_invh"]) / scale) < 1e-8


@pytest.mark.parametrize("case", ["p1", "p3", "p2", "p8", "p12"])
def test_apeglm_shrinkage_templates_match_reference_at_the_other_widths_and_indices(case):
    """The two register widths no other file fits (p = 1 with the intercept shrunk, p = 3 with its last column) and the
    first / last column as the shrunken coefficient at p = 2, 8, 12 (kat_shrink_rest.npz, the unmodified utils.nbinomGLM)."""
    k = np.load(os.path.join(os.path.dirname(__file__), "golden", "kat_shrink_rest.npz"))
    kk = load_kat(case)
    G, sidx = int(k[f"{case}_G"]), int(k[f"{case}_sidx"])
    assert sidx == {"p1": 0, "p3": 2, "p2": 0, "p8": 7, "p12": 11}[case]
    for tag in "ab":
        b, ih, cv = hs.shrink(kk["counts"][:, :G], kk["X"], k[f"{case}_size"], np.log(kk["sf"]), 15.0,
                              float(k[f"{case}{tag}_scale"]), sidx)
        assert (cv == k[f"{case}{tag}_conv"]).all()
        np.testing.assert_allclose(b, k[f"{case}{tag}_beta"], rtol=1e-6, atol=1e-9)
        scale = np.abs(k[f"{case}{tag}_invh"]).max(axis=(1, 2), keepdims=True)
        assert np.max(np.abs(ih - k[f"{case}{tag}_invh"]) / scale) < 1e-8


@pytest.mark.parametrize("case", ["p2", "p4", "p8", "p12"])
@pytest.mark.parametrize("optimizer,tag", [("BFGS", "bfgs"), ("Newton-CG", "ncg")])
def test_apeglm_shrinkage_other_optimizers_match_reference(case, optimizer, tag):
    """utils.nbinomGLM(optimizer="BFGS" | "Newton-CG") of the unmodified reference (kat_shrink_opt.npz; ds.py never passes
    them, the Inference interface allows them) against dsq_bfgs.h's restatements of scipy's two methods: convergence flags
    equal - the files contain fits that scipy gives up on - Newton-CG to 1e-9 on every gene, BFGS to the resolution of
    its own stopping rule (max |g| <= 1e-8 on a flat scaled objective: the first iterate that meets it depends on the
    rounding of numpy's BLAS products in the inverse-Hessian update; <= 1e-6 absolute on the coefficients)."""
    k = np.load(os.path.join(os.path.dirname(__file__), "golden", "kat_shrink_opt.npz"))
    kk = load_kat(case)
    G, sidx = int(k[f"{case}_G"]), int(k[f"{case}_sidx"])
    b, ih, cv = hs.shrink(kk["counts"][:, :G], kk["X"], k[f"{case}_size"], np.log(kk["sf"]), 15.0, float(k[f"{case}_scale"]),
                          sidx, optimizer)
    assert (cv == k[f"{case}_{tag}_conv"]).all()
    rtol, atol = (1e-9, 1e-11) if optimizer == "Newton-CG" else (5e-4, 2e-6)
    np.testing.assert_allclose(b, k[f"{case}_{tag}_beta"], rtol=rtol, atol=atol)
    scale = np.abs(k[f"{case}_{tag}_invh"]).max(axis=(1, 2), keepdims=True)
    assert np.max(np.abs(ih - k[f"{case}_{tag}_invh"]) / scale) < (1e-8 if optimizer == "Newton-CG" else 2e-6)


@pytest.mark.parametrize("case", ["p16", "p24", "p40", "p48"])
def test_apeglm_shrinkage_wide_designs_match_reference(case):
    """Designs of 13 ... 48 columns (shrink_gene_wide: run-time p, Hessian row by row, inverse in the LDS workspace) against
    outputs of the unmodified utils.nbinomGLM (kat_shrink_wide.npz; 33 ... 48 columns, round 6: kat_shrink_wider.npz)."""
    k = np.load(os.path.join(os.path.dirname(__file__), "golden",
                             "kat_shrink_wider.npz" if case in ("p40", "p48") else "kat_shrink_wide.npz"))
    kk = load_kat(case)
    G, sidx = int(k[f"{case}_G"]), int(k[f"{case}_sidx"])
    for tag in "ab":
        b, ih, cv = hs.shrink(kk["counts"][:, :G], kk["X"], k[f"{case}_size"], np.log(kk["sf"]), 15.0,
                              float(k[f"{case}{tag}_scale"]), sidx)
        assert (cv == k[f"{case}{tag}_conv"]).all()
        np.testing.assert_allclose(b, k[f"{case}{tag}_beta"], rtol=1e-6, atol=1e-9)
        scale = np.abs(k[f"{case}{tag}_invh"]).max(axis=(1, 2), keepdims=True)
        assert np.max(np.abs(ih - k[f"{case}{tag}_invh"]) / scale) < 1e-8


@pytest.mark.parametrize("case", ["p8", "p4cat", "p2"])
def test_cell_path_matches_the_general_path_and_the_reference(case):
    """Designs with few distinct rows: per-cell weight sums + entry-parallel X^T W X (dsq_linalg.h, CellDesign)
    against the per-sample accumulation and against the reference KATs (p8: 30 cells)."""
    if case in ("p8", "p2"):  # p8: 30 cells (sums in LDS); p2: 2 cells (sums in registers, IRLS only)
        k = load_kat(case)
        counts, X, sf = k["counts"], k["X"], k["sf"]
        mu_hat, mom, fitted = k["mu_hat"], k["mom"], k["fitted"]
    else:  # 2 x 3 factorial with an interaction-free design: p = 4, 6 cells
        rng = np.random.default_rng(8)
        N = 90
        a, b = np.arange(N) % 2, (np.arange(N) // 2) % 3
        X = np.column_stack([np.ones(N), a == 1, b == 1, b == 2]).astype(float)
        counts, _ = orc.synth_counts(80, N, "2level", 8)
        sf = orc.size_factors_ratio(counts)[0]
        mom = orc.mom_dispersions(counts / sf[:, None], X, sf, 1e-8, float(N))
        _, mu_hat, _, _ = orc.irls(counts, sf, X, mom, 0.5, 1e-8)
        fitted = mom * 1.1
    N, P = X.shape
    maxd = float(max(10, N))
    for kw in (dict(), dict(prior_var=0.7, prior_reg=True)):
        start = mom if not kw else fitted
        ag, cg, _ = hs.alpha_mle(counts, X, mu_hat, start, 1e-8, maxd, **kw)
        if case == "p2":
            continue  # the dispersion kernel uses cells from 5 upwards
        ac, cc = hs.alpha_mle_cell(counts, X, mu_hat, start, 1e-8, maxd, **kw)
        assert (cc == cg).all()
        assert_close(ac, ag, 1e-6, 0, "cell vs general dispersion")
    if case == "p8":
        assert_close(ac, k["map_alpha"], 1e-6, 0, "cell MAP alpha vs reference")
    disp = np.clip(ag, 1e-8, maxd)
    cutoff = f_dist.ppf(0.99, P, N - P)
    contrast = np.zeros(P)
    contrast[1] = 1.0
    rd = orc.robust_mom_disp(counts / sf[:, None], X)
    g = hs.lfc_fit(counts, sf, X, disp, cells=False, robust_disp=rd, cutoff=cutoff, contrast=contrast)
    c = hs.lfc_fit(counts, sf, X, disp, cells=True, robust_disp=rd, cutoff=cutoff, contrast=contrast)
    assert (g["conv"] == c["conv"]).all()
    for key, tol in (("beta", 1e-9), ("mu", 1e-9), ("H", 1e-9), ("cooks", 1e-8), ("se", 1e-10), ("stat", 1e-8), ("p", 1e-7)):
        assert_close(c[key], g[key], tol, 1e-12 if key != "p" else 1e-300, f"cell vs general {key}")
    for fc, fg in zip(c["flags"], g["flags"]):
        assert (fc == fg).all()
    # the fused epilogue = the separate stages: Cook's from the (mu, H) layers, Wald from beta
    ck, rd2, fl = hs.cooks(counts, sf, X, g["mu"], g["H"], cutoff)
    assert_close(g["cooks"], ck, 1e-13, 1e-300, "fused cooks")
    assert_close(rd2, rd, 1e-11, 0, "robust disp")
    for fa, fb in zip(g["flags"], fl):
        assert (fa == fb).all()
    pw, sw, sew = hs.wald(X, disp, g["beta"], sf, np.diag(np.repeat(1e-6, P)), contrast, 0.0, None)
    assert_close(g["se"], sew, 1e-13, 0, "fused wald se")
    assert_close(g["p"], pw, 1e-11, 1e-300, "fused wald p")
    if case in ("p8", "p2"):
        assert_close(c["beta"], k["lfc_beta"], 1e-8, 1e-10, "cell beta vs reference")
        assert_close(c["H"], k["lfc_H"], 1e-8, 1e-12, "cell H vs reference")
        assert_close(c["se"], k["wald_se_none"], 1e-9, 0, "cell wald se vs reference")


@pytest.mark.parametrize("case", ["p4", "p8", "p12", "p16", "p24", "p40", "p48"])
def test_wide_path_vs_reference_kats(case):
    """Run-time-P path (dsq_wide.h: LDS matrices, lane-parallel Cholesky / inverse, chunked Gram accumulation)
    against the reference KATs, incl. the widths the register path cannot hold (p = 16, 24); with and without the
    design's cell structure."""
    k = load_kat(case)
    counts, X, sf = k["counts"], k["X"], k["sf"]
    N, P = X.shape
    maxd = float(max(10, N))
    tol = 1e-7 if P <= 8 else 2e-6
    m = hs.mom_wide(counts, sf, X, 1e-8, maxd)
    assert_close(m["rough"], k["rough"], 1e-9, 1e-13, "rough")
    assert_close(m["moments"], k["moments"], 1e-10, 1e-14, "moments")
    assert_close(m["lin_mu"], k["lin_mu"], 1e-10, 0, "lin_mu")
    n_cells = len(np.unique(X, axis=0))
    for cells in ([False, True] if n_cells <= 64 else [False]):
        a, c = hs.alpha_mle_wide(counts, X, k["mu_hat"], k["mom"], 1e-8, maxd, cells=cells)
        assert (c == k["gw_conv"]).all()
        assert_close(a, k["gw_alpha"], tol, 0, "genewise alpha")
        a, c = hs.alpha_mle_wide(counts, X, k["mu_hat"], k["fitted"], 1e-8, maxd, cells=cells,
                                 prior_var=float(k["prior_var"]), prior_reg=True)
        assert (c == k["map_conv"]).all()
        assert_close(a, k["map_alpha"], tol, 0, "MAP alpha")
        r = hs.lfc_fit(counts, sf, X, k["mom"], cells=cells, entry="hs_lfc_fit_wide")
        # the success flag of the L-BFGS-B rescue of a diverged low-count gene is decided at rounding-noise level
        # (the oracle needed the reference's own start-vector arithmetic to reproduce it): one such gene in p16
        assert (r["conv"] != k["irls_conv"]).sum() <= (1 if case == "p16" else 0)
        assert_close(r["beta"], k["irls_beta"], 1e-8, 1e-10, "irls beta")
        assert_close(r["mu"], k["irls_mu"], 1e-8, 1e-10, "irls mu")
        assert_close(r["H"], k["irls_H"], 1e-8, 1e-12, "irls H")
        disp = np.clip(k["map_alpha"], 1e-8, maxd)
        cutoff = f_dist.ppf(0.99, P, N - P)
        rd = orc.robust_mom_disp(k["normed"], X)
        r = hs.lfc_fit(counts, sf, X, disp, cells=cells, robust_disp=rd, cutoff=cutoff, contrast=k["contrast"],
                       entry="hs_lfc_fit_wide")
        assert (r["conv"] == k["lfc_conv"]).all()
        assert_close(r["beta"], k["lfc_beta"], 1e-8, 1e-10, "lfc beta")
        assert_close(r["H"], k["lfc_H"], 1e-8, 1e-12, "lfc H")
        assert_close(r["se"], k["wald_se_none"], 1e-8, 0, "wald se")
        assert_close(r["stat"], k["wald_stat_none"], 1e-7, 1e-11, "wald stat")
        assert_close(r["p"], k["wald_p_none"], 1e-6, 1e-300, "wald p")
        ref_ck = orc.cooks_distance(counts, k["normed"], X, k["lfc_mu"], k["lfc_H"])
        assert_close(r["cooks"], ref_ck, 1e-7, 1e-300, "cooks")


@pytest.mark.parametrize("kind", ["two_cells", "whole", "mixed_sizes", "ties"])
def test_robust_dispersion_large_cells_bucket_path(kind):
    """Cells of 129 samples or more take the one-pass bucket path of robust_disp_gene (dsq_stats.h, bucket_rank_sum) instead
    of a sort: against the oracle's sort-based restatement of utils.py:914-960 on genes built to stress it - mostly zero
    counts (the zero block sits at either trimming boundary), constant genes, two-valued genes, a single huge outlier (all
    other values in one bucket -> the selection fallback), heavy ties from equal size factors."""
    rng = np.random.default_rng(5)
    if kind in ("two_cells", "ties"):
        N = 700
        X = np.column_stack([np.ones(N), (np.arange(N) % 2).astype(float)])
    elif kind == "whole":
        N = 520
        X = np.column_stack([np.ones(N), rng.normal(size=N)])  # no cell with 3 replicates: one pseudo-cell of all samples
    else:
        N = 600  # cells of 300, 200 (bucket path) and 4 x 25 (sorted)
        lv = np.concatenate([np.zeros(300), np.ones(200), 2 + np.arange(100) // 25]).astype(int)
        X = np.column_stack([np.ones(N)] + [(lv == k).astype(float) for k in range(1, 6)])
    G = 64
    sf = np.exp(rng.normal(0, 0.3, N))
    sf[: N // 2] = 1.0  # equal size factors: exact ties among the normalised counts
    if kind == "ties":
        sf[:] = 1.0     # integer values only: every bucket is a block of ties, gene 7 overflows a boundary bucket
    mean = np.exp(rng.uniform(np.log(0.05), np.log(3000), G))
    counts = rng.negative_binomial(2.0, 2.0 / (2.0 + mean[None, :] * sf[:, None])).astype(np.int64)
    counts[:, 0] = 7                                     # constant
    counts[:, 1] = np.where(rng.random(N) < 0.5, 3, 11)  # two values
    counts[:, 2] = 0; counts[5, 2] = 1                   # all zero but one
    counts[:, 3] = rng.poisson(100, N); counts[17, 3] = 2_000_000  # one huge outlier
    counts[:, 4] = np.where(rng.random(N) < 0.9, 0, rng.poisson(5, N))   # zeros beyond the upper trimming boundary
    counts[:, 5] = np.where(rng.random(N) < 0.12, 0, rng.poisson(50, N))  # zero block ends near the lower boundary
    counts[:, 6] = np.where(rng.random(N) < 0.125, 0, 1 + rng.poisson(2, N))
    counts[:, 7] = 100000 + rng.poisson(2, N); counts[33, 7] = 2_000_000_000  # > 128 values in a boundary bucket: selection
    normed = counts / sf[:, None]
    mu = np.maximum(normed.mean(0)[None, :] * sf[:, None], 0.5)
    H = np.full((N, G), 0.01)
    ck, rd, _ = hs.cooks(counts, sf, X, mu, H, 10.0)
    ref = orc.robust_mom_disp(normed, X)
    assert_close(rd, ref, 1e-10, 1e-13, "robust dispersions")
    # the replacement value of the outlier refit (dds.py:1332-1352) takes the same bucket path
    assert_close(hs.trimmed_base_mean(counts, sf, 0.2), orc.trimmed_mean(normed, 0.2, axis=0), 1e-12, 1e-300, "trimmed mean")


@pytest.mark.parametrize("bad", [0.0, np.nan])
def test_robust_dispersion_keeps_the_nan_of_a_non_finite_mean(bad):
    """A size factor of 0 or NaN under a positive count: the mean of the normalised counts is inf / NaN, and
    np.maximum(alpha, 0.04) (utils.py:959) keeps the NaN of (v - m) / m^2 - it is not floored to 0.04.  Sorted cells and
    the bucket path."""
    rng = np.random.default_rng(4)
    for N in (60, 400):
        X = np.column_stack([np.ones(N), (np.arange(N) % 2).astype(float)])
        sf = np.exp(rng.normal(0, 0.3, N))
        counts = rng.negative_binomial(2.0, 2.0 / (2.0 + 50 * sf[:, None] * np.ones((1, 6)))).astype(np.int64) + 1
        sf[7] = bad
        with np.errstate(all="ignore"):
            ref = orc.robust_mom_disp(counts / sf[:, None], X)
        assert np.isnan(ref).all()
        _, rd, _ = hs.cooks(counts, sf, X, np.ones((N, 6)), np.full((N, 6), 0.01), 10.0)
        assert_close(rd, ref, 1e-10, 0, f"robust dispersions N={N}")


@pytest.mark.parametrize("shape", ["3factor_500", "3factor_90", "ragged"])
def test_robust_dispersion_small_cells_batched(shape):
    """Designs whose cells all have at most 64 samples sort several cells per pass (dsq_stats.h, seg_trimmed_variances):
    against the oracle's restatement of utils.py:914-960 and against the one-cell-at-a-time path, for 30 cells of 16-17
    samples (the c4 benchmark design), 30 cells of 3 samples, and cells of 3 ... 64 samples side by side (one of them
    excluded for having 2 replicates), with all-zero, constant and outlier genes."""
    rng = np.random.default_rng(11)
    if shape == "ragged":
        sizes = [3, 4, 5, 7, 8, 9, 16, 17, 23, 24, 31, 32, 33, 64, 2]
        lv = np.repeat(np.arange(len(sizes)), sizes)
        rng.shuffle(lv)
        N = len(lv)
        X = np.column_stack([np.ones(N)] + [(lv == k).astype(float) for k in range(1, len(sizes))])
    else:
        N = int(shape.split("_")[1])
        _, X = orc.synth_counts(4, N, "3factor", 3)
    G = 48
    sf = np.exp(rng.normal(0, 0.3, N))
    mean = np.exp(rng.uniform(np.log(0.05), np.log(3000), G))
    counts = rng.negative_binomial(2.0, 2.0 / (2.0 + mean[None, :] * sf[:, None])).astype(np.int64)
    counts[:, 0] = 0; counts[3, 0] = 2
    counts[:, 1] = 9
    counts[:, 2] = rng.poisson(40, N); counts[1, 2] = 3_000_000
    normed = counts / sf[:, None]
    ref = orc.robust_mom_disp(normed, X)
    _, cnt = orc.design_cells(X)
    seg = 1
    while seg < max(c for c in cnt if c >= 3):
        seg *= 2
    got = hs.robust_disp_seg(counts, sf, X, max(seg, 2))
    assert_close(got, ref, 1e-11, 1e-13, "batched cells")
    assert_close(hs.robust_disp_seg(counts, sf, X, 0), ref, 1e-11, 1e-13, "one cell at a time")


@pytest.mark.parametrize("mu, alpha", [(10, 0.5), (10, 0.1), (3, 0.5), (9, 0.05)])
def test_ref_nb_nll_moments(mu, alpha):
    """The reference's tests/test_utils.py:11-33 (`test_nb_nll_moments`) on the ENGINE's loss (the device templates of
    dsq_alpha.h, host instantiation) and on the oracle's: exp(-nll) over the counts 0 ... 10 (mu + mu^2 / alpha) is a
    probability distribution with the NB mean mu and variance mu + alpha mu^2 (sums instead of the reference's Monte Carlo
    draw, so the tolerances are tight)."""
    ys = np.arange(int(10 * (mu + mu ** 2 / alpha)))
    one = np.ones((1, 1))
    f_engine = np.array([hs.alpha_eval(np.array([y]), np.array([float(mu)]), one, np.log(alpha), cr_reg=False)[0] for y in ys])
    f_oracle = np.array([orc.nb_nll(np.array([y]), np.array([float(mu)]), alpha) for y in ys])
    for f in (f_engine, f_oracle):
        p = np.exp(-f)
        assert abs(p.sum() - 1.0) < 1e-9
        mean = (ys * p).sum()
        var = ((ys - mean) ** 2 * p).sum()
        assert abs(mean - mu) < 1e-6 * mu
        assert abs(var - (mu * alpha + 1) * mu) < 1e-5 * (mu * alpha + 1) * mu
    np.testing.assert_allclose(f_engine, f_oracle, rtol=1e-11, atol=1e-11)
