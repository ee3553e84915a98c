"""Inputs and oracle-side expectations shared by the likelihood-ratio tests (host and GPU)."""
import numpy as np
import pandas as pd

from oracle import nbglm_oracle as orc
from tests.helpers import load_kat

CASES = ("p2", "p4", "p8m", "p16", "p65", "p128")
CHISQ_DFS = (1, 2, 3, 4, 7, 16, 47, 64, 127)


def lrt_case(case):
    """(counts of the fixture's genes, sf, X, X_reduced, fixture fields of the case)."""
    k, f = load_kat(case), load_kat("lrt")
    gi = f[f"{case}_genes"]
    fx = {name[len(case) + 1:]: v for name, v in f.items() if name.startswith(case + "_")}
    return np.ascontiguousarray(k["counts"][:, gi]), k["sf"], k["X"], np.ascontiguousarray(k["X"][:, fx["cols"]]), fx


_grid = {}


def chisq_grid():
    """x grid, {df: 50-digit survival function as (float value, mpf)}, and the bound on the relative error the issue
    sets: 8 x the worst relative error of scipy.stats.chi2.sf on the same grid where the truth is >= 1e-300 (the factor
    covers sums of up to 64 terms and a <= 1-ulp exp).  Computed once per process."""
    if not _grid:
        import mpmath
        from scipy.stats import chi2

        xs = np.geomspace(1e-8, 1400.0, 120)
        truth, worst = {}, 0.0
        with mpmath.workdps(50):
            for df in CHISQ_DFS:
                t = [mpmath.gammainc(mpmath.mpf(df) / 2, mpmath.mpf(float(x)) / 2, mpmath.inf, regularized=True)
                     for x in xs]
                truth[df] = t
                sp = chi2.sf(xs, df)
                for tv, s in zip(t, sp):
                    if tv >= mpmath.mpf("1e-300"):
                        worst = max(worst, float(abs(mpmath.mpf(float(s)) - tv) / tv))
        _grid.update(xs=xs, truth=truth, bound=8.0 * worst, scipy_worst=worst)
    return _grid


def chisq_check(fn, label):
    """fn(x array, df) -> survival function; asserts the bound of chisq_grid() and returns the worst relative error."""
    import mpmath

    g = chisq_grid()
    worst, where = 0.0, None
    with mpmath.workdps(50):
        for df in CHISQ_DFS:
            out = fn(g["xs"], df)
            for x, o, tv in zip(g["xs"], out, g["truth"][df]):
                if tv >= mpmath.mpf("1e-300"):
                    e = float(abs(mpmath.mpf(float(o)) - tv) / tv)
                    if e > worst:
                        worst, where = e, (df, float(x))
                else:
                    assert 0.0 <= o <= 1e-299, (df, x, o)
    print(f"{label}: worst relative error {worst:.3e} at (df, x) = {where}; scipy {g['scipy_worst']:.3e}; "
          f"bound {g['bound']:.3e}")
    assert worst <= g["bound"], (worst, where, g["bound"])
    return worst


def facade_scenario():
    """300 genes x 24 samples, ~batch + condition (2 x 3 cells of 4 replicates, min_replicates = 4), two injected
    Cook's outliers: gene 5 - one huge count on an expressed gene (replaced and refitted) - and gene 9 - a single count
    on an otherwise empty gene (all zero after the replacement)."""
    N, G = 24, 300
    i = np.arange(N)
    meta = pd.DataFrame({"batch": np.where(i % 2 == 0, "a", "b"), "condition": np.array(["x", "y", "z"])[(i // 2) % 3]},
                        index=[f"s{k}" for k in i])
    X = np.column_stack([np.ones(N), i % 2 == 1, (i // 2) % 3 == 1, (i // 2) % 3 == 2]).astype(float)
    rng = np.random.default_rng(24)
    beta = np.vstack([rng.normal(6.0, 1.0, G), rng.normal(0, 0.4, G), rng.normal(0, 0.6, G), rng.normal(0, 0.6, G)])
    beta[2:, ::3] = 0.0  # a third of the genes: no condition effect
    disp = 4 / 2.0 ** beta[0] + 0.05
    sf = np.exp(rng.normal(0, 0.2, N))
    mu = sf[:, None] * 2.0 ** (X @ beta)
    counts = rng.negative_binomial(1 / disp[None, :], (1 / disp[None, :]) / (1 / disp[None, :] + mu)).astype(np.int64)
    counts[7, 5] = 400 * counts[:, 5].max()
    counts[:, 9] = 0
    counts[3, 9] = 5000
    counts = pd.DataFrame(counts, index=meta.index, columns=[f"g{j}" for j in range(G)])
    return counts, meta, X


def rebuilt_counts(counts, X, ref, min_replicates):
    """The counts with the Cook's outliers of ref.replaced imputed, as dds.py:1329-1358 builds them (from the oracle's
    layers)."""
    from scipy.stats import f as f_dist

    N, p = X.shape
    sf = np.asarray(ref.size_factors)
    cid, cnt = orc.design_cells(X)
    replaceable = cnt[cid] >= min_replicates
    with np.errstate(invalid="ignore"):
        idx = ref.cooks > f_dist.ppf(0.99, p, N - p)
    rp = np.nonzero(ref.replaced)[0]
    out = np.array(counts, dtype=np.int64)
    sub = out[:, rp].copy()
    tbm = orc.trimmed_mean(sub / sf[:, None], trim=0.2, axis=0)
    repl = (tbm[:, None] * sf[None, :]).astype(int).T
    m = replaceable[:, None] & idx[:, rp]
    sub[m] = repl[m]
    out[:, rp] = sub
    return out


def oracle_lrt(counts, X, Xr, ref, fit_counts):
    """(stat, pvalue, reduced beta, reduced flags, stat_ref_err) from oracle functions: orc.irls on both designs at ref's
    dispersions and size factors over fit_counts, 2 (nb_nll_reduced - nb_nll_full), chi2.sf; the rules for all-zero genes
    of the issue.  stat_ref_err: max |float64 - long double| of that difference, the reference's own cancellation error
    (as tests/golden/make_golden_lrt.py stores it for the fixture cases)."""
    from scipy.stats import chi2

    G = counts.shape[1]
    sf, disp = np.asarray(ref.size_factors), np.asarray(ref.dispersions)
    use = np.asarray(ref.non_zero, bool) & ~np.asarray(ref.new_all_zeroes, bool)
    ui = np.nonzero(use)[0]
    bf, muf, _, _ = orc.irls(fit_counts[:, ui], sf, X, disp[ui])
    br, mur, _, cr = orc.irls(fit_counts[:, ui], sf, Xr, disp[ui])
    stat, p = np.full(G, np.nan), np.full(G, np.nan)
    beta_r, conv = np.full((G, Xr.shape[1]), np.nan), np.full(G, np.nan)
    L, err = np.longdouble, 0.0

    def nll_ld(y, mu, alpha):  # utils.nb_nll without its lgamma terms (those of the other model: they cancel exactly)
        y, mu, r = y.astype(L), mu.astype(L), L(1.0) / L(alpha)
        with np.errstate(divide="ignore", invalid="ignore"):
            return ((y + r) * np.log(r + mu) - np.where(y > 0, y * np.log(mu), L(0.0))).sum()

    for k, g in enumerate(ui):
        y = fit_counts[:, g]
        stat[g] = 2.0 * (orc.nb_nll(y, mur[:, k], disp[g]) - orc.nb_nll(y, muf[:, k], disp[g]))
        err = max(err, abs(float(2.0 * (nll_ld(y, mur[:, k], disp[g]) - nll_ld(y, muf[:, k], disp[g])) - L(stat[g]))))
    p[ui] = chi2.sf(stat[ui], X.shape[1] - Xr.shape[1])
    beta_r[ui], conv[ui] = br, cr.astype(float)
    z = np.asarray(ref.new_all_zeroes, bool)
    stat[z], p[z] = 0.0, 1.0
    return stat, p, beta_r, conv, err
