"""Independent reference of the quasi-likelihood F-test in numpy / scipy: limma's squeezeVar with
scipy.special's polygamma functions, the NB unit deviance as written in the issue, the end-to-end test from oracle fits
(oracle.nbglm_oracle.irls at the trend dispersion) and scipy.stats.f.sf.  Shares no code with pydeseq2_amd.ql."""
import numpy as np
from scipy.special import digamma, polygamma

from oracle import nbglm_oracle as orc


def trigamma_inverse(x):
    """limma's trigammaInverse (scalar): Newton on 1 / trigamma from 0.5 + 1 / x."""
    if x > 1e7:
        return 1.0 / np.sqrt(x)
    if x < 1e-6:
        return 1.0 / x
    y = 0.5 + 1.0 / x
    for _ in range(50):
        tri = float(polygamma(1, y))
        dif = tri * (1.0 - tri / x) / float(polygamma(2, y))
        y += dif
        if -dif / y < 1e-8:
            break
    return y


def squeeze_var(s2, df):
    """(s2_post, df0, s02, df_total): limma's squeezeVar / fitFDist, no trend, not robust, over s2 > 0 and finite."""
    s2 = np.asarray(s2, dtype=float)
    ok = np.isfinite(s2) & (s2 > 0)
    z = np.log(s2[ok])
    e = z - digamma(df / 2) + np.log(df / 2)
    ebar = e.mean()
    v = e.var(ddof=1) - float(polygamma(1, df / 2))
    if v > 0:
        df0 = 2.0 * trigamma_inverse(v)
        s02 = float(np.exp(ebar + digamma(df0 / 2) - np.log(df0 / 2)))
        post = (df0 * s02 + df * s2) / (df0 + df)
    else:
        df0, s02 = np.inf, float(np.exp(ebar))
        post = np.where(np.isnan(s2), np.nan, s02)
    return post, df0, s02, min(df0 + df, ok.sum() * df)


def unit_deviance(y, mu, r):
    """The NB unit deviance, formula for formula (numpy doubles)."""
    y, mu = np.asarray(y, dtype=float), np.asarray(mu, dtype=float)
    with np.errstate(divide="ignore", invalid="ignore"):
        pos = 2.0 * (y * np.log(y / mu) - (y + r) * np.log((y + r) / (mu + r)))
    return np.where(y > 0, pos, 2.0 * r * np.log1p(mu / r))


def ql_reference(fit_counts, sf, X, Xr, trend, use):
    """The whole test on the genes ``use`` of samples x genes counts: oracle IRLS fits of both designs at the dispersions
    ``trend``, deviances in numpy (the numerator in long double from the analytic difference, so that the reference's own
    cancellation stays below its fit tolerance), squeeze_var, scipy.stats.f.sf (chi2.sf for df0 = inf).
    Returns a dict of G-vectors (NaN outside ``use``) and the prior's scalars."""
    from scipy.stats import chi2, f

    fit_counts, sf, trend = np.asarray(fit_counts), np.asarray(sf, float), np.asarray(trend, float)
    N, G = fit_counts.shape
    P, Pr = X.shape[1], Xr.shape[1]
    ui = np.nonzero(use)[0]
    bf, muf, _, cf = orc.irls(fit_counts[:, ui], sf, X, trend[ui])
    br, mur, _, cr = orc.irls(fit_counts[:, ui], sf, Xr, trend[ui])
    nan = lambda *s: np.full(s, np.nan)  # noqa: E731
    out = dict(num=nan(G), dev=nan(G), s2=nan(G), F=nan(G), p=nan(G), beta_f=nan(G, P), beta_r=nan(G, Pr), conv_f=nan(G),
               conv_r=nan(G))
    L = np.longdouble
    for k, g in enumerate(ui):
        y, r = fit_counts[:, g].astype(float), 1.0 / trend[g]
        out["dev"][g] = unit_deviance(y, muf[:, k], r).sum()
        ef, er = (X @ bf[k]).astype(L), (Xr @ br[k]).astype(L)
        mf, mr = sf.astype(L) * np.exp(ef), sf.astype(L) * np.exp(er)
        out["num"][g] = float(2 * (y.astype(L) * (ef - er) - (y.astype(L) + L(r)) * (np.log(L(r) + mf) - np.log(L(r) + mr))).sum())
    out["s2"] = out["dev"] / (N - P)
    out["beta_f"][ui], out["beta_r"][ui], out["conv_f"][ui], out["conv_r"][ui] = bf, br, cf, cr
    post, df0, s02, df_total = squeeze_var(out["s2"], N - P)
    out["F"] = np.maximum(out["num"], 0.0) / ((P - Pr) * post)
    out["p"] = f.sf(out["F"], P - Pr, df_total) if np.isfinite(df0) else chi2.sf((P - Pr) * out["F"], P - Pr)
    # (df_total is squeeze_var's capped value also for df0 = inf, where the test above is the chi-square limit)
    out.update(s2_post=post, df0=df0, s02=s02, df_total=df_total, df_test=P - Pr)
    return out
