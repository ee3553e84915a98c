"""Dense restatement of the regularized-log transformation in numpy (test infrastructure): what DESeq2's rlogData ->
fitNbinomGLMs -> fitBeta computes for rlog(), written the way DESeq2 writes it - N + 1 explicit design columns and, per
iteration, a QR solve of the augmented least-squares problem [sqrt(W) X ; sqrt(Lambda)] beta = [sqrt(W) z ; 0] -
deliberately NOT through the arrowhead formulas of csrc/dsq_rlog.h.  The statement of the algorithm is DESIGN.md 6h.
Also the weighted upper-quantile estimate of the prior variance, by direct construction."""
import numpy as np
from scipy.special import gammaln

LN2 = np.log(2.0)
MAXIT, TOL, MINMU, MAXBETA = 100, 1e-4, 0.5, 30.0
Z975 = 1.959963984540054  # qnorm(0.975)


def nb_logpmf(y, mu, size):
    return (gammaln(y + size) - gammaln(size) - gammaln(y + 1.0) + size * np.log(size / (size + mu))
            + y * np.log(mu / (size + mu)))


def rlog_gene(y, sf, disp, base_mean, beta_prior_var):
    """One gene -> (rlog [N] log2, intercept log2, n_iter, converged, [c_0, c_1, ...])."""
    y, sf = np.asarray(y, float), np.asarray(sf, float)
    N = y.size
    X = np.hstack([np.ones((N, 1)), np.eye(N)])
    lam = np.concatenate([[1e-6 / LN2 ** 2], np.full(N, 1.0 / (beta_prior_var * LN2 ** 2))])
    ridge = np.diag(np.sqrt(lam))
    beta = np.concatenate([[np.log(base_mean)], np.zeros(N)])
    mu = np.maximum(sf * np.exp(X @ beta), MINMU)
    dev_old, cs, n_iter, conv = 0.0, [], MAXIT, False
    for t in range(MAXIT):
        w = mu / (1.0 + disp * mu)
        z = np.log(mu / sf) + (y - mu) / mu
        sw = np.sqrt(w)
        Aug = np.vstack([sw[:, None] * X, ridge])
        rhs = np.concatenate([sw * z, np.zeros(N + 1)])
        Q, R = np.linalg.qr(Aug)
        beta = np.linalg.solve(R, Q.T @ rhs)
        if (np.abs(beta) > MAXBETA).any():
            break
        mu = np.maximum(sf * np.exp(X @ beta), MINMU)
        dev = -2.0 * nb_logpmf(y, mu, 1.0 / disp).sum()
        c = abs(dev - dev_old) / (abs(dev) + 0.1)
        cs.append(c)
        if np.isnan(c):
            break
        if t > 0 and c < TOL:
            n_iter = t + 1
            conv = n_iter < MAXIT
            break
        dev_old = dev
    return (beta[0] + beta[1:]) / LN2, beta[0] / LN2, n_iter, conv, cs


def rlog(counts, sf, disp, base_mean, beta_prior_var):
    """counts: samples x genes -> (rlog N x G, intercept, n_iter, converged, list of per-iteration c per gene)."""
    counts = np.asarray(counts)
    N, G = counts.shape
    out, b0 = np.empty((N, G)), np.empty(G)
    it, cv, cs = np.empty(G, int), np.empty(G, bool), []
    for g in range(G):
        out[:, g], b0[g], it[g], cv[g], c = rlog_gene(counts[:, g], sf, disp[g], base_mean[g], beta_prior_var)
        cs.append(c)
    return out, b0, it, cv, cs


def borderline(cs, rel=1e-6):
    """Does some c_t, t >= 1, lie within `rel` (relative) of the tolerance?  (Then two correct algebras may count
    differently.)"""
    return any(abs(c - TOL) <= rel * TOL for c in cs[1:])


def weighted_upper_quantile(absd, weights, upper=0.05):
    """Hmisc::wtd.quantile(abs d, weights, 1 - upper, normwt = TRUE) by direct construction: the weights scaled to sum
    to n, the sorted values with their running weight, and the type-7 order statistic read off it."""
    x, w = np.asarray(absd, float).ravel(), np.asarray(weights, float).ravel()
    n = x.size
    w = w * (n / w.sum())
    o = np.argsort(x, kind="stable")
    x, cs = x[o], np.cumsum(w[o])
    order = 1.0 + (n - 1) * (1.0 - upper)
    low = max(np.floor(order), 1.0)
    high = min(low + 1.0, float(n))
    fr = order % 1.0

    def Q(v):
        k = np.nonzero(cs >= v)[0]
        return x[k[0]] if k.size else x[-1]

    return (1.0 - fr) * Q(low) + fr * Q(high)


def prior_var(counts, sf, disp_fit, has_counts=None):
    """beta_prior_var of rlog (DESeq2's matchWeightedUpperQuantileForVariance over log2 (nc + 0.5) - log2 (bm + 0.5))."""
    counts = np.asarray(counts, float)
    keep = np.ones(counts.shape[1], bool) if has_counts is None else np.asarray(has_counts, bool)
    nc = counts[:, keep] / np.asarray(sf, float)[:, None]
    bm = nc.mean(0)
    d = np.log2(nc + 0.5) - np.log2(bm + 0.5)
    w = np.broadcast_to(1.0 / (1.0 / bm + np.asarray(disp_fit, float)[keep]), d.shape)
    q = weighted_upper_quantile(np.abs(d), w)
    return float((q / Z975) ** 2)
