"""Host half of the regularized-log transformation: the prior variance of the sample coefficients.

DESeq2's rlogData estimates one scalar for all genes by matching the upper 5 % weighted quantile of the log2 differences
between every normalised count and its gene's mean to a zero-centred normal (matchWeightedUpperQuantileForVariance with
Hmisc's wtd.quantile(normwt = TRUE)).  One sort of N x G values, outside the kernel (a device version is a
follow-up); the per-gene fit is csrc/dsq_rlog.h."""
import numpy as np

_Z975 = 1.959963984540054  # the normal distribution's 97.5 % point


def weighted_upper_quantile(values, weights, upper=0.05):
    """The 1 - ``upper`` quantile of ``values`` under ``weights`` scaled to sum to their number n: with the values sorted
    and ``cs`` the running sum of their weights, Q(v) is the first value whose cs >= v (the last if none), and the result
    interpolates Q at the order statistic 1 + (n - 1)(1 - upper) like R's default quantile.  Tied values need no merging:
    the first entry that reaches v carries the tied value."""
    x = np.asarray(values, dtype=np.float64).ravel()
    w = np.asarray(weights, dtype=np.float64).ravel()
    n = x.size
    if n == 0 or w.size != n:
        raise ValueError("weighted_upper_quantile: values and weights of the same non-zero length")
    order = np.argsort(x)  # (any order inside a run of tied values gives the same answer)
    x = x[order]
    cs = np.cumsum(w[order] * (n / w.sum()))
    pos = 1.0 + (n - 1) * (1.0 - upper)
    low = max(np.floor(pos), 1.0)
    high = min(low + 1.0, float(n))
    fr = pos % 1.0
    k = np.minimum(np.searchsorted(cs, [low, high], side="left"), n - 1)
    return float((1.0 - fr) * x[k[0]] + fr * x[k[1]])


def beta_prior_var(counts, size_factors, fitted_dispersions):
    """``counts``: samples x genes, genes WITH counts only; ``fitted_dispersions``: their trend dispersions.  Every entry
    of a gene weighs 1 / (1 / base mean + dispersion)."""
    nc = np.asarray(counts, dtype=np.float64) / np.asarray(size_factors, dtype=np.float64)[:, None]
    bm = nc.mean(0)
    d = np.abs(np.log2(nc + 0.5) - np.log2(bm + 0.5))
    w = np.broadcast_to(1.0 / (1.0 / bm + np.asarray(fitted_dispersions, dtype=np.float64)), d.shape)
    q = weighted_upper_quantile(d, w)
    return (q / _Z975) ** 2
