"""Host half of the regularized-log transformation: the prior variance of the sample coefficients, and the call.

DESeq2's rlogData estimates one scalar for all genes by matching the upper 5 % weighted quantile of the log2 differences
between every normalised count and its gene's mean to a zero-centred normal (matchWeightedUpperQuantileForVariance with
Hmisc's wtd.quantile(normwt = TRUE)).  One sort of N x G values, outside the kernel (a device version is a
follow-up); the per-gene fit is csrc/dsq_rlog.h, launched by ``rlog`` below (``DeseqPipeline.rlog`` delegates to it)."""
import ctypes as C

import numpy as np

from ._lib import DeviceScope, gather_rows_i32

_vp = C.c_void_p

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


def rlog(pipe, res, prior_var=None):
    """Regularized-log transformation (DESeq2's rlog(); csrc/dsq_rlog.h) of the resident counts, post hoc
    like wald() / lrt(): per gene a ridge-penalised NB GLM with an intercept and one coefficient per sample, fitted at
    the TREND dispersions ``res.fitted_dispersions`` from the intercept log ``res.normed_means`` with the size factors
    of ``res`` - a result of ``deseq2()`` or of ``deseq2(stop_after_trend=True)``.  ``prior_var`` (log2 scale):
    the prior variance of the sample coefficients; None: estimated on the host from all genes with counts
    (``beta_prior_var`` above).  One launch.
    Returns (rlog N x G in log2, intercept, converged, n_iter, beta_prior_var); genes without counts: rlog 0 in every
    sample, intercept / converged / n_iter NaN."""
    G, N, ctx = pipe.G, pipe.N, pipe.ctx
    if res.fitted_dispersions is None:
        raise ValueError("rlog(): the result carries no fitted_dispersions (run deseq2(), or "
                         "deseq2(stop_after_trend=True), first).")
    nz = np.asarray(res.non_zero, dtype=bool)
    nzi = np.nonzero(nz)[0]
    Gn = len(nzi)
    fit = np.asarray(res.fitted_dispersions, dtype=np.float64)[nzi]
    if not (np.isfinite(fit) & (fit > 0)).all():
        raise ValueError("rlog(): fitted_dispersions is not a finite positive number on every gene with counts.")
    if prior_var is not None and not (np.isfinite(prior_var) and prior_var > 0):
        raise ValueError(f"rlog(): beta_prior_var must be a finite positive number (got {prior_var}).")
    sf = np.ascontiguousarray(res.size_factors, dtype=np.float64)
    out = np.zeros((N, G))
    b0, conv, nit = np.full(G, np.nan), np.full(G, np.nan), np.full(G, np.nan)
    if Gn == 0:
        return out, b0, conv, nit, (float(prior_var) if prior_var is not None else np.nan)
    if prior_var is None:
        prior_var = beta_prior_var(pipe.d_raw.to_host()[:, nzi], sf, fit)
        if not (np.isfinite(prior_var) and prior_var > 0):
            raise ValueError(f"rlog(): the estimated beta_prior_var is {prior_var} (no count differs from its "
                             "gene's mean, as with a single sample): give beta_prior_var.")
    prior_var = float(prior_var)
    with DeviceScope(ctx) as s:
        d_sf, d_fit = s.upload(sf), s.upload(fit)
        d_bm = s.upload(np.asarray(res.normed_means, dtype=np.float64)[nzi])
        d_y = pipe.d_y if Gn == G else gather_rows_i32(s, ctx, pipe.d_y.ptr, pipe.ldn, nzi, N)
        d_out = s.empty((Gn, N), np.float64)
        d_b0, d_cv, d_it = s.empty((Gn,), np.float64), s.empty((Gn,), np.uint8), s.empty((Gn,), np.int32)
        pipe._k("rlog", Gn, "dsq_dev_rlog", _vp(d_y.ptr), pipe.ldn, _vp(d_sf.ptr), N, Gn, _vp(d_fit.ptr), _vp(d_bm.ptr),
                C.c_double(prior_var), _vp(d_out.ptr), _vp(d_b0.ptr), _vp(d_cv.ptr), _vp(d_it.ptr))
        out[:, nzi] = d_out.to_host().T
        b0[nzi], conv[nzi], nit[nzi] = d_b0.to_host(), d_cv.to_host(), d_it.to_host()
    return out, b0, conv, nit, prior_var
