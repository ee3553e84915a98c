"""limma-voom (Law et al. 2014), post hoc: log-CPM and an unweighted first fit per gene by k_voom_fit1, the
mean-variance trend on the host (R's ``lowess`` with ``delta``, restated here as ``lowess_delta``), precision weights from
the trend's knots and the weighted fit by k_voom_wls (csrc/dsq_voom.h), the moderation of the residual variances by
``ql.squeeze_var`` (limma's squeezeVar) and the p-value of the moderated t by k_ql_score (F = t^2 on (1, df_total) degrees
of freedom).  ``DeseqPipeline.voom`` delegates here."""
import ctypes as C
import math
from typing import NamedTuple

import numpy as np

from ._lib import DeviceScope
from .ql import score_df, squeeze_var

_vp, c_double = C.c_void_p, C.c_double

VOOM_MAX_P = 48  # DSQ_VOOM_MAX_P: the run-time-P family on the wave's LDS workspace
VOOM_MAX_KNOTS = 256  # kVoomMaxKnots
LOG2_1E6 = math.log2(1e6)


# -------------------------------------------------------------------------------------------------------------- lowess
class Lowess(NamedTuple):
    fitted: np.ndarray  # the smooth at every point, in the order of the input
    knot_x: np.ndarray  # the anchors of the last pass (the points a local fit was made at): strictly increasing
    knot_y: np.ndarray


def _seq_sum(v):
    """The sum of a vector added front to back, as clowess's loops add (numpy's reduction adds pairwise)."""
    return float(np.cumsum(v)[-1]) if v.shape[0] else 0.0


def _local_fit(x, y, i, nleft, nright, rw, span_range):
    """R's ``lowest`` at x[i] over the window [nleft, nright] (0-based, inclusive): -> (value, ok)."""
    n = x.shape[0]
    xs = x[i]
    h = max(xs - x[nleft], x[nright] - xs)
    h9, h1 = 0.999 * h, 0.001 * h
    # the scan runs from nleft until the first point right of xs beyond 0.999 h: ties of xs and points within h past
    # nright are included.  Every such point has x <= xs + h: a slice bounded by that holds the whole scan.
    hi = min(n, int(np.searchsorted(x, xs + h, side="right")) + 1)
    xv = x[nleft:hi]
    r = np.abs(xv - xs)
    stop = np.nonzero((r > h9) & (xv > xs))[0]
    m = int(stop[0]) if stop.size else xv.shape[0]
    xv, r = xv[:m], r[:m]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = r / h
        q = q * q * q
        t = 1.0 - q
        w = np.where(r <= h9, np.where(r <= h1, 1.0, t * t * t), 0.0)
    if rw is not None:
        w = w * rw[nleft:nleft + m]
    a = _seq_sum(w)
    if not a > 0.0:
        return 0.0, False
    w = w / a
    if h > 0.0:
        a = _seq_sum(w * xv)
        b = xs - a
        d = xv - a
        c = _seq_sum(w * d * d)
        if math.sqrt(c) > 0.001 * span_range:
            b /= c
            w = w * (b * d + 1.0)
    return _seq_sum(w * y[nleft:nleft + m]), True


def lowess_delta(x, y, f=2.0 / 3.0, iter=3, delta=None) -> Lowess:  # noqa: A002 - R's argument name
    """R's ``lowess(x, y, f, iter, delta)`` (Cleveland's ``clowess``; ``delta`` defaults to 1 % of the range of x as in R),
    with the anchors of the last pass.  Local linear fits with tricube weights over the ns = clamp(int(f n + 1e-7), 2, n)
    nearest points, ``iter`` robustness passes with bisquare weights of the residuals (6 median |residual|), a local fit
    only every ``delta`` along x and linear interpolation between the fitted anchors; points with the x of an anchor take
    its value.  x need not be sorted (a stable sort, as R's order()); host only.  Not ``summary.lowess`` - the
    reference's 50-point smoother of the independent filter - which stays as it is."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if x.shape != y.shape or x.shape[0] < 1:
        raise ValueError("lowess_delta: x and y must be vectors of one length, at least one point")
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        raise ValueError("lowess_delta: x and y must be finite")
    n = x.shape[0]
    order = np.argsort(x, kind="stable")
    x, y = x[order], y[order]
    if delta is None:
        delta = 0.01 * (x[-1] - x[0])
    delta = float(delta)
    ys = np.empty(n)
    if n < 2:
        ys[0] = y[0]
        return Lowess(ys[np.argsort(order, kind="stable")], x.copy(), ys.copy())
    ns = max(2, min(n, int(f * n + 1e-7)))
    span_range = x[-1] - x[0]
    rw = None
    anchors = []
    for it in range(iter + 1):
        nleft, nright, last, i = 0, ns - 1, -1, 0
        anchors = []
        while True:
            while nright < n - 1 and x[i] - x[nleft] > x[nright + 1] - x[i]:
                nleft += 1
                nright += 1
            v, ok = _local_fit(x, y, i, nleft, nright, rw, span_range)
            ys[i] = v if ok else y[i]
            anchors.append(i)
            if last < i - 1:  # interpolate between the two anchors
                denom = x[i] - x[last]
                alpha = (x[last + 1:i] - x[last]) / denom
                ys[last + 1:i] = alpha * ys[i] + (1.0 - alpha) * ys[last]
            last = i
            cut = x[last] + delta
            # the points up to cut: those with the x of the anchor copy its value and move `last` on
            j = int(np.searchsorted(x, cut, side="right"))  # first index with x > cut
            k = int(np.searchsorted(x, x[last], side="right"))  # first index with x > x[last]
            if k > last + 1:
                ys[last + 1:k] = ys[last]
                last = k - 1
            i = max(last + 1, j - 1)
            if last >= n - 1:
                break
        res = y - ys
        if it >= iter:
            break
        ares = np.abs(res)
        sc = _seq_sum(ares) / n
        srt = np.sort(ares)
        m1 = n // 2
        cmad = 3.0 * (srt[m1] + srt[n - m1 - 1])
        if cmad < 1e-7 * sc:
            break
        c9, c1 = 0.999 * cmad, 0.001 * cmad
        with np.errstate(divide="ignore", invalid="ignore"):
            q = ares / cmad
            t = 1.0 - q * q
            rw = np.where(ares <= c1, 1.0, np.where(ares <= c9, t * t, 0.0))
    a = np.asarray(anchors, dtype=np.int64)
    inv = np.empty(n, dtype=np.int64)
    inv[order] = np.arange(n)
    return Lowess(ys[inv], x[a].copy(), ys[a].copy())


def knot_eval(knot_x, knot_y, lam):
    """The trend at ``lam``: linear between the knots, the end values outside (k_voom_wls's table lookup, on the host)."""
    return np.interp(np.asarray(lam, dtype=np.float64), knot_x, knot_y)


# -------------------------------------------------------------------------------------------------------------- inputs
def check_design(N, P, full_rank=True):
    """What voom needs of a design, on the host before any launch."""
    if P < 1 or P > VOOM_MAX_P:
        raise ValueError(f"voom fits designs of 1 ... {VOOM_MAX_P} columns (got {P}).")
    if N - P < 1:
        raise ValueError(f"voom needs residual degrees of freedom: {N} samples and {P} design columns leave none.")
    if not full_rank:
        raise ValueError("voom needs a design of full column rank (the first fit goes through its pseudo-inverse and the "
                         "weighted fit through a Cholesky factor).")


def library_sizes(lib_size, N, size_factors=None, colsums=None):
    """The library sizes L_n voom divides by.  "size_factors": sf_n / geomean_n(sf_n / colsum_n) - the column sums times
    normalisation factors of geometric mean 1, how DESeq2's size factors map onto edgeR's lib.size x norm.factors;
    "colsums": the plain column sums (limma's default for a matrix); or N positive finite numbers."""
    if isinstance(lib_size, str):
        if lib_size not in ("size_factors", "colsums"):
            raise ValueError(f"lib_size must be 'size_factors', 'colsums' or {N} positive numbers (got {lib_size!r}).")
        if colsums is None:
            raise ValueError(f"lib_size={lib_size!r} needs the column sums of the counts.")
        cs = np.asarray(colsums, dtype=np.float64).reshape(-1)
        if cs.shape[0] != N or not (cs > 0.0).all():
            raise ValueError("voom: every sample needs at least one count (a library size of zero).")
        if lib_size == "colsums":
            return cs
        sf = np.asarray(size_factors, dtype=np.float64).reshape(-1)
        if sf.shape[0] != N or not (np.isfinite(sf) & (sf > 0.0)).all():
            raise ValueError("voom: lib_size='size_factors' needs N positive finite size factors.")
        return sf / math.exp(math.fsum(np.log(sf / cs).tolist()) / N)
    L = np.asarray(lib_size, dtype=np.float64).reshape(-1)
    if L.shape[0] != N or not (np.isfinite(L) & (L > 0.0)).all():
        raise ValueError(f"lib_size must be 'size_factors', 'colsums' or {N} positive finite numbers.")
    return L


def norm_factors(L, colsums):
    """L_n / colsum_n: the normalisation factors the library sizes imply."""
    return np.asarray(L, dtype=np.float64) / np.asarray(colsums, dtype=np.float64)


def sample_offsets(L):
    """log2(L_n + 1) - log2(1e6): what the kernels subtract from log2(y + 0.5)."""
    return np.log2(np.asarray(L, dtype=np.float64) + 1.0) - LOG2_1E6


def check_contrasts(contrasts, P):
    c = np.atleast_2d(np.asarray(contrasts, dtype=np.float64))
    if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] != P:
        raise ValueError("The contrast vectors must have the same length as the design matrix (K x P, K >= 1).")
    if not np.isfinite(c).all() or not (c != 0.0).any(axis=1).all():
        raise ValueError("The contrast vectors must be finite and none all zero.")
    return np.ascontiguousarray(c)


def voom_trend(amean, sigma1, off, span=0.5):
    """The mean-variance trend of voom from the first fit: lowess of sqrt(sigma1) on Abar + mean_n off_n over the genes
    with counts (finite Abar), f = span, 3 robustness passes, delta = 1 % of the range.  -> (knot_x, knot_y): the anchors
    of the last pass.  ValueError: fewer than 2 genes with counts, a knot value that is not a positive finite number,
    more than 256 knots."""
    amean, sigma1 = np.asarray(amean, dtype=np.float64), np.asarray(sigma1, dtype=np.float64)
    use = np.isfinite(amean) & np.isfinite(sigma1)
    if int(use.sum()) < 2:
        raise ValueError(f"voom: {int(use.sum())} gene(s) with counts; the mean-variance trend needs at least 2.")
    sx = amean[use] + math.fsum(np.asarray(off, dtype=np.float64).tolist()) / len(off)
    sy = np.sqrt(sigma1[use])
    lo = lowess_delta(sx, sy, f=span, iter=3, delta=0.01 * (sx.max() - sx.min()))
    return check_knots(lo.knot_x, lo.knot_y)


def check_knots(kx, ky):
    kx, ky = np.ascontiguousarray(kx, dtype=np.float64), np.ascontiguousarray(ky, dtype=np.float64)
    if kx.shape[0] > VOOM_MAX_KNOTS:
        raise ValueError(f"voom: the trend has {kx.shape[0]} knots; the device table holds {VOOM_MAX_KNOTS}.")
    if not (np.isfinite(ky) & (ky > 0.0)).all() or not np.isfinite(kx).all():
        raise ValueError("voom: the mean-variance trend is not a positive finite number at every knot (its fourth power "
                         "is the variance the precision weights invert).")
    if kx.shape[0] == 1:  # every gene at one mean: a constant trend, as a table of two knots
        kx, ky = np.array([kx[0], kx[0] + 1.0]), np.array([ky[0], ky[0]])
    if not (np.diff(kx) > 0.0).all():
        raise ValueError("voom: the knots of the trend are not strictly increasing.")
    return kx, ky


# ---------------------------------------------------------------------------------------------------------------- test
class VoomResult(NamedTuple):
    pvalue: np.ndarray  # K x G
    t: np.ndarray  # K x G moderated t
    est: np.ndarray  # K x G contrast estimates, log2
    lfcSE: np.ndarray  # K x G: sqrt(s2_post) u
    sigma2: np.ndarray  # G residual variance of the weighted fit
    s2_post: np.ndarray  # G moderated
    df0: float
    s02: float
    df_total: float  # the denominator degrees of freedom of the test: ql.score_df(), infinite when df0 is
    beta: np.ndarray  # G x P weighted-fit coefficients, log2
    Amean: np.ndarray  # G mean log-CPM
    knots: tuple  # (knot_x, knot_y)


def _fit(pipe, s, off, contrasts, span, layers):
    """Both launches; -> host (beta1, amean, sigma1, knots, beta, sigma2, est, u, d_E, d_w)."""
    G, N, P, D = pipe.G, pipe.N, pipe.P, pipe.design
    K = contrasts.shape[0]
    d_off = s.upload(off)
    d_b1 = s.empty((G, P), np.float64)
    d_as = s.empty((2 * G,), np.float64)
    pipe._k("voom_fit1", G, "dsq_dev_voom_fit1", _vp(pipe.d_y.ptr), pipe.ldn, _vp(d_off.ptr), _vp(pipe.d_Xt.ptr),
            _vp(pipe.d_pinv.ptr), D.ldx, P, N, G, _vp(d_b1.ptr), _vp(d_as.ptr), _vp(d_as.ptr + 8 * G))
    o = d_as.to_host()
    amean, sigma1 = o[:G], o[G:]
    kx, ky = voom_trend(amean, sigma1, off, span)
    d_k = s.upload(np.concatenate([kx, ky]))
    d_c = s.upload(contrasts)
    d_beta = s.empty((G, P), np.float64)
    d_o = s.empty((G * (1 + 2 * K),), np.float64)
    d_E = d_w = None
    if layers:
        d_E, d_w = s.empty((G, N), np.float64, ld=pipe.ldn), s.empty((G, N), np.float64, ld=pipe.ldn)
    pipe._k("voom_wls", G, "dsq_dev_voom_wls", _vp(pipe.d_y.ptr), pipe.ldn, _vp(d_off.ptr), _vp(pipe.d_Xt.ptr), D.ldx, P,
            N, G, _vp(d_b1.ptr), _vp(d_k.ptr), _vp(d_k.ptr + 8 * len(kx)), len(kx), _vp(d_c.ptr), K, _vp(d_beta.ptr),
            _vp(d_o.ptr), _vp(d_o.ptr + 8 * G), _vp(d_o.ptr + 8 * G * (1 + K)),
            _vp(d_E.ptr) if layers else None, _vp(d_w.ptr) if layers else None, pipe.ldn if layers else 0)
    o = d_o.to_host()
    return (amean, (kx, ky), d_beta.to_host(), o[:G], o[G:G * (1 + K)].reshape(G, K), o[G * (1 + K):].reshape(G, K),
            d_E, d_w)


def voom_test(pipe, res, contrasts, lib_size, span=0.5) -> VoomResult:
    """limma's voom -> lmFit -> contrasts.fit -> eBayes of K contrasts (K x P) on the resident ORIGINAL counts of
    ``pipe``, with the library sizes ``lib_size`` (N positive numbers: ``library_sizes``).  Two launches for all K
    contrasts; the trend, the moderation and the refusals on the host.  NaN for genes without counts."""
    G, N, P = pipe.G, pipe.N, pipe.P
    check_design(N, P, pipe.design.full_rank)
    contrasts = check_contrasts(contrasts, P)
    K = contrasts.shape[0]
    off = sample_offsets(library_sizes(lib_size, N))
    with DeviceScope(pipe.ctx) as s:
        amean, knots, beta, sigma2, est, u, _, _ = _fit(pipe, s, off, contrasts, span, False)
        sq = squeeze_var(sigma2, N - P)
        live = np.nonzero(~np.isnan(sq.s2_post))[0]
        F, pv = np.full((K, G), np.nan), np.full((K, G), np.nan)
        n = len(live)
        if n > 0:
            with np.errstate(invalid="ignore", divide="ignore"):
                tu = (est[live] / u[live]) ** 2  # n x K
            d_in = s.upload(np.concatenate([tu.T.reshape(-1), sq.s2_post[live]]))
            d_o = s.empty((2 * n * K,), np.float64)
            for k in range(K):
                pipe._k("voom_score", n, "dsq_dev_ql_score", _vp(d_in.ptr + 8 * n * k), _vp(d_in.ptr + 8 * n * K), n, 1,
                        c_double(score_df(sq)), _vp(d_o.ptr + 8 * n * k), _vp(d_o.ptr + 8 * n * (K + k)))
            o = d_o.to_host()
            F[:, live], pv[:, live] = o[:n * K].reshape(K, n), o[n * K:].reshape(K, n)
    with np.errstate(invalid="ignore"):
        t = np.sign(est.T) * np.sqrt(F)
        se = np.sqrt(sq.s2_post)[None, :] * u.T
    return VoomResult(pv, t, est.T.copy(), se, sigma2, sq.s2_post, sq.df0, sq.s02, score_df(sq), beta, amean, knots)


def voom_layers(pipe, lib_size, span=0.5):
    """The voom transformation alone: (E, weights) as N x G arrays - log-CPM and the precision weights of the design of
    ``pipe`` - and the knots of the trend.  NaN columns for genes without counts."""
    G, N, P = pipe.G, pipe.N, pipe.P
    check_design(N, P, pipe.design.full_rank)
    off = sample_offsets(library_sizes(lib_size, N))
    c = np.zeros((1, P))
    c[0, 0] = 1.0
    with DeviceScope(pipe.ctx) as s:
        _, knots, _, _, _, _, d_E, d_w = _fit(pipe, s, off, c, span, True)
        E, w = d_E.to_host(), d_w.to_host()
    return np.ascontiguousarray(E[:, :N].T), np.ascontiguousarray(w[:, :N].T), knots
