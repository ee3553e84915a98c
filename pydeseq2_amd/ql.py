"""Quasi-likelihood F-test of a contrast or a nested reduced design (edgeR's glmQLFit / glmQLFTest, Lund et al. 2012;
DESIGN.md 6n), post hoc: both designs fitted at the TREND dispersion by the IRLS launcher of the LFC stage, the deviances
by k_ql_dev, the moderation of the per-gene quasi-likelihood dispersions on the host (limma's squeezeVar), F and its
p-value by k_ql_score (csrc/dsq_ql.h).  ``DeseqPipeline.ql`` delegates here."""
import ctypes as C
import math
import os
from typing import NamedTuple

import numpy as np

from ._design import DesignPack
from ._lib import DeviceScope, DsqCells, gather_rows_i32
from .lrt import check_reduced_design

_vp, c_double = C.c_void_p, C.c_double


# ---------------------------------------------------------------------------------------------------------------- host
def _polygamma(n, x):
    """psi^(n)(x) for n = 0, 1, 2 and x > 0: upward recurrence to x >= 15, then the asymptotic series (next term < 1e-18
    relative there).  Plain Python floats, the same bits on every platform."""
    s = 0.0
    while x < 15.0:
        s += (1.0 / x, 1.0 / (x * x), 2.0 / (x * x * x))[n]
        x += 1.0
    r, r2 = 1.0 / x, 1.0 / (x * x)
    if n == 0:  # ln x - 1/2x - sum B_2k / (2k x^2k)
        t = r2 * (1 / 12 - r2 * (1 / 120 - r2 * (1 / 252 - r2 * (1 / 240 - r2 * (1 / 132 - r2 * (691 / 32760 - r2 / 12))))))
        return math.log(x) - 0.5 * r - t - s
    if n == 1:  # 1/x + 1/2x^2 + sum B_2k / x^(2k+1)
        t = r2 * (1 / 6 - r2 * (1 / 30 - r2 * (1 / 42 - r2 * (1 / 30 - r2 * (5 / 66 - r2 * (691 / 2730 - r2 * 7 / 6))))))
        return r + 0.5 * r2 + r * t + s
    # -1/x^2 - 1/x^3 - sum (2k+1) B_2k / x^(2k+2)
    t = r2 * (1 / 2 - r2 * (1 / 6 - r2 * (1 / 6 - r2 * (3 / 10 - r2 * (5 / 6 - r2 * (691 / 210 - r2 * 35 / 2))))))
    return -r2 - r * r2 - r2 * t - s


def digamma(x):
    return _polygamma(0, float(x))


def trigamma(x):
    return _polygamma(1, float(x))


def trigamma_inverse(v):
    """y with trigamma(y) = v (v > 0): limma's trigammaInverse.  v > 1e7: 1 / sqrt(v); v < 1e-6: 1 / v; otherwise Newton's
    iteration on 1 / trigamma, which is convex in y and so converges monotonically from below from y = 1/2 + 1/v:
        y <- y + tri (1 - tri / v) / psi''(y),   tri = trigamma(y),
    until -step / y < 1e-8, at most 50 steps."""
    v = float(v)
    if not v > 0.0:
        raise ValueError("trigamma_inverse: the argument must be positive")
    if v > 1e7:
        return 1.0 / math.sqrt(v)
    if v < 1e-6:
        return 1.0 / v
    y = 0.5 + 1.0 / v
    for _ in range(50):
        tri = _polygamma(1, y)
        dif = tri * (1.0 - tri / v) / _polygamma(2, y)
        y += dif
        if -dif / y < 1e-8:
            break
    return y


class SqueezeVar(NamedTuple):
    s2_post: np.ndarray  # moderated dispersions, NaN where s2 is NaN
    df0: float  # prior degrees of freedom (inf: no gene-specific variability found)
    s02: float  # prior (typical) dispersion
    df_total: float  # min(df0 + df, n_used * df)
    n_used: int


def squeeze_var(s2, df) -> SqueezeVar:
    """Empirical-Bayes moderation of per-gene variances s2 on df degrees of freedom each: limma's squeezeVar / fitFDist
    without trend and without robust estimation.  Over the genes with s2 > 0 and finite:
        e = log s2 - psi(df / 2) + log(df / 2),  ebar = mean e,  v = var(e, ddof = 1) - psi'(df / 2);
        v > 0: df0 = 2 trigamma_inverse(v), s0^2 = exp(ebar + psi(df0 / 2) - log(df0 / 2));  else df0 = inf, s0^2 = exp(ebar);
        s2_post = (df0 s0^2 + df s2) / (df0 + df)   (s0^2 for df0 = inf),   df_total = min(df0 + df, n_used df).
    Sums by math.fsum: the result does not depend on the order or the blocking of a vectorised sum.  Every gene with a
    finite s2 (zero included) gets an s2_post; NaN stays NaN.  Host only."""
    s2 = np.asarray(s2, dtype=np.float64)
    df = float(df)
    if not df >= 1.0:
        raise ValueError(f"squeeze_var: the residual degrees of freedom must be at least 1 (got {df}).")
    use = np.isfinite(s2) & (s2 > 0.0)
    n = int(use.sum())
    if n < 2:
        raise ValueError(f"squeeze_var: {n} gene(s) with a positive finite dispersion; the moderation needs at least 2.")
    h = 0.5 * df
    shift = math.log(h) - digamma(h)
    e = [math.log(v) + shift for v in s2[use].tolist()]
    ebar = math.fsum(e) / n
    var = math.fsum((x - ebar) * (x - ebar) for x in e) / (n - 1)
    v = var - trigamma(h)
    if v > 0.0:
        df0 = 2.0 * trigamma_inverse(v)
        s02 = math.exp(ebar + digamma(0.5 * df0) - math.log(0.5 * df0))
    else:
        df0, s02 = math.inf, math.exp(ebar)
    if math.isinf(df0):
        post = np.where(np.isnan(s2), np.nan, s02)
    else:
        post = (df0 * s02 + df * s2) / (df0 + df)
    return SqueezeVar(post, df0, s02, min(df0 + df, n * df), n)


def score_df(sq: SqueezeVar) -> float:
    """The denominator degrees of freedom F is referred to: df_total - or infinity when df0 is infinite (no gene-specific
    variability found), where the test is F's chi-square limit chisq_sf(df_test F, df_test) and df_total's cap n_used df,
    which bounds a FINITE df0 + df, does not apply."""
    return math.inf if math.isinf(sq.df0) else sq.df_total


def null_space_reduced(X, c):
    """For a contrast vector c over the columns of the full design X (N x P): X @ Nc with Nc (P x (P - 1)) an orthonormal
    basis of c's null space - the design of the hypothesis c . beta = 0, nested in X and of rank P - 1, so that any
    contrast is testable against the full design with one numerator degree of freedom.  The basis is that of the SVD of
    c^T with each column's sign fixed (largest entry positive): deterministic.  Host only."""
    X = np.asarray(X, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    if c.shape[0] != X.shape[1]:
        raise ValueError("The contrast vector must have the same length as the design matrix.")
    if not np.isfinite(c).all() or not np.any(c != 0.0):
        raise ValueError("The contrast vector must be finite and not all zero.")
    if X.shape[1] < 2:
        raise ValueError("A contrast of a one-column design leaves no reduced design to test it against.")
    _, _, vt = np.linalg.svd(c[None, :] / np.abs(c).max(), full_matrices=True)
    Nc = vt[1:].T.copy()
    for j in range(Nc.shape[1]):
        if Nc[np.argmax(np.abs(Nc[:, j])), j] < 0.0:
            Nc[:, j] = -Nc[:, j]
    Nc[np.abs(Nc) < 1e-15] = 0.0
    return np.ascontiguousarray(X @ Nc)


def check_residual_df(N, P):
    if N - P < 1:
        raise ValueError(f"The quasi-likelihood F-test needs residual degrees of freedom: {N} samples and {P} design "
                         "columns leave none.")


def check_ql_inputs(N, P, fitted_dispersions, non_zero=None):
    """What the quasi-likelihood test needs of a fit, checked on the host before anything is launched: residual degrees
    of freedom, and trend dispersions - finite and positive on every gene with counts."""
    check_residual_df(N, P)
    if fitted_dispersions is None:
        raise ValueError("The quasi-likelihood F-test runs at the trend dispersions: this fit carries no "
                         "fitted_dispersions (it was made without a trend stage; run deseq2() or fit_dispersion_trend()).")
    fit = np.asarray(fitted_dispersions, dtype=np.float64)
    nz = np.ones(fit.shape, bool) if non_zero is None else np.asarray(non_zero, dtype=bool)
    if not (np.isfinite(fit[nz]) & (fit[nz] > 0.0)).all():
        raise ValueError("The quasi-likelihood F-test runs at the trend dispersions: fitted_dispersions is not a finite "
                         "positive number on every gene with counts.")
    return fit


class QlResult(NamedTuple):
    pvalue: np.ndarray
    F: np.ndarray
    s2: np.ndarray  # per-gene quasi-likelihood dispersion: full-model deviance / (N - P)
    s2_post: np.ndarray  # moderated
    df0: float
    s02: float
    LFC: np.ndarray  # full design at the trend dispersion, G x P, natural log
    reduced_LFC: np.ndarray  # G x P_reduced
    converged: np.ndarray  # full fit
    reduced_converged: np.ndarray
    deviance: np.ndarray  # full model's residual deviance
    num: np.ndarray  # D_reduced - D_full
    df_total: float  # the denominator degrees of freedom of the test: score_df(), infinite when df0 is
    df_test: int


def ql_test(pipe, res, reduced_design) -> QlResult:
    """Quasi-likelihood F-test of a nested reduced design on the fit ``res``, post hoc like lrt().  Both designs are fitted
    at the trend dispersions ``res.fitted_dispersions`` by dsq_dev_lfc_fit2 without epilogue, with the size factors and
    settings of fit_LFC, on the counts the final LFC was fitted on (the replaced counts of the last pass for the refitted
    genes); the final LFCs of ``res`` belong to the MAP dispersions and are not reused.  k_ql_dev gives D_r - D_f, D_f and
    s2 = D_f / (N - P), squeeze_var moderates s2 over the genes with counts, k_ql_score gives F and p - on (df_test,
    df_total) degrees of freedom, or by chisq_sf(df_test F, df_test) when the moderation ends with df0 = infinity.
    Everything that can be refused is refused on the host before the first launch; only squeeze_var's "fewer than 2 genes
    with a positive finite dispersion" needs the deviances and is raised after the fits.
    NaN for all-zero genes; genes whose counts all became zero in the refit: F 0, p 1, coefficients 0 (the Wald rule) -
    they take no part in the moderation."""
    Xr = check_reduced_design(pipe.design.X, reduced_design)
    G, N, P, ctx = pipe.G, pipe.N, pipe.P, pipe.ctx
    fit = check_ql_inputs(N, P, res.fitted_dispersions, res.non_zero)
    Dr = DesignPack(Xr, pipe.min_replicates)
    Pr = Dr.P
    nzi = np.nonzero(np.asarray(res.non_zero, dtype=bool))[0]
    nan = lambda *shape: np.full(shape, np.nan)  # noqa: E731
    num, dev, s2, F, pv = nan(G), nan(G), nan(G), nan(G), nan(G)
    beta_f, beta_r, conv_f, conv_r = nan(G, P), nan(G, Pr), nan(G), nan(G)
    refitted = np.asarray(res.refitted, dtype=bool) if res.refitted is not None else np.zeros(G, dtype=bool)
    keep = pipe._replace_keep
    if refitted.any() and (keep is None or keep["naz"] is None):
        raise RuntimeError("ql(): the replaced counts of this result's refit are gone (another pass has run since)")
    z = np.asarray(res.new_all_zeroes, dtype=bool) if res.new_all_zeroes is not None else np.zeros(G, dtype=bool)
    with DeviceScope(ctx) as s:
        d_sf = s.upload(res.size_factors, dtype=np.float64)
        d_Xr, d_pinv_r = s.upload(Dr.Xt), s.upload(Dr.pinvXt)
        cells_r = None
        if Dr.cell_path and not os.environ.get("DSQ_NO_CELL_PATH"):
            cells_r = DsqCells(s.upload(Dr.cell_of).ptr, s.upload(Dr.Xc).ptr, s.upload(Dr.XXc).ptr, int(Dr.n_design_cells))
        Df = pipe.design

        def fit_at(d_y, Gs, d_X, d_pinv, D, Pk, d_disp, cells):
            d_b, d_cv = s.empty((Gs, Pk), np.float64), s.empty((Gs,), np.uint8)
            pipe._k("ql_fit", Gs, "dsq_dev_lfc_fit2", _vp(d_y.ptr), pipe.ldn, _vp(d_sf.ptr), _vp(d_X.ptr),
                    _vp(d_pinv.ptr), D.ldx, N, Gs, Pk, int(D.full_rank), _vp(d_disp.ptr), c_double(pipe.min_mu),
                    c_double(pipe.beta_tol), c_double(-30.0), c_double(30.0), pipe.irls_maxiter, _vp(d_b.ptr), None,
                    None, _vp(d_cv.ptr), None, cells, None, None, c_double(0.0), None, None, None, None, None,
                    None, None, c_double(0.0), 0, None, None, None, None, 0)
            return d_b, d_cv

        def run(d_y, idx):
            """Both fits + deviances of the rows of d_y, which are the genes idx -> host vectors."""
            Gs = len(idx)
            d_disp = s.upload(fit[idx])
            d_bf, d_cf = fit_at(d_y, Gs, pipe.d_Xt, pipe.d_pinv, Df, P, d_disp, pipe._cells_arg())
            d_br, d_cr = fit_at(d_y, Gs, d_Xr, d_pinv_r, Dr, Pr, d_disp,
                                C.byref(cells_r) if cells_r is not None else None)
            d_out = s.empty((3 * Gs,), np.float64)
            pipe._k("ql_dev", Gs, "dsq_dev_ql_deviance", _vp(d_y.ptr), pipe.ldn, _vp(d_sf.ptr), _vp(pipe.d_Xt.ptr),
                    Df.ldx, P, _vp(d_Xr.ptr), Dr.ldx, Pr, N, Gs, _vp(d_disp.ptr), _vp(d_bf.ptr), _vp(d_br.ptr),
                    _vp(d_out.ptr), _vp(d_out.ptr + 8 * Gs), _vp(d_out.ptr + 16 * Gs))
            o = d_out.to_host()
            return (o[:Gs], o[Gs:2 * Gs], o[2 * Gs:], d_bf.to_host(), d_br.to_host(), d_cf.to_host().astype(float),
                    d_cr.to_host().astype(float))

        main = nzi[~refitted[nzi]]  # (the refitted genes run once, below, on their replaced counts)
        if len(main) > 0:
            d_y = pipe.d_y if len(main) == G else gather_rows_i32(s, ctx, pipe.d_y.ptr, pipe.ldn, main, N)
            num[main], dev[main], s2[main], beta_f[main], beta_r[main], conv_f[main], conv_r[main] = run(d_y, main)
        if refitted.any():  # their final LFC was fitted on the replaced counts: so are the two models here
            rows = np.nonzero(~keep["naz"])[0]
            gidx = (keep["rp"] if keep["nzi"] is None else keep["nzi"][keep["rp"]])[rows]
            if not np.array_equal(np.sort(gidx), np.nonzero(refitted)[0]):
                raise RuntimeError("ql(): the kept replaced counts belong to another result")
            d_y2 = gather_rows_i32(s, ctx, pipe._replace_buf.ptr, pipe.ldn, rows, N)
            num[gidx], dev[gidx], s2[gidx], beta_f[gidx], beta_r[gidx], conv_f[gidx], conv_r[gidx] = run(d_y2, gidx)
        s2_in = s2.copy()
        s2_in[z] = np.nan  # (all zero after the replacement: no data, no part in the prior)
        sq = squeeze_var(s2_in, N - P)
        live = np.nonzero(~np.isnan(sq.s2_post))[0]
        if len(live) > 0:
            d_in = s.upload(np.concatenate([num[live], sq.s2_post[live]]))
            d_o = s.empty((2 * len(live),), np.float64)
            pipe._k("ql_score", len(live), "dsq_dev_ql_score", _vp(d_in.ptr), _vp(d_in.ptr + 8 * len(live)), len(live),
                    P - Pr, c_double(score_df(sq)), _vp(d_o.ptr), _vp(d_o.ptr + 8 * len(live)))
            o = d_o.to_host()
            F[live], pv[live] = o[:len(live)], o[len(live):]
    s2_post = sq.s2_post.copy()
    if z.any():
        F[z], pv[z], beta_f[z], beta_r[z] = 0.0, 1.0, 0.0, 0.0
    return QlResult(pv, F, s2, s2_post, sq.df0, sq.s02, beta_f, beta_r, conv_f, conv_r, dev, num, score_df(sq), P - Pr)
