"""Hidden-batch factors (RUVSeq's RUVg and RUVr) and batch removal (limma's ``removeBatchEffect``): host side.

The three per-gene operations run on the device (csrc/dsq_proj.h: dsq_dev_log_counts, dsq_dev_nb_residuals,
dsq_dev_project_out), and so does the N x N Gram of the control genes (dsq_dev_sample_gram, pca.py).  What stays on the
host is N x N or smaller: ``eigh`` of the Gram, the choice of the factors, ``(W^T W)^-1`` and the pseudo-inverse of the
batch design.  Every refusal is decided here, before any device work.  DESIGN.md 6l is the statement; neither RUVSeq nor
limma is a measured reference.

    Y      = log(y / sf + eps)                              (log_counts)
    S      = Gram over the control genes of Y (RUVg) or of the deviance residuals (RUVr), centred per gene
    W      = the leading eigenvectors of S whose singular value the Gram route resolves
    alpha  = (W^T W)^-1 W^T Y,  Y' = Y - W alpha            (project_out with P = W (W^T W)^-1, B = W)
    counts = max(rint(exp(Y') - eps), 0)

Matrices are host arrays N x G (samples x genes) or ``DeviceArray``s in the engine's gene-major form G x N."""
import ctypes as C
import warnings
from dataclasses import dataclass

import numpy as np

from . import pca as _pca
from ._lib import DSQ_MAX_P, DSQ_PROJ_MAX_Q, GENE_MAJOR, SAMPLE_MAJOR, DeviceArray, DeviceScope, launch, split

_vp = C.c_void_p
U = 2.0 ** -52
POST = {None: 0, "exp": 1, "round": 2}
KIND = {"deviance": 0, "pearson": 1}


def gamma(n):
    """gamma_n = n u / (1 - n u), u = 2^-52."""
    return n * U / (1.0 - n * U)


@dataclass
class RuvResult:
    """``W`` N x q: the factors of unwanted variation (columns ``W_1`` ...; the façade makes it a DataFrame),
    ``singular_values``: all N of sqrt(max(lambda_i, 0)), descending, ``k_eff``: how many of the k requested the Gram route
    resolves, ``alpha`` q x G: the genes' coefficients on W, ``genes``: the control genes used, ``corrected`` N x G:
    Y' (None unless asked for), ``normalized_counts`` N x G (None unless asked for)."""
    W: object
    singular_values: np.ndarray
    k_eff: int
    alpha: object
    genes: object
    corrected: object = None
    normalized_counts: object = None


# ---------------------------------------------------------------------------------------------------------------- inputs
class _Counts:
    """int32 counts on the device, gene-major [G][ld]: a host N x G array is uploaded (transposed) into the scope that
    first asks for its pointer, a DeviceArray or a (pointer, ld, N, G) tuple of a pipeline's resident counts is taken as
    it is."""

    def __init__(self, counts):
        if isinstance(counts, tuple):
            self.ptr, self.ld, self.N, self.G = counts
        elif isinstance(counts, DeviceArray):
            if len(counts.shape) != 2 or counts.dtype != np.int32:
                raise ValueError("a DeviceArray of counts must be a two-dimensional int32 matrix, genes x samples.")
            self.ptr, self.ld = counts.ptr, int(counts.ld)
            self.G, self.N = counts.shape
        else:
            a = np.asarray(counts)
            if a.ndim != 2:
                raise ValueError(f"the counts must be two-dimensional, samples x genes (got shape {a.shape}).")
            if a.size and (not np.issubdtype(a.dtype, np.number) or (a < 0).any() or (a != np.floor(a)).any()
                           or a.max() >= 2.0 ** 31):
                raise ValueError("the counts must be non-negative integers below 2^31.")
            self.N, self.G = a.shape
            self.host = np.ascontiguousarray(a.T, dtype=np.int32)
            self.ptr, self.ld = None, self.N
        if self.N < 1:
            raise ValueError("at least one sample is needed.")

    def pointer(self, s):
        if self.ptr is None:
            self.ptr = s.upload(self.host).ptr if self.G else 0
        return self.ptr


def _size_factors(sf, N, needed=True):
    if sf is None:
        if needed:
            raise ValueError("size_factors are needed (normalized=True).")
        return None
    sf = np.ascontiguousarray(sf, dtype=np.float64)
    if sf.shape != (N,):
        raise ValueError(f"size_factors: one per sample (got shape {sf.shape} for {N} samples).")
    if not (np.isfinite(sf) & (sf > 0)).all():
        raise ValueError("the size factors must be finite and positive.")
    return sf


def _check_eps(epsilon):
    if not (np.isfinite(epsilon) and epsilon > 0):
        raise ValueError(f"epsilon must be a finite positive number (got {epsilon}).")
    return float(epsilon)


def check_q(q):
    if q > DSQ_PROJ_MAX_Q:
        raise ValueError(f"the projection takes at most DSQ_PROJ_MAX_Q = {DSQ_PROJ_MAX_Q} columns (got {q}).")


def project_plan(ctx, N):
    """(waves per workgroup, where a row stays between the passes - 2 registers, 1 LDS, 0 nowhere -, dynamic LDS bytes) of
    the projection of rows of N doubles."""
    ctx = split(ctx)[1]
    w, s, b = C.c_int(), C.c_int(), C.c_size_t()
    if ctx.lib.dsq_project_plan(int(N), C.byref(w), C.byref(s), C.byref(b)) != 0:
        raise ValueError(f"project_plan: at least one sample is needed (got N = {N}).")
    return w.value, s.value, b.value


# ------------------------------------------------------------------------------------------------------- device stages
def _dev_log_counts(who, s, cnt, sf, normalized, eps):
    """-> DeviceArray [G][N] float64 of the scope s"""
    d_out = s.empty((cnt.G, cnt.N), np.float64)
    d_sf = s.upload(sf) if sf is not None else None
    launch(who, "log_counts", cnt.G, "dsq_dev_log_counts", _vp(cnt.pointer(s)), cnt.ld,
           _vp(d_sf.ptr) if d_sf is not None else None, cnt.N, cnt.G, int(bool(normalized)), C.c_double(eps),
           _vp(d_out.ptr), cnt.N)
    return d_out


def _check_fit(N, G, design, beta, dispersions):
    X = np.asarray(design, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] != N or not 1 <= X.shape[1] <= DSQ_MAX_P:
        raise ValueError(f"design: a matrix of {N} rows and 1 ... {DSQ_MAX_P} columns (got shape {X.shape}).")
    beta = np.ascontiguousarray(beta, dtype=np.float64)
    disp = np.ascontiguousarray(dispersions, dtype=np.float64)
    if beta.shape != (G, X.shape[1]) or disp.shape != (G,):
        raise ValueError(f"beta must be {G} x {X.shape[1]} and dispersions of length {G} (got {beta.shape}, {disp.shape}).")
    return np.ascontiguousarray(X.T), beta, disp


def _dev_residuals(who, s, cnt, sf, Xt, beta, disp, kind):
    """-> DeviceArray [G][N] float64 of the scope s"""
    d_out = s.empty((cnt.G, cnt.N), np.float64)
    if cnt.G:
        d_sf, d_Xt, d_b, d_d = (s.upload(a) for a in (sf, Xt, beta, disp))
        launch(who, "nb_residuals", cnt.G, "dsq_dev_nb_residuals", _vp(cnt.pointer(s)), cnt.ld, _vp(d_sf.ptr),
               _vp(d_Xt.ptr), cnt.N, Xt.shape[0], cnt.N, cnt.G, _vp(d_d.ptr), _vp(d_b.ptr), kind, _vp(d_out.ptr), cnt.N)
    return d_out


def _check_PB(P, B, N):
    P = np.asarray(P, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    if P.ndim != 2 or B.shape != P.shape or P.shape[0] != N or P.shape[1] < 1:
        raise ValueError(f"P and B: two matrices of {N} rows and the same q >= 1 columns (got {P.shape}, {B.shape}).")
    check_q(P.shape[1])
    return np.ascontiguousarray(P.T), np.ascontiguousarray(B.T)


def _dev_project(who, s, d_x, ld, N, G, Pt, Bt, post, eps, d_out, ldo, want_coef):
    """out = x - (x P) B^T on gene-major device rows; d_out may be d_x.  -> the G x q coefficients on the host, or None"""
    q = Pt.shape[0]
    d_Pt, d_Bt = s.upload(Pt), s.upload(Bt)
    d_c = s.empty((G, q), np.float64) if want_coef and G else None
    launch(who, "project_out", G, "dsq_dev_project_out", _vp(d_x), ld, _vp(d_Pt.ptr), _vp(d_Bt.ptr), N, q, N, G,
           post, C.c_double(eps), _vp(d_out), ldo, _vp(d_c.ptr) if d_c is not None else None)
    return d_c.to_host() if d_c is not None else (np.zeros((0, q)) if want_coef else None)


class _GeneMajor:
    """A float64 matrix as gene-major device rows: a host N x G array is uploaded and transposed on the device
    (dsq_dev_f64_to_gene_major), a sample-major DeviceArray is transposed into a copy, a gene-major one is taken as it is."""

    def __init__(self, x, layout):
        R = _pca._Resident(x, layout)
        self.N, self.G = R.N, R.G
        if self.N < 1:
            raise ValueError("at least one sample is needed.")
        self._R = R

    def pointer(self, s):
        """(pointer, pitch) of the rows, which the scope s owns unless they are the caller's; call once, after every
        refusal"""
        R = self._R
        if R.layout == GENE_MAJOR:
            return R.ptr(s), R.ld
        d_gm = s.empty((self.G, self.N), np.float64)
        if self.G:
            if R.ld != self.G:
                raise ValueError("a sample-major DeviceArray must be contiguous (ld == G).")
            with DeviceScope(s.ctx) as t:  # (an uploaded sample-major copy lives until the transposition has run)
                s.ctx.call("dsq_dev_f64_to_gene_major", _vp(R.ptr(t)), SAMPLE_MAJOR, self.N, self.G, _vp(d_gm.ptr),
                           self.N)
        return d_gm.ptr, self.N


# ------------------------------------------------------------------------------------------------------- public stages
def log_counts(ctx, counts, size_factors=None, normalized=True, epsilon=1.0):
    """``log(y / sf + epsilon)`` (``normalized=False``: ``log(y + epsilon)``) of ``counts`` - a host N x G array of
    non-negative integers or an int32 ``DeviceArray`` G x N - as a host N x G array."""
    eps = _check_eps(epsilon)
    cnt = _Counts(counts)
    sf = _size_factors(size_factors, cnt.N, normalized)
    if cnt.G == 0:
        return np.zeros((cnt.N, 0))
    with DeviceScope(split(ctx)[1]) as s:
        out = _dev_log_counts(ctx, s, cnt, sf if normalized else None, normalized, eps).to_host().T
    return np.ascontiguousarray(out)


def nb_residuals(ctx, counts, size_factors, design, beta, dispersions, kind="deviance"):
    """Residuals of the NB GLM of a finished fit, N x G: ``mu = sf exp(design @ beta_g)`` (``beta`` G x P, natural log),
    ``kind="deviance"``: sign(y - mu) sqrt(D), ``"pearson"``: (y - mu) / sqrt(mu + alpha mu^2).  A gene without counts, or
    with a NaN coefficient or dispersion: NaN."""
    if kind not in KIND:
        raise ValueError(f"kind must be 'deviance' or 'pearson' (got {kind!r}).")
    cnt = _Counts(counts)
    sf = _size_factors(size_factors, cnt.N)
    Xt, beta, disp = _check_fit(cnt.N, cnt.G, design, beta, dispersions)
    if cnt.G == 0:
        return np.zeros((cnt.N, 0))
    with DeviceScope(split(ctx)[1]) as s:
        out = _dev_residuals(ctx, s, cnt, sf, Xt, beta, disp, KIND[kind]).to_host().T
    return np.ascontiguousarray(out)


def project_out(ctx, x, P, B, post=None, epsilon=1.0, layout=SAMPLE_MAJOR, return_coef=False, inplace=False):
    """``x - (x P) B^T`` for an N x G matrix ``x`` (a host array, or a ``DeviceArray`` in ``layout``) and two N x q
    matrices, q <= 64; ``post``: None, "exp" (``exp(.) - epsilon``) or "round" (``max(rint(exp(.) - epsilon), 0)``).
    Returns the N x G result (with ``return_coef``: and the G x q coefficients ``x P``).  ``inplace`` (a gene-major
    ``DeviceArray`` only): the rows are overwritten on the device and nothing but the coefficients is returned."""
    if post not in POST:
        raise ValueError(f"post must be None, 'exp' or 'round' (got {post!r}).")
    eps = _check_eps(epsilon)
    if inplace and not (isinstance(x, DeviceArray) and layout == GENE_MAJOR):
        raise ValueError("inplace: a gene-major DeviceArray only.")
    M = _GeneMajor(x, layout)
    Pt, Bt = _check_PB(P, B, M.N)
    if M.G == 0:  # (nothing to launch, as log_counts and nb_residuals)
        coef = np.zeros((0, Pt.shape[0])) if return_coef else None
        return coef if inplace else ((np.zeros((M.N, 0)), coef) if return_coef else np.zeros((M.N, 0)))
    with DeviceScope(split(ctx)[1]) as s:
        ptr, ld = M.pointer(s)
        if inplace:
            return _dev_project(ctx, s, ptr, ld, M.N, M.G, Pt, Bt, POST[post], eps, ptr, ld, return_coef)
        d_out = s.empty((M.G, M.N), np.float64)
        coef = _dev_project(ctx, s, ptr, ld, M.N, M.G, Pt, Bt, POST[post], eps, d_out.ptr, M.N, return_coef)
        out = np.ascontiguousarray(d_out.to_host().T)
    return (out, coef) if return_coef else out


# ---------------------------------------------------------------------------------------------------------------- RUV
def factors_from_gram(S, k, n_genes, drop=0):
    """The factors of unwanted variation from the N x N Gram S over ``n_genes`` control genes: d_i = sqrt(max(lambda_i,
    0)) descending, k_eff = min(k, #{i: d_i > max(1e-8, 4 d_1 sqrt(gamma_{K+2}))}) - a singular value below the second term
    is rounding noise of the Gram route - and W = U[:, drop:k_eff], the entry of largest magnitude of every
    column positive (the first on ties).  -> (W, d, k_eff); a UserWarning when k_eff < k."""
    from scipy.linalg import eigh

    S = np.asarray(S, dtype=np.float64)
    w, Um = eigh(S)
    w, Um = np.maximum(w[::-1], 0.0), Um[:, ::-1]
    d = np.sqrt(w)
    floor = max(1e-8, 4.0 * d[0] * np.sqrt(gamma(n_genes + 2)))
    k_eff = min(int(k), int(np.count_nonzero(d > floor)))
    if k_eff < k:
        warnings.warn(f"ruv(): only {k_eff} of the {k} requested factors have a singular value above the resolution of the "
                      f"Gram route ({floor:.3g}); the others are left out.", UserWarning, stacklevel=3)
    W = np.ascontiguousarray(Um[:, drop:k_eff])
    if W.shape[1]:
        top = np.argmax(np.abs(W), axis=0)
        W = W * np.where(W[top, np.arange(W.shape[1])] < 0, -1.0, 1.0)
    return W, d, k_eff


def check_ruv_args(N, G, k, controls, drop, method="g", has_counts=None):
    """The refusals that need no device work; returns the control genes as int32 indices."""
    if method not in ("g", "r"):
        raise ValueError(f"method must be 'g' (RUVg) or 'r' (RUVr), got {method!r}.")
    if int(k) != k or k < 1:
        raise ValueError(f"ruv(): k must be a positive integer (got {k}).")
    if int(drop) != drop or drop < 0 or drop >= k:
        raise ValueError(f"ruv(): drop must lie in 0 ... k - 1 = {int(k) - 1} (got {drop}).")
    if k > N:
        raise ValueError(f"ruv(): k = {k} factors from {N} samples.")
    check_q(int(k) - int(drop))
    if controls is None:
        if method == "g":
            raise ValueError("ruv(method='g') needs control genes.")
        if has_counts is None:
            raise ValueError("ruv(method='r'): which genes have counts is needed to choose the default controls.")
        sel = np.nonzero(np.asarray(has_counts, dtype=bool))[0].astype(np.int32)
    else:
        c = np.asarray(controls)
        if c.dtype == bool:
            if c.shape != (G,):
                raise ValueError(f"controls: a boolean mask of length {G}.")
            c = np.nonzero(c)[0]
        sel = _pca._gene_list(c, G)
    if len(sel) == 0:
        raise ValueError("ruv(): no control genes.")
    if method == "r" and has_counts is not None and not np.asarray(has_counts, dtype=bool)[sel].all():
        raise ValueError("ruv(method='r'): a control gene has no counts (its residuals are undefined).")
    return sel


def ruv(ctx, counts, size_factors, k, controls=None, method="g", normalized=True, epsilon=1.0, center=True, drop=0,
        return_counts=False, round=True, corrected=False, fit=None):
    """RUVg (``method="g"``) or RUVr (``"r"``) of ``counts`` (host N x G, or an int32 DeviceArray G x N): k factors of
    unwanted variation from the control genes ``controls`` (indices or a mask) of the log counts - for RUVr of the deviance
    residuals of ``fit = (design, beta, dispersions[, has_counts])``, by default over all genes with counts - and the coefficients of
    ALL genes on them.  ``return_counts``: the normalised counts (``round=False``: unrounded); ``corrected``: Y' itself.
    Returns a RuvResult.  ValueError: see check_ruv_args; fewer resolved factors than ``drop`` + 1."""
    eps = _check_eps(epsilon)
    cnt = _Counts(counts)
    N, G = cnt.N, cnt.G
    sf = _size_factors(size_factors, N, normalized or method == "r")
    has = None
    if method == "r":
        if fit is None:
            raise ValueError("ruv(method='r') needs fit = (design, beta, dispersions) of a finished pass.")
        Xt, beta, disp = _check_fit(N, G, *fit[:3])
        has = fit[3] if len(fit) > 3 else None
        if has is None and not isinstance(counts, (tuple, DeviceArray)):
            has = (cnt.host != 0).any(axis=1)
    sel = check_ruv_args(N, G, k, controls, drop, method, has)
    with DeviceScope(split(ctx)[1]) as s:
        d_Y = _dev_log_counts(ctx, s, cnt, sf if normalized else None, normalized, eps)
        d_R = _dev_residuals(ctx, s, cnt, sf, Xt, beta, disp, 0) if method == "r" else None
        R = _pca._Resident(d_R if d_R is not None else d_Y, GENE_MAJOR)
        S = _pca._gram_on_device(ctx, s, R, sel, center).to_host()
        if not np.isfinite(S).all():
            raise ValueError("ruv(): the Gram of the control genes is not finite (a control gene without a fit?).")
        W, d, k_eff = factors_from_gram(S, k, len(sel), drop)
        if W.shape[1] == 0:
            raise ValueError(f"ruv(): no factor is left (k_eff = {k_eff}, drop = {drop}).")
        Pm = W @ np.linalg.inv(W.T @ W)
        Pt, Bt = _check_PB(Pm, W, N)
        out = RuvResult(W, d, k_eff, None, sel)
        coef = None
        if return_counts:
            d_o = s.empty((G, N), np.float64)
            coef = _dev_project(ctx, s, d_Y.ptr, N, N, G, Pt, Bt, 2 if round else 1, eps, d_o.ptr, N, True)
            out.normalized_counts = np.ascontiguousarray(d_o.to_host().T)
        if corrected or coef is None:  # (in place: the log counts are not needed again)
            coef = _dev_project(ctx, s, d_Y.ptr, N, N, G, Pt, Bt, 0, eps, d_Y.ptr, N, True)
            if corrected:
                out.corrected = np.ascontiguousarray(d_Y.to_host().T)
        out.alpha = np.ascontiguousarray(coef.T)
    return out


# ------------------------------------------------------------------------------------------------------ batch removal
def _sum_to_zero(labels, N, what):
    lab = np.asarray(labels)
    if lab.shape != (N,):
        raise ValueError(f"{what}: one label per sample (got shape {lab.shape} for {N} samples).")
    levels = sorted(set(lab.tolist()))
    L = len(levels)
    X = np.zeros((N, L - 1))
    for j, lv in enumerate(levels[:-1]):
        X[lab == lv, j] = 1.0
    X[lab == levels[-1], :] = -1.0
    return X


def batch_design(N, batch=None, batch2=None, covariates=None, design=None):
    """The matrices of limma's removeBatchEffect for N samples: -> (D, X_b, blocks).  D: the terms to protect (``design``:
    an N x p matrix; None: the intercept alone).  X_b: what is removed - ``batch`` and ``batch2`` as factors in sum-to-zero
    coding over their sorted levels (L - 1 columns, the last level -1), ``covariates`` (N or N x c) centred by their
    column means.  blocks: (name, number of columns) of the parts of X_b.  ValueError: nothing to remove, a shape that
    does not fit, more than DSQ_PROJ_MAX_Q columns, or F = [D | X_b] rank deficient (the dependent block is named)."""
    D = np.ones((N, 1)) if design is None else np.asarray(design, dtype=np.float64)
    if D.ndim != 2 or D.shape[0] != N:
        raise ValueError(f"design: a matrix of {N} rows (got shape {D.shape}).")
    parts = []
    if batch is not None:
        parts.append(("batch", _sum_to_zero(batch, N, "batch")))
    if batch2 is not None:
        parts.append(("batch2", _sum_to_zero(batch2, N, "batch2")))
    if covariates is not None:
        c = np.asarray(covariates, dtype=np.float64)
        c = c[:, None] if c.ndim == 1 else c
        if c.ndim != 2 or c.shape[0] != N:
            raise ValueError(f"covariates: {N} rows (got shape {c.shape}).")
        if not np.isfinite(c).all():
            raise ValueError("covariates must be finite.")
        parts.append(("covariates", c - c.mean(axis=0)))
    parts = [(n, x) for n, x in parts if x.shape[1]]
    if not parts:
        raise ValueError("remove_batch_effect(): nothing to remove (give batch, batch2 or covariates; a factor needs two levels).")
    Xb = np.hstack([x for _, x in parts])
    check_q(Xb.shape[1])
    if not np.isfinite(D).all():
        raise ValueError("design must be finite.")
    rank = np.linalg.matrix_rank
    if D.shape[1] and rank(D) < D.shape[1]:
        raise ValueError("remove_batch_effect(): the design is rank deficient by itself.")
    F = D
    for name, x in parts:
        F2 = np.hstack([F, x])
        if rank(F2) < F2.shape[1]:
            raise ValueError(f"remove_batch_effect(): [design | batch terms] is rank deficient: the columns of {name!r} "
                             f"depend on the design or on the terms before them.")
        F = F2
    return D, Xb, [(n, x.shape[1]) for n, x in parts]


def batch_projection(D, Xb):
    """P = the X_b columns of pinv([D | X_b])^T (N x q) and B = X_b: X - (X P) B^T takes the fitted batch terms out."""
    F = np.hstack([D, Xb])
    return np.ascontiguousarray(np.linalg.pinv(F).T[:, D.shape[1]:]), np.ascontiguousarray(Xb)


def remove_batch_effect(ctx, x, batch=None, batch2=None, covariates=None, design=None, layout=SAMPLE_MAJOR):
    """limma's ``removeBatchEffect`` of an N x G matrix (host array, or a DeviceArray in ``layout``): per gene the least
    squares fit of [design | batch terms], and the fitted batch terms subtracted.  See batch_design.  -> N x G."""
    M = _GeneMajor(x, layout)
    D, Xb, _ = batch_design(M.N, batch, batch2, covariates, design)
    P, B = batch_projection(D, Xb)
    Pt, Bt = _check_PB(P, B, M.N)
    if M.G == 0:
        return np.zeros((M.N, 0))
    with DeviceScope(split(ctx)[1]) as s:
        ptr, ld = M.pointer(s)
        d_out = s.empty((M.G, M.N), np.float64)
        _dev_project(ctx, s, ptr, ld, M.N, M.G, Pt, Bt, 0, 1.0, d_out.ptr, M.N, False)
        return np.ascontiguousarray(d_out.to_host().T)
