"""Sample PCA and sample-to-sample distances of a transformed matrix (DESeq2's ``plotPCA(returnData = TRUE)`` and
``dist(t(assay(vsd)))``): host side.

The per-gene variances, the centred N x N Gram matrix over the selected genes and the distances run on the device
(csrc/dsq_gram.h: dsq_dev_row_meanvar, dsq_dev_sample_gram, dsq_dev_gram_dist); the selection of the most variable genes
(a stable sort of G numbers) and the eigendecomposition of the N x N Gram (``scipy.linalg.eigh``) stay on the host.
DESIGN.md 6j is the statement.

Accuracy.  Every entry of the Gram S carries an absolute error of at most ``gamma_{K+2} sum_g |x~_ig x~_jg|`` plus the
first-order term of the centring error (tests/pca_ref.py: ``gram_bound``).  A squared distance ``S_ii + S_jj - 2 S_ij``
inherits the sum of the bounds of its three entries as an ABSOLUTE error: near-duplicate samples lose relative accuracy
accordingly (two identical samples are at distance exactly 0).  Eigenvalues of the Gram carry an absolute error
proportional to ``trace(S)``: the smallest components are rounding noise; prcomp's SVD of the centred matrix would
resolve them, the Gram route cannot."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import GENE_MAJOR, SAMPLE_MAJOR, DeviceArray, DeviceScope, launch, split

_vp = C.c_void_p


@dataclass
class PcaResult:
    """``scores`` N x k (prcomp's ``$x``: U sqrt(Lambda), the entry of largest magnitude of every component positive),
    ``variance`` (``sdev^2`` = Lambda / (N - 1)), ``variance_ratio`` (plotPCA's ``percentVar`` = Lambda / trace),
    ``total_variance`` (trace / (N - 1)), ``genes`` (the genes used, in order of decreasing variance)."""
    scores: object
    variance: np.ndarray
    variance_ratio: np.ndarray
    total_variance: float
    genes: object


def select_genes(rv, ntop):
    """The first min(ntop, G) genes of R's ``order(rv, decreasing = TRUE)`` (stable: ties go to the lower index);
    ``ntop=None``: all genes in gene order.  A non-finite variance: ValueError."""
    rv = np.asarray(rv, dtype=np.float64)
    bad = np.nonzero(~np.isfinite(rv))[0]
    if len(bad):
        raise ValueError(f"pca(): the row variance of {len(bad)} gene(s) is not finite (first: gene {int(bad[0])}); "
                         f"the matrix must be finite and have at least two samples.")
    if ntop is None:
        return np.arange(len(rv), dtype=np.int32)
    return np.argsort(-rv, kind="stable")[:min(int(ntop), len(rv))].astype(np.int32)


def check_pca_args(N, G, ntop, n_components):
    """The refusals that need no data; returns K, the number of genes that will be used."""
    if N < 2:
        raise ValueError(f"pca(): at least two samples are needed (got N = {N}).")
    if ntop is not None and int(ntop) < 1:
        raise ValueError(f"pca(): ntop must be at least 1 (got {ntop}).")
    K = G if ntop is None else min(int(ntop), G)
    if n_components is not None and not 1 <= int(n_components) <= min(N, K):
        raise ValueError(f"pca(): n_components must lie in 1 ... min(N, K) = {min(N, K)} (got {n_components}).")
    return K


def pca_from_gram(S, n_components=None, genes=None):
    """``prcomp(center = TRUE, scale. = FALSE)`` through the centred N x N Gram S = X~ X~^T: S = U Lambda U^T, eigenvalues
    descending, negative rounding noise clipped to 0.  With ``n_components`` only the top of the spectrum is solved
    (``subset_by_index``); the ratios take the trace from the diagonal."""
    from scipy.linalg import eigh

    S = np.asarray(S, dtype=np.float64)
    N = S.shape[0]
    if n_components is None:
        w, U = eigh(S)
    else:
        k = int(n_components)
        if not 1 <= k <= N:
            raise ValueError(f"pca(): n_components must lie in 1 ... {N} (got {n_components}).")
        w, U = eigh(S, subset_by_index=[N - k, N - 1])
    w, U = np.maximum(w[::-1], 0.0), U[:, ::-1]
    scores = U * np.sqrt(w)
    top = np.argmax(np.abs(scores), axis=0)  # (the first on ties)
    scores = scores * np.where(scores[top, np.arange(scores.shape[1])] < 0, -1.0, 1.0)
    tr = float(np.trace(S))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = w / tr
    return PcaResult(scores, w / (N - 1), ratio, tr / (N - 1), genes)


class _Resident:
    """The matrix on the device: a host N x G array is uploaded once (sample-major) into the scope that first asks for its
    pointer, a DeviceArray is taken as it is (and stays the caller's)."""

    def __init__(self, x, layout):
        if isinstance(x, DeviceArray):
            if len(x.shape) != 2 or x.dtype != np.float64:
                raise ValueError("a DeviceArray input must be a two-dimensional float64 matrix.")
            if layout not in (SAMPLE_MAJOR, GENE_MAJOR):
                raise ValueError(f"layout must be SAMPLE_MAJOR (0) or GENE_MAJOR (1), got {layout}.")
            self.layout, self.ld, self.dev = layout, int(x.ld), x
            self.N, self.G = x.shape if layout == SAMPLE_MAJOR else x.shape[::-1]
            self.host = None
        else:
            a = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
            if a.ndim != 2:
                raise ValueError(f"the matrix must be two-dimensional, samples x genes (got shape {a.shape}).")
            self.host, self.layout, self.dev = a, SAMPLE_MAJOR, None
            self.N, self.G = a.shape
            self.ld = self.G

    def ptr(self, s):
        if self.dev is None:
            self.dev = s.upload(self.host)
        return self.dev.ptr


def _meanvar(who, s, R, want_var):
    """-> (device means, owned by the scope s; host variances or None)"""
    d_mv = s.empty((2 if want_var else 1, R.G), np.float64)
    launch(who, "row_meanvar", R.G, "dsq_dev_row_meanvar", _vp(R.ptr(s)), R.layout, R.N, R.G, R.ld, _vp(d_mv.ptr),
           _vp(d_mv.ptr + 8 * R.G) if want_var else None)
    rv = None
    if want_var:
        rv = np.empty(R.G)
        s.ctx.d2h(rv, d_mv.ptr + 8 * R.G)
    return d_mv, rv


def _gram(who, s, R, sel, d_mean):
    """-> the N x N Gram on the device (a DeviceArray of the scope s)"""
    K = R.G if sel is None else len(sel)
    d_S = s.empty((R.N, R.N), np.float64)
    d_sel = s.upload(sel, dtype=np.int32) if sel is not None and K else None
    n_work = int(s.ctx.lib.dsq_sample_gram_work_doubles(R.N, K)) if R.G else 0
    d_work = s.empty(n_work, np.float64) if n_work else None
    launch(who, "sample_gram", K, "dsq_dev_sample_gram", _vp(R.ptr(s)) if R.G else None, R.layout, R.N, R.G, R.ld,
           _vp(d_sel.ptr) if d_sel is not None else None, K, _vp(d_mean.ptr) if d_mean is not None else None,
           _vp(d_work.ptr) if d_work is not None else None, _vp(d_S.ptr), R.N)
    return d_S


def _gene_list(genes, G):
    if genes is None:
        return None
    sel = np.asarray(genes)
    if sel.ndim != 1 or (len(sel) and not np.issubdtype(sel.dtype, np.integer)):
        raise ValueError("genes: a one-dimensional list of gene indices.")
    if len(sel) and (sel.min() < 0 or sel.max() >= G):
        raise ValueError(f"genes: an index outside 0 ... {G - 1}.")
    return sel.astype(np.int32)


def row_variances(ctx, x, layout=SAMPLE_MAJOR):
    """Per-gene variance over the samples (R's ``rowVars``: two-pass, divisor N - 1; one sample: NaN) of ``x``: a host
    N x G array, or a ``DeviceArray`` in ``layout`` (SAMPLE_MAJOR: N x G, GENE_MAJOR: G x N)."""
    R = _Resident(x, layout)
    if R.N < 1:
        raise ValueError("row_variances(): at least one sample is needed.")
    if R.G == 0:
        return np.zeros(0)
    with DeviceScope(split(ctx)[1]) as s:
        return _meanvar(ctx, s, R, True)[1]


def _gram_on_device(who, s, R, sel, center):
    d_mean = _meanvar(who, s, R, False)[0] if center and R.G else None
    return _gram(who, s, R, sel, d_mean)


def sample_gram(ctx, x, genes=None, center=True, layout=SAMPLE_MAJOR):
    """The N x N Gram matrix ``X~ X~^T`` of the samples over ``genes`` (indices, in the order given; None: all), each gene
    centred by its mean over the samples unless ``center=False``.  Exactly symmetric."""
    R = _Resident(x, layout)
    if R.N < 1:
        raise ValueError("sample_gram(): at least one sample is needed.")
    sel = _gene_list(genes, R.G)
    with DeviceScope(split(ctx)[1]) as s:
        return _gram_on_device(ctx, s, R, sel, center).to_host()


def pca(ctx, x, ntop=500, n_components=None, layout=SAMPLE_MAJOR):
    """Principal components of the samples from the ``ntop`` most variable genes of ``x`` (DESeq2's ``plotPCA``:
    ``prcomp`` of the selected, centred, unscaled genes; ``ntop=None``: all genes).  ``n_components``: only the leading
    components (a partial eigensolve); None: all N.  Returns a PcaResult; ``genes`` holds the indices of the genes used in
    order of decreasing variance.  ValueError: fewer than two samples, ``ntop < 1``, ``n_components`` outside
    1 ... min(N, K), a non-finite row variance."""
    R = _Resident(x, layout)
    check_pca_args(R.N, R.G, ntop, n_components)
    if R.G == 0:
        raise ValueError("pca(): the matrix has no genes.")
    with DeviceScope(split(ctx)[1]) as s:
        d_mv, rv = _meanvar(ctx, s, R, True)
        sel = select_genes(rv, ntop)
        S = _gram(ctx, s, R, None if ntop is None else sel, d_mv).to_host()
    return pca_from_gram(S, n_components, sel)


def sample_distances(ctx, x, genes=None, layout=SAMPLE_MAJOR):
    """Euclidean distances between the samples (R's ``dist``) over ``genes`` (None: all), N x N with a zero diagonal, from
    the centred Gram (the centring cancels in a difference and conditions the Gram better); see the module docstring
    for the accuracy."""
    R = _Resident(x, layout)
    if R.N < 1:
        raise ValueError("sample_distances(): at least one sample is needed.")
    sel = _gene_list(genes, R.G)
    with DeviceScope(split(ctx)[1]) as s:
        d_S = _gram_on_device(ctx, s, R, sel, True)
        d_D = s.empty((R.N, R.N), np.float64)
        launch(ctx, "gram_dist", R.N, "dsq_dev_gram_dist", _vp(d_S.ptr), R.N, R.N, _vp(d_D.ptr), R.N)
        return d_D.to_host()
