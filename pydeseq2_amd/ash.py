"""Adaptive shrinkage of log fold changes (Stephens' ashr, as DESeq2's ``lfcShrink(type="ashr")`` calls it): host side.

The grid of the mixture's standard deviations (``ashr::autoselect.mixsd``) and the s-values (``qval.from.lfdr`` of the
local false sign rates) are a few numpy lines per contrast; the fit of the mixture proportions over all genes and the
per-gene posterior run on the device (csrc/dsq_ash.h, dsq_dev_ash).  DESIGN.md 6i is the statement of the algorithm."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

ASH_MAX_M = 48  # DSQ_ASH_MAX_M
MAX_ITER = 100
_vp = C.c_void_p


def used_genes(b, s):
    """A gene takes part if its LFC and SE are finite and the SE is positive."""
    b, s = np.asarray(b, dtype=np.float64), np.asarray(s, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(b) & np.isfinite(s) & (s > 0)


def mixsd_grid(b, s, mult=np.sqrt(2.0), max_m=ASH_MAX_M):
    """Standard deviations of the mixture components for LFCs ``b`` with standard errors ``s`` (``autoselect.mixsd`` with
    mode 0 and no point mass): ``mult^e sigma_max`` for e over R's ``(-npoint):0``, which counts DOWN when npoint is
    negative.  No used gene: an empty grid.  More than ``max_m`` components: ValueError."""
    b, s = np.asarray(b, dtype=np.float64), np.asarray(s, dtype=np.float64)
    u = used_genes(b, s)
    if not u.any():
        return np.zeros(0)
    b, s = b[u], s[u]
    smin = s.min() / 10.0
    d = b * b - s * s
    smax = 2.0 * np.sqrt(d.max()) if (d > 0).any() else 8.0 * smin
    npoint = int(np.ceil(np.log2(smax / smin) / np.log2(mult)))
    if abs(npoint) + 1 > max_m:
        raise ValueError(f"ash: the grid of this contrast has {abs(npoint) + 1} mixture components; at most {max_m} "
                         f"(DSQ_ASH_MAX_M) are supported.")
    e = np.arange(-npoint, 1) if npoint >= 0 else np.arange(-npoint, -1, -1)
    return mult ** e.astype(np.float64) * smax


def svalues(lfsr):
    """s-values: over the genes with an lfsr, in ascending order of it (stable), the running mean; NaN elsewhere."""
    lfsr = np.asarray(lfsr, dtype=np.float64)
    out = np.full(lfsr.shape, np.nan)
    idx = np.nonzero(~np.isnan(lfsr))[0]
    if len(idx):
        o = idx[np.argsort(lfsr[idx], kind="stable")]
        out[o] = np.cumsum(lfsr[o]) / np.arange(1, len(o) + 1)
    return out


@dataclass
class AshResult:
    """Row k: contrast k.  ``pi`` / ``grid``: lists of K vectors (their lengths differ)."""
    post_mean: np.ndarray
    post_sd: np.ndarray
    lfsr: np.ndarray
    svalue: np.ndarray
    pi: list
    grid: list
    n_iter: np.ndarray
    converged: np.ndarray
    kkt: np.ndarray
    loglik: np.ndarray


def ash(pipe, lfc, se, grids=None, max_iter=MAX_ITER):
    """Adaptive shrinkage of K contrasts (``lfc``, ``se``: K x G, or one vector each) on the device of ``pipe`` (a
    DeseqPipeline, or a ``_lib.Context``): one upload, dsq_dev_ash (the fit and the posterior kernel), one download.
    ``grids``: the K grids (default: ``mixsd_grid`` of each contrast).  A contrast without used genes gets NaN everywhere."""
    from ._lib import DeviceScope, launch, split

    b = np.ascontiguousarray(np.atleast_2d(np.asarray(lfc, dtype=np.float64)))
    s = np.ascontiguousarray(np.atleast_2d(np.asarray(se, dtype=np.float64)))
    if b.shape != s.shape or b.ndim != 2:
        raise ValueError(f"ash(): lfc and se must have the same K x G shape (got {b.shape} and {s.shape}).")
    K, G = b.shape
    if grids is None:
        grids = [mixsd_grid(b[k], s[k]) for k in range(K)]
    grids = [np.asarray(g, dtype=np.float64) for g in grids]
    if len(grids) != K:
        raise ValueError("ash(): one grid per contrast.")
    mk = np.array([len(g) for g in grids], np.int32)
    if mk.max(initial=0) > ASH_MAX_M:
        raise ValueError(f"ash(): at most {ASH_MAX_M} (DSQ_ASH_MAX_M) mixture components per contrast.")
    for k in range(K):  # (a grid for a contrast without used genes: nothing to fit)
        if mk[k] and not used_genes(b[k], s[k]).any():
            mk[k] = 0
    ldm = max(1, int(mk.max(initial=0)))
    sd = np.zeros((K, ldm))
    for k in range(K):
        sd[k, :mk[k]] = grids[k][:mk[k]]
    nan = np.full((K, G), np.nan)
    res = AshResult(nan.copy(), nan.copy(), nan.copy(), nan.copy(), [np.full(len(g), np.nan) for g in grids], grids,
                    np.zeros(K, np.int32), np.zeros(K, bool), np.full(K, np.nan), np.full(K, np.nan))
    if G == 0 or K == 0 or not mk.any():
        return res
    # one buffer each way: doubles first, then the int32 and uint8 vectors
    in_d = np.concatenate([b.ravel(), s.ravel(), sd.ravel()])
    h_in = np.concatenate([in_d.view(np.uint8), mk.view(np.uint8)])
    n_out_d = K * ldm + 3 * K * G + 2 * K
    h_out = np.zeros(8 * n_out_d + 4 * K + K, np.uint8)
    h_out[:8 * n_out_d].view(np.float64)[:] = np.nan  # (a skipped contrast's outputs are not written)
    with DeviceScope(split(pipe)[1]) as sc:
        d_in, d_out = sc.upload(h_in), sc.upload(h_out)
        i0, o0 = d_in.ptr, d_out.ptr
        o_pi, o_pm, o_ps, o_fs = o0, o0 + 8 * K * ldm, o0 + 8 * (K * ldm + K * G), o0 + 8 * (K * ldm + 2 * K * G)
        o_kkt = o0 + 8 * (K * ldm + 3 * K * G)
        o_ll, o_it = o_kkt + 8 * K, o0 + 8 * n_out_d
        launch(pipe, "ash", K * G, "dsq_dev_ash", _vp(i0), _vp(i0 + 8 * K * G), G, G, K, _vp(i0 + 16 * K * G),
               _vp(i0 + 8 * in_d.size), ldm, int(max_iter), _vp(o_pi), _vp(o_pm), _vp(o_ps), _vp(o_fs), _vp(o_it),
               _vp(o_it + 4 * K), _vp(o_kkt), _vp(o_ll))
        out = d_out.to_host()
    od = out[:8 * n_out_d].view(np.float64)
    pi = od[:K * ldm].reshape(K, ldm)
    res.post_mean, res.post_sd, res.lfsr = (od[K * ldm + j * K * G:K * ldm + (j + 1) * K * G].reshape(K, G).copy()
                                            for j in range(3))
    res.kkt, res.loglik = od[K * ldm + 3 * K * G:][:K].copy(), od[K * ldm + 3 * K * G + K:][:K].copy()
    res.n_iter = out[8 * n_out_d:8 * n_out_d + 4 * K].view(np.int32).copy()
    res.converged = out[8 * n_out_d + 4 * K:].astype(bool)
    res.pi = [pi[k, :mk[k]].copy() if mk[k] else np.full(len(grids[k]), np.nan) for k in range(K)]
    res.svalue = np.stack([svalues(res.lfsr[k]) for k in range(K)])
    return res
