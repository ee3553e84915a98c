"""Wald tests (``DeseqStats.run_wald_test``, pydeseq2/ds.py:303-360) of a finished fit, post hoc: one contrast
(dsq_dev_wald) or K contrasts in one launch (dsq_dev_wald_multi).  ``DeseqPipeline.wald`` / ``wald_multi`` delegate here."""
import ctypes as C

import numpy as np

from ._lib import ALT, DeviceScope

_vp, c_double = C.c_void_p, C.c_double


def _inputs(pipe, res, contrasts, multi, lfc_null, alt_hypothesis, lfc, ridge):
    """Every refusal, the default ridge and the host arrays of both tests -> (contrasts, ridge, (size factors,
    coefficients, dispersions)); the three are uploaded by the caller, once its scope is open."""
    if alt_hypothesis not in ALT:
        raise KeyError(alt_hypothesis)
    if lfc_null < 0 and alt_hypothesis in {"greaterAbs", "lessAbs"}:
        raise ValueError(f"The alternative hypothesis being {alt_hypothesis}, please provide a "
                         f"positive lfc_null value (got {lfc_null}).")
    P = pipe.P
    contrasts = np.ascontiguousarray(contrasts, dtype=np.float64)
    if multi:
        if contrasts.ndim != 2:
            raise ValueError("wald_multi() takes a K x P matrix of contrasts; use wald() for a single contrast vector.")
        if contrasts.shape[0] < 1 or contrasts.shape[1] != P:
            raise ValueError(f"contrasts must be K x {P} with K >= 1 (got {contrasts.shape[0]} x {contrasts.shape[1]}).")
    ridge = np.ascontiguousarray(np.diag(np.repeat(1e-6, P)) if ridge is None else ridge, dtype=np.float64)
    host = tuple(np.ascontiguousarray(a, dtype=np.float64)
                 for a in (res.size_factors, res.LFC if lfc is None else lfc, res.dispersions))
    return contrasts, ridge, host


def wald(pipe, res, contrast, lfc_null=0.0, alt_hypothesis=None, lfc=None, ridge=None):
    """Wald test only (ds.py:303-360) on the dispersions / LFCs of ``res`` (e.g. another contrast or
    alternative hypothesis after ``deseq2()``; ``lfc``: other coefficients, e.g. shrunk ones; ``ridge``: other
    ridge matrix, ds.py:326-334).  Returns (pvalue, stat, lfcSE), NaN for all-zero genes."""
    contrast, ridge, host = _inputs(pipe, res, contrast, False, lfc_null, alt_hypothesis, lfc, ridge)
    G, N, P, D = pipe.G, pipe.N, pipe.P, pipe.design
    with DeviceScope(pipe.ctx) as s:
        d_sf, d_beta, d_disp = (s.upload(a) for a in host)
        d_out = s.empty((3 * G,), np.float64)
        pipe.ctx.call("dsq_dev_wald", None, pipe.ldn, _vp(d_sf.ptr), _vp(pipe.d_Xt.ptr), D.ldx, N, G, P, _vp(d_disp.ptr),
                      _vp(d_beta.ptr), _vp(ridge.ctypes.data), _vp(contrast.ctypes.data), c_double(np.log(2) * lfc_null),
                      ALT[alt_hypothesis], _vp(d_out.ptr), _vp(d_out.ptr + 8 * G), _vp(d_out.ptr + 16 * G))
        o = d_out.to_host()
    pv, st, se = o[:G].copy(), o[G:2 * G].copy(), o[2 * G:].copy()
    z = np.asarray(res.new_all_zeroes, dtype=bool)
    if z.any():  # ds.py:357-360
        se[z], st[z], pv[z] = 0.0, 0.0, 1.0
    return pv, st, se


def wald_multi(pipe, res, contrasts, lfc_null=0.0, alt_hypothesis=None, lfc=None, ridge=None):
    """Wald tests of K contrasts of the same fit (``contrasts``: K x P) in one launch: per gene X^T W X is accumulated
    and factored once (k_wald_multi / k_wald_multi_wide), only the per-contrast tail repeats.  One upload of size
    factors, coefficients and dispersions, one download.  Arguments as wald(); returns (pvalue, stat, lfcSE), each
    K x G, row k what wald(res, contrasts[k], ...) returns.  (Single process: DistributedDeseq has no counterpart.)"""
    contrasts, ridge, host = _inputs(pipe, res, contrasts, True, lfc_null, alt_hypothesis, lfc, ridge)
    G, N, P, D, K = pipe.G, pipe.N, pipe.P, pipe.design, contrasts.shape[0]
    with DeviceScope(pipe.ctx) as s:
        d_sf, d_beta, d_disp = (s.upload(a) for a in host)
        d_con = s.upload(contrasts)
        d_out = s.empty((3 * G * K,), np.float64)
        pipe.ctx.call("dsq_dev_wald_multi", None, pipe.ldn, _vp(d_sf.ptr), _vp(pipe.d_Xt.ptr), D.ldx, N, G, P,
                      _vp(d_disp.ptr), _vp(d_beta.ptr), _vp(ridge.ctypes.data), _vp(d_con.ptr), K,
                      c_double(np.log(2) * lfc_null), ALT[alt_hypothesis], _vp(d_out.ptr), _vp(d_out.ptr + 8 * G * K),
                      _vp(d_out.ptr + 16 * G * K))
        o = d_out.to_host().reshape(3, G, K)
    pv, st, se = (np.ascontiguousarray(o[i].T) for i in range(3))
    z = np.asarray(res.new_all_zeroes, dtype=bool)
    if z.any():  # ds.py:357-360
        se[:, z], st[:, z], pv[:, z] = 0.0, 0.0, 1.0
    return pv, st, se
