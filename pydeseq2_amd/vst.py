"""Variance-stabilising transformation (pydeseq2/dds.py:440-514), post hoc: of the resident counts, or of new samples
with the training fit.  ``DeseqPipeline.vst_transform`` / ``vst_transform_new`` delegate here."""
import ctypes as C

import numpy as np

from ._lib import I32, I64, DeviceScope

_vp, c_double = C.c_void_p, C.c_double


def _dev_vst(s, d_counts, count_type, N, G, d_sf, trend_coeffs, mean_disp):
    """The closed form on N x G counts -> the host matrix"""
    if trend_coeffs is not None:
        mode, a0, a1 = 0, float(trend_coeffs[0]), float(trend_coeffs[1])
    else:
        mode, a0, a1 = 1, float(mean_disp), 0.0
    d_out = s.empty((N, G), np.float64)
    s.ctx.call("dsq_dev_vst", _vp(d_counts.ptr), count_type, N, G, _vp(d_sf.ptr), mode, c_double(a0), c_double(a1),
               _vp(d_out.ptr))
    return d_out.to_host()


def vst_transform(pipe, size_factors, trend_coeffs=None, mean_disp=None):
    """Variance-stabilised counts N x G (dds.py:440-514) from the resident raw counts."""
    with DeviceScope(pipe.ctx) as s:
        d_sf = s.upload(size_factors, dtype=np.float64)
        return _dev_vst(s, pipe.d_raw, pipe._count_type, pipe.N, pipe.G, d_sf, trend_coeffs, mean_disp)


def vst_transform_new(pipe, counts, logmeans, filtered, trend_coeffs=None, mean_disp=None):
    """Variance-stabilised NEW samples (M x G): their size factors are the medians of
    log(count) - training logmeans over the training-usable genes (preprocessing.py:59-102 as called from
    dds.py:471-484), then the same closed form."""
    ctx = pipe.ctx
    counts = np.ascontiguousarray(counts if counts.dtype in (np.int32, np.int64) else counts.astype(np.int64))
    M, G = counts.shape
    if G != pipe.G:
        raise ValueError("new counts must have the genes of the fitted dataset")
    ct = I32 if counts.dtype == np.int32 else I64
    lm = np.where(np.asarray(filtered, dtype=bool), np.asarray(logmeans, dtype=float), -np.inf)
    with DeviceScope(ctx) as s:
        d_c, d_lm = s.upload(counts), s.upload(lm)
        d_work = s.empty((ctx.lib.dsq_size_factors_work_doubles(M, G),), np.float64)
        d_sf = s.empty((M,), np.float64)
        ctx.call("dsq_dev_size_factors_new", _vp(d_c.ptr), ct, M, G, _vp(d_lm.ptr), None, _vp(d_work.ptr), _vp(d_sf.ptr))
        return _dev_vst(s, d_c, ct, M, G, d_sf, trend_coeffs, mean_disp)
