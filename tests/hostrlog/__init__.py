"""ctypes front-end of the TEST-ONLY host build of the regularized-log templates (see hostrlog.cpp)."""
import ctypes as C

import numpy as np

from .build import build

_lib = None

ONE_LANE, WAVE64, WAVE64_ROW = 0, 1, 2


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def rlog(counts, sf, disp, base_mean, beta_prior_var, mode=ONE_LANE):
    """samples x genes counts -> (rlog N x G log2, intercept, converged, n_iter); mode: ONE_LANE, WAVE64 (64 lanes in the
    device's order, the device's choice between registers and the output row) or WAVE64_ROW."""
    y = np.ascontiguousarray(np.asarray(counts).T, dtype=np.int32)
    G, N = y.shape
    sf = np.ascontiguousarray(sf, dtype=np.float64)
    d = np.ascontiguousarray(disp, dtype=np.float64)
    bm = np.ascontiguousarray(base_mean, dtype=np.float64)
    assert sf.shape == (N,) and d.shape == (G,) and bm.shape == (G,)
    out, b0 = np.full((G, N), np.nan), np.full(G, np.nan)
    conv, it = np.zeros(G, np.uint8), np.zeros(G, np.int32)
    rc = lib().hr_rlog(_p(y, C.c_int32), C.c_int(N), _p(sf, C.c_double), C.c_int(N), C.c_int(G), _p(d, C.c_double),
                       _p(bm, C.c_double), C.c_double(beta_prior_var), C.c_int(mode), _p(out, C.c_double),
                       _p(b0, C.c_double), _p(conv, C.c_uint8), _p(it, C.c_int32))
    assert rc == 0
    return np.ascontiguousarray(out.T), b0, conv.astype(bool), it
