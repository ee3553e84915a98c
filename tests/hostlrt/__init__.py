"""ctypes front-end of the TEST-ONLY host build of the likelihood-ratio templates (see hostlrt.cpp)."""
import ctypes as C

import numpy as np

from .build import build

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def chisq_sf(x, df):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    assert lib().hl_chisq_sf(_p(x, C.c_double), C.c_int(x.size), C.c_int(int(df)), _p(out, C.c_double)) == 0
    return out


def lrt(counts, sf, X, X_reduced, disp, beta, beta_reduced, wave64=False):
    """(stat, pvalue) of samples x genes counts; wave64: the 64 lane sums added in the device's order."""
    y = np.ascontiguousarray(np.asarray(counts).T, dtype=np.int32)
    G, N = y.shape
    Xf = np.ascontiguousarray(np.asarray(X, dtype=np.float64).T)
    Xr = np.ascontiguousarray(np.asarray(X_reduced, dtype=np.float64).T)
    sf = np.ascontiguousarray(sf, dtype=np.float64)
    d = np.ascontiguousarray(disp, dtype=np.float64)
    bf = np.ascontiguousarray(beta, dtype=np.float64)
    br = np.ascontiguousarray(beta_reduced, dtype=np.float64)
    assert bf.shape == (G, Xf.shape[0]) and br.shape == (G, Xr.shape[0])
    stat, p = np.empty(G), np.empty(G)
    rc = lib().hl_lrt(_p(y, C.c_int32), C.c_int(N), _p(sf, C.c_double), _p(Xf, C.c_double), C.c_int(N),
                      C.c_int(Xf.shape[0]), _p(Xr, C.c_double), C.c_int(N), C.c_int(Xr.shape[0]), C.c_int(N), C.c_int(G),
                      _p(d, C.c_double), _p(bf, C.c_double), _p(br, C.c_double), C.c_int(int(wave64)),
                      _p(stat, C.c_double), _p(p, C.c_double))
    assert rc == 0
    return stat, p
