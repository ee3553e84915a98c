"""ctypes front-end of the TEST-ONLY host build of the quasi-likelihood templates (see hostql.cpp)."""
import ctypes as C

import numpy as np

from .build import build

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def f_sf(F, d1, d2):
    F = _f64(F)
    out = np.empty_like(F)
    assert lib().hq_f_sf(_p(F), C.c_int(F.size), C.c_int(int(d1)), C.c_double(float(d2)), _p(out)) == 0
    return out


def score(num, s2_post, df_test, df_total):
    """(F, pvalue) of ql_score, elementwise."""
    num, s2_post = _f64(num), _f64(s2_post)
    assert num.shape == s2_post.shape
    F, p = np.empty_like(num), np.empty_like(num)
    assert lib().hq_score(_p(num), _p(s2_post), C.c_int(num.size), C.c_int(int(df_test)), C.c_double(float(df_total)),
                          _p(F), _p(p)) == 0
    return F, p


def unit_deviance(y, mu, r):
    y, mu, r = np.broadcast_arrays(_f64(y), _f64(mu), _f64(r))
    y, mu, r = _f64(y), _f64(mu), _f64(r)
    out = np.empty_like(y)
    assert lib().hq_unit_deviance(_p(y), _p(mu), _p(r), C.c_int(y.size), _p(out)) == 0
    return out


def deviance(counts, sf, X, X_reduced, disp, beta, beta_reduced, wave64=False):
    """(num, deviance, s2) of samples x genes counts; wave64: the 64 lane sums added in the device's order."""
    y = np.ascontiguousarray(np.asarray(counts).T, dtype=np.int32)
    G, N = y.shape
    Xf = np.ascontiguousarray(np.asarray(X, dtype=np.float64).T)
    Xr = np.ascontiguousarray(np.asarray(X_reduced, dtype=np.float64).T)
    sf, d, bf, br = _f64(sf), _f64(disp), _f64(beta), _f64(beta_reduced)
    assert bf.shape == (G, Xf.shape[0]) and br.shape == (G, Xr.shape[0])
    num, dev, s2 = np.empty(G), np.empty(G), np.empty(G)
    rc = lib().hq_deviance(_p(y, C.c_int32), C.c_int(N), _p(sf), _p(Xf), C.c_int(N), C.c_int(Xf.shape[0]), _p(Xr),
                           C.c_int(N), C.c_int(Xr.shape[0]), C.c_int(N), C.c_int(G), _p(d), _p(bf), _p(br),
                           C.c_int(int(wave64)), _p(num), _p(dev), _p(s2))
    assert rc == 0
    return num, dev, s2
