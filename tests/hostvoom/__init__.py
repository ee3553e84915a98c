"""ctypes front-end of the TEST-ONLY host build of the voom row functions (see hostvoom.cpp)."""
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


def lookup(kx, kf, lam):
    kx, kf, lam = _f64(kx), _f64(kf), _f64(lam)
    out = np.empty_like(lam)
    assert lib().hv_lookup(_p(kx), _p(kf), C.c_int(kx.size), _p(lam), C.c_int(lam.size), _p(out)) == 0
    return out


def fit1(counts, off, X, pinvXt=None):
    """(beta1 G x P, amean, sigma1) of samples x genes counts."""
    y = np.ascontiguousarray(np.asarray(counts).T, dtype=np.int32)
    G, N = y.shape
    X = np.asarray(X, dtype=np.float64)
    Xt = np.ascontiguousarray(X.T)
    pinv = np.ascontiguousarray(np.linalg.pinv(X)) if pinvXt is None else _f64(pinvXt)
    P = Xt.shape[0]
    off = _f64(off)
    b1, am, s1 = np.empty((G, P)), np.empty(G), np.empty(G)
    rc = lib().hv_fit1(_p(y, C.c_int32), C.c_int(N), _p(off), _p(Xt), _p(pinv), C.c_int(N), C.c_int(P), C.c_int(N),
                       C.c_int(G), _p(b1), _p(am), _p(s1))
    assert rc == 0
    return b1, am, s1


def wls(counts, off, X, beta1, kx, kf, contrasts, layers=False):
    """(beta G x P, sigma2, est G x K, u G x K, E, w) - E, w gene-major G x N or None."""
    y = np.ascontiguousarray(np.asarray(counts).T, dtype=np.int32)
    G, N = y.shape
    Xt = np.ascontiguousarray(np.asarray(X, dtype=np.float64).T)
    P = Xt.shape[0]
    off, b1, kx, kf = _f64(off), _f64(beta1), _f64(kx), _f64(kf)
    c = _f64(np.atleast_2d(contrasts))
    K = c.shape[0]
    beta, s2, est, u = np.empty((G, P)), np.empty(G), np.empty((G, K)), np.empty((G, K))
    E = np.empty((G, N)) if layers else None
    w = np.empty((G, N)) if layers else None
    rc = lib().hv_wls(_p(y, C.c_int32), C.c_int(N), _p(off), _p(Xt), C.c_int(N), C.c_int(P), C.c_int(N), C.c_int(G),
                      _p(b1), _p(kx), _p(kf), C.c_int(kx.size), _p(c), C.c_int(K), _p(beta), _p(s2), _p(est), _p(u),
                      _p(E) if layers else None, _p(w) if layers else None, C.c_int(N))
    assert rc == 0
    return beta, s2, est, u, E, w
