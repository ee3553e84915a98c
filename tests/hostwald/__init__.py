"""ctypes front-end of the TEST-ONLY host build of the multi-contrast Wald templates (see hostwald.cpp)."""
import ctypes as C

import numpy as np

from .build import build

_lib = None
ALT = {None: 0, "greaterAbs": 1, "lessAbs": 2, "greater": 3, "less": 4}


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def wald_multi(X, disp, lfc, ridge, contrasts, lfc_null=0.0, alt_hypothesis=None, mu=None, sf=None, wide=False):
    """(pvalue, stat, se), each K x G, of the K x P ``contrasts``; ``mu`` (N x G) or, without it, ``sf``: mu = sf exp(X
    beta).  ``lfc_null`` on the natural-log scale.  wide: the run-time-P templates instead of the register ones."""
    Xt = np.ascontiguousarray(np.asarray(X, dtype=np.float64).T)
    P, N = Xt.shape
    b = np.ascontiguousarray(lfc, dtype=np.float64)
    G = b.shape[0]
    d = np.ascontiguousarray(disp, dtype=np.float64)
    r = np.ascontiguousarray(ridge, dtype=np.float64)
    c = np.ascontiguousarray(contrasts, dtype=np.float64)
    K = c.shape[0]
    assert b.shape == (G, P) and c.shape == (K, P) and r.shape == (P, P) and (mu is None) != (sf is None)
    m = None if mu is None else np.ascontiguousarray(np.asarray(mu, dtype=np.float64).T)
    s = None if sf is None else np.ascontiguousarray(sf, dtype=np.float64)
    out = [np.full((G, K), np.nan) for _ in range(3)]
    rc = lib().hwm_wald_multi(_p(m), C.c_int(N), _p(s), _p(Xt), C.c_int(N), C.c_int(N), C.c_int(G), C.c_int(P), _p(d),
                              _p(b), _p(r), _p(c), C.c_int(K), C.c_double(lfc_null), C.c_int(ALT[alt_hypothesis]),
                              C.c_int(int(wide)), *[_p(a) for a in out])
    assert rc == 0
    return tuple(np.ascontiguousarray(a.T) for a in out)
