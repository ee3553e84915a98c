"""ctypes front-end of the TEST-ONLY host build of the adaptive-shrinkage templates (see hostash.cpp)."""
import ctypes as C

import numpy as np

from .build import build

_lib = None

ONE_WAVE, WAVES4 = 1, 4


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def ash(lfc, se, grids, nw=WAVES4, max_iter=100):
    """lfc, se: K x G; grids: a list of K arrays of standard deviations (an empty one: the contrast is skipped).
    Returns a dict of K-row arrays as dsq_dev_ash writes them, and the number of passes over the genes."""
    b = np.ascontiguousarray(np.atleast_2d(lfc), dtype=np.float64)
    s = np.ascontiguousarray(np.atleast_2d(se), dtype=np.float64)
    K, G = b.shape
    assert s.shape == (K, G) and len(grids) == K
    mk = np.array([len(g) for g in grids], np.int32)
    ldm = max(1, int(mk.max()))
    sd = np.zeros((K, ldm))
    for k, g in enumerate(grids):
        sd[k, :len(g)] = g
    o = dict(pi=np.full((K, ldm), np.nan), post_mean=np.full((K, G), np.nan), post_sd=np.full((K, G), np.nan),
             lfsr=np.full((K, G), np.nan), n_iter=np.zeros(K, np.int32), converged=np.zeros(K, np.uint8),
             kkt=np.full(K, np.nan), loglik=np.full(K, np.nan), passes=np.zeros(K, np.int32))
    rc = lib().ha_ash(_p(b, C.c_double), _p(s, C.c_double), C.c_int(G), C.c_int(G), C.c_int(K), _p(sd, C.c_double),
                      _p(mk, C.c_int32), C.c_int(ldm), C.c_int(max_iter), C.c_int(nw), _p(o["pi"], C.c_double),
                      _p(o["post_mean"], C.c_double), _p(o["post_sd"], C.c_double), _p(o["lfsr"], C.c_double),
                      _p(o["n_iter"], C.c_int32), _p(o["converged"], C.c_uint8), _p(o["kkt"], C.c_double),
                      _p(o["loglik"], C.c_double), _p(o["passes"], C.c_int32))
    assert rc == 0
    o["converged"] = o["converged"].astype(bool)
    o["m"] = mk
    return o
