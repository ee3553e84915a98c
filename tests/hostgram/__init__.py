"""ctypes front-end of the TEST-ONLY host build of the sample-Gram templates (see hostgram.cpp)."""
import ctypes as C

import numpy as np

from .build import build

_lib = None
SAMPLE_MAJOR, GENE_MAJOR = 0, 1


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.hg_work_doubles.restype = C.c_size_t
    return _lib


def _p(a, t=C.c_double):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def consts():
    out = np.zeros(4, np.int32)
    lib().hg_consts(_p(out, C.c_int))
    return dict(T=int(out[0]), chunk=int(out[1]), ld=int(out[2]), target=int(out[3]))


def plan(N, K):
    out = np.zeros(6, np.int32)
    lib().hg_plan(C.c_int(N), C.c_int(K), _p(out, C.c_int))
    return dict(zip(("pad", "nt", "ntiles", "chunks", "slices", "cps"), (int(v) for v in out)))


def tile_rc(t):
    out = np.zeros(2, np.int32)
    lib().hg_tile_rc(C.c_int(t), _p(out, C.c_int))
    return int(out[0]), int(out[1])


def work_doubles(N, K):
    return int(lib().hg_work_doubles(C.c_int(N), C.c_int(K)))


def _dims(x, layout):
    return x.shape if layout == SAMPLE_MAJOR else x.shape[::-1]


def row_meanvar(x, layout=SAMPLE_MAJOR):
    """x: [N][G] (sample-major) or [G][N] (gene-major), C-contiguous.  -> mean, var"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    N, G = _dims(x, layout)
    mean, var = np.full(G, -7.0), np.full(G, -7.0)
    rc = lib().hg_row_meanvar(_p(x), C.c_int(layout), C.c_int(N), C.c_int(G), C.c_int(x.shape[1]), _p(mean), _p(var))
    assert rc == 0
    return mean, var


def sample_gram(x, layout=SAMPLE_MAJOR, sel=None, mean=None):
    """-> S [N][N] as launch_sample_gram composes it."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    N, G = _dims(x, layout)
    sel = None if sel is None else np.ascontiguousarray(sel, dtype=np.int32)
    K = G if sel is None else len(sel)
    mean = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64)
    work = np.full(max(1, work_doubles(N, K)), np.nan)
    S = np.full((N, N), np.nan)
    rc = lib().hg_sample_gram(_p(x), C.c_int(layout), C.c_int(N), C.c_int(G), C.c_int(x.shape[1]), _p(sel, C.c_int32),
                              C.c_int(K), _p(mean), _p(work), _p(S), C.c_int(N))
    assert rc == 0
    return S


def gram_dist(S):
    S = np.ascontiguousarray(S, dtype=np.float64)
    N = S.shape[0]
    D = np.full((N, N), np.nan)
    assert lib().hg_gram_dist(_p(S), C.c_int(N), C.c_int(N), _p(D), C.c_int(N)) == 0
    return D
