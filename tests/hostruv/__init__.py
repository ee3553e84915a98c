"""ctypes front-end of the TEST-ONLY host build of the hidden-batch templates (see hostruv.cpp)."""
import ctypes as C

import numpy as np

from .build import build

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def plan(N):
    """(rc, waves, staged, lds_bytes) of proj_plan(N)."""
    w, s, b = C.c_int(-1), C.c_int(-1), C.c_size_t(12345)
    rc = lib().hv_plan(C.c_int(N), C.byref(w), C.byref(s), C.byref(b))
    return rc, w.value, s.value, b.value


def log_counts(y, sf, N, normalized, eps, out):
    """y: [G][ldn] int32, out: [G][ld] float64 written in place; sf None: a null pointer (normalized false only).  -> rc"""
    assert y.dtype == np.int32 and out.dtype == np.float64 and y.flags.c_contiguous and out.flags.c_contiguous
    assert sf is not None or not normalized
    sf = np.ascontiguousarray(sf, dtype=np.float64) if sf is not None else None
    return lib().hv_log_counts(_p(y), C.c_int(y.shape[1]), _p(sf), C.c_int(N), C.c_int(y.shape[0]), C.c_int(int(normalized)),
                               C.c_double(eps), _p(out), C.c_int(out.shape[1]))


def nb_residuals(y, sf, Xt, N, disp, beta, kind, out):
    """y: [G][ldn] int32, Xt: [P][ldx], beta: [G][P], out: [G][ld] written in place.  -> rc"""
    assert y.dtype == np.int32 and out.dtype == np.float64 and y.flags.c_contiguous and out.flags.c_contiguous
    sf, Xt, disp, beta = (np.ascontiguousarray(a, dtype=np.float64) for a in (sf, Xt, disp, beta))
    return lib().hv_nb_residuals(_p(y), C.c_int(y.shape[1]), _p(sf), _p(Xt), C.c_int(Xt.shape[1]), C.c_int(Xt.shape[0]),
                                 C.c_int(N), C.c_int(y.shape[0]), _p(disp), _p(beta), C.c_int(kind), _p(out),
                                 C.c_int(out.shape[1]))


def project_out(x, Pt, Bt, N, post, eps, out, coef=None, q=None):
    """x: [G][ld], Pt / Bt: [q][ldp], out: [G][ldo] written in place (may be x), coef: [G][q] or None.  -> rc"""
    for a in (x, Pt, Bt, out):
        assert a.dtype == np.float64 and a.flags.c_contiguous
    q = Pt.shape[0] if q is None else q
    return lib().hv_project_out(_p(x), C.c_int(x.shape[1]), _p(Pt), _p(Bt), C.c_int(Pt.shape[1]), C.c_int(q), C.c_int(N),
                                C.c_int(x.shape[0]), C.c_int(post), C.c_double(eps), _p(out), C.c_int(out.shape[1]),
                                _p(coef))
