"""ctypes front-end of the TEST-ONLY host build of the rank-sum templates (see hostrank.cpp)."""
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


def plan(L):
    """(rc, waves, lds_bytes) of rank_plan(L)."""
    w, b = C.c_int(-1), C.c_size_t(12345)
    rc = lib().hr_plan(C.c_int(L), C.byref(w), C.byref(b))
    return rc, w.value, b.value


def check_layout(order, seg, pad, S, N, cap_strata=None, cap_order=None):
    """None, or the message rank_check_layout refuses the layout with."""
    order, seg, pad = (np.ascontiguousarray(a, dtype=np.int32) for a in (order, seg, pad))
    why = C.c_char_p()
    rc = lib().hr_check_layout(_p(order, C.c_int32), _p(seg, C.c_int32), _p(pad, C.c_int32), C.c_int(S),
                               C.c_int(len(seg) - 1 if cap_strata is None else cap_strata),
                               C.c_int(len(order) if cap_order is None else cap_order), C.c_int(N), C.byref(why))
    assert (rc == 0) == (why.value is None)
    return None if rc == 0 else why.value.decode()


def ranksum(y, ldn, sf, N, packed, alt):
    """y: [G][ldn] int32; packed: pydeseq2_amd.ranktest.PackedLayouts; alt: dsq_alt's code.  (rc, dict of K x G arrays)."""
    y = np.ascontiguousarray(y, dtype=np.int32)
    sf = np.ascontiguousarray(sf, dtype=np.float64)
    G, K = y.shape[0], len(packed.nstrata)
    o = {k: np.full((K, G), np.nan) for k in ("stat", "pvalue", "usum", "ties")}
    rc = lib().hr_ranksum(_p(y, C.c_int32), C.c_int(ldn), _p(sf, C.c_double), C.c_int(N), C.c_int(G), C.c_int(K),
                          _p(packed.order, C.c_int32), C.c_int(packed.ldo), _p(packed.seg, C.c_int32),
                          _p(packed.pad, C.c_int32), C.c_int(packed.lds), _p(packed.nstrata, C.c_int32),
                          _p(packed.labels, C.c_int8), C.c_int(packed.ldl), C.c_int(alt), _p(o["stat"], C.c_double),
                          _p(o["pvalue"], C.c_double), _p(o["usum"], C.c_double), _p(o["ties"], C.c_double), C.c_int(G))
    return rc, o
