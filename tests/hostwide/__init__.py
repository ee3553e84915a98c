"""ctypes front-end of the TEST-ONLY host build of the run-time-P templates over the workspace of the designs wider
than 48 columns (see hostwide.cpp).  Same calling conventions as tests/hostsim's *_wide entry points."""
import ctypes as C

import numpy as np

from tests.hostsim import cell_plan, design_pack, gene_major

from .build import build

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def mom(counts, sf, X, min_disp, max_disp, min_mu=0.5):
    y = gene_major(counts)
    G, N = y.shape
    Xt, pinv, _ = design_pack(X)
    sf = np.ascontiguousarray(sf, dtype=np.float64)
    out = [np.empty(G) for _ in range(4)]
    mu = np.empty((G, N))
    rc = lib().hw_mom(_p(y, C.c_int32), C.c_int(N), _p(sf, C.c_double), _p(Xt, C.c_double), _p(pinv, C.c_double),
                      C.c_int(N), C.c_int(N), C.c_int(G), C.c_int(Xt.shape[0]), C.c_double(min_disp),
                      C.c_double(max_disp), C.c_double(min_mu), *[_p(a, C.c_double) for a in out], _p(mu, C.c_double))
    assert rc == 0
    return dict(normed_mean=out[0], rough=out[1], moments=out[2], mom=out[3], lin_mu=mu.T)


def alpha_mle(counts, X, mu, alpha_hat, min_disp, max_disp, prior_var=None, cr_reg=True, prior_reg=False):
    y = gene_major(counts)
    G, N = y.shape
    m = np.ascontiguousarray(np.asarray(mu, dtype=np.float64).T)
    Xt, _, _ = design_pack(X)
    ah = np.ascontiguousarray(alpha_hat, dtype=np.float64)
    out, conv = np.empty(G), np.empty(G, np.uint8)
    rc = lib().hw_alpha_mle(_p(y, C.c_int32), _p(m, C.c_double), C.c_int(N), _p(Xt, C.c_double), C.c_int(N),
                            C.c_int(N), C.c_int(G), C.c_int(Xt.shape[0]), _p(ah, C.c_double), C.c_double(min_disp),
                            C.c_double(max_disp), C.c_double(prior_var if prior_var is not None else 1.0),
                            C.c_int(cr_reg), C.c_int(prior_reg), _p(out, C.c_double), _p(conv, C.c_uint8))
    assert rc == 0
    return out, conv.astype(bool)


def lfc_fit(counts, sf, X, disp, robust_disp=None, cutoff=0.0, contrast=None, lfc_null=0.0, alt=0, min_replicates=7,
            maxiter=250):
    """IRLS (+ L-BFGS-B rescue) and the fused epilogue: Cook's bookkeeping if robust_disp is given, Wald if contrast is.
    A small maxiter sends every gene through the rescue (utils.py:374-413)."""
    y = gene_major(counts)
    G, N = y.shape
    Xt, pinv, fr = design_pack(X)
    P = Xt.shape[0]
    sf = np.ascontiguousarray(sf, dtype=np.float64)
    d = np.ascontiguousarray(disp, dtype=np.float64)
    _, _, _, _, flags = cell_plan(X, min_replicates)
    beta, conv = np.empty((G, P)), np.empty(G, np.uint8)
    mu, H = np.empty((G, N)), np.empty((G, N))
    ck = np.empty((G, N)) if robust_disp is not None else None
    fl = [np.empty(G, np.uint8) for _ in range(4)]
    pv, st, se = np.empty(G), np.empty(G), np.empty(G)
    rd = np.ascontiguousarray(robust_disp, dtype=np.float64) if robust_disp is not None else None
    ridge = np.ascontiguousarray(np.diag(np.repeat(1e-6, P))) if contrast is not None else None
    cvec = np.ascontiguousarray(contrast, dtype=np.float64) if contrast is not None else None
    rc = lib().hw_lfc_fit(_p(y, C.c_int32), C.c_int(N), _p(sf, C.c_double), _p(Xt, C.c_double), _p(pinv, C.c_double),
                          C.c_int(N), C.c_int(N), C.c_int(G), C.c_int(P), _p(d, C.c_double), C.c_double(0.5),
                          C.c_double(1e-8), C.c_int(fr), _p(rd, C.c_double),
                          _p(flags, C.c_uint8) if rd is not None else None, C.c_double(cutoff), _p(ck, C.c_double),
                          *[_p(a, C.c_uint8) for a in fl], _p(ridge, C.c_double), _p(cvec, C.c_double),
                          C.c_double(lfc_null), C.c_int(alt), _p(beta, C.c_double), _p(mu, C.c_double),
                          _p(H, C.c_double), _p(conv, C.c_uint8), _p(pv, C.c_double), _p(st, C.c_double),
                          _p(se, C.c_double), C.c_int(maxiter))
    assert rc == 0
    out = dict(beta=beta, conv=conv.astype(bool), p=pv, stat=st, se=se, mu=mu.T, H=H.T)
    if ck is not None:
        out["cooks"] = ck.T
    return out
