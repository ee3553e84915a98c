"""References for the device unit tests of the p x p algebra (tests/test_devunit_gram.py, tests/test_devunit_linalg.py).

mpmath at 120 bits is the ground truth, and dot products of doubles in it cost microseconds per term: the shapes of
those tests hold 10^8 terms.  So the full arrays are compared with double-double sums built from error-free
transformations (Dekker's split and product, Knuth's two-sum: every product of two doubles is held exactly, a sum of N
terms carries a relative error of about N 2^-104), vectorised over genes and entries, and `mp_dot` recomputes sampled
entries in mpmath to show both that the double-double value agrees with it to 2^-95 of the sum of absolute terms and that
the device result meets its bound against mpmath itself."""
import mpmath
import numpy as np

U = 2.0**-53
MP_PREC = 120


def gamma(k):
    """gamma_k = k u / (1 - k u)"""
    return k * U / (1.0 - k * U)


def _split(a):
    c = 134217729.0 * a  # 2^27 + 1
    h = c - (c - a)
    return h, a - h


def _two_prod(a, b, sa=None, sb=None):
    ah, al = sa if sa is not None else _split(a)
    bh, bl = sb if sb is not None else _split(b)
    p = a * b
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def dd_dot(Uk, Vk, w=None):
    """sum_k Uk[g, k, i] Vk[g, k, j] (w[g, k]) -> (hi, lo, sum of absolute terms), each [G, I, J]; hi + lo is the sum
    to double-double accuracy.  Vk may also be [G, K, 1] against Uk [G, K, I] (matrix-vector shapes)."""
    Uk, Vk = np.asarray(Uk, np.float64), np.asarray(Vk, np.float64)
    G, K = Uk.shape[:2]
    su, sv = _split(Uk), _split(Vk)
    sw = _split(w) if w is not None else None
    shape = np.broadcast_shapes(Uk[:, 0, :, None].shape, Vk[:, 0, None, :].shape)
    hi, lo, ab = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    with np.errstate(all="ignore"):
        for k in range(K):
            u, v = Uk[:, k, :, None], Vk[:, k, None, :]
            ph, pl = _two_prod(u, v, (su[0][:, k, :, None], su[1][:, k, :, None]),
                               (sv[0][:, k, None, :], sv[1][:, k, None, :]))
            if w is None:
                parts = (ph, pl)
                ab += np.abs(ph)
            else:
                wk = w[:, k, None, None]
                a, b = _two_prod(ph, wk, None, (sw[0][:, k, None, None], sw[1][:, k, None, None]))
                parts = (a, b, pl * wk)
                ab += np.abs(a)
            for t in parts:
                hi, e = _two_sum(hi, t)
                lo += e
    return hi, lo, ab


def dd_gram_tri(X, w):
    """sum_n X[g, n, i] X[g, n, j] w[g, n] for the lower triangle only -> (hi, lo, sum of absolute terms, (i, j)),
    each [G, P (P + 1) / 2] in np.tril_indices order: half the work of dd_dot(X, X, w)"""
    X, w = np.asarray(X, np.float64), np.asarray(w, np.float64)
    G, N, P = X.shape
    ii, jj = np.tril_indices(P)
    xh, xl = _split(X)
    wh, wl = _split(w)
    hi, lo, ab = (np.zeros((G, ii.size)) for _ in range(3))
    for n in range(N):
        ph, pl = _two_prod(X[:, n, ii], X[:, n, jj], (xh[:, n, ii], xl[:, n, ii]), (xh[:, n, jj], xl[:, n, jj]))
        wn = w[:, n, None]
        a, b = _two_prod(ph, wn, None, (wh[:, n, None], wl[:, n, None]))
        ab += np.abs(a)
        for t in (a, b, pl * wn):
            hi, e = _two_sum(hi, t)
            lo += e
    return hi, lo, ab, (ii, jj)


def dd_weighted_sum(hi, lo, x):
    """sum_i (hi + lo)[..., i] x[..., i] -> (hi, lo)"""
    H, L = np.zeros(hi.shape[:-1]), np.zeros(hi.shape[:-1])
    for i in range(hi.shape[-1]):
        p, e = _two_prod(hi[..., i], x[..., i])
        H, e2 = _two_sum(H, p)
        L += (e + e2) + lo[..., i] * x[..., i]
    return H, L


def err_vs_dd(got, hi, lo):
    """|got - (hi + lo)|"""
    with np.errstate(all="ignore"):
        return np.abs((got - hi) - lo)


def mp_dot(*factors):
    """(sum_k prod of the factors' k-th entries, sum of the absolute terms) in mpmath at MP_PREC bits"""
    with mpmath.workprec(MP_PREC):
        s, a = mpmath.mpf(0), mpmath.mpf(0)
        for vals in zip(*factors):
            t = mpmath.mpf(1)
            for v in vals:
                t *= mpmath.mpf(float(v))
            s += t
            a += abs(t)
        return s, a


def mp_err(got, ref):
    """|got - ref| as a double (ref: mpmath)"""
    with mpmath.workprec(MP_PREC):
        return float(abs(mpmath.mpf(float(got)) - ref))


def dd_agrees_with_mp(hi, lo, ref, absum):
    """the double-double value is within 2^-95 of the sum of absolute terms of the mpmath value"""
    with mpmath.workprec(MP_PREC):
        d = abs(mpmath.mpf(float(hi)) + mpmath.mpf(float(lo)) - ref)
        return d <= mpmath.ldexp(absum, -95)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))
