"""Restatement, by another route, of the sample PCA / sample distances of pydeseq2_amd/pca.py: rowVars
with math.fsum, R's stable order, PCA by numpy's SVD of the centred matrix (NOT through a Gram), distances from explicit
differences; and the entrywise error bound of a centred Gram summed in floating point."""
import math

import numpy as np

U = 2.0 ** -53


def gamma(n):
    return n * U / (1.0 - n * U)


def row_means(x):
    x = np.asarray(x, dtype=np.float64)
    return np.array([math.fsum(x[:, g]) for g in range(x.shape[1])]) / x.shape[0]


def row_vars(x):
    """rowVars of the N x G matrix: two-pass with correctly rounded sums; one sample: NaN."""
    x = np.asarray(x, dtype=np.float64)
    N, G = x.shape
    m = row_means(x)
    q = np.array([math.fsum((x[:, g] - m[g]) ** 2) for g in range(G)])
    with np.errstate(invalid="ignore", divide="ignore"):
        return q / (N - 1)


def meanvar_bounds(x):
    """Bounds of |mean - m| and |var - rv| for a two-pass computation in floating point, ANY order of the sums, fused or not.
    mean: a sum of N terms (gamma_{N-1} sum|x|) and one division: e_m = gamma_N mean|x|, plus gamma_1 of the reference's own
    rounding: gamma_{N+1} mean|x|.
    var: with the computed mean m^, sum (x - m^)^2 = sum (x - m)^2 + N (m^ - m)^2 exactly (sum (x - m) = 0); every term
    takes the rounding of the difference (twice, squared), of the square, the sum of N terms and one division:
    gamma_{N+3}, plus the reference's own: |rv^ - rv| <= gamma_{N+4} (rv + c) + c,  c = N e_m^2 / (N - 1)."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    em = gamma(N + 1) * np.abs(x).mean(0)
    rv = row_vars(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = N * em * em / (N - 1)
    return em, gamma(N + 4) * (rv + c) + c


def order_by_variance(rv, ntop):
    """order(rv, decreasing = TRUE)[1:min(ntop, G)]: ties go to the lower index."""
    idx = sorted(range(len(rv)), key=lambda g: -rv[g])  # (Python's sort is stable)
    return np.array(idx[:len(rv) if ntop is None else min(ntop, len(rv))], dtype=np.int64)


def sign_rule(scores):
    s = np.array(scores, dtype=np.float64)
    for c in range(s.shape[1]):
        a = np.abs(s[:, c])
        if s[int(np.nonzero(a == a.max())[0][0]), c] < 0:
            s[:, c] = -s[:, c]
    return s


def pca_svd(x, ntop=500):
    """prcomp(center = TRUE, scale. = FALSE) of the ntop most variable genes through the SVD of the centred matrix."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    genes = order_by_variance(row_vars(x), ntop)
    xs = x[:, genes]
    xc = xs - row_means(xs)
    u, s, _ = np.linalg.svd(xc, full_matrices=False)
    lam = s * s
    return dict(genes=genes, scores=sign_rule(u * s), variance=lam / (N - 1), variance_ratio=lam / lam.sum(),
                total_variance=lam.sum() / (N - 1), lam=lam)


def relative_gaps(lam, k):
    """For each of the first k components the smaller relative gap of its eigenvalue to its neighbours'."""
    lam = np.asarray(lam, dtype=np.float64)
    out = []
    for c in range(k):
        g = [(lam[c - 1] - lam[c]) / lam[c]] if c > 0 else []
        if c + 1 < len(lam):
            g.append((lam[c] - lam[c + 1]) / lam[c])
        out.append(min(g))
    return np.array(out)


def distances(x):
    """dist(): from explicit differences, correctly rounded sums."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    D = np.zeros((N, N))
    for i in range(N):
        for j in range(i):
            D[i, j] = D[j, i] = math.sqrt(math.fsum((x[i] - x[j]) ** 2))
    return D


def _two_prod(a, b):
    """a b = p + e exactly (Dekker / Veltkamp; no overflow for the magnitudes used here)."""
    p = a * b
    c = 134217729.0  # 2^27 + 1
    ah = c * a - (c * a - a); al = a - ah
    bh = c * b - (c * b - b); bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def centred_exact(x):
    """The exactly centred data as hi + lo (K x N each): the mean from the correctly rounded sum, the difference in
    64-bit-mantissa arithmetic."""
    assert np.finfo(np.longdouble).nmant >= 63
    x = np.asarray(x, dtype=np.float64)
    N, G = x.shape
    s = np.array([math.fsum(x[:, g]) for g in range(G)]).astype(np.longdouble)
    xc = (x.astype(np.longdouble) - s / np.longdouble(N)).T
    hi = xc.astype(np.float64)
    return hi, (xc - hi).astype(np.float64)


def gram_ref(x, center=True):
    """N x N Gram of the (exactly centred) N x K matrix, every entry one correctly rounded sum."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    hi, lo = centred_exact(x) if center else (np.ascontiguousarray(x.T), np.zeros(x.T.shape))
    S = np.zeros((N, N))
    for i in range(N):
        for j in range(i + 1):
            p, e = _two_prod(hi[:, i], hi[:, j])
            S[i, j] = S[j, i] = math.fsum(np.concatenate([p, e, hi[:, i] * lo[:, j], lo[:, i] * hi[:, j]]))
    return S


def gram_bound(x):
    """Entrywise bound of |S - S_ref| for a centred Gram over the K columns of the N x K matrix x, summed in floating point in
    ANY order, fused or not, from values centred in floating point with means that were computed in floating point:
    gamma_{K+2} sum_g |x~_i x~_j|, plus the centring error e <= u |x~| + gamma_{N+1} mean|x_g| per value to first order,
    sum_g (e_i |x~_j| + |x~_i| e_j) (and the second-order term sum_g e_i e_j, which is far below either)."""
    x = np.asarray(x, dtype=np.float64)
    N, K = x.shape
    a = np.abs(centred_exact(x)[0]).T  # N x K
    e = U * a + gamma(N + 1) * np.abs(x).mean(0)
    return gamma(K + 2) * (a @ a.T) + (e @ a.T + a @ e.T) + e @ e.T
