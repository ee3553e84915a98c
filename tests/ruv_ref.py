"""Restatement of the hidden-batch operations by another route, and the rounding bounds the engine is held to.

  * every logarithm and residual in mpmath (120 bits), from the exact rational value of its inputs;
  * the projection sums exactly: each product split into two doubles (Dekker), all of them added by math.fsum;
  * W from numpy.linalg.svd of the centred control matrix (not from its Gram);
  * batch removal by numpy.linalg.lstsq, gene by gene.

u = 2^-52 throughout and every rounding counts as u (as in 6k), although one rounding is at most u / 2: the bounds are
statements about the operation sequences of csrc/dsq_proj.h, written out next to each function, never fitted."""
import math

import mpmath
import numpy as np

mpmath.mp.prec = 120
U = 2.0 ** -52
mpf = mpmath.mpf


def gamma(n):
    return n * U / (1.0 - n * U)


# ----------------------------------------------------------------------------------------------------- exact summation
def two_prod(a, b):
    """a * b = p + e exactly (Dekker / Veltkamp; no overflow for the magnitudes used here)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    p = a * b
    c = 134217729.0
    ah = a * c; ah = ah - (ah - a); al = a - ah
    bh = b * c; bh = bh - (bh - b); bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def dot_exact(a, b):
    """sum_n a_n b_n rounded once"""
    p, e = two_prod(a, b)
    return math.fsum(np.concatenate([p, e]).tolist())


# ---------------------------------------------------------------------------------------------------------- log counts
def log_counts(y, sf, normalized, eps):
    """y [G][N] -> (Y correctly rounded from mpmath, bound).
    Sequence: v = fl(y / sf) (u), x = fl(v + eps) (u): x carries a relative error of at most u (two roundings of u / 2
    each, both terms positive), which the logarithm turns into an ABSOLUTE u; flog_t itself is within 1 ulp of the correct
    rounding, 1.5 ulp <= 1.5 u |Y| of the truth (tests/test_devunit_math.py), except for x in [0.5, 1) where that file
    holds it to the absolute 3 * 2^-54 + 2^-59."""
    G, N = y.shape
    ref, bound = np.empty((G, N)), np.empty((G, N))
    for g in range(G):
        for n in range(N):
            v = mpf(int(y[g, n])) / mpf(float(sf[n])) if normalized else mpf(int(y[g, n]))
            L = mpmath.log(v + mpf(eps))
            ref[g, n] = float(L)
            x = (float(y[g, n]) / float(sf[n]) if normalized else float(y[g, n])) + eps  # the device's own argument
            own = 3 * 2.0 ** -54 + 2.0 ** -59 if 0.5 <= x < 1.0 else 1.5 * U * abs(ref[g, n])
            bound[g, n] = U + own
    return ref, bound


# ----------------------------------------------------------------------------------------------------------- residuals
C_A, C_B, C_P = 6, 8, 4


def residuals(y, sf, X, beta, disp, kind):
    """y [G][N], X [N][P], beta [G][P] -> (residuals from mpmath, bound); NaN rows where the engine must give NaN.

    Deviance.  Device sequence per sample: eta by P fmas (relative gamma_P on sum |x beta|, absolute on eta), mu = fl(sf *
    fexp_t(eta)): exp within 1.5 ulp (count 2 u), one product (u) - eps_mu = gamma_{P+1} sum_j |x_nj beta_gj| + 3 u is the
    relative error of the device's mu.  r = fl(1 / alpha) (u).
      A = y * L_A, L_A = +-flog1p_t(fl(fl(|y - mu|) / min(y, mu))): subtraction u, division u (the logarithm amplifies the
          relative error of its argument by at most 1), logarithm 2 u, product u: 5 u |A|; the final subtraction A - B rounds
          once more, u |A - B| <= u (|A| + |B|): C_A = 6.
      B = fl(y + r) * +-flog1p_t(fl(fl(|y - mu|) / fl(min(y, mu) + r))): the same numerator, two more roundings for y + r and
          min(y, mu) + r: 7 u |B|, and the final subtraction: C_B = 8.
      y = 0: r * flog1p_t(fl(mu / r)): division, logarithm (2 u), product: 4 u |B| <= C_B u |B|.
    |Delta(D/2)| <= C_A u |A| + C_B u |B| + |r (mu - y) / (mu + r)| eps_mu + u r |log((y + r) / (mu + r)) - (y - mu) / (mu + r)|
    (the third term: d(D/2)/dmu times the error of mu; the fourth: d(D/2)/dr times the error of r).  Through the root:
    Delta res <= Delta D / (2 sqrt(D_ref)), or sqrt(Delta D) where D_ref < Delta D; the root itself rounds once: + u |res|.

    Pearson.  t = fl(alpha mu), V = fma(t, mu, mu): 2 u on V (positive terms), the root halves it and rounds (u + u), the
    numerator rounds once (u |y - mu|), the quotient once: C_P = 4, gamma_4 |res|; the error of mu enters through
    d res / d mu = -1 / sqrt(V) - (y - mu) (1 + 2 alpha mu) / (2 V^1.5), times mu eps_mu."""
    G, N = y.shape
    P = X.shape[1]
    ref, bound = np.full((G, N), np.nan), np.full((G, N), np.nan)
    for g in range(G):
        if not y[g].any() or np.isnan(beta[g]).any() or np.isnan(disp[g]):
            continue
        a = mpf(float(disp[g]))
        r = 1 / a
        for n in range(N):
            eta = mpmath.fsum(mpf(float(X[n, j])) * mpf(float(beta[g, j])) for j in range(P))
            mu = mpf(float(sf[n])) * mpmath.exp(eta)
            eps_mu = gamma(P + 1) * float(np.abs(X[n] * beta[g]).sum()) + 3 * U
            yy = mpf(int(y[g, n]))
            if kind == 1:
                V = mu + a * mu * mu
                res = (yy - mu) / mpmath.sqrt(V)
                dmu = -1 / mpmath.sqrt(V) - (yy - mu) * (1 + 2 * a * mu) / (2 * V ** mpf(1.5))
                ref[g, n] = float(res)
                bound[g, n] = gamma(C_P) * abs(ref[g, n]) + float(abs(dmu) * mu) * eps_mu
                continue
            B = (yy + r) * mpmath.log((yy + r) / (mu + r))
            A = yy * mpmath.log(yy / mu) if yy > 0 else mpf(0)
            h = A - B
            res = mpmath.sign(yy - mu) * mpmath.sqrt(max(2 * h, mpf(0)))
            ref[g, n] = float(res)
            dh = (C_A * U * float(abs(A)) + C_B * U * float(abs(B)) + float(abs(r * (mu - yy) / (mu + r))) * eps_mu
                  + U * float(r * abs(mpmath.log((yy + r) / (mu + r)) - (yy - mu) / (mu + r))))
            dD, D = 2 * dh, float(2 * h)
            root = dD / (2 * math.sqrt(D)) if D >= dD and D > 0 else math.sqrt(dD)
            bound[g, n] = root + U * abs(ref[g, n])
    return ref, bound


# ---------------------------------------------------------------------------------------------------------- projection
def projection(x, P, B):
    """x [G][N], P and B [N][q] -> dict: coef [G][q] and out [G][N], both exact sums rounded once, and their bounds.

    coef: lane l adds ceil(N / 64) products by fma (one rounding each), the butterfly adds 6 more levels:
        |Delta c_gj| <= gamma_{ceil(N / 64) + 7} sum_n |x_gn P_nj|.
    out: v = x, then q fmas v = fl(v - c_j B_nj): the partial sum after step k is out + sum_{j > k} c_j B_nj, so the q
    roundings (u / 2 each in truth) add up to at most (u / 2) (q |out| + (q - 1) sum_j |c_j B_nj|).  That is within
        u |out| + gamma_{q+1} sum_j |c_j B_nj|
    for q <= 2 always, and for larger q where sum_j |c_j B_nj| >= |out| (q - 2) / (q + 3) - `out_cond` says where that
    holds, and the cases are built so that it does.  The error of c_j itself adds |B_nj| Delta c_j."""
    G, N = x.shape
    q = P.shape[1]
    coef, cb = np.empty((G, q)), np.empty((G, q))
    for g in range(G):
        for j in range(q):
            coef[g, j] = dot_exact(x[g], P[:, j])
            cb[g, j] = gamma(-(-N // 64) + 7) * float(np.abs(x[g] * P[:, j]).sum())
    out, ob, cond = np.empty((G, N)), np.empty((G, N)), np.empty((G, N), dtype=bool)
    for g in range(G):
        for n in range(N):
            p, e = two_prod(-coef[g], B[n])
            out[g, n] = math.fsum([x[g, n]] + p.tolist() + e.tolist())
            t = float(np.abs(coef[g] * B[n]).sum())
            ob[g, n] = U * abs(out[g, n]) + float((np.abs(B[n]) * cb[g]).sum()) + gamma(q + 1) * t
            cond[g, n] = q <= 2 or t >= abs(out[g, n]) * (q - 2) / (q + 3)
    return dict(coef=coef, coef_bound=cb, out=out, out_bound=ob, out_cond=cond)


def exp_post(out, out_bound, eps):
    """exp(out) - eps and its bound: the error of out is amplified to exp(out) expm1(out_bound), fexp_t is within 1.5 ulp
    (count 2 u) and the subtraction rounds once (u on the result)."""
    e = np.array([[float(mpmath.exp(mpf(float(v)))) for v in row] for row in out])
    val = np.array([[float(mpmath.exp(mpf(float(v))) - mpf(eps)) for v in row] for row in out])
    return val, e * np.expm1(out_bound) + 2 * U * e + U * np.abs(val)


# ---------------------------------------------------------------------------------------------------------------- RUV
def size_factors(counts):
    """median of ratios over the genes without a zero (DESeq2's estimateSizeFactors)"""
    with np.errstate(divide="ignore"):
        lc = np.log(counts.astype(np.float64))
    ok = np.isfinite(lc).all(axis=0)
    return np.exp(np.median(lc[:, ok] - lc[:, ok].mean(axis=0), axis=1))


def ruvg(Y, controls, k, center=True, drop=0):
    """Y N x G -> (W, singular values of the control matrix, Y', alpha) through the SVD of the centred control matrix."""
    Yc = Y[:, controls] - (Y[:, controls].mean(0) if center else 0.0)
    Um, d, _ = np.linalg.svd(Yc, full_matrices=False)
    W = Um[:, drop:k]
    top = np.argmax(np.abs(W), 0)
    W = W * np.where(W[top, np.arange(W.shape[1])] < 0, -1.0, 1.0)
    alpha = np.linalg.solve(W.T @ W, W.T @ Y)
    return W, d, Y - W @ alpha, alpha


def gram_route_error(Yc):
    """A bound dS on ||S_computed - Yc Yc^T||_2 plus what the two eigen-solvers add, for the N x K (centred) control matrix
    Yc.  Three sources, each at most N gamma_{K+2} trace(S):
      * an entry of the computed Gram carries gamma_{K+2} sum_g |y_ig y_jg| <= gamma_{K+2} sqrt(S_ii S_jj), so
        the Frobenius norm of that error is at most gamma_{K+2} trace(S);
      * the first-order term of the centring error (6j) is of the same form;
      * eigh of S and the SVD of Yc are backward stable: each leaves p(N) u ||S||_2 with a modest polynomial p that LAPACK
        does not publish as a number - p(N) = N is ASSUMED here, not derived.
    The factor 4 is the three sources and, for the vectors, the sqrt(2) between the sine of an angle and the difference of
    two unit vectors."""
    return 4 * Yc.shape[0] * gamma(Yc.shape[1] + 2) * float(np.sum(Yc * Yc))


def factor_tolerance(Yc, d, k):
    """Davis-Kahan: the sine of the angle between an eigenvector of S and that of S + Delta S is at most ||Delta S||_2 over
    its eigenvalue's distance to the others, here at least (the smallest relative gap) * lambda_k; every entry of a column of
    W moves by no more than the column does."""
    return gram_route_error(Yc) / (gaps(d, k).min() * d[k - 1] ** 2)


def gaps(d, upto):
    """relative eigenvalue gaps (lambda_i - lambda_{i+1}) / lambda_i of the first `upto` components (to the next one)"""
    lam = np.asarray(d, dtype=np.float64) ** 2
    return (lam[:upto] - lam[1:upto + 1]) / lam[:upto]


def remove_batch(x, D, Xb):
    """x N x G: per gene the least-squares fit of [D | Xb] (numpy.linalg.lstsq, one gene at a time) and the fitted batch
    terms subtracted."""
    F = np.hstack([D, Xb])
    out = np.empty_like(x)
    for g in range(x.shape[1]):
        coef = np.linalg.lstsq(F, x[:, g], rcond=None)[0]
        out[:, g] = x[:, g] - Xb @ coef[D.shape[1]:]
    return out
