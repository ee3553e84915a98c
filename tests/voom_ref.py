"""Independent reference of limma-voom: a scalar, loop-by-loop ``clowess`` written from the rules of R's
lowess.c, log-CPM, precision weights and the weighted fits by numpy.linalg.lstsq on sqrt(w)-scaled rows in float64 (refined
with extended-precision residuals: see wls), the moderation by tests/ql_ref.squeeze_var (scipy's polygamma), p-values by
scipy.stats.t (mpmath where df_total >= 1e6), and the per-gene arithmetic in mpmath at 50 digits for a handful of genes.
Shares no code with pydeseq2_amd.voom."""
import math

import numpy as np

from tests import ql_ref

C0 = math.log2(1e6)


# -------------------------------------------------------------------------------------------------------------- lowess
def _lowest(x, y, n, xs, nleft, nright, w, userw, rw):
    rng = x[n - 1] - x[0]
    h = max(xs - x[nleft], x[nright] - xs)
    h9, h1 = 0.999 * h, 0.001 * h
    a = 0.0
    j = nleft
    while j < n:
        w[j] = 0.0
        r = abs(x[j] - xs)
        if r <= h9:
            if r <= h1:
                w[j] = 1.0
            else:
                q = r / h
                t = 1.0 - q * q * q
                w[j] = t * t * t
            if userw:
                w[j] *= rw[j]
            a += w[j]
        elif x[j] > xs:
            break
        j += 1
    nrt = j - 1
    if a <= 0.0:
        return 0.0, False
    for j in range(nleft, nrt + 1):
        w[j] /= a
    if h > 0.0:
        a = 0.0
        for j in range(nleft, nrt + 1):
            a += w[j] * x[j]
        b = xs - a
        c = 0.0
        for j in range(nleft, nrt + 1):
            c += w[j] * (x[j] - a) * (x[j] - a)
        if math.sqrt(c) > 0.001 * rng:
            b /= c
            for j in range(nleft, nrt + 1):
                w[j] *= b * (x[j] - a) + 1.0
    ys = 0.0
    for j in range(nleft, nrt + 1):
        ys += w[j] * y[j]
    return ys, True


def clowess(x, y, f, nsteps, delta):
    """R's clowess on SORTED x (python lists / floats, one operation at a time) -> (ys, anchors of the last pass)."""
    x, y = [float(v) for v in x], [float(v) for v in y]
    n = len(x)
    ys = [0.0] * n
    if n < 2:
        return [y[0]], [0]
    ns = max(2, min(n, int(f * n + 1e-7)))
    rw, res, w = [0.0] * n, [0.0] * n, [0.0] * n
    anchors = []
    it = 1
    while it <= nsteps + 1:
        nleft, nright, last, i = 0, ns - 1, -1, 0
        anchors = []
        while True:
            if nright < n - 1:
                d1 = x[i] - x[nleft]
                d2 = x[nright + 1] - x[i]
                if d1 > d2:
                    nleft += 1
                    nright += 1
                    continue
            v, ok = _lowest(x, y, n, x[i], nleft, nright, w, it > 1, rw)
            ys[i] = v if ok else y[i]
            anchors.append(i)
            if last < i - 1:
                denom = x[i] - x[last]
                for j in range(last + 1, i):
                    alpha = (x[j] - x[last]) / denom
                    ys[j] = alpha * ys[i] + (1.0 - alpha) * ys[last]
            last = i
            cut = x[last] + delta
            i = last + 1
            while i < n:
                if x[i] > cut:
                    break
                if x[i] == x[last]:
                    ys[i] = ys[last]
                    last = i
                i += 1
            i = max(last + 1, i - 1)
            if last >= n - 1:
                break
        for i in range(n):
            res[i] = y[i] - ys[i]
        sc = 0.0
        for i in range(n):
            sc += abs(res[i])
        sc /= n
        if it > nsteps:
            break
        srt = sorted(abs(v) for v in res)
        m1 = n // 2
        cmad = 3.0 * (srt[m1] + srt[n - m1 - 1])
        if cmad < 1e-7 * sc:
            break
        c9, c1 = 0.999 * cmad, 0.001 * cmad
        for i in range(n):
            r = abs(res[i])
            if r <= c1:
                rw[i] = 1.0
            elif r <= c9:
                q = r / cmad
                t = 1.0 - q * q
                rw[i] = t * t
            else:
                rw[i] = 0.0
        it += 1
    return ys, anchors


# ---------------------------------------------------------------------------------------------------------------- voom
def logcpm(counts, L):
    """samples x genes: log2((y + 0.5) / (L + 1) 1e6)."""
    return np.log2((np.asarray(counts, dtype=float) + 0.5) / (np.asarray(L, dtype=float)[:, None] + 1.0) * 1e6)


def effective_lib_sizes(sf, colsums):
    nf = np.asarray(sf, float) / np.asarray(colsums, float)
    nf = nf / np.exp(np.mean(np.log(nf)))
    return np.asarray(colsums, float) * nf


def first_fit(counts, X, L):
    """(beta1 G x P, amean, sigma1) by lstsq; NaN for genes without counts."""
    counts = np.asarray(counts)
    N, G = counts.shape
    P = X.shape[1]
    E = logcpm(counts, L)
    b = np.linalg.lstsq(X, E, rcond=None)[0]
    rss = ((E - X @ b) ** 2).sum(0)
    s1 = np.sqrt(rss / (N - P))
    am = E.mean(0)
    z = counts.sum(0) == 0
    b, s1, am = b.T.copy(), s1.copy(), am.copy()
    b[z], s1[z], am[z] = np.nan, np.nan, np.nan
    return b, am, s1


def trend_knots(amean, sigma1, L, span=0.5):
    """The anchors of the last lowess pass over the genes with counts: (knot_x, knot_y)."""
    use = np.isfinite(amean)
    sx = amean[use] + np.mean(np.log2(np.asarray(L, float) + 1.0)) - C0
    sy = np.sqrt(sigma1[use])
    o = np.argsort(sx, kind="stable")
    sx, sy = sx[o], sy[o]
    ys, a = clowess(sx, sy, span, 3, 0.01 * (sx[-1] - sx[0]))
    return sx[a], np.asarray(ys)[a]


LD = np.longdouble


def _interp_ld(lam, kx, ky):
    kx, ky = np.asarray(kx).astype(LD), np.asarray(ky).astype(LD)
    i = np.clip(np.searchsorted(kx, lam, side="right") - 1, 0, len(kx) - 2)
    v = ky[i] + (lam - kx[i]) / (kx[i + 1] - kx[i]) * (ky[i + 1] - ky[i])
    return np.where(lam <= kx[0], ky[0], np.where(lam >= kx[-1], ky[-1], v))


def _chol_solve_ld(M, B):
    P = M.shape[0]
    Lm = np.zeros_like(M)
    for j in range(P):
        Lm[j, j] = np.sqrt(M[j, j] - (Lm[j, :j] ** 2).sum())
        Lm[j + 1:, j] = (M[j + 1:, j] - Lm[j + 1:, :j] @ Lm[j, :j]) / Lm[j, j]
    Y = np.zeros_like(B)
    for i in range(P):
        Y[i] = (B[i] - Lm[i, :i] @ Y[:i]) / Lm[i, i]
    for i in range(P - 1, -1, -1):
        Y[i] = (Y[i] - Lm[i + 1:, i] @ Y[i + 1:]) / Lm[i, i]
    return Y


def wls(counts, X, L, beta1, kx, ky, contrasts):
    """Weighted fits from given beta1 and knots: dict of E, w (samples x genes), beta (G x P), sigma2, est, u (G x K),
    kappa = cond_2(diag(sqrt w) X)^2 per gene.  NaN for genes whose beta1 is NaN.
    The fit is numpy.linalg.lstsq on the sqrt(w)-scaled rows in float64, then refined twice with the residual taken in
    extended precision (x87 long double, eps 1.1e-19): with one residual degree of freedom sigma2 is what is left of E
    after the fit, and the plain float64 solution carries an error of its own there - up to 3e4 eps in sigma2 - that is
    larger than the error of the code under test.  E, lambda and w are formed in extended precision from the same double
    inputs and rounded once; u through the normal equations in extended precision (error 1e-19 kappa, against bounds of
    eps kappa)."""
    assert np.finfo(LD).eps < 2e-19, "the reference needs an extended-precision long double"
    counts = np.asarray(counts)
    N, G = counts.shape
    P = X.shape[1]
    c = np.atleast_2d(np.asarray(contrasts, float))
    K = c.shape[0]
    Xl, cl = X.astype(LD), c.astype(LD)
    off = np.log2(np.asarray(L, float) + 1.0) - C0  # (the double the kernels are given)
    El = np.log2(counts.astype(LD) + LD(0.5)) - off.astype(LD)[:, None]
    lam = Xl @ np.nan_to_num(np.asarray(beta1)).astype(LD).T + off.astype(LD)[:, None]
    wl = _interp_ld(lam, kx, ky) ** -4
    E, w = El.astype(float), wl.astype(float)
    nan = lambda *s: np.full(s, np.nan)  # noqa: E731
    beta, s2, est, u, kappa = nan(G, P), nan(G), nan(G, K), nan(G, K), nan(G)
    for g in range(G):
        if np.isnan(beta1[g]).any():
            E[:, g], w[:, g] = np.nan, np.nan
            continue
        swl = np.sqrt(wl[:, g])
        A = (Xl * swl[:, None]).astype(float)
        b = np.linalg.lstsq(A, (El[:, g] * swl).astype(float), rcond=None)[0].astype(LD)
        for _ in range(2):
            r = (El[:, g] - Xl @ b) * swl
            b = b + np.linalg.lstsq(A, r.astype(float), rcond=None)[0].astype(LD)
        r = El[:, g] - Xl @ b
        beta[g], s2[g] = b.astype(float), float((wl[:, g] * r * r).sum() / (N - P))
        sv = np.linalg.svd(A, compute_uv=False)
        kappa[g] = (sv[0] / sv[-1]) ** 2
        Al = Xl * swl[:, None]
        Z = _chol_solve_ld(Al.T @ Al, cl.T.copy())  # P x K
        for k in range(K):
            est[g, k] = float(cl[k] @ b)
            u[g, k] = float(np.sqrt(cl[k] @ Z[:, k]))
    return dict(E=E, w=w, beta=beta, sigma2=s2, est=est, u=u, kappa=kappa)


def t_pvalue(t, df):
    """Two-sided p-value of t on df degrees of freedom (the normal limit for df = inf)."""
    from scipy import stats

    t = np.asarray(t, dtype=float)
    if not np.isfinite(df):
        return 2.0 * stats.norm.sf(np.abs(t))
    if df < 1e6:
        return 2.0 * stats.t.sf(np.abs(t), df)
    import mpmath

    out = np.full(t.shape, np.nan)
    with mpmath.workdps(50):
        for i, v in np.ndenumerate(t):
            if np.isfinite(v):
                x = mpmath.mpf(df) / (mpmath.mpf(df) + mpmath.mpf(float(v)) ** 2)
                out[i] = float(mpmath.betainc(mpmath.mpf(df) / 2, mpmath.mpf(1) / 2, 0, x, regularized=True))
    return out


def voom_reference(counts, X, L, contrasts, span=0.5):
    """The whole route: dict with E, w, knots, beta, sigma2, s2_post, df0, s02, df_total, est, u, t, p (K x G), kappa."""
    counts = np.asarray(counts)
    N, P = X.shape
    b1, am, s1 = first_fit(counts, X, L)
    kx, ky = trend_knots(am, s1, L, span)
    out = wls(counts, X, L, b1, kx, ky, contrasts)
    post, df0, s02, df_total = ql_ref.squeeze_var(out["sigma2"], N - P)
    dfs = df_total if np.isfinite(df0) else np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (out["est"] / (out["u"] * np.sqrt(post)[:, None])).T
    out.update(beta1=b1, amean=am, sigma1=s1, knots=(kx, ky), s2_post=post, df0=df0, s02=s02, df_total=dfs, t=t,
               p=t_pvalue(t, dfs), lfcSE=(out["u"] * np.sqrt(post)[:, None]).T)
    return out


# -------------------------------------------------------------------------------------------------------------- mpmath
def gene_truth(y, off, X, beta1, kx, ky, contrasts, dps=50):
    """One gene in mpmath from the double inputs taken exactly (off, beta1 and the knots as the kernel gets them): dict of
    E, lam, w (lists), beta, sigma2, est, u as mpf, and sigma1 / amean / beta1 of the unweighted fit."""
    import mpmath

    with mpmath.workdps(dps):
        mp = mpmath.mpf
        N, P = X.shape
        Xm = mpmath.matrix([[mp(float(v)) for v in row] for row in X])
        E = [mpmath.log(mp(int(v)) + mp("0.5"), 2) - mp(float(o)) for v, o in zip(y, off)]
        Ev = mpmath.matrix(E)
        # unweighted
        b1_true = mpmath.lu_solve(Xm.T * Xm, Xm.T * Ev)
        r1 = Ev - Xm * b1_true
        sigma1 = mpmath.sqrt(sum(v * v for v in r1) / (N - P))
        amean = sum(E) / N
        # weighted, from the beta1 given
        b1 = [mp(float(v)) for v in beta1]
        kxm, kym = [mp(float(v)) for v in kx], [mp(float(v)) for v in ky]
        lam, w = [], []
        for n in range(N):
            lm = sum(Xm[n, j] * b1[j] for j in range(P)) + mp(float(off[n]))
            if lm <= kxm[0]:
                fv = kym[0]
            elif lm >= kxm[-1]:
                fv = kym[-1]
            else:
                i = max(j for j in range(len(kxm)) if kxm[j] <= lm)
                fv = kym[i] + (lm - kxm[i]) / (kxm[i + 1] - kxm[i]) * (kym[i + 1] - kym[i])
            lam.append(lm)
            w.append(fv ** -4)
        M, rhs = mpmath.zeros(P, P), mpmath.zeros(P, 1)
        for i in range(P):
            wx = [w[n] * Xm[n, i] for n in range(N)]
            rhs[i] = sum(wx[n] * E[n] for n in range(N))
            for j in range(i + 1):
                M[i, j] = M[j, i] = sum(wx[n] * Xm[n, j] for n in range(N))
        b = mpmath.lu_solve(M, rhs)
        r = Ev - Xm * b
        s2 = sum(w[n] * r[n] * r[n] for n in range(N)) / (N - P)
        Mi = mpmath.inverse(M)
        est, u = [], []
        for c in np.atleast_2d(contrasts):
            cm = mpmath.matrix([mp(float(v)) for v in c])
            est.append((cm.T * b)[0])
            u.append(mpmath.sqrt((cm.T * Mi * cm)[0]))
        return dict(E=E, lam=lam, w=w, beta=[b[j] for j in range(P)], sigma2=s2, est=est, u=u,
                    beta1=[b1_true[j] for j in range(P)], sigma1=sigma1, amean=amean)
