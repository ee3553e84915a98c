"""Dense restatement of adaptive shrinkage in numpy / scipy (test infrastructure): the statement of DESIGN.md 6i written
the plain way - the n x M likelihood matrix in memory, the quadratic subproblem through scipy.optimize.nnls on the
Cholesky factor of H, the fit run on to min grad >= -1e-13 - and deliberately not through the chunked sums and the
normal-equation active set of csrc/dsq_ash.h.  The posterior of single genes is also available in mpmath."""
import numpy as np
from scipy.optimize import nnls
from scipy.special import ndtr

DELTA, DECREASE, CUT, MIN_STEP = 1e-8, 0.01, 0.75, 1e-8
TIGHT = 1e-13


def used(b, s):
    with np.errstate(invalid="ignore"):
        return np.isfinite(b) & np.isfinite(s) & (s > 0)


def grid(b, s, mult=np.sqrt(2.0)):
    """autoselect.mixsd with mode 0: (npoint, standard deviations)."""
    u = used(b, s)
    b, s = b[u], s[u]
    smin = s.min() / 10
    d = b * b - s * s
    smax = 2 * np.sqrt(d.max()) if (d > 0).any() else 8 * smin
    npoint = int(np.ceil(np.log2(smax / smin) / np.log2(mult)))
    e = list(range(-npoint, 1)) if npoint >= 0 else list(range(-npoint, -1, -1))  # R's (-npoint):0
    return npoint, np.array([mult ** k * smax for k in e])


def loglik_matrix(b, s, sd):
    v = s[:, None] ** 2 + sd[None, :] ** 2
    return -0.5 * np.log(v) - 0.5 * b[:, None] ** 2 / v


def lik(b, s, sd):
    """(L scaled to a row maximum of 1, the row maxima of the logarithms)"""
    l = loglik_matrix(b, s, sd)
    top = l.max(1)
    return np.exp(l - top[:, None]), top


def objective(L, x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.log(L @ x).mean() + x.sum()


def factor(H):
    """C with H = C^T C: the Cholesky factor; where rounding has cost H its definiteness (entries of 1e16 beside the 1e-8
    on the diagonal, late in a fit with outlying genes), the symmetric eigen-factor with the eigenvalues held at the
    1e-8 they cannot fall below in exact arithmetic."""
    try:
        return np.linalg.cholesky(H).T
    except np.linalg.LinAlgError:
        lam, V = np.linalg.eigh(H)
        return np.sqrt(np.maximum(lam, DELTA))[:, None] * V.T


def fit(L, tol=TIGHT, maxit=300):
    """-> (x, iterations, converged): the Newton scheme of the statement with the stop at min grad >= -tol."""
    n, M = L.shape
    x = np.full(M, 1.0 / M)
    for it in range(maxit + 1):
        r = 1.0 / (L @ x)
        Z = L * r[:, None]
        g = 1.0 - Z.mean(0)
        if g.min() >= -tol:
            return x, it, True
        if it == maxit:
            break
        with np.errstate(over="ignore", invalid="ignore"):
            H = Z.T @ Z / n + DELTA * np.eye(M)
        if not np.isfinite(H).all():  # (a gene whose u has all but vanished: the scheme has broken down)
            return x, it, False
        C = factor(H)
        y, _ = nnls(C, -np.linalg.solve(C.T, g - H @ x), maxiter=100 * M)
        p = y - x
        f0, gp, t = objective(L, x), g @ p, 1.0
        while not objective(L, x + t * p) <= f0 + DECREASE * t * gp:
            t *= CUT
            if t < MIN_STEP:
                break
        x = x + t * p
    return x, maxit, False


def kkt_residual(L, pi):
    """max_m d_m - 1 at pi, from a dense L"""
    return float(((L / (L @ pi)[:, None]).mean(0)).max() - 1.0)


def posterior(b, s, sd, pi):
    """-> (PosteriorMean, PosteriorSD, lfsr) of the genes (all used)"""
    l = loglik_matrix(b, s, sd)
    w = pi[None, :] * np.exp(l - l.max(1)[:, None])
    w /= w.sum(1, keepdims=True)
    t = sd[None, :] ** 2 / (sd[None, :] ** 2 + s[:, None] ** 2)
    mu, v = t * b[:, None], t * s[:, None] ** 2
    pm = (w * mu).sum(1)
    psd = np.sqrt(np.maximum((w * (v + mu * mu)).sum(1) - pm * pm, 0.0))
    z = mu / np.sqrt(v)
    lfsr = np.minimum((w * ndtr(-z)).sum(1), (w * ndtr(z)).sum(1))
    return pm, psd, lfsr


def posterior_mp(b, s, sd, pi, dps=40):
    """One gene in mpmath -> (PosteriorMean, PosteriorSD, lfsr) as floats."""
    import mpmath as mp

    with mp.workdps(dps):
        b, s = mp.mpf(float(b)), mp.mpf(float(s))
        ws, mus, vs = [], [], []
        for g, p in zip(sd, pi):
            g2, p = mp.mpf(float(g)) ** 2, mp.mpf(float(p))
            v = s * s + g2
            ws.append(p * mp.exp(-mp.log(v) / 2 - b * b / (2 * v)))
            t = g2 / v
            mus.append(t * b)
            vs.append(t * s * s)
        tot = mp.fsum(ws)
        ws = [w / tot for w in ws]
        pm = mp.fsum(w * m for w, m in zip(ws, mus))
        var = mp.fsum(w * (v + m * m) for w, m, v in zip(ws, mus, vs)) - pm * pm
        neg = mp.fsum(w * mp.ncdf(-m / mp.sqrt(v)) for w, m, v in zip(ws, mus, vs))
        pos = mp.fsum(w * mp.ncdf(m / mp.sqrt(v)) for w, m, v in zip(ws, mus, vs))
        return float(pm), float(mp.sqrt(max(var, 0))), float(min(neg, pos))


def svalues(lfsr):
    """the direct loop: running mean over the genes in ascending (stable) order of lfsr"""
    out = np.full(len(lfsr), np.nan)
    idx = sorted((i for i in range(len(lfsr)) if not np.isnan(lfsr[i])), key=lambda i: lfsr[i])
    tot = 0.0
    for k, i in enumerate(idx):
        tot += lfsr[i]
        out[i] = tot / (k + 1)
    return out


def ash(b, s, sd=None, tol=TIGHT):
    """One contrast -> dict(grid, pi, post_mean, post_sd, lfsr, n_iter, converged, loglik, n); unused genes: NaN."""
    b, s = np.asarray(b, float), np.asarray(s, float)
    u = used(b, s)
    G = len(b)
    o = dict(post_mean=np.full(G, np.nan), post_sd=np.full(G, np.nan), lfsr=np.full(G, np.nan), n=int(u.sum()))
    if not u.any():
        o.update(grid=np.zeros(0), pi=np.zeros(0), n_iter=0, converged=False, loglik=np.nan)
        return o
    if sd is None:
        sd = grid(b, s)[1]
    L, top = lik(b[u], s[u], sd)
    x, it, conv = fit(L, tol)
    pi = x / x.sum()
    o["post_mean"][u], o["post_sd"][u], o["lfsr"][u] = posterior(b[u], s[u], sd, pi)
    o.update(grid=sd, pi=pi, n_iter=it, converged=conv,
             loglik=float((np.log(L @ x) + top).sum() - 0.5 * u.sum() * np.log(2 * np.pi)))
    return o
