"""Inputs, high-precision truths and bounds shared by the quasi-likelihood tests (host and GPU)."""
import numpy as np
import pandas as pd

EPS = 2.220446049250313e-16

# the grid of the F distribution's survival function (the issue's): numerator df x denominator df x F
F_D1 = (1, 2, 3, 7, 20, 127)
F_D2 = (2.5, 10.3, 97.7, 1003.2, 1e5 + 0.4, 1e6 + 0.7, 3e7 + 0.3)
F_F = (0.0, 1e-3, 0.5, 1.0, 3.0, 30.0, 300.0, 3e4)

# Error constants c of  |p - truth| <= c eps (1 + |ln truth|) truth,  measured on the grid with the host build (x86-64,
# glibc) and asserted at twice the measured value, rounded up, as the issue sets it (the margin covers another libm's
# log1p / lgamma); the device build is asserted at four times the host-measured value.  DESIGN.md 7.
F_SF_C_HOST_MEASURED = 37.2  # at (d1, d2, F) = (127, 1e5 + 0.4, 1): p = 0.48
F_SF_C_HOST = 75.0  # 2 x measured, rounded up
F_SF_C_DEVICE = 150.0  # 4 x measured, rounded up
# Error constant c_D of  |D_f - truth| <= c_D eps sum(|term1| + |term2|)  (term1 = 2 y log(y / mu), term2 = 2 (y + r)
# log((y + r) / (mu + r)); y = 0: the one term 2 r log1p(mu / r)), measured the same way.
DEV_C_MEASURED = 1.14  # one count (y = 0, mu = 3e7, r = 1e8); whole genes of the likelihood-ratio fixture: 0.25
DEV_C = 2.3  # 2 x measured, rounded up

_cache = {}


def _series(A, B, Cc, z, dps):
    """sum_k (A)_k (B)_k / ((Cc)_k k!) z^k for |z| < 1 in mpmath, the working precision raised by the size of the largest
    term (the series alternates when B < 0)."""
    import mpmath

    guard = 30
    while True:
        with mpmath.workdps(dps + guard):
            A_, B_, C_, z_ = (mpmath.mpf(v) for v in (A, B, Cc, z))
            t, s, big, k = mpmath.mpf(1), mpmath.mpf(0), mpmath.mpf(1), 0
            tol = mpmath.mpf(10) ** (-(dps + 10))
            while True:
                s += t
                ratio = (A_ + k) * (B_ + k) / ((C_ + k) * (k + 1)) * z_
                t *= ratio
                k += 1
                big = max(big, abs(t))
                if t == 0 or (k > 5 and abs(t) < tol * abs(s) and abs(ratio) < 0.9):
                    break
            need = int(mpmath.log10(big / abs(s))) + 30
            if need <= guard:
                return +s
        guard = need + 10


def f_sf_truth(F, d1, d2, dps=400):
    """I_x(d2 / 2, d1 / 2), x = d2 / (d2 + d1 F), to ``dps`` digits as an mpf - or None where it is PROVEN below 1e-300.
    mpmath's betainc does not converge for large a; the hypergeometric series z^a 2F1(a, 1 - b; a + 1; z) / (a B(a, b))
    does, on the side where z < 1/2 (the other side by I_x(a, b) = 1 - I_y(b, a)).  The proof of smallness, which spares
    the series with millions of terms: 2F1(a + b, 1; a + 1; x) has term ratios (a + b + k) x / (a + 1 + k) <= rho =
    max(x, x (a + b) / (a + 1)), so for rho < 1   I_x(a, b) <= x^a y^b / (a B(a, b) (1 - rho))."""
    import mpmath

    with mpmath.workdps(dps + 30):
        a, b = mpmath.mpf(d2) / 2, mpmath.mpf(d1) / 2
        t = mpmath.mpf(d1) * mpmath.mpf(F)
        x, y = mpmath.mpf(d2) / (mpmath.mpf(d2) + t), t / (mpmath.mpf(d2) + t)
        lB = mpmath.loggamma(a) + mpmath.loggamma(b) - mpmath.loggamma(a + b)
        rho = max(x, x * (a + b) / (a + 1))
        if rho < 1:
            bound = a * mpmath.log(x) + b * mpmath.log(y) - mpmath.log(a) - lB - mpmath.log(1 - rho)
            if bound < mpmath.log(mpmath.mpf("1e-300")) - 1:
                return None
        if x < 0.5:
            return mpmath.exp(a * mpmath.log(x) - lB) * _series(a, 1 - b, a + 1, x, dps) / a
        return 1 - mpmath.exp(b * mpmath.log(y) - lB) * _series(b, 1 - a, b + 1, y, dps) / b


def f_sf_grid():
    """[(d1, d2, F array, truths as mpf)] over the grid, F = 0 and the points whose truth is below 1e-300 left out.
    Computed once per process (a few seconds)."""
    if "f" not in _cache:
        import mpmath

        rows = []
        for d1 in F_D1:
            for d2 in F_D2:
                pts = [(F, f_sf_truth(F, d1, d2)) for F in F_F if F > 0]
                pts = [(F, t) for F, t in pts if t is not None and t >= mpmath.mpf("1e-300")]
                rows.append((d1, d2, np.array([F for F, _ in pts]), [t for _, t in pts]))
        _cache["f"] = rows
    return _cache["f"]


def f_sf_check(fn, label, c_bound):
    """fn(F array, d1, d2) -> survival function; prints the measured c, asserts c <= c_bound and returns it."""
    import mpmath

    worst, where, n = 0.0, None, 0
    with mpmath.workdps(60):
        for d1, d2, Fs, truths in f_sf_grid():
            if len(Fs) == 0:
                continue
            out = fn(Fs, d1, d2)
            for F, o, tv in zip(Fs, out, truths):
                c = float(abs(mpmath.mpf(float(o)) - tv) / tv) / (EPS * (1.0 + abs(float(mpmath.log(tv)))))
                n += 1
                if c > worst:
                    worst, where = c, (d1, d2, float(F), float(tv))
    print(f"{label}: c = {worst:.1f} at (d1, d2, F, p) = {where} over {n} points; bound {c_bound}")
    assert n >= 150
    assert worst <= c_bound, (worst, where, c_bound)
    return worst


def deviance_truth(counts, sf, X, disp, beta, dps=50):
    """(D_f, S) per gene in mpmath from the double inputs taken exactly: D = sum d(y, mu), mu = sf exp(X beta), and
    S = sum(|term1| + |term2|) of the issue's error convention.  counts: samples x genes."""
    import mpmath

    N, G = counts.shape
    D, S = [], []
    with mpmath.workdps(dps):
        Xm = [[mpmath.mpf(float(v)) for v in row] for row in np.asarray(X, float)]
        for g in range(G):
            r = 1 / mpmath.mpf(float(disp[g]))
            b = [mpmath.mpf(float(v)) for v in beta[g]]
            d = s = mpmath.mpf(0)
            for n in range(N):
                mu = mpmath.mpf(float(sf[n])) * mpmath.exp(mpmath.fsum(x * c for x, c in zip(Xm[n], b)))
                y = mpmath.mpf(int(counts[n, g]))
                if y > 0:
                    t1, t2 = 2 * y * mpmath.log(y / mu), 2 * (y + r) * mpmath.log((y + r) / (mu + r))
                    d += t1 - t2
                    s += abs(t1) + abs(t2)
                else:
                    t = 2 * r * mpmath.log1p(mu / r)
                    d += t
                    s += t
            D.append(d)
            S.append(s)
    return D, S


def unit_deviance_truth(y, mu, r, dps=50):
    """(d, |term1| + |term2|) of one count in mpmath."""
    import mpmath

    with mpmath.workdps(dps):
        y, mu, r = mpmath.mpf(float(y)), mpmath.mpf(float(mu)), mpmath.mpf(float(r))
        if y > 0:
            t1, t2 = 2 * y * mpmath.log(y / mu), 2 * (y + r) * mpmath.log((y + r) / (mu + r))
            return t1 - t2, abs(t1) + abs(t2)
        t = 2 * r * mpmath.log1p(mu / r)
        return t, t


def ql_scenario(N, G=200, seed=5, outlier=False, spread=0.5):
    """Counts with gene-specific dispersions spread around a trend (a log-normal factor of sd ``spread`` = 0.5: the
    quasi-likelihood dispersions then vary by more than their sampling error, so the moderation finds a finite df0 -
    checked by the tests; spread = 0: every gene at the trend, and with few genes the sample variance of log s2 can fall
    below trigamma(df / 2): df0 = infinity).
    N = 6: ~condition (3 + 3); otherwise ~batch + condition, two levels each in balanced cells.  A third of the genes has
    no condition effect.  outlier: gene 5 gets one huge count (replaced and refitted when min_replicates allows).
    Returns (counts DataFrame samples x genes, metadata, X, X_reduced, contrast vector, trend dispersion of the truth)."""
    i = np.arange(N)
    rng = np.random.default_rng(seed)
    if N == 6:
        meta = pd.DataFrame({"condition": np.where(i % 2 == 0, "x", "y")}, index=[f"s{k}" for k in i])
        X = np.column_stack([np.ones(N), i % 2 == 1]).astype(float)
        beta = np.vstack([rng.normal(6.0, 1.0, G), rng.normal(0, 0.6, G)])
    else:
        meta = pd.DataFrame({"batch": np.where(i % 2 == 0, "a", "b"), "condition": np.where((i // 2) % 2 == 0, "x", "y")},
                            index=[f"s{k}" for k in i])
        X = np.column_stack([np.ones(N), i % 2 == 1, (i // 2) % 2 == 1]).astype(float)
        beta = np.vstack([rng.normal(6.0, 1.0, G), rng.normal(0, 0.4, G), rng.normal(0, 0.6, G)])
    beta[-1, ::3] = 0.0
    trend = 4 / 2.0 ** beta[0] + 0.05
    disp = trend * np.exp(rng.normal(0, spread, G))
    sf = np.exp(rng.normal(0, 0.2, N))
    mu = sf[:, None] * 2.0 ** (X @ beta)
    counts = rng.negative_binomial(1 / disp[None, :], (1 / disp[None, :]) / (1 / disp[None, :] + mu)).astype(np.int64)
    if outlier:
        counts[7, 5] = 400 * counts[:, 5].max()
    counts = pd.DataFrame(counts, index=meta.index, columns=[f"g{j}" for j in range(G)])
    c = np.zeros(X.shape[1])
    c[-1] = 1.0
    return counts, meta, X, np.ascontiguousarray(X[:, :-1]), c, trend
