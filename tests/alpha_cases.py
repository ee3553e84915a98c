"""Cases and the mpmath reference of the dispersion objective (csrc/dsq_alpha.h, dsq_k_alpha_rows.hip,
dsq_k_alpha_rowsc.hip): the host comparison (tests/test_alpha_objective_host.py) and the device unit
(tests/test_devunit_alpha.py).  Needs no GPU.

The objective in log alpha, alpha = exp(la), a = 1 / alpha, w_n = mu_n / (1 + mu_n alpha):

    f = n a log(alpha) + sum_n [ -(lgamma(y+a) - lgamma(y+1) - lgamma(a)) + (y+a) log(a+mu) - y log(mu) ]   nb_nll
        + 1/2 log det(X^T W X)                                                                               Cox-Reid
        + (la - la_hat)^2 / (2 prior_var)                                                                    prior
    g = -alpha a^2 sum_n [ psi(a) - psi(y+a) + log(1 + mu alpha) + (y - mu) / (mu + a) ]                    alpha dnb_nll
        + 1/2 alpha tr((X^T W X)^-1 X^T dW X),  dW = -W^2
        + (la - la_hat) / prior_var

(pydeseq2's nb_nll / dnb_nll and fit_alpha_mle's loss / dloss), evaluated in mpmath at tests/devunit/ref.py's MP_PREC.

Error scale.  An fp64 evaluation cannot be closer to these values than a few rounding errors of its own TERMS, and the
terms of the engine are larger than the result: S_f and S_g are the sums of the absolute values of the terms as the
kernels form them,

    per sample   y <= 9:  |lgamma(a) - lgamma(y+a)| (one logarithm of an exact product),
                 y >= 10: |lgamma(a)| + |lgamma(y+a)|  (both sides take the difference of two evaluations);
                 |y| (|L1| + |log alpha|) + |a L1|,  L1 = log1p(mu alpha);  |lgamma(y+1)| + |y log mu|  (the constant)
    S_g: a times [the digamma terms likewise, |L1|, |(y - mu) alpha / (1 + mu alpha)|]  (alpha a^2 = a)
    plus |1/2 log det|, |1/2 alpha tr(M^-1 dM)| and the prior terms.

Never a run of the code under test."""
import math

import mpmath as mp
import numpy as np

from tests.devunit.ref import MP_PREC

EPS = 2.0 ** -52
MIN_MU = 0.5
MIN_DISP = 1e-8
SMALL_COUNT = 9  # dsq_alpha.h kSmallCount: exact recurrences up to here, Stirling differences beyond

# Bounds in units of EPS * S.  Host (tests/test_alpha_objective_host.py measures and asserts them): the smallest powers of
# two that cover the worst ratios of hs.alpha_eval.  Device: 4 x the host's measured worst ratio, rounded up to a power
# of two - the device replaces libm's log / exp / lgamma by the table and Stirling forms (<= 1 ulp each,
# tests/test_devunit_math.py) and sums per lane, then across 64 lanes.
HOST_WORST_F, HOST_WORST_G = 0.9115, 4.1384
K_H_F, K_H_G = 1.0, 8.0
K_D_F, K_D_G = 4.0, 32.0

NS = (1, 15, 16, 17, 63, 64, 65, 150, 257)
EDGE_COUNTS = (0, 1, 9, 10, 63, 64, 127, 128, 255, 256, 257, 511, 512, 513, 65533)


# ------------------------------------------------------------------------------------------------ mu_hat
def mu_linear(sf, X, coef, min_mu=MIN_MU):
    """max(sf (x . coef), min_mu) with the sum of products formed left to right in fp64 as the kernels' staging loops form
    it.  (For designs of zeros and ones every product is exact, so a fused multiply-add gives the same bits.)"""
    X = np.asarray(X, np.float64)
    yh = np.zeros(X.shape[0])
    for j in range(X.shape[1]):
        yh = yh + X[:, j] * float(coef[j])
    return np.maximum(np.asarray(sf, np.float64) * yh, min_mu)


def mu_cells(sf, cell_of, cell_mu):
    """sf * cell_mu[cell], unclamped (the IRLS route)"""
    return np.asarray(sf, np.float64) * np.asarray(cell_mu, np.float64)[np.asarray(cell_of)]


# ------------------------------------------------------------------------------------------------ the reference
_cache = {}


def _key(y, mu, X, la):
    return (np.asarray(y, np.int64).tobytes(), np.asarray(mu, np.float64).tobytes(),
            np.asarray(X, np.float64).tobytes(), np.asarray(X).shape, float(la))


def parts(y, mu, X, la):
    """The three parts of the objective at la, each (f, g, S_f, S_g) with f, g mpmath numbers and S floats: 'nll', 'cr'
    (None where X^T W X is singular, e.g. fewer samples than columns), and 'prior' as a function (la_hat, prior_var) ->
    the same tuple.  Cached per (gene, design, la): the references are shared by every test that needs them."""
    k = _key(y, mu, X, la)
    if k in _cache:
        return _cache[k]
    y = np.asarray(y, np.int64)
    muf = np.asarray(mu, np.float64)
    X = np.asarray(X, np.float64)
    n = len(y)
    with mp.workprec(MP_PREC):
        lam = mp.mpf(float(la))
        alpha = mp.exp(lam)
        a = 1 / alpha
        lga, psa = mp.loggamma(a), mp.digamma(a)
        per_count = {}
        for c in np.unique(y):
            c = int(c)
            lgz, psz = mp.loggamma(c + a), mp.digamma(c + a)
            if c <= SMALL_COUNT:
                sl, sd = abs(lga - lgz), abs(psa - psz)
            else:
                sl, sd = abs(lga) + abs(lgz), abs(psa) + abs(psz)
            per_count[c] = (lgz, psz, sl, sd, mp.loggamma(c + 1))
        f = n * a * lam
        gs = mp.mpf(0)
        Sf = mp.mpf(0)
        Sg = mp.mpf(0)
        w = []
        for yi, m in zip(y.tolist(), muf.tolist()):
            lgz, psz, sl, sd, lgy1 = per_count[yi]
            m = mp.mpf(m)
            lm = mp.log(m)
            f += -(lgz - lgy1 - lga) + (yi + a) * mp.log(a + m) - yi * lm
            L1 = mp.log1p(m * alpha)
            r1 = 1 / (1 + m * alpha)
            gs += psa - psz + L1 + (yi - m) / (m + a)
            Sf += sl + yi * (abs(L1) + abs(lam)) + abs(a * L1) + abs(lgy1) + abs(yi * lm)
            Sg += sd + abs(L1) + abs((yi - m) * alpha * r1)
            w.append(m * r1)
        g = -alpha * a * a * gs
        nll = (f, g, float(Sf), float(a * Sg))
        # Cox-Reid: X^T W X = sum over the design's distinct rows of (sum of w) x x^T
        P = X.shape[1]
        rows, inv = np.unique(X, axis=0, return_inverse=True)
        inv = np.asarray(inv).ravel()
        ws = [mp.mpf(0)] * len(rows)
        dws = [mp.mpf(0)] * len(rows)
        for wi, r in zip(w, inv.tolist()):
            ws[r] += wi
            dws[r] -= wi * wi
        M, dM = mp.zeros(P), mp.zeros(P)
        for r, x in enumerate(rows.tolist()):
            for i in range(P):
                if x[i] == 0.0:
                    continue
                for j in range(i + 1):
                    if x[j] == 0.0:
                        continue
                    t = mp.mpf(x[i]) * mp.mpf(x[j])
                    M[i, j] += t * ws[r]
                    dM[i, j] += t * dws[r]
        for i in range(P):
            for j in range(i):
                M[j, i], dM[j, i] = M[i, j], dM[i, j]
        cr = None
        if n >= P and np.linalg.matrix_rank(X) == P:
            det = mp.det(M)
            Mi = mp.inverse(M)
            tr = mp.mpf(0)
            for i in range(P):
                for j in range(P):
                    tr += Mi[i, j] * dM[j, i]
            fc, gc = mp.log(det) / 2, alpha * tr / 2
            cr = (fc, gc, float(abs(fc)), float(abs(gc)))

        def prior(la_hat, prior_var):
            with mp.workprec(MP_PREC):
                d = lam - mp.mpf(float(la_hat))
                pv = mp.mpf(float(prior_var))
                fp, gp = d * d / (2 * pv), d / pv
                return fp, gp, float(abs(fp)), float(abs(gp))

    out = {"nll": nll, "cr": cr, "prior": prior}
    _cache[k] = out
    return out


def objective(y, mu, X, la, la_hat=0.0, prior_var=1.0, cr_reg=True, prior_reg=False):
    """(f, g, S_f, S_g): f and g as mpmath numbers at MP_PREC, the error scales as floats"""
    p = parts(y, mu, X, la)
    terms = [p["nll"]]
    if cr_reg:
        assert p["cr"] is not None, "X^T W X is singular"
        terms.append(p["cr"])
    if prior_reg:
        terms.append(p["prior"](la_hat, prior_var))
    with mp.workprec(MP_PREC):
        return (mp.fsum(t[0] for t in terms), mp.fsum(t[1] for t in terms), sum(t[2] for t in terms),
                sum(t[3] for t in terms))


def nll_constant(y, mu):
    """(sum lgamma(y+1) - y log mu, sum of the absolute terms)"""
    with mp.workprec(MP_PREC):
        c, S = mp.mpf(0), mp.mpf(0)
        for yi, m in zip(np.asarray(y).tolist(), np.asarray(mu, np.float64).tolist()):
            t1, t2 = mp.loggamma(yi + 1), yi * mp.log(mp.mpf(m))
            c += t1 - t2
            S += abs(t1) + abs(t2)
        return c, float(S)


def ratio(got, ref, S):
    """|got - ref| in units of EPS * S"""
    with mp.workprec(MP_PREC):
        return float(abs(mp.mpf(float(got)) - ref) / (mp.mpf(EPS) * mp.mpf(S)))


def pow2_ceil(v):
    return 2.0 ** math.ceil(math.log2(v)) if v > 0 else 1.0


# ------------------------------------------------------------------------------------------------ designs
def treatment_cells(P):
    """P cells of a one-factor design in treatment coding: x_0 = e_0, x_c = e_0 + e_c"""
    Xc = np.zeros((P, P))
    Xc[:, 0] = 1.0
    for c in range(1, P):
        Xc[c, c] = 1.0
    return Xc


def binary_cells(P, C, seed=0):
    """C distinct non-zero rows of zeros and ones, rank P (a design's cells need not form a full factorial)"""
    rng = np.random.default_rng(1000 * P + C + seed)
    assert C <= 2 ** P - 1
    for _ in range(1000):
        codes = 1 + rng.choice(2 ** P - 1, C, replace=False)
        Xc = np.zeros((C, P))
        for j in range(P):
            Xc[:, j] = (codes >> j) & 1
        if np.linalg.matrix_rank(Xc) == P and np.linalg.cond(Xc.T @ Xc) < 1e4:
            return Xc
    raise AssertionError("no full-rank cell set found")


def cell_tables(Xc):
    """XX [C][T]: x_i x_j of the cells' rows, packed lower triangle in the engine's order tri(i, j) = i (i + 1) / 2 + j"""
    C, P = Xc.shape
    ii = [i for i in range(P) for j in range(i + 1)]
    jj = [j for i in range(P) for j in range(i + 1)]
    return np.ascontiguousarray(Xc[:, ii] * Xc[:, jj])


def design(P, N, cells=False):
    """X [N][P] and the cell of every sample: treatment coding of a permutation of n mod P.  cells = False: the last
    column also carries a covariate of five levels that are no binary fractions (the general path's p (p + 1) / 2
    accumulators see products that round; few distinct rows keep the reference's X^T W X cheap)."""
    Xc = treatment_cells(P)
    cell_of = (np.arange(N) * 7 + 3) % P if N >= P else np.arange(N) % P
    X = Xc[cell_of].copy()
    if not cells and P >= 2:
        X[:, P - 1] += 0.375 * np.cos(1.0 + np.arange(N) % 5)
    return X, cell_of.astype(np.int32), Xc


# ------------------------------------------------------------------------------------------------ genes
def required_nb(y):
    """memo blocks k_alpha picks from the gene's largest count"""
    return min(4, (int(np.max(y)) >> 6) + 1)


def nb_counts(rng, mu, alpha):
    r = 1.0 / alpha
    return rng.poisson(rng.gamma(r, np.asarray(mu) / r)).astype(np.int64)


def make_gene(kind, N, seed):
    """One gene of N samples: (y, mu, alpha_true).  kind:
      'max63' ... 'max257', 'max513': NB counts capped at that value, which at least one sample holds, with the edges
          below it placed on further samples (a memo block boundary on each side)
      'big': counts >= 256 up to 65 533 mixed with counts of every memo block
      'single': all zero but one count (1, 9 or 10 by seed)
      'clamp': low mean, mu at the min_mu clamp for most samples
      'plain': unmodified NB counts."""
    rng = np.random.default_rng(seed)
    sf = rng.uniform(0.5, 2.0, N)
    alpha = float(rng.choice([0.01, 0.05, 0.3, 1.5]))
    if kind == "single":
        mu = np.maximum(sf * 0.2, MIN_MU)
        y = np.zeros(N, np.int64)
        y[seed % N] = (1, 9, 10)[seed % 3]
        return y, mu, alpha
    if kind == "clamp":
        mu = np.maximum(sf * 0.3, MIN_MU)
        y = nb_counts(rng, mu, alpha)
        return y, mu, alpha
    if kind == "plain":
        mu = np.maximum(sf * 30.0, MIN_MU)
        return nb_counts(rng, mu, alpha), mu, alpha
    if kind == "big":
        q = 200.0
        cap = 65533
        forced = [5, 70, 130, 200, 256, 257, 511, 512, 513, 65533, 255, 1000, 63, 64, 127, 128]
    else:
        cap = int(kind[3:])
        q = cap / 2.0
        forced = [cap] + [c for c in EDGE_COUNTS if c < cap][::-1]
    mu = np.maximum(sf * q, MIN_MU)
    y = np.minimum(nb_counts(rng, mu, alpha), cap)
    pos = rng.permutation(N)
    for p, c in zip(pos, forced):
        y[p] = c
    return y, mu, alpha


KINDS = ("max63", "max64", "max127", "max128", "max255", "max256", "max257", "big", "single", "clamp", "plain", "max513")


def eval_las(alpha_true, N, half):
    """la in {log alpha_true, log alpha_true +- 1, log 1e-8, -15, -8, 3, log N}: the even or the odd half"""
    la0 = math.log(alpha_true)
    full = [la0, la0 + 1.0, la0 - 1.0, math.log(MIN_DISP), -15.0, -8.0, 3.0, math.log(N)]
    return full[half::2]


def eval_cases(P, cells=False):
    """[(name, y, mu, X, cell_of, Xc, la, la_hat, prior_var)] for the direct evaluations at width P: every kind of gene,
    N cycling through NS (N >= P + 1, and N = 1 at P = 1), each gene at four of the eight la values."""
    ns = [N for N in NS if N >= P + 1]
    out = []
    for i, kind in enumerate(KINDS):
        N = ns[(i + P) % len(ns)]
        y, mu, at = make_gene(kind, N, 100 * P + i)
        X, cell_of, Xc = design(P, N, cells)
        for la in eval_las(at, N, i % 2):
            out.append((f"P{P}-{kind}-N{N}", y, mu, X, cell_of, Xc, la, math.log(at) + 0.5, 0.25 + 0.5 * (i % 3)))
    if P == 1:
        for i, c in enumerate((0, 1, 10, 300)):
            y, mu = np.array([c], np.int64), np.array([max(0.7 * c, MIN_MU)])
            X, cell_of, Xc = design(1, 1, cells)
            for la in (-2.0, math.log(MIN_DISP), 0.0):
                out.append((f"P1-one-sample-{c}", y, mu, X, cell_of, Xc, la, -1.0, 1.0))
    return out


# ------------------------------------------------------------------------------------------------ row-kernel cases
# (route, P, C, N): k_alpha_rows<P> (P = C), k_alpha_rows_c<P> from coefficients ("coef") and from per-cell mu_hat
# ("cell_mu").  N = 600 at (8, 30) makes the many-cell kernel take its 256-entry tail table; the others take 512.
ROW_DESIGNS = [("rows", 1, 1, 17), ("rows", 2, 2, 33), ("rows", 3, 3, 65), ("rows", 4, 4, 150),
               ("coef", 3, 5, 33), ("coef", 5, 6, 65), ("coef", 8, 30, 600), ("coef", 8, 32, 70),
               ("cell_mu", 3, 3, 17), ("cell_mu", 8, 30, 70)]
ROWSC_TAIL = {("coef", 3, 5, 33): 512, ("coef", 5, 6, 65): 512, ("coef", 8, 30, 600): 256, ("coef", 8, 32, 70): 512,
              ("cell_mu", 3, 3, 17): 512, ("cell_mu", 8, 30, 70): 512}
ROW_TAIL = 512  # dsq_launch.h kRowTail
# the MAP fit (prior term on, centred at alpha_hat as the product centres it): one design per kernel and route
ROW_PRIOR_DESIGNS = [("rows", 2, 2, 33), ("coef", 8, 32, 70), ("cell_mu", 3, 3, 17)]
ROW_PRIOR_VAR = 0.5
ROW_RUNS = [(s, False) for s in ROW_DESIGNS] + [(s, True) for s in ROW_PRIOR_DESIGNS]


def row_run_id(run):
    s, prior = run
    return f"{s[0]}-P{s[1]}-C{s[2]}-N{s[3]}" + ("-prior" if prior else "")
# generator seeds with which the host optimiser evaluates no point twice in its first ten evaluations (a line search that
# falls back to its best point does): tests/test_alpha_objective_host.py checks it
ROW_SEEDS = {("coef", 5, 6, 65): 1, ("coef", 8, 30, 600): 1, ("cell_mu", 8, 30, 70): 5}


def row_case(route, P, C, N, n_genes=12, seed=None):
    """One launch's inputs: dict with y [G][N], sf, cell_of, Xc, XX, coef or cell_mu, mu [G][N] (what the kernel forms),
    X [N][P], alpha_true, alpha_hat, tail.  Genes alternate between counts around the tail table's size (tail - 1,
    tail, tail + 1 and up to 65 533: the second sweep) and counts below it; gene 1 is all zero but one count, gene 2 sits
    at the min_mu clamp (coefficient routes)."""
    if seed is None:
        seed = ROW_SEEDS.get((route, P, C, N), 0)
    rng = np.random.default_rng(7919 * P + 31 * C + N + seed)
    tail = ROW_TAIL if route == "rows" else ROWSC_TAIL[(route, P, C, N)]
    Xc = treatment_cells(P) if route == "rows" or C == P else binary_cells(P, C)
    cell_of = rng.permutation(np.arange(N) % C).astype(np.int32)
    sf = rng.uniform(0.5, 2.0, N)
    G = n_genes
    y = np.zeros((G, N), np.int64)
    mu = np.zeros((G, N))
    coef = np.zeros((G, P))
    cell_mu = np.zeros((G, C))
    at = np.zeros(G)
    for g in range(G):
        at[g] = float(rng.choice([0.02, 0.1, 0.4, 1.2]))
        level = [tail / 2.0, 20.0, 3.0, 150.0][g % 4]
        if g == 1:
            level = 0.3
        if g == 2:
            level = 0.2
        if route == "cell_mu":
            cell_mu[g] = level * rng.uniform(0.6, 1.6, C)
            mu[g] = mu_cells(sf, cell_of, cell_mu[g])
        else:
            coef[g] = level * rng.uniform(0.3, 0.9, P) / max(1.0, P / 3.0)
            coef[g, 0] = level * 0.6
            mu[g] = mu_linear(sf, Xc[cell_of], coef[g])
        y[g] = nb_counts(rng, mu[g], at[g])
        if g == 1:
            y[g] = 0
            y[g, N // 2] = 10
        elif g % 4 == 0:
            forced = [tail - 1, tail, tail + 1, 65533 if g % 8 == 0 else 4 * tail, 1, 0, 9, 10]
            for p, c in zip(rng.permutation(N), forced):
                y[g, p] = c
        else:
            y[g] = np.minimum(y[g], tail - 1)  # no second sweep for this gene
    return dict(route=route, P=P, C=C, N=N, G=G, y=y, mu=mu, sf=sf, cell_of=cell_of, Xc=Xc, XX=cell_tables(Xc),
                coef=coef, cell_mu=cell_mu, X=Xc[cell_of], alpha_true=at, tail=tail, min_disp=MIN_DISP,
                max_disp=float(max(10, N)), min_mu=MIN_MU)


def row_genes(spec):
    """genes per launch: fewer at the long rows (the reference costs N per evaluation)"""
    return 8 if spec[3] >= 600 else 12


def choose_alpha_hat(case, prior_reg=False, prior_var=1.0):
    """alpha_hat per gene with |g(log alpha_hat)| > 1e-3 by the reference alone: alpha_true e^(+-1), pushed further out
    until the reference's gradient says so.  With prior_reg the prior is centred at alpha_hat (as the product does), so
    the gradient there is the likelihood's."""
    ah = np.zeros(case["G"])
    for g in range(case["G"]):
        s = 1.0 if g % 2 == 0 else -1.0
        for k in range(1, 6):
            cand = min(max(case["alpha_true"][g] * math.exp(s * k), 2 * case["min_disp"]), case["max_disp"] / 2)
            la = math.log(cand)
            _, gr, _, _ = objective(case["y"][g], case["mu"][g], case["X"], la, la, prior_var, True, prior_reg)
            if abs(float(gr)) > 1e-3:
                break
        else:
            raise AssertionError(f"gene {g}: no start with |g| > 1e-3")
        ah[g] = cand
    return ah


def queue_case(n_distinct=50, N=20, P=2):
    """The distinct genes of the slot / queue test (k_alpha_rows<P>): high-count genes (counts >= 512 up to 65 533: the
    second sweep, a long tail table, n_big > 0) alternate with genes that are zero but for one small count (a tail table
    of one or two entries, n_big = 0), so that a slot refilled from the queue meets what the other kind left behind."""
    rng = np.random.default_rng(4242)
    Xc = treatment_cells(P)
    cell_of = (np.arange(N) % P).astype(np.int32)
    sf = rng.uniform(0.5, 2.0, N)
    y = np.zeros((n_distinct, N), np.int64)
    coef = np.zeros((n_distinct, P))
    ah = np.zeros(n_distinct)
    for g in range(n_distinct):
        if g % 2 == 0:
            level = float(rng.choice([300.0, 2000.0, 20000.0]))
            coef[g] = level * np.array([0.6] + [0.4] * (P - 1))
            at = float(rng.choice([0.05, 0.3, 1.0]))
            mu = mu_linear(sf, Xc[cell_of], coef[g])
            y[g] = np.minimum(nb_counts(rng, mu, at), 65533)
            y[g, rng.integers(N)] = (512, 513, 65533, 1000)[(g // 2) % 4]
            ah[g] = at * math.exp(1.0 if g % 4 == 0 else -1.0)
        else:
            coef[g] = 0.3 * np.array([0.6] + [0.4] * (P - 1))
            y[g, rng.integers(N)] = (1, 2, 9, 10)[(g // 2) % 4]
            ah[g] = (0.01, 0.5)[(g // 2) % 2]
    return dict(route="rows", P=P, C=P, N=N, G=n_distinct, y=y, sf=sf, cell_of=cell_of, Xc=Xc, coef=coef, alpha_hat=ah,
                min_disp=MIN_DISP, max_disp=float(max(10, N)), min_mu=MIN_MU)
