"""Cases, models and mpmath references of the apeGLM shrinkage (csrc/dsq_shrink.h, dsq_k_shrink.hip): the host tests
(tests/test_shrink_cases_host.py), the device unit (tests/test_devunit_shrink.py) and the product kernels' inverse
(tests/test_gpu_shrink_hessian.py).  Needs no GPU.  DESIGN.md 7e.

The objective (unscaled), d_n = eta_n + offset_n - log size, e_n = exp(-|d_n|), eta = X beta:

    f   = prior - sum_n [ y_n eta_n - (y_n + size) (max(eta_n + offset_n, log size) + log1p(e_n)) ]
    g_j = prior'_j - sum_n [ y_n - (y_n + size) sig(d_n) ] x_nj,          sig(d) = 1 / (1 + exp(-d))
    prior = sum_{j != s} beta_j^2 / (2 sigma0^2) + log1p((beta_s / sigma)^2)
    H   = X^T diag(fr) X + 1 h^T,   fr = (y + size) size e^(eta + offset) / (size + e^(eta + offset))^2,
          h_j = 1 / sigma0^2 (j != s), 2 (sigma^2 - beta_s^2) / (sigma^2 + beta_s^2)^2 (j == s): the reference adds h_j to
          EVERY row of column j (utils.py:1099-1110), so H is not symmetric

evaluated in mpmath at 50 digits from the float64 inputs read exactly.

Error scale.  No fp64 evaluation is closer to these values than a few roundings of its own terms:

    S_f   = sum_n [ |y eta| + (y + size) (|eta + offset| + |log size| + log1p(e)) ] + |prior terms|
    S_g,j = sum_n ( y + (y + size) sig(d) ) |x_nj| + |prior'_j|

and an inverse is judged as  ||D||_inf / (EPS kappa_inf ||H^-1||_inf).  Never a run of the code under test."""
import functools
from fractions import Fraction

import mpmath as mp
import numpy as np

from oracle import nbglm_oracle as orc

EPS = 2.0 ** -52
DPS = 50
SIGMA0 = 15.0
FR_BITS = 240  # (the Hessian's weights are > 2^-60 in these cases: 180 bits, 54 digits)

NARROW_P = (1, 2, 3, 4, 5, 8, 9, 12)  # shrink_fn<P>: the dense, the 8-lane and the 16-lane optimiser's widths and their edges
WIDE_P = (13, 16, 17, 24, 25, 32, 33, 40, 41, 48)  # shrink_fn_wide: p == PB and p == previous PB + 1
OBJ_SHAPES = ((3, 1), (63, 5), (64, 9), (65, 1), (130, 5))  # (N, G): fewer samples than lanes / columns, one pass +- 1, three passes
OBJ_SHAPES_WIDE = ((3, 5), (63, 1), (64, 1), (65, 9), (130, 1))
SIZES = (0.1, 1.0, 1e8)
SIGMAS = (1e-3, 1.0, 1e3)
COUNT_KINDS = ("zero", "ones", "byte", "short", "int_max")
BETA_KINDS = ("optimum", "start", "origin", "switch", "corner")
INT_MAX = 2 ** 31 - 1

HESS_P = tuple(range(1, 13)) + WIDE_P
HESS_SIGMAS = (0.05, 0.3, 1.0)

# Measured by tests/test_shrink_cases_host.py, which asserts every one of them again (units of EPS * S resp.
# EPS kappa_inf ||H^-1||_inf).  The reference's own error: the oracle's nbinom_fn / nbinom_grad (numpy) against mpmath, and
# numpy.linalg.inv of the oracle's Hessian against mpmath's inverse at the same coefficients.
R_F, R_G, R_INV = 2.2206, 51.818, 2.2609
# The device's bounds follow from them: 4 x resp. 8 x the reference's error, rounded up to a power of two.
K_F, K_G, K_INV = 16.0, 256.0, 32.0
# The host build's own worst ratios and the powers of two that cover them
HOST_F, HOST_G, HOST_INV = 3.2033, 15.981, 3.0041
K_H_F, K_H_G, K_H_INV = 4.0, 16.0, 4.0


def pow2_ceil(x):
    return 2.0 ** int(np.ceil(np.log2(x)))


def wide_inst(p):
    """(PMAX, PB) of the k_shrink_wide launch_shrink picks for p design columns"""
    return (16, 16) if p <= 16 else (32, 24) if p <= 24 else (32, 32) if p <= 32 else (48, 40) if p <= 40 else (48, 48)


def inst_of(p):
    return None if p <= 12 else wide_inst(p)


# ------------------------------------------------------------------------------------------------ objective cases
def _counts(rng, kind, N, mu):
    y = rng.negative_binomial(2.0, 2.0 / (2.0 + mu)).astype(np.int64)
    if kind == "zero":
        y[:] = 0
    elif kind == "ones":
        y = (rng.random(N) < 0.6).astype(np.int64)
        y[0] = 1
    elif kind == "byte":
        y[::2] = np.where(np.arange(N)[::2] % 4 == 0, 255, 256)
    elif kind == "short":
        y[::2] = np.where(np.arange(N)[::2] % 4 == 0, 65535, 65536)
    elif kind == "int_max":
        y[N // 2] = INT_MAX
    return y


def _obj_gene(rng, p, N, k, wide):
    """One gene: k picks the kinds in mixed radix, so the genes of one width run through their combinations."""
    ck, bk = COUNT_KINDS[k % 5], BETA_KINDS[(k // 5 + k) % 5]
    size, sigma = SIZES[k % 3], SIGMAS[(k // 3) % 3]
    sidx = (0, p // 2, p - 1)[k % 3] if wide else k % p
    sf = 10.0 ** rng.uniform(-1.0, 1.0, N)  # two decades
    offset = np.log(sf)
    X = np.column_stack([np.ones(N)] + [0.5 * rng.normal(size=N) for _ in range(p - 1)])
    b_true = np.concatenate([[rng.uniform(2.0, 6.0)], rng.normal(0, 0.4, p - 1)])
    y = _counts(rng, ck, N, np.minimum(sf * np.exp(X @ b_true), 1e6))
    if bk == "optimum":
        b = b_true
        if N >= p:
            bf = orc.nbinom_glm_gene(X, y.astype(float), size, offset, SIGMA0, sigma, sidx)[0]
            b = bf if np.isfinite(bf).all() and np.abs(bf).max() < 50 else b_true
    elif bk == "start":
        b = 0.1 * (-1.0) ** np.arange(p)
    elif bk == "origin":
        b = np.zeros(p)
    elif bk == "switch":
        # d = eta + offset - log size within 1e-9 of 0 for every third sample: both sides of the `d > 0` switch, and d = 0
        # up to the rounding of eta itself
        b = b_true * 0.5
        eta = X @ b
        n3 = np.arange(0, N, 3)
        offset[n3] = np.log(size) - eta[n3] + np.array([-1e-9, 0.0, 1e-9])[np.arange(n3.size) % 3]
    else:
        # the corners of grid_fit_shrink2's 60 x 60 grid, covariates scaled so that exp(-|d|) underflows on both sides
        X = 60.0 * rng.normal(size=(N, p))
        b = 30.0 * np.where((k >> (np.arange(p) % 8)) & 1, -1.0, 1.0)
        X[0, :], X[1 % N, :] = 60.0 * np.sign(b), -60.0 * np.sign(b)
    return dict(y=y, offset=offset, X=X, b=np.asarray(b, np.float64), size=size, sigma=sigma, sidx=sidx, counts=ck, beta=bk)


@functools.lru_cache(maxsize=None)
def objective_cases(p):
    """The launches of width p: a list of dicts with N, G and the genes' arrays y [G][N], offset [G][N], X [G][N][p],
    b [G][p], size / sigma / sidx [G] and the kinds (counts, beta) per gene.  Never changed by a test."""
    rng = np.random.default_rng(7100 + p)
    wide = p > 12
    out, k = [], p  # (the widths start their run through the kinds at different places)
    for N, G in (OBJ_SHAPES_WIDE if wide else OBJ_SHAPES):
        genes = []
        for _ in range(G):
            genes.append(_obj_gene(rng, p, N, k, wide))
            k += 1
        c = dict(p=p, N=N, G=G, inst=inst_of(p), sigma0=np.full(G, SIGMA0),
                 counts=[q["counts"] for q in genes], beta=[q["beta"] for q in genes])
        for key in ("y", "offset", "X", "b", "size", "sigma", "sidx"):
            c[key] = np.array([q[key] for q in genes])
            c[key].setflags(write=False)
        out.append(c)
    return out


def objective_ref(y, offset, X, b, size, sigma0, sigma, sidx):
    """(f, g [p], S_f, S_g [p], dmin, dmax): f and g as mpmath numbers, the scales as floats, the range of d"""
    N, p = X.shape
    with mp.workdps(DPS):
        bm = [mp.mpf(float(v)) for v in b]
        sz, s0, sg = mp.mpf(float(size)), mp.mpf(float(sigma0)), mp.mpf(float(sigma))
        lsz = mp.log(sz)
        s = mp.mpf(0)
        S = mp.mpf(0)
        gks, gas = [], []
        rows = [[mp.mpf(float(v)) for v in X[n]] for n in range(N)]
        dmin, dmax = mp.inf, -mp.inf
        for n in range(N):
            xr = rows[n]
            yv = mp.mpf(int(y[n]))
            eta = mp.fdot(xr, bm)
            eo = eta + mp.mpf(float(offset[n]))
            d = eo - lsz
            dmin, dmax = min(dmin, d), max(dmax, d)
            e = mp.exp(-abs(d))
            l1 = mp.log1p(e)
            s += yv * eta - (yv + sz) * (max(eo, lsz) + l1)
            S += abs(yv * eta) + (yv + sz) * (abs(eo) + abs(lsz) + l1)
            sig = (1 if d > 0 else e) / (1 + e)
            gks.append(yv - (yv + sz) * sig)
            gas.append(yv + (yv + sz) * sig)
        gr = [mp.fdot(gks, [r[j] for r in rows]) for j in range(p)]
        Sg = [mp.fdot(gas, [abs(r[j]) for r in rows]) for j in range(p)]
        prior = mp.log1p((bm[sidx] / sg) ** 2)
        for j in range(p):
            if j != sidx:
                prior += bm[j] ** 2 / (2 * s0 * s0)
        g = []
        for j in range(p):
            dp = 2 * bm[j] / (sg * sg + bm[sidx] ** 2) if j == sidx else bm[j] / (s0 * s0)
            g.append(dp - gr[j])
            Sg[j] += abs(dp)
        return prior - s, g, float(S + prior), np.array([float(v) for v in Sg]), float(dmin), float(dmax)


@functools.lru_cache(maxsize=None)
def objective_refs(p):
    """objective_ref of every gene of objective_cases(p): a list (launch) of lists (gene)"""
    return [[objective_ref(c["y"][k], c["offset"][k], c["X"][k], c["b"][k], c["size"][k], SIGMA0, c["sigma"][k],
                           int(c["sidx"][k])) for k in range(c["G"])] for c in objective_cases(p)]


def ratio(val, ref, S):
    """|val - ref| in units of EPS S, the difference taken in mpmath (inf for a NaN or infinite val)"""
    if not np.isfinite(val):
        return np.inf
    with mp.workdps(DPS):
        return float(abs(mp.mpf(float(val)) - ref) / (EPS * mp.mpf(S)))


def objective_ratios(c, refs, f, g):
    """worst (f, g) ratios of one launch's results f [G], g [G][>= p] against its references"""
    wf = max(ratio(f[k], refs[k][0], refs[k][2]) for k in range(c["G"]))
    wg = max(ratio(g[k][j], refs[k][1][j], refs[k][3][j]) for k in range(c["G"]) for j in range(c["p"]))
    return wf, wg


def oracle_objective(c, k):
    """(f, g) of gene k by the oracle (numpy): the reference whose own error sets the bounds"""
    a = (c["X"][k], c["y"][k].astype(np.float64), c["size"][k], c["offset"][k], SIGMA0, c["sigma"][k], int(c["sidx"][k]))
    with np.errstate(all="ignore"):
        return float(orc.nbinom_fn(c["b"][k], *a)), orc.nbinom_grad(c["b"][k], *a)


# ------------------------------------------------------------------------------------------------ Gauss-Jordan model
def gauss_jordan(H):
    """numpy.float64 model of the inverse both device versions compute (dsq_shrink.h): Gauss-Jordan with partial
    pivoting on [H | I], the pivot search from the diagonal down, replaced on strictly greater.  Returns (inverse,
    [(column, row) of every exchange])."""
    H = np.array(H, dtype=np.float64)
    p = H.shape[0]
    inv = np.eye(p)
    swaps = []
    for c in range(p):
        pv, mx = c, abs(H[c, c])
        for r in range(c + 1, p):
            if abs(H[r, c]) > mx:
                mx, pv = abs(H[r, c]), r
        if pv != c:
            H[[c, pv]], inv[[c, pv]] = H[[pv, c]], inv[[pv, c]]
            swaps.append((c, pv))
        d = 1.0 / H[c, c]
        H[c] *= d
        inv[c] *= d
        for r in range(p):
            if r != c:
                fct = H[r, c]
                H[r] = H[r] - fct * H[c]
                inv[r] = inv[r] - fct * inv[c]
    return inv, swaps


def moves_row(swaps, s):
    """an exchange put another row at position s"""
    return any(s in sw for sw in swaps)


# ------------------------------------------------------------------------------------------------ Hessian cases
TEETH = ((4.0, 0.25, 0.5, 1.0, 2.0), (0.25, 0.5, 1.0, 2.0, 4.0), (1.0, 2.0, 4.0, 0.25, 0.5))
# Beyond 12 columns milder teeth and larger counts: with sixteen-fold scales L-BFGS-B takes hundreds of iterations on the
# flat scaled objective, and the last bits of the loss then decide where two builds of the same optimiser stop
TEETH_WIDE = ((2.0, 0.5, 1.0), (0.5, 1.0, 2.0), (1.0, 2.0, 0.5))
# Seeds picked so that tests/test_shrink_cases_host.py's claims about the exchanges hold at every width (the design of a
# launch is shared by its genes, so whether its first column is exchanged is one draw per launch, not per gene)
SEED_BUMP = {4: 1, 12: 5, 32: 1, 33: 32}


def saw_tooth(p, i=0):
    """the covariates' scales: a saw-tooth over factors of two, so that later columns outweigh an earlier pivot; launch
    i starts the tooth at another place"""
    t = TEETH[i] if p <= 12 else TEETH_WIDE[i]
    return np.array([1.0] + [t[(j - 1) % len(t)] for j in range(1, p)])


def _hess_case(p, i):
    rng = np.random.default_rng(9300 + 10 * p + i + 1000 * SEED_BUMP.get(p, 0))
    # (N + 1 >= p: X^T F X + 1 h^T has rank <= N + 1)
    N = (5, 64 + (p & 1), 130)[i] if p <= 4 else (64, 65, 130)[(p + i) % 3]
    G = (9 if i == 1 else 5) if p <= 12 else 3 if p <= 32 else 1
    sidx = (0, p - 1, p // 2)[i]
    sigma = HESS_SIGMAS[i]
    s = saw_tooth(p, i)
    u = rng.normal(size=N)
    X = np.column_stack([np.ones(N)] + [s[j] * (0.6 * u + 0.8 * rng.normal(size=N)) for j in range(1, p)])
    sf = np.exp(rng.normal(0, 0.2, N))
    beta = np.vstack([rng.uniform(*((3.0, 6.0) if p <= 12 else (5.0, 8.0)), G)] + [rng.normal(0, 0.3 / (s[j] * np.sqrt(p)), G) for j in range(1, p)])
    disp = rng.uniform(0.05, 0.5, G)
    mu = sf[:, None] * np.exp(X @ beta)
    counts = rng.negative_binomial(1 / disp[None, :], 1 / (1 + disp[None, :] * mu)).astype(np.int64)
    c = dict(p=p, N=N, G=G, sidx=sidx, sigma=sigma, X=X, sf=sf, offset=np.log(sf), counts=counts, size=1 / disp)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def hessian_cases(p):
    """Three launches of width p (shrink index first / last / interior, prior scale 0.05 / 0.3 / 1): dicts with X [N][p],
    sf, offset [N], counts [N][G], size [G], sidx, sigma.  Never changed by a test."""
    return [_hess_case(p, i) for i in range(3)]


@functools.lru_cache(maxsize=None)
def oracle_fits(p):
    """orc.nbinom_glm_gene of every gene of hessian_cases(p): per launch (beta [G][p], inv_hessian [G][p][p], converged
    [G], H [G][p][p]: the oracle's float64 Hessian at its beta)"""
    out = []
    for c in hessian_cases(p):
        r = [orc.nbinom_glm_gene(c["X"], c["counts"][:, g].astype(np.float64), c["size"][g], c["offset"], SIGMA0,
                                 c["sigma"], c["sidx"]) for g in range(c["G"])]
        H = [orc.nbinom_hess(x[0], c["X"], c["counts"][:, g].astype(np.float64), c["size"][g], c["offset"], SIGMA0,
                             c["sigma"], c["sidx"]) for g, x in enumerate(r)]
        out.append((np.array([x[0] for x in r]), np.array([x[1] for x in r]), np.array([x[2] for x in r], bool), np.array(H)))
    return out


_inv_cache = {}
INV_BITS = 320


def _inverse(H):
    """Inverse of an mpmath matrix to the working precision: Newton's iteration X += X (I - H X) from numpy's inverse, in
    integers scaled by 2^INV_BITS (every step is exact but for the final shift; the residual is checked)."""
    p = H.rows
    one = 1 << (2 * INV_BITS)
    Hf = [[int(mp.nint(mp.ldexp(H[i, j], INV_BITS))) for j in range(p)] for i in range(p)]
    X0 = np.linalg.inv(np.array([[float(H[i, j]) for j in range(p)] for i in range(p)]))
    Xf = [[int(Fraction(float(v)) * 2 ** INV_BITS) for v in row] for row in X0]
    for _ in range(8):
        Xt = list(zip(*Xf))
        R = [[(one if i == j else 0) - sum(a * b for a, b in zip(Hf[i], Xt[j])) for j in range(p)] for i in range(p)]
        if max(abs(v) for row in R for v in row) >> (2 * INV_BITS - 200) == 0:  # ||I - H X||_max < 2^-200
            break
        Rt = list(zip(*R))
        Xf = [[Xf[i][j] + (sum(a * b for a, b in zip(Xf[i], Rt[j])) >> (2 * INV_BITS)) for j in range(p)] for i in range(p)]
    else:
        raise ArithmeticError("the Newton iteration for the reference inverse did not converge")
    return mp.matrix([[mp.ldexp(mp.mpf(v), -INV_BITS) for v in row] for row in Xf])


def hessian_ref(c, g, beta):
    """The reference's Hessian at beta and its inverse in mpmath: (H^-1 as an mpmath matrix, ||H^-1||_inf, kappa_inf).
    Cached per (case, gene, beta)."""
    key = (c["p"], c["N"], c["sidx"], g, np.asarray(beta, np.float64).tobytes())
    if key in _inv_cache:
        return _inv_cache[key]
    X, p, N, s = c["X"], c["p"], c["N"], c["sidx"]
    with mp.workdps(DPS):
        bm = [mp.mpf(float(v)) for v in beta]
        sz, s0, sg = mp.mpf(float(c["size"][g])), mp.mpf(SIGMA0), mp.mpf(float(c["sigma"]))
        # X^T diag(fr) X in integers: a float64 is an integer over a power of two, fr is kept to 2^-FR_BITS of its size
        shift = [max(Fraction(float(v)).denominator.bit_length() - 1 for v in X[:, j]) for j in range(p)]
        cols = [[int(Fraction(float(v)) * 2 ** shift[j]) for v in X[:, j]] for j in range(p)]
        fr = []
        for n in range(N):
            e = mp.exp(mp.fdot([mp.mpf(float(v)) for v in X[n]], bm) + mp.mpf(float(c["offset"][n])))
            f = (mp.mpf(int(c["counts"][n, g])) + sz) * sz * e / (sz + e) ** 2
            fr.append(int(mp.nint(mp.ldexp(f, FR_BITS))))
        b2, s2 = bm[s] ** 2, sg * sg
        hd = [2 * (s2 - b2) / (s2 + b2) ** 2 if j == s else 1 / (s0 * s0) for j in range(p)]
        H = mp.matrix(p, p)
        for i in range(p):
            wi = [f * x for f, x in zip(fr, cols[i])]
            for j in range(i + 1):
                v = mp.ldexp(mp.mpf(sum(a * x for a, x in zip(wi, cols[j]))), -(FR_BITS + shift[i] + shift[j]))
                H[i, j] = v + hd[j]
                H[j, i] = v + hd[i]
        Hi = _inverse(H)
        ni = mp.mnorm(Hi, mp.inf)  # (the largest row sum; mp.norm would take the largest entry)
        out = (Hi, float(ni), float(mp.mnorm(H, mp.inf) * ni))
    _inv_cache[key] = out
    return out


def inverse_ratio(inv, ref):
    """||inv - H^-1||_inf / (EPS kappa_inf ||H^-1||_inf) of a float64 inverse against hessian_ref's triple"""
    Hi, ni, kappa = ref
    inv = np.asarray(inv, np.float64)
    if not np.isfinite(inv).all():
        return np.inf
    p = inv.shape[0]
    with mp.workdps(DPS):
        err = max(sum(abs(mp.mpf(float(inv[i, j])) - Hi[i, j]) for j in range(p)) for i in range(p))
        return float(err / (EPS * kappa * ni))
