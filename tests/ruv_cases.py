"""Seeded inputs of the hidden-batch tests (tests/test_ruv_host.py, tests/test_gpu_ruv.py).

Shapes: the smallest at which the kernels of csrc/dsq_proj.h can go wrong - N around the wavefront (1, 2, 63, 64, 65, 129),
every edge of the launch plan +- 1 and one row beyond the LDS path, G in {1, 5, 67} (less than, more than and no multiple
of the four genes of a workgroup), q around the chunks of eight columns and at its limit, P in {1, 2, 8, 13, 49}.  Every
matrix has a row pitch above N; the padding of the inputs holds NaN (or a count that must never be read), that of the
outputs a guard value."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

PAD_COUNT = 2_000_000_000   # in the padding of a row of counts
GUARD = -7.25               # what an output holds before the call
NS = (1, 2, 63, 64, 65, 129)
GS = (1, 5, 67)
QS = (1, 2, 7, 8, 9, 64)
PS = (1, 2, 8, 13, 49)
PLAN_EDGES = (1024, 4800, 9664, 16320)   # the last N of a row in registers and of 4, 2 and 1 wavefronts per workgroup with
                                         # their rows in LDS (proj_plan)
BEYOND_LDS = 20000
MIN_DISP, MAX_DISP = 1e-8, 10.0


def padded(a, extra, fill):
    """rows of `a` with `extra` more columns of `fill`"""
    out = np.full((a.shape[0], a.shape[1] + extra), fill, dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return np.ascontiguousarray(out)


# ---------------------------------------------------------------------------------------------------------- log counts
@dataclass
class LogCase:
    name: str
    y: np.ndarray        # [G][ldn] int32
    sf: np.ndarray
    N: int
    normalized: bool
    eps: float


def log_cases():
    out = []
    k = 0
    for N in NS:
        for normalized, eps in ((True, 1.0), (False, 1.0), (True, 0.5), (True, 1e-3)):
            G = GS[k % 3]
            rng = np.random.default_rng(1000 + k)
            sf = np.exp(rng.normal(0, 0.3, N))
            sf[::3] = rng.choice([0.5, 1.0, 2.0], len(sf[::3]))
            y = rng.negative_binomial(2, 2 / (2 + rng.choice([0.3, 5.0, 3000.0], (G, 1)) * sf[None, :]))
            y[:, ::5] = 0
            if G > 1:
                y[1] = 0                       # a gene without counts: log(eps) throughout
                y[2, :] = rng.integers(0, 3, N)  # y / sf + eps in [0.5, 1) now and then (flog_t's absolute form)
            y[-1, -1] = 2**31 - 1
            out.append(LogCase(f"N{N}-G{G}-{'norm' if normalized else 'raw'}-eps{eps}", padded(y.astype(np.int32), 3, PAD_COUNT),
                               sf, N, normalized, eps))
            k += 1
    return out


# ----------------------------------------------------------------------------------------------------------- residuals
@dataclass
class ResCase:
    name: str
    y: np.ndarray        # [G][ldn] int32
    sf: np.ndarray
    Xt: np.ndarray       # [P][ldx], NaN in the padding
    beta: np.ndarray     # [G][P]
    disp: np.ndarray
    N: int
    P: int
    nan_rows: tuple      # genes that must come back as NaN rows


def _res_case(name, rng, N, G, P):
    sf = np.exp(rng.normal(0, 0.25, N))
    X = np.ones((N, P))
    X[:, 1:] = rng.normal(0, 1, (N, P - 1))
    if P > 1:
        X[:, 1] = np.arange(N) % 2
    beta = np.zeros((G, P))
    beta[:, 0] = rng.choice([-1.0, 2.0, 6.0], G)
    beta[:, 1:] = rng.normal(0, 0.5 / np.sqrt(P), (G, P - 1))
    disp = np.exp(rng.uniform(np.log(1e-3), np.log(2.0), G))
    mu = sf[None, :] * np.exp(beta @ X.T)
    y = rng.negative_binomial(1 / disp[:, None], 1 / (1 + disp[:, None] * mu))
    nan_rows = []
    if G >= 5:
        y[1] = 0; nan_rows.append(1)             # no counts
        beta[2, P - 1] = np.nan; nan_rows.append(2)
        disp[3] = np.nan; nan_rows.append(3)
        disp[0], disp[4] = MIN_DISP, MAX_DISP
    if G >= 67:
        beta[10, 0], beta[11, 0] = 30.0, -30.0   # mu at the clamp of the coefficients
        beta[10, 1:], beta[11, 1:] = 0.0, 0.0
        y[11] = 0; y[11, 0] = 1
        y[12, 1:] = 0                            # a single count
    return ResCase(name, padded(y.astype(np.int32), 2, PAD_COUNT), sf, padded(np.ascontiguousarray(X.T), 3, np.nan), beta,
                   disp, N, P, tuple(nan_rows))


def res_cases():
    out = []
    k = 0
    for N in NS:
        for P in PS:
            G = GS[k % 3] if P <= 13 else (1, 5)[k % 2]
            out.append(_res_case(f"N{N}-G{G}-P{P}", np.random.default_rng(2000 + k), N, G, P))
            k += 1
    # y == mu to the last bit: P = 1, x = 1, beta = 0 (fexp_t(0) = 1 exactly) and size factors that are the counts
    N = 65
    rng = np.random.default_rng(2999)
    y = rng.integers(1, 2000, (3, N))
    y[1:] = y[0]
    y[2, ::2] += 1
    c = ResCase("equal", padded(y.astype(np.int32), 2, PAD_COUNT), y[0].astype(np.float64), padded(np.ones((1, N)), 3, np.nan),
                np.zeros((3, 1)), np.array([0.1, MIN_DISP, MAX_DISP]), N, 1, ())
    out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------------- projection
@dataclass
class ProjCase:
    name: str
    x: np.ndarray        # [G][ld], NaN in the padding
    Pt: np.ndarray       # [q][ldp], NaN in the padding
    Bt: np.ndarray
    N: int
    q: int
    eps: float

    @property
    def G(self):
        return self.x.shape[0]


def _proj_case(name, rng, N, G, q, pad=3):
    """q <= 2: x like log counts and two unrelated random matrices.  q > 2: the projection as RUV and batch removal use it,
    B random, P = pinv(B)^T and x = B a + noise - the output is the small residual of the fit, so sum_j |c_j B_nj| stays
    far above |out| (q - 2) / (q + 3), the condition of ruv_ref's output bound."""
    Bm = rng.normal(0, 1.0, (N, q))
    if q <= 2:
        x = rng.normal(5.0, 2.0, (G, N))
        Pm = rng.normal(0, 1.0, (N, q)) / N
    else:
        x = rng.normal(0, 3.0, (G, q)) @ Bm.T + 0.05 * rng.normal(0, 1.0, (G, N))
        Pm = np.linalg.pinv(Bm).T
    if G > 1:
        x[1] = 0.0  # a row of zeros stays a row of zeros
    return ProjCase(name, padded(x, pad, np.nan), padded(np.ascontiguousarray(Pm.T), pad + 2, np.nan),
                    padded(np.ascontiguousarray(Bm.T), pad + 2, np.nan), N, q, 1.0)


def proj_small_cases():
    out = []
    k = 0
    for N in NS:
        for q in QS:
            out.append(_proj_case(f"N{N}-G{GS[k % 3]}-q{q}", np.random.default_rng(3000 + k), N, GS[k % 3], q, pad=(0, 3)[k % 2]))
            k += 1
    return out


def proj_long_cases():
    """Each edge of the launch plan +- 1, the LDS path at wider q, and one row length beyond the LDS path."""
    out = []
    k = 0
    for e in PLAN_EDGES:
        for N in (e - 1, e, e + 1):
            out.append(_proj_case(f"N{N}-G5-q2", np.random.default_rng(3500 + k), N, 5, 2))
            k += 1
    for k, (N, q) in enumerate(((1025, 7), (1025, 9), (1500, 64))):   # the LDS path through every chunk width (8, 4, 2, 1)
        out.append(_proj_case(f"N{N}-G5-q{q}", np.random.default_rng(3550 + k), N, 5, q))
    out.append(_proj_case(f"N{BEYOND_LDS}-G3-q2", np.random.default_rng(3600), BEYOND_LDS, 3, 2))
    out.append(_proj_case(f"N{BEYOND_LDS}-G3-q9", np.random.default_rng(3601), BEYOND_LDS, 3, 9))
    return out


# ----------------------------------------------------------------------------------------------------------- behaviour
@dataclass
class Cohort:
    seed: int
    counts: np.ndarray   # N x G
    cond: np.ndarray
    batch: np.ndarray
    sf_true: np.ndarray
    controls: np.ndarray


def cohort(seed, N=24, G=400, nctl=100, planted=1):
    """N samples, G genes, the last nctl of them null controls, a balanced two-level hidden batch (orthogonal to the
    condition) with N(0, 0.7^2) log effects on every gene, controls included; NB counts with dispersion 0.05.
    ``planted`` > 1 adds further balanced hidden factors with effects of 0.7 / 2^(i-1)... each (for the gap conditions)."""
    rng = np.random.default_rng(seed)
    cond = np.arange(N) % 2
    batch = (np.arange(N) // 2) % 2
    base = np.exp(rng.normal(5.0, 1.0, G))
    beta_c = np.zeros(G)
    de = rng.choice(G - nctl, (G - nctl) // 4, replace=False)
    beta_c[de] = rng.choice([-1.0, 1.0], len(de))
    gam = rng.normal(0, 0.7, G)
    sf = np.exp(rng.normal(0, 0.2, N))
    sf /= np.exp(np.log(sf).mean())
    eta = np.outer(cond, beta_c) + np.outer(batch - 0.5, gam)
    for i in range(1, planted):
        f = (np.arange(N) // (2 ** (i + 1))) % 2
        eta = eta + np.outer(f - 0.5, rng.normal(0, 0.7 / 1.6 ** i, G))
    mu = sf[:, None] * base[None, :] * np.exp(eta)
    a = 0.05
    y = rng.negative_binomial(1 / a, 1 / (1 + a * mu))
    return Cohort(seed, y, cond, batch, sf, np.arange(G - nctl, G))


SEEDS = (0, 1, 2, 3, 4, 5)
MIN_CORR, MAX_LEFT = 0.95, 0.1   # |corr(W_1, batch)| and the batch effect left in Y' relative to that of Y


def batch_effect(M, batch):
    """mean over the genes of |mean of batch 1 - mean of batch 0| of an N x G matrix"""
    return float(np.abs(M[batch == 1].mean(0) - M[batch == 0].mean(0)).mean())


@lru_cache(maxsize=None)
def behaviour_case(seed):
    """The cohort and the restatement's RUVg (k = 1) of it; asserts first that the restatement ALONE stays within the
    limits the engine is held to."""
    from tests import ruv_ref as rr

    c = cohort(seed)
    sf = rr.size_factors(c.counts)
    Y = np.log(c.counts / sf[:, None] + 1.0)
    W, d, Yp, alpha = rr.ruvg(Y, c.controls, 1)
    r = abs(np.corrcoef(W[:, 0], c.batch)[0, 1])
    left = batch_effect(Yp, c.batch) / batch_effect(Y, c.batch)
    assert r >= MIN_CORR and left <= MAX_LEFT, (seed, r, left)
    return c, sf, Y, W, d, Yp, alpha
