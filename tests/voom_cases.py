"""Inputs and bounds shared by the voom tests (host and GPU)."""
import math

import numpy as np
import pandas as pd

from pydeseq2_amd import synth
from tests import voom_ref as vr

EPS = 2.220446049250313e-16
C0 = math.log2(1e6)

# ---- Error constants.  Conventions, for one gene with kappa = cond_2(diag(sqrt w) X)^2 from the reference:
#   beta:    ||beta - truth||_2          <= C eps kappa ||truth||_2
#   est_k:   |est - truth|               <= C eps kappa ||c_k||_2 ||beta||_2     (est = c . beta may cancel to zero)
#   u_k:     |u - truth|                 <= C eps kappa u
#   sigma2:  |sigma2 - truth|            <= C eps sigma2                          (relative)
#   E_n:     |E - truth|                 <= C eps (|log2(y + 0.5)| + |off_n|)     (relative to the two terms E is the
#            difference of: log-CPM itself passes through zero, where no logarithm of a quotient has a relative error)
# C measured for the HOST build (x86-64, g++ -O2 -ffp-contract=off), once, over ALL 257 genes of all 42 (N, P) cases of
# kernel_case() against a truth in extended precision (x87 long double: normal equations and Cholesky at eps 1.1e-19),
# and against mpmath at 50 digits on every gene of the N = P + 1 cases up to P = 17 and a sample of the others: where both
# were taken they agree to three digits (sigma2 at (17, 16): 9585 and 9588).  tests/test_voom_host.py re-measures the
# genes of mp_cases() against mpmath and prints the values with -s.  Asserted for the host build at twice the measured
# value rounded up, for the device at four times it: the margins F_SF_C_HOST / F_SF_C_DEVICE of tests/ql_cases.py use (the
# device's Gram matrix runs through the matrix cores in another order of additions).
VOOM_C_HOST_MEASURED = 12.4  # est 12.4, beta 12.0 at (N, P) = (1000, 1) - a sum of a thousand terms at kappa = 1; u 2.24
VOOM_C_HOST = 25.0
VOOM_C_DEVICE = 50.0
# sigma2 and sigma1: the residuals are what is left of E after the fit, so their relative error grows with |E| / |residual|
# and is largest where one residual degree of freedom is left (N = P + 1): 9585 eps at (17, 16), 4852 eps for sigma1; the
# cases with N >= 63 stay below 36 eps (sigma2) and 21 eps (sigma1).
VOOM_C_REL_MEASURED = 9585.0
VOOM_C_REL_HOST = 19200.0
VOOM_C_REL_DEVICE = 38400.0
# E and Abar (the device's are the host's bits: one bound); beta1 against cond_2(X)^2 (sums of N products through pinv X)
VOOM_C_E_MEASURED = 1.6  # Abar 1.59; E itself 0.91
VOOM_C_E = 3.2
VOOM_C_FIT1_MEASURED = 10.5  # (18, 17)
VOOM_C_FIT1 = 21.0
KAPPA_MAX = 1e6  # the condition on the test designs (checked on the CPU: test_voom_host.py)

KERNEL_P = (1, 2, 12, 13, 16, 17, 48)
KERNEL_G = (1, 3, 4, 5, 257)
KERNEL_K = (1, 3)


def kernel_N(P):
    return (P + 1, 63, 64, 65, 129, 1000)


def design(N, P, rng):
    """N x P, intercept first, of full rank and well conditioned at any N > P (also N = P + 1): orthonormal columns
    scaled to unit entries, mixed by a mild upper-triangular matrix so that the design is not orthogonal."""
    A = np.column_stack([np.ones(N), rng.normal(size=(N, P - 1))]) if P > 1 else np.ones((N, 1))
    Q, R = np.linalg.qr(A)
    Q = Q * np.sign(np.diag(R))[None, :] * math.sqrt(N)
    T = np.eye(P) + np.triu(rng.uniform(-0.3, 0.3, (P, P)), 1) / math.sqrt(P)
    X = Q @ T
    X[:, 0] = 1.0
    return np.ascontiguousarray(X)


_cache = {}


def kernel_case(N, P, G=257, K=3):
    """Inputs of both kernels: counts (samples x genes; rows containing zeros, gene 1 without counts when G > 1), library
    sizes, offsets, design, pinv, a knot table of 17 knots over the range of the fitted values, K contrasts (the first a
    single coefficient, the others dense).  One per (N, P), cached; slice the genes and the contrasts for smaller G, K."""
    key = (N, P)
    if key not in _cache:
        rng = np.random.default_rng(100000 + 1000 * N + P)
        X = design(N, P, rng)
        beta = rng.normal(0, 0.5 / math.sqrt(P), (P, G))
        beta[0] = rng.uniform(1.0, 10.0, G)
        mu = 2.0 ** (X @ beta)
        counts = rng.poisson(mu * rng.gamma(4.0, 0.25, (N, G))).astype(np.int64)
        counts[::5, ::3] = 0
        counts[:, 1] = 0
        L = np.maximum(counts.sum(1), 1).astype(float) * np.exp(rng.normal(0, 0.1, N))
        off = np.log2(L + 1.0) - C0
        kx = np.linspace(-2.0, 14.0, 17)
        ky = 0.45 + 1.2 / (1.0 + np.exp(0.6 * (kx - 4.0))) + 0.01 * np.cos(kx)
        c = rng.normal(size=(K, P))
        c[0] = 0.0
        c[0, P - 1] = 1.0
        _cache[key] = dict(counts=counts, L=L, off=off, X=X, pinv=np.ascontiguousarray(np.linalg.pinv(X)), kx=kx, ky=ky,
                           contrasts=np.ascontiguousarray(c))
    return _cache[key]


def mp_cases():
    """(N, P, genes) whose host results are held against mpmath: small shapes at every width class and chunk count."""
    return [(3, 2, (0, 2, 3)), (65, 2, (0, 2, 3)), (14, 13, (0, 2)), (64, 13, (0, 4)), (129, 17, (0, 5)), (100, 48, (0, 7))]


def voom_scenario(G=400, N=24, seed=11):
    """The end-to-end scenario: synth.synth_counts at a two-factor p = 4 design (condition x batch, 2 and 3 levels) with
    the metadata that rebuilds it, five genes without counts.  -> (counts DataFrame, metadata, formula)."""
    counts, X = synth.synth_counts(G, N, "2factor", seed=seed)
    cond = np.where(X[:, 1] > 0, "b", "a")
    batch = np.where(X[:, 2] > 0, "y", np.where(X[:, 3] > 0, "z", "x"))
    idx = [f"s{k}" for k in range(N)]
    counts[:, [3, 50, 51, 200, G - 1]] = 0
    meta = pd.DataFrame({"condition": cond, "batch": batch}, index=idx)
    return pd.DataFrame(counts, index=idx, columns=[f"g{j}" for j in range(G)]), meta, "~condition + batch"


def scenario_design(meta):
    c, b = meta["condition"].to_numpy(), meta["batch"].to_numpy()
    return np.column_stack([np.ones(len(c)), c == "b", b == "y", b == "z"]).astype(float)


def check_against_reference(kc, got, c_abs, c_rel, label, G=None, K=None, ref=None):
    """beta, sigma2, est, u, E of ``got`` (b1, am, s1, beta, s2, est, u, E, w: the layers gene-major or None) against the
    float64 reference with the bounds of tests/voom_cases.py at the constants given; NaN exactly where the reference has
    it (the reference is refined in extended precision: its own error is far inside them).  ``ref``: vr.wls of the whole
    case, else computed here.  Prints the largest ratios; returns them and the reference used."""
    b1, _, _, beta, s2, est, u, E, w = got
    counts, c = kc["counts"][:, :G], kc["contrasts"][:K]
    if ref is None:
        ref = vr.wls(counts, kc["X"], kc["L"], b1, kc["kx"], kc["ky"], c)
    else:  # the reference of all genes and contrasts of the case (from the same beta1), cut down
        ref = {k: (v[:G] if k in ("beta", "sigma2", "kappa") else v[:G, :K] if k in ("est", "u") else v[:, :G])
               for k, v in ref.items()}
    live = ~np.isnan(ref["sigma2"])
    assert np.array_equal(live, ~np.isnan(s2)) and np.array_equal(live, ~np.isnan(b1).any(1))
    assert np.isnan(beta[~live]).all() and np.isnan(est[~live]).all() and np.isnan(u[~live]).all()
    kap, nb = ref["kappa"][live], np.linalg.norm(ref["beta"][live], axis=1)
    r_beta = np.linalg.norm(beta[live] - ref["beta"][live], axis=1) / (EPS * kap * nb)
    r_est = np.abs(est[live] - ref["est"][live]) / (EPS * kap[:, None] * nb[:, None] * np.linalg.norm(c, axis=1)[None, :])
    r_u = np.abs(u[live] - ref["u"][live]) / (EPS * kap[:, None] * ref["u"][live])
    r_s2 = np.abs(s2[live] - ref["sigma2"][live]) / (EPS * ref["sigma2"][live])
    worst = dict(beta=r_beta.max(initial=0), est=r_est.max(initial=0), u=r_u.max(initial=0), sigma2=r_s2.max(initial=0))
    if E is not None:
        scale = np.abs(np.log2(counts + 0.5)) + np.abs(kc["off"])[:, None]
        r_E = np.abs(E.T - ref["E"])[:, live] / (EPS * scale[:, live])
        worst["E"] = r_E.max(initial=0)
        assert np.isnan(E[~live]).all() and np.isnan(w[~live]).all()
        assert np.allclose(w[live], ref["w"].T[live], rtol=1e-12, atol=0)
    print(f"{label}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f"  (bounds {c_abs} / {c_rel} / E {VOOM_C_E})")
    assert max(worst["beta"], worst["est"], worst["u"]) <= c_abs, worst
    assert worst["sigma2"] <= c_rel and worst.get("E", 0.0) <= VOOM_C_E, worst
    return worst, ref
