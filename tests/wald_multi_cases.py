"""Shared inputs of the multi-contrast Wald tests (host build and GPU): the contrast set of a fixture, the alternatives
with the null values of tests/test_gpu_parity.py, the oracle's reference (computed once per fixture and alternative),
and the tolerances of the Wald KAT test."""
import functools

import numpy as np

from oracle import nbglm_oracle as orc
from tests.helpers import load_kat

# (alt_hypothesis, lfc_null on the log2 scale), tests/test_gpu_parity.py:117
ALTS = ((None, 0.0), ("greater", 0.5), ("less", -0.5), ("greaterAbs", 0.5), ("lessAbs", 0.5))
ALT_CODE = {None: 0, "greaterAbs": 1, "lessAbs": 2, "greater": 3, "less": 4}
# tests/test_gpu_parity.py:120-122
TOL = {"se": (1e-10, 0.0), "stat": (1e-9, 1e-13), "p": (1e-8, 1e-300)}


def contrast_set(k):
    """The fixture's own contrast, every unit vector, one pairwise difference of two columns (designs with at least two
    columns), four dense seeded-normal vectors: P + 6 contrasts (P = 1: 6)."""
    P = k["X"].shape[1]
    rows = [np.asarray(k["contrast"], dtype=float)] + list(np.eye(P))
    if P >= 2:
        d = np.zeros(P)
        d[P - 1], d[P // 2 - (P == 2)] = 1.0, -1.0  # last column against a middle one (P = 2: against the intercept)
        rows.append(d)
    rows += list(np.random.default_rng(1000 + P).normal(size=(4, P)))
    return np.ascontiguousarray(np.stack(rows))


@functools.lru_cache(maxsize=None)
def kat(case):
    """(k, disp, mu, ridge, contrasts) of kat_<case>.npz with the Wald inputs test_inference_vs_reference_kats uses."""
    k = load_kat(case)
    N, P = k["X"].shape
    disp = np.clip(k["map_alpha"], 1e-8, float(max(10, N)))
    mu = np.exp(k["X"] @ k["lfc_beta"].T) * k["sf"][:, None]
    return k, disp, mu, np.diag(np.repeat(1e-6, P)), contrast_set(k)


@functools.lru_cache(maxsize=None)
def oracle_ref(case, alt):
    """(p, stat, se), each K x G, of orc.wald_test for every contrast of the set; computed once, read-only."""
    k, disp, mu, ridge, cons = kat(case)
    null = dict(ALTS)[alt]
    out = [np.stack(a) for a in zip(*(orc.wald_test(k["X"], disp, k["lfc_beta"], mu, ridge, c, np.log(2) * null, alt)
                                       for c in cons))]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def excess(a, b, rtol, atol):
    """max of |a - b| / (atol + rtol |b|) (1 = at the tolerance); NaN / inf patterns must agree."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape
    fin = np.isfinite(b)
    assert (np.isnan(a) == np.isnan(b)).all() and (a[~fin & ~np.isnan(b)] == b[~fin & ~np.isnan(b)]).all()
    err, tol = np.abs(a[fin] - b[fin]), atol + rtol * np.abs(b[fin])
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(err == 0.0, 0.0, err / tol)  # (an exact zero, e.g. the SE of an all-zero gene, has tolerance 0)
    return float(frac.max()) if fin.any() else 0.0


def check(got, ref, what):
    """got / ref: (p, stat, se); every entry within TOL.  Returns the largest fractions of the tolerances used."""
    used = {}
    for name, g, r in zip(("p", "stat", "se"), got, ref):
        used[name] = excess(g, r, *TOL[name])
        assert used[name] <= 1.0, f"{what}: {name} at {used[name]:.3g} of its tolerance"
    return used
