"""Seeded inputs of the adaptive-shrinkage tests (host build and GPU), with the dense restatement's answer computed once
per set (tests/ash_ref, run on to min grad >= -1e-13), and the checks both builds are held to.

Constructions (G genes): plain - s = exp(N(-1.5, 0.6)), 30 % of the genes carry an effect N(0, 1), b = effect + s N(0, 1);
null - b = 0.5 s N(0, 1), so that no b^2 exceeds s^2 and sigma_max = 8 sigma_min; heavy - effects 2 t_2; wide-se - log s ~
N(-1.5, 2.5), effects N(0, 3) (a grid of about 45 components).  The NaN / zero-SE variant of a set makes 10 % of its genes
unused (NaN or infinite LFC, NaN, zero or negative SE), among them the first and the last gene and, from G = 192 on, the
whole chunk of genes 64 ... 127.  forced(M): the plain set of 203 genes on a grid of exactly M components.

Two sets of the G x construction table lie outside what the code takes and are kept as what they are.  wide-se at G = 3000
selects a grid of 56 components, more than DSQ_ASH_MAX_M = 48: the selection must refuse it (test_ash_host), and the fit
runs on the 48 widest of them.  heavy at G = 3000 does not meet the condition on the inputs under any seed tried (1 ... 6):
among 3000 draws of 2 t_2 one gene lies several hundred standard errors out, the first Newton step takes all weight off
the components only that gene needs, its u falls to 1e-106 and H to 1e212, and the scheme of the statement - the
restatement included - stops without converging.  breakdown() is that set: the builds must then say "not converged" and
still return proportions and finite posteriors ("limits")."""
import functools

import numpy as np

from tests import ash_ref

SIZES = (1, 2, 5, 63, 64, 65, 203, 3000)
KINDS = ("plain", "null", "heavy", "wide-se")
FORCED_M = (1, 16, 17, 32, 33, 48)
MAX_REF_ITER = 30  # condition on the inputs: the restatement converges within this many iterations on every set

# Largest difference of a build's posterior values from the restatement that the tests accept, relative to max(1, |value|):
# ten times the largest one measured over all sets on the two host builds, 8.56e-10 (lfsr, heavy G = 203 with unused genes,
# which stops at a KKT residual of 8.9e-9 where the restatement runs on to 1e-13; DESIGN.md 6i, "agreement").
POST_TOL = 8.6e-9


SEEDS = {"plain": 1, "null": 1, "heavy": 1, "wide-se": 10}


class Case:
    def __init__(self, name, b, s, sd=None, suitable=True):
        self.name, self.b, self.s = name, b, s
        self.ref = ash_ref.ash(b, s, sd)
        self.sd = self.ref["grid"]
        self.M = len(self.sd)
        assert self.M <= 48, f"{name}: the seeded inputs are unsuitable (M = {self.M})"
        if self.ref["n"] and suitable:
            assert self.ref["converged"] and self.ref["n_iter"] <= MAX_REF_ITER, \
                f"{name}: the seeded inputs are unsuitable ({self.ref['n_iter']} iterations of the restatement)"


def _draw(kind, G, seed):
    rng = np.random.default_rng([seed, G, KINDS.index(kind)])
    if kind == "wide-se":
        s = np.exp(rng.normal(-1.5, 2.5, G))
        eff = rng.normal(0, 3, G)
    else:
        s = np.exp(rng.normal(-1.5, 0.6, G))
        if kind == "plain":
            eff = np.where(rng.random(G) < 0.3, rng.normal(0, 1.0, G), 0.0)
        elif kind == "heavy":
            eff = 2.0 * rng.standard_t(2, G)
        else:
            return 0.5 * s * rng.normal(size=G), s
    return eff + s * rng.normal(size=G), s


@functools.lru_cache(maxsize=None)
def case(kind, G):
    b, s = _draw(kind, G, SEEDS[kind])
    sd = ash_ref.grid(b, s)[1]
    return Case(f"{kind} G={G}", b, s, sd[-48:] if len(sd) > 48 else None)


@functools.lru_cache(maxsize=None)
def breakdown():
    b, s = _draw("heavy", 3000, SEEDS["heavy"])
    c = Case("heavy G=3000", b, s, suitable=False)
    assert not c.ref["converged"]
    return c


@functools.lru_cache(maxsize=None)
def nan_case(kind, G):
    b, s = (a.copy() for a in _draw(kind, G, SEEDS[kind]))
    rng = np.random.default_rng([SEEDS[kind], G, 99])
    out = np.zeros(G, bool)
    out[[0, G - 1]] = True
    if G >= 192:
        out[64:128] = True
    rest = np.nonzero(~out)[0]
    extra = max(0, int(round(0.1 * G)) - int(out.sum()))
    out[rng.choice(rest, size=min(extra, len(rest) - 1), replace=False)] = True
    for j, g in enumerate(np.nonzero(out)[0]):
        how = j % 5
        if how == 0: b[g] = np.nan
        elif how == 1: s[g] = 0.0
        elif how == 2: s[g] = np.nan
        elif how == 3: b[g] = np.inf
        else: s[g] = -s[g]
    sd = ash_ref.grid(b, s)[1]
    return Case(f"{kind} G={G} with unused genes", b, s, sd[-48:] if len(sd) > 48 else None)


@functools.lru_cache(maxsize=None)
def forced(M, G=203):
    b, s = _draw("plain", G, 1)
    smax = 2 * np.sqrt((b * b - s * s).max())
    return Case(f"forced M={M}", b, s, np.sqrt(2.0) ** np.arange(-(M - 1), 1, dtype=float) * smax)


def all_cases():
    cs = [case(k, G) for k in KINDS for G in SIZES if (k, G) != ("heavy", 3000)]
    cs += [nan_case(k, G) for k, G in (("plain", 5), ("plain", 65), ("plain", 203), ("heavy", 203), ("wide-se", 3000))]
    return cs + [forced(M) for M in FORCED_M]


def loglik_tol(c):
    """Both fits stop with every d_m - 1 <= 1e-8, so each is within n 1e-8 of the maximum of sum_g log u_g (the duality
    gap of this problem is n max_m (d_m - 1)), and sum x is within 1e-8 of 1 (sum_m x_m d_m = 1 identically): n 3e-8, and
    the rounding of a sum of n terms."""
    return 3e-8 * c.ref["n"] + 1e-12 * abs(c.ref["loglik"])


def check(c, got, k=0, what="", tol=POST_TOL):
    """Row k of `got` (the arrays dsq_dev_ash writes, as tests/hostash.ash returns them) against the case: converged; the KKT
    residual recomputed here from the returned pi and a dense L at most 1e-8 (the stopping rule); sum pi = 1 within 1e-12
    and pi >= 0; loglik; the posterior values; NaN exactly on the unused genes.  Returns the largest differences."""
    what = f"{what} {c.name}"
    u = ash_ref.used(c.b, c.s)
    M = c.M
    pi = got["pi"][k][:M]
    assert got["converged"][k], f"{what}: not converged after {got['n_iter'][k]} iterations"
    assert 1 <= got["n_iter"][k] + 1 <= 101
    assert (pi >= 0).all() and abs(pi.sum() - 1.0) <= 1e-12, f"{what}: pi sums to {pi.sum()!r}"
    L, _ = ash_ref.lik(c.b[u], c.s[u], c.sd)
    res = ash_ref.kkt_residual(L, pi)
    assert res <= 1e-8, f"{what}: KKT residual {res:.3g}"
    assert abs(got["kkt"][k] - res) <= 2e-8, f"{what}: reported residual {got['kkt'][k]!r} vs {res!r}"
    assert abs(got["loglik"][k] - c.ref["loglik"]) <= loglik_tol(c), \
        f"{what}: loglik {got['loglik'][k]!r} vs {c.ref['loglik']!r}"
    worst = {}
    for key in ("post_mean", "post_sd", "lfsr"):
        a, e = got[key][k][:len(c.b)], c.ref[key]
        assert np.array_equal(np.isnan(a), ~u), f"{what}: {key} is NaN exactly on the unused genes"
        d = np.abs(a[u] - e[u]) / np.maximum(1.0, np.abs(e[u]))
        worst[key] = float(d.max())
        assert worst[key] <= tol, f"{what}: {key} differs by {worst[key]:.3g} (gene {np.nonzero(u)[0][d.argmax()]})"
    return worst
