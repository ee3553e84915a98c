"""Cases and references of the parametric dispersion trend (csrc/dsq_trend.h, dsq_trend_grid.h, dsq_k_trend.hip): the host
comparison (tests/test_trend_cases_host.py) and the device unit (tests/test_devunit_trend.py).  Needs no GPU.

One evaluation at (a0, a1) over the kept genes, cov = 1 / mean, t = clip(disp) (numpy.clip: a NaN stays a NaN),
mu = a0 + a1 cov:

    f  =  nanmean(t / mu + log mu)            g0 = -nanmean((t / mu - 1) / mu)        g1 = -nanmean((t / mu - 1) cov / mu)

with one NaN-free count per mean (default_inference.py:209-217).  The initial mask drops the genes whose covariate is
NaN or infinite (dds.py:1225-1231), a filter pass at (a0, a1) those with t / mu outside [1e-4, 15) (dds.py:1254-1264).

References.  mpmath at 40 digits up to MP_MAX genes; beyond, the terms in numpy.longdouble and their sum with math.fsum
on the high and low halves of every term, taken twice so that the sum keeps more than a double
(tests/test_trend_cases_host.py checks this form against mpmath at every size up to MP_MAX).  Values come back as
numpy.longdouble.

Error scale (DESIGN 7c's convention): EPS S / count, S the sum of the absolute values of the terms as the kernels form
them - |t / mu| and |log mu| enter separately, the gradient's r = t / mu - 1 as |t / mu| + 1.

Never a run of the code under test."""
import math
import warnings

import mpmath as mp
import numpy as np

from oracle import nbglm_oracle as orc

EPS = 2.0 ** -52
MIN_DISP, MAX_DISP = 1e-8, 100.0
MP_DPS = 40
MP_MAX = 3073

# the capacities of the code: 512 threads x 4 register genes per workgroup, 32 workgroups, crossover at 3072
SIZES_ONE = (1, 2, 3, 12, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 3071)  # one workgroup; from 2049 on it spills
SIZES_GRID = (3072, 3073, 16383, 16384, 16385, 65535, 65536, 65537, 70001)     # 32 workgroups hold 65 536 in registers
SIZES_FORCED = (1, 65, 513)                                                    # the grid where most workgroups are empty
SIZES = SIZES_ONE + SIZES_GRID
KINDS = ("clean", "outliers", "nan_means", "flat", "at_min", "nan_disp")
RAW_SIZES = (65, 2048, 2049, 5000)

# Bounds in units of EPS S / count.  Host (tests/test_trend_cases_host.py measures and asserts them): the smallest powers
# of two over the worst ratios of hs.trend_eval.  Device: 4 x the host's measured worst ratio, rounded up to a power of
# two (DESIGN 7c's rule).  The host's worst f is a one-gene case at (1, 1): mu = 1 + 1 / mean is rounded to an ulp of 1
# while the terms are 0.085 and log mu = 0.009 - the unit does not count the rounding of mu itself.
HOST_WORST_F, HOST_WORST_G = 4.7094, 1.3940
K_H_F, K_H_G = 8.0, 2.0
K_D_F, K_D_G = 32.0, 8.0
COEF_TOL = 1e-9  # the fit against the oracle (the bound of tests/test_hostsim_stress.py)
# The device's fit against the oracle: the host tests' bound.  Measured on an MI355X, every launch shape: at most 8.9e-12
# in all 138 cases, which leaves more than the 4 x margin.
COEF_TOL_DEV = 1e-9
FACTR_EPS = 2.2e-9  # scipy's factr * eps = 1e7 * 2.2e-16: the stopping rule of both optimisers, relative to max(|f|, 1)


def pow2_ceil(x):
    return 2.0 ** math.ceil(math.log2(x))


# ------------------------------------------------------------------------------------------------ the data
def make(kind, n):
    """(genewise dispersions, normalised means) of one case, seeded by n: the kinds of
    tests/test_hostsim_stress.py::test_trend_fit_failure_modes_and_odd_inputs"""
    rng = np.random.default_rng(n)
    nm = np.exp(rng.normal(4, 2, n))
    true = 0.05 + 3.0 / nm
    noisy = true * np.exp(rng.normal(0, 0.3, n))
    idx = np.arange(n)
    if kind == "clean":
        return noisy, nm
    if kind == "outliers":
        noisy[::17] *= 1e4
        return noisy, nm
    if kind == "nan_means":  # every 9th NaN, and means of 0: an infinite covariate
        return noisy, np.where(idx % 9 == 0, np.nan, np.where(idx % 9 == 4, 0.0, nm))
    if kind == "flat":
        return np.full(n, 0.2) * np.exp(rng.normal(0, 0.05, n)), nm
    if kind == "at_min":
        true[: n // 2] = 1e-8
        return true * np.exp(rng.normal(0, 0.3, n)), nm
    if kind == "nan_disp":
        noisy[::13] = np.nan
        return noisy, nm
    raise ValueError(kind)


def make_raw(n):
    """(targets, covariates) of the one-fit mode: unclipped targets, NaN among them from 2049 genes on"""
    gw, nm = make("clean", n)
    if n >= 2049:
        gw[5::13] = np.nan
    return gw, 1.0 / nm


def clip(gw):
    with np.errstate(invalid="ignore"):
        return np.clip(gw, MIN_DISP, MAX_DISP)  # keeps NaN


def init_mask(means):
    with np.errstate(divide="ignore"):
        cov = 1.0 / np.asarray(means, np.float64)
    return np.isfinite(cov)


# ------------------------------------------------------------------------------------------------ high precision
def _ld(x):
    """an mpf as numpy.longdouble (through its high and low double)"""
    hi = float(x)
    if hi != hi or hi in (math.inf, -math.inf):
        return np.longdouble(hi)
    return np.longdouble(hi) + np.longdouble(float(x - hi))


def _fsum_ld(terms):
    """the sum of longdouble terms, exact to well below a double's rounding: fsum over the halves, then over the halves
    and the first result's negative"""
    if terms.size == 0:
        return np.longdouble(0.0)
    hi = terms.astype(np.float64)
    lo = (terms - hi.astype(np.longdouble)).astype(np.float64)
    parts = np.concatenate([hi, lo]).tolist()
    s1 = math.fsum(parts)
    s2 = math.fsum(parts + [-s1])
    return np.longdouble(s1) + np.longdouble(s2)


def _terms_mp(t, cov, a0, a1):
    """per gene (mpf): t / mu, log mu, 1 / mu, cov"""
    with mp.workdps(MP_DPS):
        A0, A1 = mp.mpf(a0), mp.mpf(a1)
        out = []
        for ti, ci in zip(t.tolist(), cov):
            mu = A0 + A1 * ci
            out.append((mp.mpf(ti) / mu, mp.log(mu), 1 / mu, ci))
        return out


def _cov(means, raw, use_mp):
    if use_mp:
        with mp.workdps(MP_DPS):
            return [mp.mpf(m) if raw else 1 / mp.mpf(m) for m in np.asarray(means, np.float64).tolist()]
    m = np.asarray(means, np.float64).astype(np.longdouble)
    return m if raw else 1 / m


def ref_eval(t, means, keep, a0, a1, raw=False, use_mp=None):
    """One evaluation over the genes keep (bool [n]) flags.  t: the targets as the fit sees them (clipped; NaN allowed),
    means: the normalised means (raw: the covariates themselves).  Returns a dict: f, g0, g1 (longdouble; NaN when the
    count is 0), cf, c0, c1, and the error units uf, ug0, ug1 = EPS S / count."""
    t = np.asarray(t, np.float64)
    keep = np.asarray(keep, bool)
    n = t.size
    use_mp = (n <= MP_MAX) if use_mp is None else use_mp
    ok = keep & ~np.isnan(t)  # mu is a positive number for every kept gene: only a NaN target makes a NaN term
    cnt = int(ok.sum())
    nan = np.longdouble(np.nan)
    if cnt == 0:
        return dict(f=nan, g0=nan, g1=nan, cf=0, c0=0, c1=0, uf=nan, ug0=nan, ug1=nan)
    ts, ms = t[ok], np.asarray(means, np.float64)[ok]
    if use_mp:
        with mp.workdps(MP_DPS):
            tr = _terms_mp(ts, _cov(ms, raw, True), a0, a1)
            f = mp.fsum(tm + lg for tm, lg, _, _ in tr)
            g0 = mp.fsum((tm - 1) * rm for tm, _, rm, _ in tr)
            g1 = mp.fsum((tm - 1) * c * rm for tm, _, rm, c in tr)
            sf = mp.fsum(abs(tm) + abs(lg) for tm, lg, _, _ in tr)
            s0 = mp.fsum((abs(tm) + 1) * rm for tm, _, rm, _ in tr)
            s1 = mp.fsum((abs(tm) + 1) * abs(c) * rm for tm, _, rm, c in tr)
            f, g0, g1, sf, s0, s1 = (_ld(v / cnt) for v in (f, -g0, -g1, sf, s0, s1))
    else:
        cov = _cov(ms, raw, False)
        mu = np.longdouble(a0) + np.longdouble(a1) * cov
        tm, lg, rm = ts.astype(np.longdouble) / mu, np.log(mu), 1 / mu
        f, g0, g1 = _fsum_ld(tm + lg), -_fsum_ld((tm - 1) * rm), -_fsum_ld((tm - 1) * cov * rm)
        sf, s0, s1 = _fsum_ld(np.abs(tm) + np.abs(lg)), _fsum_ld((np.abs(tm) + 1) * rm), \
            _fsum_ld((np.abs(tm) + 1) * np.abs(cov) * rm)
        f, g0, g1, sf, s0, s1 = (v / cnt for v in (f, g0, g1, sf, s0, s1))
    return dict(f=f, g0=g0, g1=g1, cf=cnt, c0=cnt, c1=cnt, uf=EPS * sf, ug0=EPS * s0, ug1=EPS * s1)


THRESHOLD_MARGIN = 1e-9


def ref_filter(t, means, keep, a0, a1):
    """The mask after one filter pass at (a0, a1): a kept gene leaves when t / (a0 + a1 / mean) is < 1e-4 or >= 15; a NaN
    ratio stays.  Raises if a ratio lies within THRESHOLD_MARGIN (relative) of a threshold, where fp64 roundings could
    decide: the kept counts are compared exactly."""
    t = np.asarray(t, np.float64).astype(np.longdouble)
    m = np.asarray(means, np.float64).astype(np.longdouble)
    keep = np.asarray(keep, bool)
    with np.errstate(all="ignore"):
        r = t / (np.longdouble(a0) + np.longdouble(a1) / m)
        for thr in (np.longdouble(1e-4), np.longdouble(15.0)):
            close = keep & (np.abs(r / thr - 1) < THRESHOLD_MARGIN)
            if close.any():
                raise AssertionError(f"a ratio within {THRESHOLD_MARGIN} of {float(thr)}: choose other data")
        return keep & ~((r < np.longdouble(1e-4)) | (r >= np.longdouble(15.0)))


def ratio(val, ref, unit):
    """|val - ref| / unit; 0 where both are NaN, inf where one is"""
    v, r = np.longdouble(val), np.longdouble(ref)
    if np.isnan(v) or np.isnan(r):
        return 0.0 if (np.isnan(v) and np.isnan(r)) else math.inf
    if v == r:
        return 0.0
    return float(np.abs(v - r) / unit)


# ------------------------------------------------------------------------------------------------ the fit
def oracle_fit(gw, means):
    """orc.fit_parametric_trend's loop (dds.py:1199-1275) on the clipped dispersions, restated to keep what the engine
    reports beside it: ok, n_outer, coef (the last fit's, also of a failed fit), n_kept and kept (the genes of the LAST
    fit, bool [n])."""
    t = clip(np.asarray(gw, np.float64))
    means = np.asarray(means, np.float64)
    with np.errstate(divide="ignore"):
        cov_all = 1 / means
    sel = np.nonzero(init_mask(means))[0]
    old, coef = np.array([0.1, 0.1]), np.array([1.0, 1.0])
    n_outer, ok, last = 0, True, sel
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        while (coef > 1e-10).all() and (np.log(np.abs(coef / old)) ** 2).sum() >= 1e-6:
            old = coef
            coef, pred, conv = orc.trend_gamma_glm(cov_all[sel], t[sel])
            coef = np.asarray(coef)
            n_outer += 1
            last = sel
            if not conv or (coef <= 1e-10).any():
                ok = False
                break
            with np.errstate(invalid="ignore"):
                r = t[sel] / pred
                sel = sel[~((r < 1e-4) | (r >= 15))]
    kept = np.zeros(t.size, bool)
    kept[last] = True
    return dict(ok=ok, n_outer=n_outer, coef=coef, n_kept=int(last.size), kept=kept)


_cache = {}


def case(kind, n):
    """gw, means, t (clipped), fit (oracle_fit) of one case; computed once"""
    key = (kind, n)
    if key not in _cache:
        gw, means = make(kind, n)
        _cache[key] = dict(kind=kind, n=n, gw=gw, means=means, t=clip(gw), fit=oracle_fit(gw, means))
    return _cache[key]


def points(c):
    """(1, 1), the oracle's optimum, 1.5 x it, and the bound (1e-12, 1e-12) where mu is tiny"""
    o = c["fit"]["coef"]
    return [(1.0, 1.0), (float(o[0]), float(o[1])), (1.5 * float(o[0]), 1.5 * float(o[1])), (1e-12, 1e-12)]


def ref_point(c, a0, a1):
    """The references of the sequence initial mask, eval, filter, eval at one point: dict with kept0, e0, kept1, e1"""
    key = (c["kind"], c["n"], a0, a1)
    if key not in _cache:
        k0 = init_mask(c["means"])
        e0 = ref_eval(c["t"], c["means"], k0, a0, a1)
        k1 = ref_filter(c["t"], c["means"], k0, a0, a1)
        e1 = ref_eval(c["t"], c["means"], k1, a0, a1)
        _cache[key] = dict(kept0=int(k0.sum()), e0=e0, kept1=int(k1.sum()), e1=e1)
    return _cache[key]


def worst_ratios(got, ref):
    """(f ratio, larger g ratio) of one evaluation {f, g0, g1} against ref_eval's dict"""
    return ratio(got["f"], ref["f"], ref["uf"]), max(ratio(got["g0"], ref["g0"], ref["ug0"]),
                                                      ratio(got["g1"], ref["g1"], ref["ug1"]))
