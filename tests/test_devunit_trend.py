"""The trend fit as the device runs it (tests/devunit/devunit_trend.hip, csrc/dsq_trend_grid.h, csrc/dsq_k_trend.hip) in
every launch shape - one workgroup, the launcher's crossover, the cooperative grid of 32 - against the references of
tests/trend_cases.py: single passes through a probe driver (all 32 leaders' copies of every total), whole fits through
dsq::launch_trend_fit itself, the raw one-fit mode, k_trend, and the product's C API in its default shape.

Bounds: counts exact; f and g within K_D EPS S / count (tc.K_D_F = 32, tc.K_D_G = 8: 4 x the host's measured worst
ratio, rounded up to a power of two); coefficients within tc.COEF_TOL_DEV = 1e-9 of the oracle.  The exchange's timeout branch is
not tested and no input here is meant to make the workgroups disagree.

Every test prints its worst figures; DESIGN section 7d has the table an MI355X gave."""
import ctypes as C
import warnings

import numpy as np
import pytest

from oracle import nbglm_oracle as orc
from tests import trend_cases as tc

gpu = pytest.mark.gpu
SHAPES = (-1, 0, 1)  # launch_trend_fit's force_grid: one workgroup, the crossover at 3072 genes, the grid


@pytest.fixture(scope="module")
def du():
    from tests import devunit

    devunit.lib()
    return devunit


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def rel_coef(got, want):
    return float(np.max(np.abs(np.asarray(got) - want) / np.abs(want)))


# ------------------------------------------------------------------------------------------------ (a) single passes
def _check_eval(du, rec, tot_slice, e_slice, ref, where):
    """one eval of a probe record against ref_eval's dict: exact counts, f and g in error units"""
    tot = rec[tot_slice]
    assert tuple(tot[3:6]) == (ref["cf"], ref["c0"], ref["c1"]), where
    got = dict(zip(("f", "g0", "g1"), rec[e_slice]))
    return tc.worst_ratios(got, ref)


@gpu
@pytest.mark.parametrize("n", tc.SIZES)
def test_probe_passes_against_the_reference(du, n):
    """init_keep, eval, filter, eval at four points, on 1 and on 32 workgroups, every kind:
    - all 32 leaders hold the same bit pattern of every total of every pass, and the timeout flag is 0;
    - kept counts and NaN-free counts are exact; f and g lie within K_D EPS S / count of the reference;
    - the two shapes lie within 2 K_D of each other (each is within K_D of the truth).
    MI355X, worst over all sizes: f 4.71 in both shapes (the host's one-gene case; beyond it 1.20 on one
    workgroup, 1.24 on 32), g 1.76 in both; between the shapes f 2.21, g 1.47."""
    nb = du.trend_grid_blocks()
    # tc.SIZES sit at the edges of these capacities
    assert nb == 32 and du.trend_capacity(1) == 2048 and du.trend_capacity(nb) == 65536
    worst = {1: [0.0, 0.0], nb: [0.0, 0.0]}
    worst_between = [0.0, 0.0]
    for kind in tc.KINDS:
        c = tc.case(kind, n)
        pts = tc.points(c)
        recs = {}
        for blocks in (1, nb):
            out, timeout = du.trend_probe(blocks, c["gw"], c["means"], tc.MIN_DISP, tc.MAX_DISP, pts)
            assert timeout == 0, (kind, n, blocks)
            for b in range(1, blocks):
                assert same_bits(out[b], out[0]), (kind, n, blocks, b)
            recs[blocks] = out[0]
        for p, (a0, a1) in enumerate(pts):
            ref = tc.ref_point(c, a0, a1)
            for blocks in (1, nb):
                r = recs[blocks][p]
                where = (kind, n, blocks, a0, a1)
                assert r[du.PROBE_KEPT0] == ref["kept0"] and r[du.PROBE_KEPT1] == ref["kept1"], where
                assert r[du.PROBE_TOT_LOAD].tolist() == [ref["kept0"], 0, 0, 0, 0, 0], where
                assert r[du.PROBE_TOT_FILTER].tolist() == [ref["kept1"], 0, 0, 0, 0, 0], where
                for tot, e, want in ((du.PROBE_TOT_E0, du.PROBE_E0, ref["e0"]), (du.PROBE_TOT_E1, du.PROBE_E1, ref["e1"])):
                    rf, rg = _check_eval(du, r, tot, e, want, where)
                    worst[blocks][0] = max(worst[blocks][0], rf)
                    worst[blocks][1] = max(worst[blocks][1], rg)
                    assert rf <= tc.K_D_F and rg <= tc.K_D_G, (where, rf, rg)
            for e, want in ((du.PROBE_E0, ref["e0"]), (du.PROBE_E1, ref["e1"])):
                one, many = recs[1][p][e], recs[nb][p][e]
                for q, unit in enumerate(("uf", "ug0", "ug1")):
                    d = tc.ratio(one[q], many[q], want[unit])
                    worst_between[min(q, 1)] = max(worst_between[min(q, 1)], d)
                    assert d <= 2 * (tc.K_D_F if q == 0 else tc.K_D_G), (kind, n, a0, a1, q, d)
    print(f"n={n} worst f/g: 1 workgroup {worst[1]}, {nb} workgroups {worst[nb]}, between the shapes {worst_between}")


# ------------------------------------------------------------------------------------------------ (b) whole fits
_loss_cache = {}


def _loss(c, kept, a0, a1):
    key = (c["kind"], c["n"], float(a0), float(a1))
    if key not in _loss_cache:
        _loss_cache[key] = tc.ref_eval(c["t"], c["means"], kept, float(a0), float(a1))["f"]
    return _loss_cache[key]


def _check_fit(out5, c, where, worst):
    """one out5 against the oracle's fit of case c"""
    fit = c["fit"]
    a0, a1, ok, n_outer, n_kept = out5
    assert ok != -1.0, where
    assert (ok == 1.0) == fit["ok"], where
    assert (n_outer, n_kept) == (fit["n_outer"], fit["n_kept"]), where
    if not fit["ok"]:
        return
    d = rel_coef([a0, a1], fit["coef"])
    worst[0] = max(worst[0], (d, where))
    # whatever path the optimiser took: the loss at its coefficients, on the genes of the oracle's last fit, is no worse
    # than the oracle's by more than the stopping rule of both (factr * eps, relative to max(|f|, 1))
    f_dev, f_orc = _loss(c, fit["kept"], a0, a1), _loss(c, fit["kept"], *fit["coef"])
    excess = float((f_dev - f_orc) / max(abs(float(f_orc)), 1.0))
    worst[1] = max(worst[1], (excess, where))
    assert excess <= tc.FACTR_EPS, (where, excess)
    assert d <= tc.COEF_TOL_DEV, (where, d)


@gpu
@pytest.mark.parametrize("force_grid", SHAPES)
def test_fit_in_every_launch_shape_against_the_oracle(du, force_grid):
    """dsq::launch_trend_fit at every size and kind: ok (never -1), n_outer and n_kept are the oracle's - with NaN
    dispersions too -, the coefficients lie within tc.COEF_TOL_DEV of the oracle's and the loss at them is no worse than
    the oracle's beyond the stopping rule.  MI355X: see DESIGN 7d."""
    worst = [(0.0, None), (-1.0, None)]
    for n in tc.SIZES:
        for kind in tc.KINDS:
            c = tc.case(kind, n)
            out = du.trend_fit(c["gw"], c["means"], tc.MIN_DISP, tc.MAX_DISP, force_grid)
            _check_fit(out[0], c, (kind, n, force_grid), worst)
    print(f"force_grid={force_grid}: worst coefficient distance {worst[0]}, worst loss excess {worst[1]}")


@gpu
@pytest.mark.parametrize("force_grid,a,b", [(1, ("clean", 16385), ("nan_means", 513)),
                                            (1, ("outliers", 70001), ("at_min", 65)),
                                            (0, ("nan_disp", 3073), ("outliers", 3071)),
                                            (-1, ("outliers", 3071), ("nan_means", 2049))])
def test_back_to_back_launches_do_not_see_each_other(du, force_grid, a, b):
    """A, B, A on one TrendGridMem and one keep mask: each launch equals its own fresh launch bit for bit - B's tagged
    words (pass numbers of another sequence) and mask are still in the buffers when the second A starts."""
    ca, cb = tc.case(*a), tc.case(*b)
    seq = du.trend_fit_seq([(ca["gw"], ca["means"]), (cb["gw"], cb["means"]), (ca["gw"], ca["means"])], tc.MIN_DISP,
                           tc.MAX_DISP, force_grid)
    fresh_a = du.trend_fit(ca["gw"], ca["means"], tc.MIN_DISP, tc.MAX_DISP, force_grid)[0]
    fresh_b = du.trend_fit(cb["gw"], cb["means"], tc.MIN_DISP, tc.MAX_DISP, force_grid)[0]
    assert not np.isnan(seq).any() and (seq[:, 2] != -1.0).all()
    assert same_bits(seq[0], fresh_a) and same_bits(seq[1], fresh_b) and same_bits(seq[2], fresh_a)
    rep = du.trend_fit(ca["gw"], ca["means"], tc.MIN_DISP, tc.MAX_DISP, force_grid, repeats=3)
    assert all(same_bits(r, fresh_a) for r in rep)


@gpu
@pytest.mark.parametrize("n", tc.RAW_SIZES)
def test_raw_one_fit_mode_against_the_oracle(du, n):
    """dsq::launch_trend_glm: unclipped targets, covariates as given, one gamma-GLM fit (2049 and 5000 spill into the
    arrays and hold NaN targets) against orc.trend_gamma_glm."""
    tg, cov = tc.make_raw(n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        co, _, conv = orc.trend_gamma_glm(cov, tg)
    out = du.trend_glm(tg, cov, repeats=2)
    assert same_bits(out[0], out[1])
    a0, a1, ok, n_outer, n_kept = out[0]
    d = rel_coef([a0, a1], co)
    print(f"raw n={n}: coefficient distance {d}")
    assert (ok == 1.0) == conv and (n_outer, n_kept) == (1, n)
    assert d <= tc.COEF_TOL_DEV


# ------------------------------------------------------------------------------------------------ (c) k_trend
@gpu
def test_k_trend_against_the_reference(du):
    """dsq::launch_trend_loss_grad with the initial mask (and without a mask where every covariate is finite) at every
    size, kind and point.  k_trend divides its three sums by ONE count - that of the NaN-free loss terms - so the
    gradient is compared on the cases without a NaN term only."""
    worst_f, worst_g = (0.0, None), (0.0, None)
    for n in tc.SIZES:
        for kind in tc.KINDS:
            c = tc.case(kind, n)
            k0 = tc.init_mask(c["means"])
            with np.errstate(divide="ignore"):
                cov = 1.0 / c["means"]
            for a0, a1 in tc.points(c):
                ref = tc.ref_point(c, a0, a1)["e0"]
                masks = [k0.astype(np.uint8)] + ([None] if k0.all() else [])
                for keep in masks:
                    f, g0, g1, cnt = du.trend_loss_grad(cov, c["t"], a0, a1, keep)
                    where = (kind, n, a0, a1, keep is None)
                    assert cnt == ref["cf"], where
                    rf = tc.ratio(f, ref["f"], ref["uf"])
                    worst_f = max(worst_f, (rf, where))
                    assert rf <= tc.K_D_F, (where, rf)
                    if not np.isnan(c["t"][k0]).any():
                        rg = max(tc.ratio(g0, ref["g0"], ref["ug0"]), tc.ratio(g1, ref["g1"], ref["ug1"]))
                        worst_g = max(worst_g, (rg, where))
                        assert rg <= tc.K_D_G, (where, rg)
    print(f"k_trend worst f {worst_f}, worst g {worst_g}")


# ------------------------------------------------------------------------------------------------ (d) the product's C API
@pytest.fixture(scope="module")
def ctx():
    from pydeseq2_amd._lib import Context

    return Context(0)


def _vp(d):
    return C.c_void_p(d.ptr)


def _capi_fit(ctx, c):
    from pydeseq2_amd._lib import DeviceArray

    n = c["n"]
    d_gw, d_nm = DeviceArray.from_host(ctx, c["gw"]), DeviceArray.from_host(ctx, c["means"])
    d_keep = DeviceArray(ctx, (n,), np.uint8)
    c2, ok, n_outer = (C.c_double * 2)(), C.c_int(-7), C.c_int(-7)
    ctx.call("dsq_dev_trend_fit", _vp(d_gw), _vp(d_nm), n, C.c_double(tc.MIN_DISP), C.c_double(tc.MAX_DISP), _vp(d_keep), c2,
             C.byref(ok), C.byref(n_outer))
    return np.array([c2[0], c2[1]]), ok.value, n_outer.value, (d_gw, d_nm, d_keep)


@gpu
@pytest.mark.parametrize("n", [3071, 3072, 65537])
def test_capi_trend_fit_default_shape(du, ctx, n):
    """dsq_dev_trend_fit on either side of the launcher's crossover and beyond the registers' capacity: the oracle's ok
    and n_outer, and the bit pattern of the test library's launch of the same unit in the same shape."""
    worst = 0.0
    for kind in tc.KINDS:
        c = tc.case(kind, n)
        coef, ok, n_outer, _ = _capi_fit(ctx, c)
        fit = c["fit"]
        assert (ok == 1) == fit["ok"] and n_outer == fit["n_outer"], (kind, n)
        lib_out = du.trend_fit(c["gw"], c["means"], tc.MIN_DISP, tc.MAX_DISP, 0)[0]
        assert same_bits(coef, lib_out[:2]), (kind, n)
        if fit["ok"]:
            d = rel_coef(coef, fit["coef"])
            worst = max(worst, d)
            assert d <= tc.COEF_TOL_DEV, (kind, n, d)
    print(f"dsq_dev_trend_fit n={n}: worst coefficient distance {worst}")


@gpu
@pytest.mark.parametrize("kind,n", [("clean", 3072), ("outliers", 65537), ("nan_disp", 3071)])
def test_capi_trend_prior_is_its_three_parts(ctx, kind, n):
    """dsq_dev_trend_prior (fit, fitted values from the coefficients on the device, MAD prior; one synchronisation) gives
    the bit patterns of dsq_dev_trend_fit + dsq_dev_trend_eval + dsq_dev_prior_mad run one after the other."""
    from pydeseq2_amd._lib import DeviceArray

    c = tc.case(kind, n)
    coef, ok, n_outer, (d_gw, d_nm, d_keep) = _capi_fit(ctx, c)
    assert ok == 1
    d_fit = DeviceArray(ctx, (n,), np.float64)
    ctx.call("dsq_dev_trend_eval", _vp(d_nm), n, C.c_double(coef[0]), C.c_double(coef[1]), _vp(d_fit))
    d_work = DeviceArray(ctx, (ctx.lib.dsq_prior_mad_work_doubles(n),), np.float64)
    sq = C.c_double()
    ctx.call("dsq_dev_prior_mad", _vp(d_gw), _vp(d_fit), n, C.c_double(tc.MIN_DISP), C.c_double(tc.MAX_DISP), _vp(d_work),
             C.byref(sq))
    fitted = d_fit.to_host()
    d_fit2 = DeviceArray(ctx, (n,), np.float64)
    c2, ok2, no2, sq2 = (C.c_double * 2)(), C.c_int(-7), C.c_int(-7), C.c_double()
    ctx.call("dsq_dev_trend_prior", _vp(d_gw), _vp(d_nm), n, C.c_double(tc.MIN_DISP), C.c_double(tc.MAX_DISP), _vp(d_keep),
             _vp(d_fit2), _vp(d_work), c2, C.byref(ok2), C.byref(no2), C.byref(sq2))
    assert (ok2.value, no2.value) == (ok, n_outer)
    assert same_bits([c2[0], c2[1]], coef)
    assert same_bits(d_fit2.to_host(), fitted)
    assert same_bits([sq2.value], [sq.value]) and np.isfinite(sq.value)


@gpu
def test_capi_trend_eval_is_a0_plus_a1_over_mean(ctx):
    """dsq_dev_trend_eval: fitted = a0 + a1 / mean in exactly this order - one IEEE division, one addition, nothing fused
    (a quotient cannot be contracted into the sum) - so numpy's a0 + a1 / means gives the same bits, NaN and zero means
    included; a1 == 0 gives a0 for every gene, whatever its mean (the mean trend)."""
    from pydeseq2_amd._lib import DeviceArray

    for n in (1, 255, 256, 257, 70001):
        means = tc.make("nan_means", n)[1]
        d_nm, d_fit = DeviceArray.from_host(ctx, means), DeviceArray(ctx, (n,), np.float64)
        for a0, a1 in ((0.05, 3.0), (1e-12, 1e-12), (0.3, 0.0)):
            ctx.call("dsq_dev_trend_eval", _vp(d_nm), n, C.c_double(a0), C.c_double(a1), _vp(d_fit))
            with np.errstate(divide="ignore"):
                want = np.full(n, a0) if a1 == 0.0 else a0 + a1 / means
            assert same_bits(d_fit.to_host(), want), (n, a0, a1)


@gpu
def test_hip_inference_trend_glm_beyond_the_registers():
    """HipInference.dispersion_trend_gamma_glm at 2049 genes (the first size at which the single workgroup reads genes
    from the arrays), NaN targets among them: coefficients and flag of orc.trend_gamma_glm, predictions a0 + a1 cov."""
    from pydeseq2_amd.inference import HipInference

    tg, cov = tc.make_raw(2049)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        co, pred_o, conv = orc.trend_gamma_glm(cov, tg)
    coef, pred, ok = HipInference(device=0).dispersion_trend_gamma_glm(cov, tg)
    d = rel_coef(coef, co)
    print(f"HipInference trend GLM n=2049: coefficient distance {d}")
    assert ok == conv and d <= tc.COEF_TOL_DEV
    assert np.max(np.abs(pred - pred_o) / np.abs(pred_o)) <= 2 * tc.COEF_TOL_DEV
