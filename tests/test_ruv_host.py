"""Hidden-batch factors and batch removal without a GPU: the host build of csrc/dsq_proj.h (tests/hostruv)
on the cases of tests/ruv_cases.py against the restatement and the derived bounds of tests/ruv_ref.py, the launch plan, and
the host side of pydeseq2_amd/ruv.py - the choice of the factors, the batch design, every refusal."""
import warnings
from functools import lru_cache

import numpy as np
import pytest

from tests import hostruv
from tests import ruv_cases as rc
from tests import ruv_ref as rr

LOG = {c.name: c for c in rc.log_cases()}
RES = {c.name: c for c in rc.res_cases()}
SMALL = {c.name: c for c in rc.proj_small_cases()}
LONG = {c.name: c for c in rc.proj_long_cases()}


def _show(what, err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    if err.size:
        print(f"{what}: worst error {np.nanmax(err):.3g}, worst error / bound {np.nanmax(ratio):.3g}")
    return ratio


# ------------------------------------------------------------------------------------------------------------- the plan
def test_plan_edges():
    # the row in registers (staged = 2) up to 64 * 16 samples; in LDS (staged = 1) with 4 wavefronts while 4 (N + 64) doubles
    # fit 152 KiB, 2 while 2 (N + 64) do, 1 while N + 64 doubles fit 128 KiB; beyond, re-read from memory (staged = 0)
    assert rc.PLAN_EDGES == (64 * 16, (152 * 1024 // 32) - 64, (152 * 1024 // 16) - 64, (128 * 1024 // 8) - 64)
    for e, (w, s, w_next, s_next) in zip(rc.PLAN_EDGES, ((4, 2, 4, 1), (4, 1, 2, 1), (2, 1, 1, 1), (1, 1, 4, 0))):
        for N, ww, ss in ((e - 1, w, s), (e, w, s), (e + 1, w_next, s_next)):
            code, waves, staged, lds = hostruv.plan(N)
            assert (code, waves, staged) == (0, ww, ss), (N, code, waves, staged)
            assert lds == waves * 8 * (64 + (N if staged == 1 else 0)) and lds <= 152 * 1024
    assert hostruv.plan(1) == (0, 4, 2, 4 * 64 * 8)
    assert hostruv.plan(rc.BEYOND_LDS) == (0, 4, 0, 4 * 64 * 8)
    for N in (0, -1):
        assert hostruv.plan(N) == (-2, 0, 0, 0)


# ---------------------------------------------------------------------------------------------------------- log counts
@lru_cache(maxsize=None)
def log_ref(name):
    c = LOG[name]
    return rr.log_counts(c.y[:, :c.N], c.sf, c.normalized, c.eps)


@pytest.mark.parametrize("name", list(LOG))
def test_log_counts_host(name):
    c = LOG[name]
    out = np.full((c.y.shape[0], c.N + 2), rc.GUARD)
    # (without normalisation no size factors are passed at all: a null pointer, which must not be read)
    assert hostruv.log_counts(c.y, c.sf if c.normalized else None, c.N, c.normalized, c.eps, out) == 0
    assert (out[:, c.N:] == rc.GUARD).all()
    ref, bound = log_ref(name)
    ratio = _show(name, np.abs(out[:, :c.N] - ref), bound)
    assert (ratio <= 1).all()
    if c.eps == 1.0:
        assert (out[:, :c.N][c.y[:, :c.N] == 0] == 0.0).all()  # log(0 + 1) exactly


def test_log_counts_host_refusals():
    c = LOG[next(iter(LOG))]
    out = np.zeros((c.y.shape[0], c.N))
    for eps in (0.0, -1.0, np.inf, np.nan):
        assert hostruv.log_counts(c.y, c.sf, c.N, True, eps, out) == -2
    assert hostruv.log_counts(c.y, c.sf, c.y.shape[1] + 1, True, 1.0, out) == -2  # ldn < N
    assert hostruv.lib().hv_log_counts(hostruv._p(c.y), c.y.shape[1], None, c.N, c.y.shape[0], 1, hostruv.C.c_double(1.0),
                                       hostruv._p(out), c.N) == -2  # normalized without size factors


# ----------------------------------------------------------------------------------------------------------- residuals
@lru_cache(maxsize=None)
def res_ref(name, kind):
    c = RES[name]
    return rr.residuals(c.y[:, :c.N], c.sf, np.ascontiguousarray(c.Xt[:, :c.N].T), c.beta, c.disp, kind)


def check_residuals(c, kind, out, ref, bound, who):
    assert (out[:, c.N:] == rc.GUARD).all(), "the padding of an output row was written"
    got = out[:, :c.N]
    for g in c.nan_rows:
        assert np.isnan(got[g]).all(), (who, g)
    assert (np.isnan(got) == np.isnan(ref)).all()
    ok = ~np.isnan(ref)
    ratio = _show(f"{who} {c.name} kind {kind}", np.abs(got - ref)[ok], bound[ok])
    assert (ratio <= 1).all()


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", list(RES))
def test_residuals_host(name, kind):
    c = RES[name]
    out = np.full((c.y.shape[0], c.N + 1), rc.GUARD)
    assert hostruv.nb_residuals(c.y, c.sf, c.Xt, c.N, c.disp, c.beta, kind, out) == 0
    check_residuals(c, kind, out, *res_ref(name, kind), "host")


@pytest.mark.parametrize("kind", [0, 1])
def test_residuals_host_equal_counts_and_means(kind):
    # y == mu to the last bit: both logarithms are +-log1p(0) = 0 and the residual is exactly 0 at any dispersion
    c = RES["equal"]
    out = np.full((3, c.N), rc.GUARD)
    assert hostruv.nb_residuals(c.y, c.sf, c.Xt, c.N, c.disp, c.beta, kind, out) == 0
    assert (out[:2] == 0.0).all()
    assert (out[2, ::2] > 0).all() and (out[2, 1::2] == 0.0).all()


# ---------------------------------------------------------------------------------------------------------- projection
@lru_cache(maxsize=None)
def proj_ref(name):
    c = SMALL[name] if name in SMALL else LONG[name]
    return rr.projection(c.x[:, :c.N], np.ascontiguousarray(c.Pt[:, :c.N].T), np.ascontiguousarray(c.Bt[:, :c.N].T))


def host_project(c, post=0, inplace=False, coef=True):
    x = c.x.copy()
    out = x if inplace else np.full((c.G, c.N + 2), rc.GUARD)
    co = np.full((c.G, c.q), rc.GUARD) if coef else None
    assert hostruv.project_out(x, c.Pt, c.Bt, c.N, post, c.eps, out, co) == 0
    if not inplace:
        assert (out[:, c.N:] == rc.GUARD).all()
        assert np.array_equal(x, c.x, equal_nan=True)
    else:
        assert np.isnan(out[:, c.N:]).all()  # the padding of x is as it was
    return out[:, :c.N].copy(), co


def check_projection(c, out, coef, who):
    R = proj_ref(c.name)
    assert R["out_cond"].all(), "the case does not meet the condition of the output bound (ruv_ref.projection)"
    r1 = _show(f"{who} {c.name} coef", np.abs(coef - R["coef"]), R["coef_bound"])
    r2 = _show(f"{who} {c.name} out", np.abs(out - R["out"]), R["out_bound"])
    assert (r1 <= 1).all() and (r2 <= 1).all()


@pytest.mark.parametrize("name", list(SMALL) + list(LONG))
def test_projection_host(name):
    c = SMALL[name] if name in SMALL else LONG[name]
    out, coef = host_project(c)
    check_projection(c, out, coef, "host")
    if c.G > 1:
        assert (out[1] == 0.0).all() and (coef[1] == 0.0).all()
    out2, _ = host_project(c, inplace=True, coef=False)
    assert np.array_equal(out.view(np.int64), out2.view(np.int64))


@pytest.mark.parametrize("name", ["N65-G67-q7", "N129-G67-q64", "N2-G5-q2", "N63-G1-q1"])
def test_projection_host_post_operations(name):
    c = SMALL[name]
    R = proj_ref(name)
    e, _ = host_project(c, post=1)
    val, bound = rr.exp_post(R["out"], R["out_bound"], c.eps)
    assert (_show(f"host {name} exp", np.abs(e - val), bound) <= 1).all()
    r, _ = host_project(c, post=2)
    assert np.array_equal(r, np.maximum(np.rint(e), 0.0))  # the rounding of its OWN unrounded output, clipped
    assert (r >= 0).all() and (r[e < -0.5] == 0).all()


def test_projection_host_refusals():
    c = SMALL["N2-G5-q2"]
    out = np.zeros((c.G, c.N))
    wide = np.zeros((65, c.N))
    assert hostruv.project_out(c.x, wide, wide, c.N, 0, 1.0, out) == -2            # q = 65
    assert hostruv.project_out(c.x, c.Pt, c.Bt, c.N, 3, 1.0, out) == -2             # unknown post
    assert hostruv.project_out(c.x, c.Pt, c.Bt, c.N, 1, 0.0, out) == -2             # eps
    assert hostruv.project_out(c.x, c.Pt, c.Bt, c.x.shape[1] + 1, 0, 1.0, out) == -2  # ld < N
    from pydeseq2_amd import ruv

    with pytest.raises(ValueError, match="DSQ_PROJ_MAX_Q = 64"):
        ruv.check_q(65)
    ruv.check_q(64)


# ------------------------------------------------------------------------------------------- the factors from the Gram
def test_gap_conditions_of_the_cohorts():
    # W is compared column by column only where the restatement alone shows relative eigenvalue gaps >= 0.1 among the
    # compared components and to the next one: as many planted factors as k
    for k in (1, 2, 3):
        c = rc.cohort(7, planted=k)
        Y = np.log(c.counts / rr.size_factors(c.counts)[:, None] + 1.0)
        _, d, _, _ = rr.ruvg(Y, c.controls, k)
        assert (rr.gaps(d, k) >= 0.1).all(), (k, rr.gaps(d, k))


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("center", [True, False])
def test_factors_from_gram_against_svd(k, center):
    from pydeseq2_amd import ruv

    c = rc.cohort(7, planted=k)
    Y = np.log(c.counts / rr.size_factors(c.counts)[:, None] + 1.0)
    Wr, d, _, _ = rr.ruvg(Y, c.controls, k, center=center)
    gaps = rr.gaps(d, k)
    assert (gaps >= 0.1).all()
    Yc = Y[:, c.controls] - (Y[:, c.controls].mean(0) if center else 0.0)
    S = Yc @ Yc.T
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        W, dd, k_eff = ruv.factors_from_gram(S, k, len(c.controls))
    assert k_eff == k and W.shape == Wr.shape
    # eigenvalues (Weyl): |d_i^2 - dd_i^2| <= ||Delta S||_2 <= rr.gram_route_error, whose docstring has the derivation and
    # says which part of it (LAPACK's constant) is assumed
    assert np.abs(dd[:k] ** 2 - d[:k] ** 2).max() <= rr.gram_route_error(Yc)
    # eigenvectors (Davis-Kahan): rr.factor_tolerance
    tol = rr.factor_tolerance(Yc, d, k)
    assert np.abs(W - Wr).max() <= tol, (np.abs(W - Wr).max(), tol)


def test_factors_from_gram_rank_and_signs():
    from pydeseq2_amd import ruv

    rng = np.random.default_rng(11)
    A = rng.normal(size=(12, 2)) @ rng.normal(size=(2, 300))   # rank 2 exactly up to rounding
    S = A @ A.T
    with pytest.warns(UserWarning, match="only 2 of the 5"):
        W, d, k_eff = ruv.factors_from_gram(S, 5, 300)
    assert k_eff == 2 and W.shape == (12, 2)
    top = np.argmax(np.abs(W), axis=0)
    assert (W[top, [0, 1]] > 0).all()
    W1, _, _ = ruv.factors_from_gram(S, 2, 300, drop=1)
    assert np.array_equal(W1[:, 0], W[:, 1])


def test_ruv_argument_refusals():
    from pydeseq2_amd import ruv

    ok = dict(N=24, G=50, k=2, controls=[1, 2, 3], drop=0)
    assert ruv.check_ruv_args(**ok).tolist() == [1, 2, 3]
    for change, msg in ((dict(drop=2), "drop"), (dict(drop=3), "drop"), (dict(k=0), "k must"), (dict(k=25), "samples"),
                        (dict(controls=None), "control genes"), (dict(controls=[50]), "index outside"),
                        (dict(controls=[]), "no control"), (dict(method="s"), "method"), (dict(k=70, N=100), "DSQ_PROJ_MAX_Q")):
        with pytest.raises(ValueError, match=msg):
            ruv.check_ruv_args(**{**ok, **change})
    has = np.ones(50, dtype=bool)
    has[3] = False
    with pytest.raises(ValueError, match="has no counts"):
        ruv.check_ruv_args(24, 50, 2, [1, 2, 3], 0, "r", has)
    assert 3 not in ruv.check_ruv_args(24, 50, 2, None, 0, "r", has).tolist()  # default: all genes with counts


# ------------------------------------------------------------------------------------------------------- batch removal
def test_batch_design_coding():
    from pydeseq2_amd import ruv

    batch = np.array(["b", "a", "c", "a", "b", "c", "a", "c"])
    D, Xb, blocks = ruv.batch_design(8, batch=batch, covariates=np.arange(8.0))
    assert D.shape == (8, 1) and (D == 1).all() and blocks == [("batch", 2), ("covariates", 1)]
    assert Xb[:, :2].tolist() == [[0, 1], [1, 0], [-1, -1], [1, 0], [0, 1], [-1, -1], [1, 0], [-1, -1]]
    assert np.array_equal(Xb[:, 2], np.arange(8.0) - 3.5)
    _, Xb2, blocks2 = ruv.batch_design(8, batch=batch, batch2=np.arange(8) % 2)
    assert blocks2 == [("batch", 2), ("batch2", 1)] and Xb2[:, 2].tolist() == [1, -1] * 4


def test_batch_design_refusals():
    from pydeseq2_amd import ruv

    batch = np.arange(8) % 2
    with pytest.raises(ValueError, match="nothing to remove"):
        ruv.batch_design(8)
    with pytest.raises(ValueError, match="nothing to remove"):
        ruv.batch_design(8, batch=np.zeros(8))
    with pytest.raises(ValueError, match="'batch2'"):
        ruv.batch_design(8, batch=batch, batch2=batch)
    with pytest.raises(ValueError, match="'batch'"):  # the protected design already holds the batch
        ruv.batch_design(8, batch=batch, design=np.column_stack([np.ones(8), batch]))
    with pytest.raises(ValueError, match="'covariates'"):
        ruv.batch_design(8, batch=batch, covariates=batch.astype(float))
    with pytest.raises(ValueError, match="rank deficient by itself"):
        ruv.batch_design(8, batch=batch, design=np.ones((8, 2)))
    with pytest.raises(ValueError, match="DSQ_PROJ_MAX_Q = 64"):
        ruv.batch_design(200, batch=np.arange(200) % 66)
    with pytest.raises(ValueError, match="one label per sample"):
        ruv.batch_design(8, batch=np.zeros(7))


def test_batch_projection_is_the_least_squares_fit():
    from pydeseq2_amd import ruv

    rng = np.random.default_rng(5)
    N, G = 24, 40
    batch, cond = (np.arange(N) // 2) % 3, np.arange(N) % 2
    x = rng.normal(6, 2, (N, G)) + np.outer(batch, rng.normal(0, 1, G))
    design = np.column_stack([np.ones(N), cond])
    D, Xb, _ = ruv.batch_design(N, batch=batch, covariates=rng.normal(size=N), design=design)
    P, B = ruv.batch_projection(D, Xb)
    got = x - (x.T @ P @ B.T).T
    ref = rr.remove_batch(x, D, Xb)
    # Not derived from an operation sequence: both routes go through LAPACK inside numpy (pinv: an SVD; lstsq: gelsd).  Both
    # are backward stable least-squares solves of F = [D | Xb], so to first order the fitted batch terms agree within
    # c u cond(F) max|x|; c = 64 N is an ALLOWANCE for LAPACK's unpublished constants, the two solves and the products
    F = np.hstack([D, Xb])
    tol = 64 * N * rr.U * np.linalg.cond(F) * np.abs(x).max()
    assert np.abs(got - ref).max() <= tol
    # what is protected stays: the fit of the design on the output equals the fit on the input within the same tolerance
    assert np.abs(np.linalg.lstsq(F, got, rcond=None)[0][D.shape[1]:]).max() <= tol
