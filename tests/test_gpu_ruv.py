"""Hidden-batch factors and batch removal on the device: dsq_dev_log_counts, dsq_dev_nb_residuals and
dsq_dev_project_out through the C ABI on the cases of tests/ruv_cases.py - equal to the host build (tests/hostruv) bit for
bit, within the derived bounds of the restatement (tests/ruv_ref.py), guard values beyond every output, reruns and the
in-place projection bit for bit, the refusals - then pydeseq2_amd.ruv, DeseqPipeline and the façade on the planted cohorts."""
import ctypes as C
import warnings

import numpy as np
import pandas as pd
import pytest

from tests import hostruv
from tests import ruv_cases as rc
from tests import ruv_ref as rr
from tests import test_ruv_host as th

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pydeseq2_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _dev(ctx, *arrays):
    from pydeseq2_amd._lib import DeviceArray

    return [DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel()) if a is not None else None for a in arrays]


def _free(ctx, held):
    ctx.sync()
    for a in held:
        if a is not None:
            a.free()


def _vp(d):
    return C.c_void_p(d.ptr) if d is not None else None


# ---------------------------------------------------------------------------------------------------------- log counts
def dev_log_counts(ctx, c, ld_extra=2):
    out = np.full((c.y.shape[0], c.N + ld_extra), rc.GUARD)
    held = _dev(ctx, c.y, c.sf if c.normalized else None, out)  # (raw counts: d_sf is null and must not be read)
    try:
        ctx.call("dsq_dev_log_counts", _vp(held[0]), c.y.shape[1], _vp(held[1]), c.N, c.y.shape[0], int(c.normalized),
                 C.c_double(c.eps), _vp(held[2]), out.shape[1])
        out = held[2].to_host().reshape(out.shape)
    finally:
        _free(ctx, held)
    return out


@pytest.mark.parametrize("name", list(th.LOG))
def test_log_counts(ctx, name):
    c = th.LOG[name]
    out = dev_log_counts(ctx, c)
    assert (out[:, c.N:] == rc.GUARD).all(), "the padding of an output row was written"
    host = np.full_like(out, rc.GUARD)
    assert hostruv.log_counts(c.y, c.sf if c.normalized else None, c.N, c.normalized, c.eps, host) == 0
    assert np.array_equal(_bits(out), _bits(host)), "device and host build differ"
    ref, bound = th.log_ref(name)
    assert (th._show(f"device {name}", np.abs(out[:, :c.N] - ref), bound) <= 1).all()
    assert np.array_equal(_bits(dev_log_counts(ctx, c)), _bits(out)), "a rerun gave other bits"


def test_log_counts_refusals(ctx):
    c = th.LOG[next(iter(th.LOG))]
    held = _dev(ctx, c.y, c.sf, np.zeros(c.y.shape[0] * c.N))
    try:
        def call(N=c.N, G=c.y.shape[0], ldn=c.y.shape[1], eps=1.0, ld=c.N, out=held[2]):
            ctx.call("dsq_dev_log_counts", _vp(held[0]), ldn, _vp(held[1]), N, G, 1, C.c_double(eps), _vp(out), ld)

        call()
        for kw in (dict(N=0), dict(G=-1), dict(ldn=c.N - 1), dict(ld=c.N - 1), dict(eps=0.0), dict(eps=float("nan")),
                   dict(eps=float("inf")), dict(out=None)):
            with pytest.raises(ValueError):
                call(**kw)
        with pytest.raises(ValueError):  # normalized without size factors
            ctx.call("dsq_dev_log_counts", _vp(held[0]), c.y.shape[1], None, c.N, c.y.shape[0], 1, C.c_double(1.0),
                     _vp(held[2]), c.N)
    finally:
        _free(ctx, held)


# ----------------------------------------------------------------------------------------------------------- residuals
def dev_residuals(ctx, c, kind, ld_extra=1):
    G = c.y.shape[0]
    out = np.full((G, c.N + ld_extra), rc.GUARD)
    held = _dev(ctx, c.y, c.sf, c.Xt, c.disp, c.beta, out)
    try:
        ctx.call("dsq_dev_nb_residuals", _vp(held[0]), c.y.shape[1], _vp(held[1]), _vp(held[2]), c.Xt.shape[1], c.P, c.N, G,
                 _vp(held[3]), _vp(held[4]), kind, _vp(held[5]), out.shape[1])
        out = held[5].to_host().reshape(out.shape)
    finally:
        _free(ctx, held)
    return out


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", list(th.RES))
def test_residuals(ctx, name, kind):
    c = th.RES[name]
    out = dev_residuals(ctx, c, kind)
    host = np.full_like(out, rc.GUARD)
    assert hostruv.nb_residuals(c.y, c.sf, c.Xt, c.N, c.disp, c.beta, kind, host) == 0
    assert np.array_equal(_bits(out), _bits(host)), "device and host build differ"
    th.check_residuals(c, kind, out, *th.res_ref(name, kind), "device")
    assert np.array_equal(_bits(dev_residuals(ctx, c, kind)), _bits(out)), "a rerun gave other bits"
    if name == "equal":
        assert (out[:2, :c.N] == 0.0).all()


def test_residuals_refusals(ctx):
    c = th.RES["N2-G5-P8"]
    G = c.y.shape[0]
    held = _dev(ctx, c.y, c.sf, c.Xt, c.disp, c.beta, np.zeros(G * c.N))
    try:
        def call(P=c.P, N=c.N, ldx=c.Xt.shape[1], kind=0, ld=c.N, beta=held[4]):
            ctx.call("dsq_dev_nb_residuals", _vp(held[0]), c.y.shape[1], _vp(held[1]), _vp(held[2]), ldx, P, N, G,
                     _vp(held[3]), _vp(beta), kind, _vp(held[5]), ld)

        call()
        for kw in (dict(P=0), dict(P=129), dict(N=0), dict(ldx=c.N - 1), dict(kind=2), dict(ld=c.N - 1), dict(beta=None)):
            with pytest.raises(ValueError):
                call(**kw)
    finally:
        _free(ctx, held)


# ---------------------------------------------------------------------------------------------------------- projection
def dev_project(ctx, c, post=0, inplace=False, coef=True, q=None):
    q = c.q if q is None else q
    out = np.full((c.G, c.N + 2), rc.GUARD)
    co = np.full((c.G, max(q, 1)), rc.GUARD)
    held = _dev(ctx, c.x, c.Pt, c.Bt, None if inplace else out, co if coef else None)
    try:
        d_out = held[0] if inplace else held[3]
        ctx.call("dsq_dev_project_out", _vp(held[0]), c.x.shape[1], _vp(held[1]), _vp(held[2]), c.Pt.shape[1], q, c.N, c.G,
                 post, C.c_double(c.eps), _vp(d_out), c.x.shape[1] if inplace else out.shape[1], _vp(held[4]))
        full = d_out.to_host().reshape(c.x.shape if inplace else out.shape)
        co = held[4].to_host().reshape(co.shape) if coef else None
        if not inplace:
            assert np.array_equal(held[0].to_host().reshape(c.x.shape), c.x, equal_nan=True), "the input was written"
    finally:
        _free(ctx, held)
    if inplace:
        assert np.isnan(full[:, c.N:]).all(), "the padding of a row was written"
    else:
        assert (full[:, c.N:] == rc.GUARD).all(), "the padding of an output row was written"
    return full[:, :c.N].copy(), co


@pytest.mark.parametrize("name", list(th.SMALL) + list(th.LONG))
def test_projection(ctx, name):
    c = th.SMALL[name] if name in th.SMALL else th.LONG[name]
    out, coef = dev_project(ctx, c)
    h_out, h_coef = th.host_project(c)
    assert np.array_equal(_bits(coef), _bits(h_coef)), "coefficients: device and host build differ"
    assert np.array_equal(_bits(out), _bits(h_out)), "output: device and host build differ"
    th.check_projection(c, out, coef, "device")
    again, coef2 = dev_project(ctx, c)
    assert np.array_equal(_bits(again), _bits(out)) and np.array_equal(_bits(coef2), _bits(coef)), "a rerun gave other bits"
    inpl, _ = dev_project(ctx, c, inplace=True, coef=False)
    assert np.array_equal(_bits(inpl), _bits(out)), "in place (d_out == d_x) gave other bits"


# (the register path, the LDS path with 4, 2 and 1 wavefronts per workgroup - the exp table is filled by 256, 128 and 64
# threads - and the row beyond it)
@pytest.mark.parametrize("name", ["N65-G67-q7", "N129-G67-q64", "N2-G5-q2", "N63-G1-q1", "N1025-G5-q9", "N4801-G5-q2",
                                  "N9665-G5-q2", f"N{rc.BEYOND_LDS}-G3-q2"])
def test_projection_post_operations(ctx, name):
    c = th.SMALL[name] if name in th.SMALL else th.LONG[name]
    R = th.proj_ref(name)
    e, _ = dev_project(ctx, c, post=1)
    h, _ = th.host_project(c, post=1)
    assert np.array_equal(_bits(e), _bits(h))
    val, bound = rr.exp_post(R["out"], R["out_bound"], c.eps)
    assert (th._show(f"device {name} exp", np.abs(e - val), bound) <= 1).all()
    r, _ = dev_project(ctx, c, post=2)
    assert np.array_equal(r, np.maximum(np.rint(e), 0.0))  # the rounding of its OWN unrounded output, clipped


def test_projection_refusals(ctx):
    from pydeseq2_amd import ruv

    c = th.SMALL["N2-G5-q2"]
    wide = rc.ProjCase("wide", c.x, np.zeros((65, c.Pt.shape[1])), np.zeros((65, c.Pt.shape[1])), c.N, 65, 1.0)
    with pytest.raises(ValueError, match="DSQ_PROJ_MAX_Q"):
        dev_project(ctx, wide)
    with pytest.raises(ValueError):
        dev_project(ctx, c, q=0)
    with pytest.raises(ValueError):
        dev_project(ctx, c, post=3)
    bad = rc.ProjCase("eps", c.x, c.Pt, c.Bt, c.N, c.q, 0.0)
    with pytest.raises(ValueError):
        dev_project(ctx, bad, post=1)
    dev_project(ctx, bad, post=0)  # (eps is not looked at without a post-operation)
    x = np.zeros((c.N, 3))
    with pytest.raises(ValueError, match="DSQ_PROJ_MAX_Q = 64"):
        ruv.project_out(ctx, x, np.zeros((c.N, 65)), np.zeros((c.N, 65)))
    with pytest.raises(ValueError, match="epsilon"):
        ruv.project_out(ctx, x, np.zeros((c.N, 1)), np.zeros((c.N, 1)), post="exp", epsilon=-1.0)


def test_project_plan_export(ctx):
    from pydeseq2_amd import ruv

    for N in [1, 64, rc.BEYOND_LDS] + [e + d for e in rc.PLAN_EDGES for d in (-1, 0, 1)]:
        code, waves, staged, lds = hostruv.plan(N)
        assert code == 0 and ruv.project_plan(ctx, N) == (waves, staged, lds)
    with pytest.raises(ValueError):
        ruv.project_plan(ctx, 0)


# ------------------------------------------------------------------------------------------------------------ the module
def test_module_on_host_arrays_and_device_arrays(ctx):
    from pydeseq2_amd import ruv
    from pydeseq2_amd._lib import GENE_MAJOR, SAMPLE_MAJOR, DeviceArray

    c = th.SMALL["N65-G67-q7"]
    x = np.ascontiguousarray(c.x[:, :c.N].T)                     # N x G
    P, B = np.ascontiguousarray(c.Pt[:, :c.N].T), np.ascontiguousarray(c.Bt[:, :c.N].T)
    want, wcoef = dev_project(ctx, c)
    out, coef = ruv.project_out(ctx, x, P, B, return_coef=True)
    assert np.array_equal(_bits(out.T), _bits(want)) and np.array_equal(_bits(coef), _bits(wcoef))
    d_sm = DeviceArray.from_host(ctx, x)
    d_gm = DeviceArray.from_host(ctx, np.ascontiguousarray(x.T))
    try:
        assert np.array_equal(_bits(ruv.project_out(ctx, d_sm, P, B, layout=SAMPLE_MAJOR).T), _bits(want))
        assert np.array_equal(_bits(ruv.project_out(ctx, d_gm, P, B, layout=GENE_MAJOR).T), _bits(want))
        assert ruv.project_out(ctx, d_gm, P, B, layout=GENE_MAJOR, inplace=True) is None
        assert np.array_equal(_bits(d_gm.to_host()), _bits(want))
    finally:
        ctx.sync()
        d_sm.free()
        d_gm.free()
    lc = next(v for v in th.LOG.values() if v.normalized and v.N == 65)
    y = np.ascontiguousarray(lc.y[:, :lc.N].T)
    got = ruv.log_counts(ctx, y, lc.sf, True, lc.eps)
    assert np.array_equal(_bits(got.T), _bits(dev_log_counts(ctx, lc)[:, :lc.N]))
    with pytest.raises(ValueError, match="epsilon"):
        ruv.log_counts(ctx, y, lc.sf, True, 0.0)
    with pytest.raises(ValueError, match="size_factors"):
        ruv.log_counts(ctx, y, None, True)
    raw = next(v for v in th.LOG.values() if not v.normalized and v.N == 65)  # no size factors anywhere on the way down
    yraw = np.ascontiguousarray(raw.y[:, :raw.N].T)
    got = ruv.log_counts(ctx, yraw, None, normalized=False, epsilon=raw.eps)
    assert np.array_equal(_bits(got.T), _bits(dev_log_counts(ctx, raw)[:, :raw.N]))
    assert ruv.project_out(ctx, np.zeros((c.N, 0)), P, B).shape == (c.N, 0)  # no genes: nothing is launched
    assert ruv.remove_batch_effect(ctx, np.zeros((8, 0)), batch=np.arange(8) % 2).shape == (8, 0)
    rcse = th.RES["N65-G5-P8"]
    yr = np.ascontiguousarray(rcse.y[:, :rcse.N].T)
    X = np.ascontiguousarray(rcse.Xt[:, :rcse.N].T)
    for kind, code in (("deviance", 0), ("pearson", 1)):
        got = ruv.nb_residuals(ctx, yr, rcse.sf, X, rcse.beta, rcse.disp, kind)
        assert np.array_equal(_bits(got.T), _bits(dev_residuals(ctx, rcse, code)[:, :rcse.N]))
    with pytest.raises(ValueError, match="kind"):
        ruv.nb_residuals(ctx, yr, rcse.sf, X, rcse.beta, rcse.disp, "working")


@pytest.mark.parametrize("k", [1, 2, 3])
def test_ruvg_against_the_svd_route(ctx, k):
    """W column by column (the cohort plants k factors: relative eigenvalue gaps >= 0.1, asserted on the restatement), alpha
    and Y' (which depend on span(W) only)."""
    from pydeseq2_amd import ruv

    c = rc.cohort(7, planted=k)
    sf = rr.size_factors(c.counts)
    Y = np.log(c.counts / sf[:, None] + 1.0)
    Wr, d, Ypr, alr = rr.ruvg(Y, c.controls, k)
    gaps = rr.gaps(d, k)
    assert (gaps >= 0.1).all()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = ruv.ruv(ctx, c.counts, sf, k, c.controls, corrected=True, return_counts=True)
    assert r.k_eff == k and r.W.shape == (24, k) and r.alpha.shape == (k, 400) and list(r.genes) == list(c.controls)
    Yc = Y[:, c.controls] - Y[:, c.controls].mean(0)
    # eigenvalues (Weyl) and eigenvectors (Davis-Kahan) of the Gram route: rr.gram_route_error / rr.factor_tolerance have the
    # derivation (and say which constant is assumed); |d - d'| = |d^2 - d'^2| / (d + d') <= dS / d
    tol = rr.factor_tolerance(Yc, d, k)
    assert (np.abs(r.singular_values[:k] - d[:k]) <= rr.gram_route_error(Yc) / d[:k]).all()
    assert np.abs(r.W - Wr).max() <= tol
    # alpha = W^T Y (W orthonormal): |Delta alpha_jg| <= sum_n |Delta W_nj| |Y_ng| <= N tol max|Y|.  Y' = Y - W alpha:
    # |Delta Y'_ng| <= sum_j (|Delta W_nj| |alpha_jg| + |W_nj| |Delta alpha_jg|) <= k (tol sqrt(N) max|Y| + N tol max|Y|)
    # <= 2 k N tol max|Y| (|alpha_jg| <= sqrt(N) max|Y|, |W_nj| <= 1); first order in tol
    scale = 2 * k * 24 * tol * np.abs(Y).max()
    assert np.abs(r.alpha - alr).max() <= scale and np.abs(r.corrected - Ypr).max() <= scale
    un = ruv.ruv(ctx, c.counts, sf, k, c.controls, return_counts=True, round=False)
    assert np.array_equal(r.normalized_counts, np.maximum(np.rint(un.normalized_counts), 0.0))
    assert np.array_equal(_bits(un.alpha), _bits(r.alpha))
    if k > 1:
        dropped = ruv.ruv(ctx, c.counts, sf, k, c.controls, drop=1)
        assert np.array_equal(dropped.W, r.W[:, 1:])


def test_ruvg_of_raw_counts_takes_no_size_factors(ctx):
    """normalized=False: Y = log(y + eps), and no size factors reach the device (the C entry gets a null pointer)."""
    from pydeseq2_amd import ruv

    c = rc.cohort(7, planted=1)
    Y = np.log(c.counts + 1.0)
    Wr, d, Ypr, alr = rr.ruvg(Y, c.controls, 1)
    assert (rr.gaps(d, 1) >= 0.1).all()
    r = ruv.ruv(ctx, c.counts, None, 1, c.controls, normalized=False, corrected=True)
    Yc = Y[:, c.controls] - Y[:, c.controls].mean(0)
    tol = rr.factor_tolerance(Yc, d, 1)
    assert np.abs(r.W - Wr).max() <= tol
    scale = 2 * 24 * tol * np.abs(Y).max()  # (as test_ruvg_against_the_svd_route, k = 1)
    assert np.abs(r.alpha - alr).max() <= scale and np.abs(r.corrected - Ypr).max() <= scale


def test_ruv_warns_when_the_gram_cannot_resolve_k(ctx):
    from pydeseq2_amd import ruv

    rng = np.random.default_rng(3)
    N, G = 8, 60
    f = np.arange(N) % 2
    counts = np.rint(np.exp(5.0 + np.outer(f, rng.normal(0, 1, G)))).astype(np.int64)  # log counts of rank 2 (mean + one factor)
    with pytest.warns(UserWarning, match="requested factors"):
        r = ruv.ruv(ctx, counts, np.ones(N), 7, np.arange(G), epsilon=1e-9)
    assert r.k_eff < 7 and r.W.shape[1] == r.k_eff


# --------------------------------------------------------------------------------------------------------------- façade
def _dds(c, design="~condition", obs=None):
    from pydeseq2_amd import DeseqDataSet

    names = [f"g{j}" for j in range(c.counts.shape[1])]
    idx = [f"s{i}" for i in range(c.counts.shape[0])]
    if obs is None:
        obs = pd.DataFrame({"condition": np.where(c.cond == 1, "B", "A"), "batch": np.where(c.batch == 1, "y", "x")}, index=idx)
    return DeseqDataSet(counts=pd.DataFrame(c.counts, index=idx, columns=names), metadata=obs, design=design), names


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_facade_ruvg_finds_the_hidden_batch(seed):
    c, sf, Y, Wr, d, Ypr, alr = rc.behaviour_case(seed)   # (asserts the limits on the restatement alone first)
    dds, names = _dds(c)
    dds.deseq2()
    ctl = [names[j] for j in c.controls]
    r = dds.ruv(k=1, control_genes=ctl, method="g", corrected=True, counts=True)
    W1 = dds.obs["W_1"].to_numpy()
    assert np.array_equal(W1, r.W["W_1"].to_numpy()) and list(r.genes) == ctl
    corr = abs(np.corrcoef(W1, c.batch)[0, 1])
    Ye = np.log(c.counts / dds.obs["size_factors"].to_numpy()[:, None] + 1.0)
    left = rc.batch_effect(r.corrected.to_numpy(), c.batch) / rc.batch_effect(Ye, c.batch)
    print(f"seed {seed}: |corr(W_1, batch)| = {corr:.4f}, batch effect left {left:.4f}")
    assert corr >= rc.MIN_CORR and left <= rc.MAX_LEFT
    assert r.normalized_counts.shape == c.counts.shape and (r.normalized_counts.to_numpy() >= 0).all()
    # the workflow's next step: the factor in the design
    dds2, _ = _dds(c, design="~W_1 + condition", obs=dds.obs)
    dds2.deseq2()
    assert list(dds2.obsm["design_matrix"].columns) == ["Intercept", "W_1", "condition[T.B]"]
    assert np.isfinite(dds2.varm["LFC"].to_numpy()).all()


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_facade_ruvr_finds_the_hidden_batch(seed):
    """method="r": held to the same two limits, and against the restatement's own values - the deviance residuals of the
    engine's fit restated in mpmath, their SVD (not the Gram), alpha by lstsq; the limits are asserted on the restatement
    first."""
    c = rc.cohort(seed)
    dds, names = _dds(c)
    dds.deseq2()
    res = dds._res
    sf = np.asarray(res.size_factors)
    X = dds.obsm["design_matrix"].to_numpy()
    Rr, Rb = rr.residuals(np.ascontiguousarray(c.counts.T), sf, X, np.asarray(res.LFC), np.asarray(res.dispersions), 0)
    assert np.isfinite(Rr).all()
    Y = np.log(c.counts / sf[:, None] + 1.0)
    Wr, d, _, _ = rr.ruvg(Rr.T, np.arange(c.counts.shape[1]), 1)
    alr = np.linalg.lstsq(Wr, Y, rcond=None)[0]
    Ypr = Y - Wr @ alr
    corr_r = abs(np.corrcoef(Wr[:, 0], c.batch)[0, 1])
    left_r = rc.batch_effect(Ypr, c.batch) / rc.batch_effect(Y, c.batch)
    assert corr_r >= rc.MIN_CORR and left_r <= rc.MAX_LEFT, (corr_r, left_r)
    r = dds.ruv(k=1, method="r", corrected=True)
    corr = abs(np.corrcoef(r.W["W_1"].to_numpy(), c.batch)[0, 1])
    left = rc.batch_effect(r.corrected.to_numpy(), c.batch) / rc.batch_effect(Y, c.batch)
    print(f"seed {seed}: RUVr |corr| = {corr:.4f} (restatement {corr_r:.4f}), left {left:.4f} (restatement {left_r:.4f})")
    assert corr >= rc.MIN_CORR and left <= rc.MAX_LEFT
    assert (rr.gaps(d, 1) >= 0.1).all()
    # Davis-Kahan: the Gram's own error (6j) plus that of the residuals it is summed over, ||Delta S|| <= 2 ||R|| ||Delta R||
    Rc = Rr.T - Rr.T.mean(0)
    dS = 24 * rr.gamma(Rc.shape[1] + 2) * np.sum(Rc * Rc) + 2 * np.linalg.norm(Rc) * np.linalg.norm(Rb)
    tol = 4 * dS / (rr.gaps(d, 1).min() * d[0] ** 2)
    assert np.abs(r.W.to_numpy() - Wr).max() <= tol
    assert len(r.genes) == int(np.asarray(res.non_zero).sum())
    pd.testing.assert_frame_equal(dds.residuals("deviance"), pd.DataFrame(dds._pipe.residuals(res, "deviance"),
                                                                           index=dds.obs_names, columns=dds.var_names))


def test_facade_refusals_come_before_device_work():
    c = rc.cohort(0)
    dds, names = _dds(c)
    with pytest.raises(ValueError, match="control_genes"):
        dds.ruv(k=1)
    with pytest.raises(ValueError, match="method"):
        dds.ruv(k=1, control_genes=names[:5], method="s")
    with pytest.raises(ValueError, match="size factors"):
        dds.ruv(k=1, control_genes=names[:5])
    with pytest.raises(ValueError, match="deseq2"):
        dds.ruv(k=1, method="r")
    with pytest.raises(ValueError, match="deseq2"):
        dds.residuals()
    assert dds._pipe_obj is None, "a refusal touched the device"
    with pytest.raises(KeyError):
        dds.remove_batch_effect(batch="batch")
    dds.deseq2()
    with pytest.raises(ValueError, match="drop"):
        dds.ruv(k=2, control_genes=names[-100:], drop=2)
    with pytest.raises(ValueError, match="type"):
        dds.residuals("working")
    with pytest.raises(ValueError, match="epsilon"):
        dds.ruv(k=1, control_genes=names[-100:], epsilon=0.0)


def test_remove_batch_effect_and_empirical_controls():
    from pydeseq2_amd import DeseqStats
    from pydeseq2_amd import ruv

    c = rc.cohort(1)
    dds, names = _dds(c)
    dds.vst()
    x = np.asarray(dds.layers["vst_counts"])
    out = dds.remove_batch_effect(batch="batch")
    assert out.shape == x.shape and np.array_equal(out, dds.layers["vst_counts_nobatch"])
    # intercept-only design: the per-batch gene means of the output agree within the projection bound (q = 1: B = +-1, c =
    # half the batch difference): |Delta out| <= u |out| + |B| Delta c + gamma_2 |c B|, Delta c <= gamma_{1+7} sum |x P|;
    # a mean over 12 samples adds gamma_12 of the largest |out|
    D, Xb, _ = ruv.batch_design(24, batch=dds.obs["batch"].to_numpy())
    P, B = ruv.batch_projection(D, Xb)
    coef = x.T @ P
    bound = (rr.U * np.abs(out) + np.abs(B) @ (rr.gamma(8) * (np.abs(x.T) @ np.abs(P))).T
             + rr.gamma(2) * (np.abs(B) @ np.abs(coef.T)))
    # P itself comes from the host's pinv (an SVD inside LAPACK): not derived from an operation sequence.  Backward stable,
    # so to first order x P is off by c u cond(F) max|x|; c = 4 N is an ALLOWANCE for LAPACK's unpublished constant
    host = 4 * 24 * rr.U * np.linalg.cond(np.hstack([D, Xb])) * np.abs(x).max()
    m1, m0 = out[c.batch == 1].mean(0), out[c.batch == 0].mean(0)
    tol = 2 * bound.max(0) + 2 * rr.gamma(12) * np.abs(out).max(0) + 2 * host
    assert (np.abs(m1 - m0) <= tol).all(), (np.abs(m1 - m0).max(), tol.min())
    assert np.abs(x[c.batch == 1].mean(0) - x[c.batch == 0].mean(0)).mean() > 0.3  # (there was a batch effect to remove)
    ref = rr.remove_batch(x, D, Xb)
    # (against lstsq: the allowance of tests/test_ruv_host.py::test_batch_projection_is_the_least_squares_fit, stated there)
    assert np.abs(out - ref).max() <= 64 * 24 * rr.U * np.linalg.cond(np.hstack([D, Xb])) * np.abs(x).max()
    # a second application changes nothing beyond the projection bound
    again = dds.remove_batch_effect(layer="vst_counts_nobatch", batch="batch")
    assert (np.abs(again - out) <= 2 * bound + 2 * host).all()
    assert "vst_counts_nobatch_nobatch" in dds.layers
    p = dds.pca(layer="vst_counts_nobatch", n_components=2)
    assert p.scores.shape == (24, 2)
    # protected design and a covariate, formula over obs
    dds.obs["depth"] = np.log(c.counts.sum(1))
    o2 = dds.remove_batch_effect(batch="batch", covariates=["depth"], design="~condition")
    X = np.column_stack([np.ones(24), c.cond])
    D2, Xb2, _ = ruv.batch_design(24, batch=dds.obs["batch"].to_numpy(), covariates=dds.obs[["depth"]].to_numpy(), design=X)
    assert np.abs(o2 - rr.remove_batch(x, D2, Xb2)).max() <= 64 * 24 * rr.U * np.linalg.cond(np.hstack([D2, Xb2])) * np.abs(x).max()
    with pytest.raises(ValueError, match="'batch'"):
        dds.remove_batch_effect(batch="batch", design="~batch")
    # the workflow's empirical controls: the genes whose raw p-value exceeds the threshold
    dds.deseq2()
    st = DeseqStats(dds, contrast=["condition", "B", "A"])
    ctl = st.empirical_controls(0.1)
    pv = st.p_values.to_numpy()
    assert list(ctl) == [n for n, p in zip(names, pv) if p > 0.1] and len(ctl) > 0
    r = dds.ruv(k=1, control_genes=ctl)
    assert list(r.genes) == list(ctl) and "W_1" in dds.obs and r.W.shape == (24, 1)
