"""Regularized-log transformation on the GPU: dsq_dev_rlog (k_rlog) against the 64-lane host build (tests/hostrlog) and the
dense QR restatement (tests/rlog_ref) over every register count and the row path, guard values, reruns, the hard set, the
argument refusals, DeseqPipeline.rlog with genes without counts, and DeseqDataSet.rlog() end to end."""
import ctypes as C
import dataclasses
import pickle

import numpy as np
import pytest

from tests import hostrlog as hr
from tests import rlog_ref
from tests.helpers import assert_close, load_dataset
from tests.rlog_cases import check_hard, check_plain, hard_set, plain_set

pytestmark = pytest.mark.gpu

_vp = C.c_void_p
GUARD = 3


@pytest.fixture(scope="module")
def ctx():
    from pydeseq2_amd._lib import Context

    return Context(0)


def _dev_rlog(ctx, counts, sf, disp, base_mean, beta_prior_var):
    """dsq_dev_rlog on samples x genes counts -> (rlog N x G, intercept, converged, n_iter); guard values behind the end
    of all four outputs are checked untouched."""
    from pydeseq2_amd._design import pad16
    from pydeseq2_amd._lib import DeviceArray

    N, G = counts.shape
    ldn = pad16(N)
    y = np.zeros((G, ldn), np.int32)
    y[:, :N] = counts.T
    d_in = [DeviceArray.from_host(ctx, np.ascontiguousarray(a, dtype=t))
            for a, t in ((y, np.int32), (sf, np.float64), (disp, np.float64), (base_mean, np.float64))]
    d_out = DeviceArray.from_host(ctx, np.full(G * N + GUARD, -7.0))
    d_b0 = DeviceArray.from_host(ctx, np.full(G + GUARD, -7.0))
    d_cv = DeviceArray.from_host(ctx, np.full(G + GUARD, 0x5A, np.uint8))
    d_it = DeviceArray.from_host(ctx, np.full(G + GUARD, -7, np.int32))
    try:
        ctx.call("dsq_dev_rlog", _vp(d_in[0].ptr), ldn, _vp(d_in[1].ptr), N, G, _vp(d_in[2].ptr), _vp(d_in[3].ptr),
                 C.c_double(beta_prior_var), _vp(d_out.ptr), _vp(d_b0.ptr), _vp(d_cv.ptr), _vp(d_it.ptr))
        ctx.sync()
        out, b0, cv, it = d_out.to_host(), d_b0.to_host(), d_cv.to_host(), d_it.to_host()
    finally:
        for a in d_in + [d_out, d_b0, d_cv, d_it]:
            a.free()
    assert (out[G * N:] == -7.0).all() and (b0[G:] == -7.0).all() and (cv[G:] == 0x5A).all() and (it[G:] == -7).all()
    assert set(np.unique(cv[:G])) <= {0, 1}
    return np.ascontiguousarray(out[:G * N].reshape(G, N).T), b0[:G], cv[:G].astype(bool), it[:G]


def _dev(ctx, s):
    return _dev_rlog(ctx, s.counts, s.sf, s.disp, s.base_mean, s.beta_prior_var)


@pytest.mark.parametrize("G", [1, 5, 203])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 130, 512, 513])
def test_kernel_shapes_vs_host_build_and_restatement(ctx, N, G):
    """Every samples-per-lane count of the register kernels (R = 1: N <= 64; 2: 65, 130; 8: 512), the last lane group
    partly filled, the row kernel (513), and blocks partly filled (four genes per block).  The plain-set rules
    (tests/rlog_cases.check_plain) against the restatement and, for the genes a wide set does not restate, against the
    64-lane host build; a second launch must give the same bits."""
    s = plain_set(N, 203).first(G)
    got = _dev(ctx, s)
    host = hr.rlog(s.counts, s.sf, s.disp, s.base_mean, s.beta_prior_var, hr.WAVE64)
    worst = check_plain(s, got, f"device N={N} G={G}", host=host)
    print(f"N={N} G={G}: largest |difference| from the restatement (rlog, intercept) = {worst}; from the host build "
          f"{np.abs(got[0] - host[0]).max():.3g}")
    assert np.array_equal(got[3], host[3]) and np.array_equal(got[2], host[2])
    assert_close(got[0], host[0], 1e-8, 1e-10, "device vs 64-lane host build")
    again = _dev(ctx, s)
    for u, v in zip(got, again):
        assert u.tobytes() == v.tobytes()


def test_hard_set(ctx):
    s = hard_set()
    easy, capped, same_row = check_hard(s, _dev(ctx, s), "device, hard set")
    assert capped > 0.05 and same_row > 0  # (the set does exercise the cap, and the intercept at the cap)


def test_edges_and_the_exit_beyond_30(ctx):
    sf = np.array([1e-7, 1.0, 1.0])
    counts = np.array([[2_000_000_000, 5, 5], [40, 50, 60], [0, 0, 0], [0, 3, 0]]).T
    disp = np.full(4, 0.1)
    bm = (counts / sf[:, None]).mean(0)
    r, b0, conv, it = _dev_rlog(ctx, counts, sf, disp, bm, 1e8)
    h = hr.rlog(counts, sf, disp, bm, 1e8, hr.WAVE64)
    assert it[0] == 100 and not conv[0] and np.isfinite(r[:, 0]).all() and np.isfinite(b0[0])
    assert (r[:, 2] == 0.0).all() and b0[2] == 0.0 and it[2] == 0 and not conv[2]  # no counts: not fitted
    assert np.array_equal(it, h[3]) and np.array_equal(conv, h[2])
    assert_close(r[:, [1, 3]], h[0][:, [1, 3]], 1e-8, 1e-10, "ordinary genes beside the edge cases")


def test_argument_refusals(ctx):
    from pydeseq2_amd._lib import DeviceArray

    d = DeviceArray.from_host(ctx, np.full(64, -7.0))
    p = _vp(d.ptr)
    ok = dict(N=4, G=2, v=0.3, out=p, b0=p, cv=p, it=p)

    def call(**kw):
        a = {**ok, **kw}
        ctx.call("dsq_dev_rlog", p, 16, p, a["N"], a["G"], p, p, C.c_double(a["v"]), a["out"], a["b0"], a["cv"], a["it"])

    for bad in (dict(N=0), dict(G=-1), dict(v=0.0), dict(v=-1.0), dict(v=float("nan")), dict(v=float("inf")),
                dict(out=None), dict(b0=None), dict(cv=None), dict(it=None)):
        with pytest.raises(ValueError):
            call(**bad)
    call(G=0)  # nothing to do, nothing written
    ctx.sync()
    assert (d.to_host() == -7.0).all()
    d.free()


def test_pipeline_rlog_with_genes_without_counts(ctx):
    """DeseqPipeline.rlog on a fitted result: the genes with counts are gathered and fitted at the engine's trend
    dispersions, size factors and normalised means; the estimated prior variance equals the direct construction's; genes
    without counts come back as 0 / NaN.  Values are held against the restatement wherever it converges clear of the
    tolerance (a condition on the inputs: at least 90 % of the genes)."""
    import pydeseq2_amd

    src = plain_set(12, 203)
    counts = src.counts.copy()
    zero = np.array([0, 7, 8, 100, 202])
    counts[:, zero] = 0
    X = np.column_stack([np.ones(12), np.arange(12) % 2])
    pipe = pydeseq2_amd.DeseqPipeline(counts, X, ctx=ctx)
    res = pipe.deseq2()
    r, b0, conv, it, bpv = pipe.rlog(res)
    r2 = pipe.rlog(res, beta_prior_var=0.4)
    with pytest.raises(ValueError, match="beta_prior_var"):
        pipe.rlog(res, beta_prior_var=0.0)
    bad = np.array(res.fitted_dispersions)
    bad[3] = np.nan
    res_bad = dataclasses.replace(res, fitted_dispersions=bad)
    with pytest.raises(ValueError, match="fitted_dispersions"):
        pipe.rlog(res_bad)
    pipe.close()
    nz = np.asarray(res.non_zero, bool)
    assert not nz[zero].any() and nz.sum() == 198
    assert (r[:, ~nz] == 0.0).all() and np.isnan(b0[~nz]).all() and np.isnan(conv[~nz]).all() and np.isnan(it[~nz]).all()
    assert bpv == pytest.approx(rlog_ref.prior_var(counts, res.size_factors, res.fitted_dispersions, nz), rel=1e-12)
    e = rlog_ref.rlog(counts[:, nz], res.size_factors, res.fitted_dispersions[nz], res.normed_means[nz], bpv)
    clear = e[3] & ~np.array([rlog_ref.borderline(c) for c in e[4]])
    assert clear.mean() >= 0.9
    assert np.array_equal(it[nz][clear], e[2][clear]) and (conv[nz][clear] == 1).all()
    assert_close(r[:, nz][:, clear], e[0][:, clear], 1e-8, 1e-10, "pipeline rlog")
    assert_close(b0[nz][clear], e[1][clear], 1e-8, 1e-10, "pipeline intercept")
    assert r2[4] == 0.4 and np.abs(r2[0] - r).max() > 1e-3  # (a wider prior shrinks less)


@pytest.mark.parametrize("use_design", [False, True])
def test_facade_rlog_end_to_end(use_design):
    """DeseqDataSet.rlog() on the synthetic data set against the restatement fed with the engine's published size factors
    and rlog_fitted_dispersions (fit_type="mean" and the default), a user-given prior variance, and the layer surviving
    copy() and pickling."""
    from pydeseq2_amd.api import DeseqDataSet

    counts, meta = load_dataset("synthetic")
    c = counts.to_numpy()

    def expect(dds, bpv):
        sf = dds.obs["size_factors"].to_numpy()
        fit = dds.var["rlog_fitted_dispersions"].to_numpy()
        e = rlog_ref.rlog(c, sf, fit, (c / sf[:, None]).mean(0), bpv)
        clear = e[3] & ~np.array([rlog_ref.borderline(k) for k in e[4]])
        assert clear.mean() >= 0.8
        return e, clear

    for ft in ("mean", None):
        dds = DeseqDataSet(counts=counts, metadata=meta, design="~condition")
        out = dds.rlog(use_design=use_design, fit_type=ft)
        assert out is dds.layers["rlog_counts"] and out.shape == c.shape
        bpv = dds.uns["rlog_beta_prior_var"]
        sf = dds.obs["size_factors"].to_numpy()
        fit = dds.var["rlog_fitted_dispersions"].to_numpy()
        if ft == "mean":
            assert np.ptp(fit) == 0.0
        assert bpv == pytest.approx(rlog_ref.prior_var(c, sf, fit), rel=1e-12)
        e, clear = expect(dds, bpv)
        assert_close(out[:, clear], e[0][:, clear], 1e-8, 1e-10, f"rlog_counts fit_type={ft}")
        assert_close(dds.var["rlog_intercept"].to_numpy()[clear], e[1][clear], 1e-8, 1e-10, "rlog_intercept")
        assert (dds.var["rlog_converged"].to_numpy()[clear] == 1).all()
    given = dds.rlog(use_design=use_design, beta_prior_var=0.25).copy()
    assert dds.uns["rlog_beta_prior_var"] == 0.25
    e, clear = expect(dds, 0.25)
    assert_close(given[:, clear], e[0][:, clear], 1e-8, 1e-10, "rlog_counts, given prior variance")
    for other in (dds.copy(), pickle.loads(pickle.dumps(dds))):
        assert np.array_equal(other.layers["rlog_counts"], given)
        assert other.uns["rlog_beta_prior_var"] == 0.25 and "rlog_intercept" in other.var
    dds.close()
