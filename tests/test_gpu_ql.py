"""Quasi-likelihood F-test on the GPU: k_ql_dev against the wave-ordered host build bit for bit, dsq_dev_f_sf against
mpmath, dsq_dev_ql_score against dsq_dev_chisq_sf and the host build, and the façade end to end against the CPU reference
(tests/ql_ref.py), with refitted genes, reruns and the release of every device buffer."""
import ctypes as C

import numpy as np
import pytest

from tests import hostql as hq
from tests import ql_ref
from tests.helpers import assert_close
from tests.ql_cases import EPS, F_SF_C_DEVICE, F_SF_C_HOST, f_sf_check, ql_scenario

pytestmark = pytest.mark.gpu

_vp = C.c_void_p


@pytest.fixture(scope="module")
def ctx():
    from pydeseq2_amd._lib import Context

    return Context(0)


def _dev_f_sf(ctx, F, d1, d2):
    from pydeseq2_amd._lib import DeviceArray

    F = np.ascontiguousarray(F, dtype=np.float64)
    d_x, d_o = DeviceArray.from_host(ctx, F), DeviceArray.from_host(ctx, np.full(F.size + 3, -7.0))
    ctx.call("dsq_dev_f_sf", _vp(d_x.ptr), int(F.size), int(d1), C.c_double(float(d2)), _vp(d_o.ptr))
    out = d_o.to_host()
    d_x.free(); d_o.free()
    assert (out[F.size:] == -7.0).all()  # nothing written behind the end
    return out[:F.size]


def test_f_sf_device_against_400_digits(ctx):
    """The grid of tests/test_ql_host.py on the device build, asserted at four times the host-measured constant (the
    device's log1p, lgamma and exp differ from the host's by a few ulp).  Measured on an MI355X: DESIGN.md 7."""
    f_sf_check(lambda F, d1, d2: _dev_f_sf(ctx, F, d1, d2), "device f_sf", F_SF_C_DEVICE)


@pytest.mark.parametrize("n", [1, 65, 257])
def test_f_sf_device_lengths_and_edges(ctx, n):
    """One element, one more than a wavefront, one more than a block; F <= 0 gives 1, NaN gives NaN; the device and the
    host build are each within their bound of the truth, hence within the sum of the bounds of each other."""
    F = np.concatenate([[0.0, -2.0, np.nan, np.inf], np.geomspace(1e-3, 900.0, 253)])[:n]
    for d1, d2 in ((3, 17.5), (127, 2e6)):
        out, host = _dev_f_sf(ctx, F, d1, d2), hq.f_sf(F, d1, d2)
        assert out[0] == 1.0 and (n < 4 or (out[1] == 1.0 and np.isnan(out[2]) and out[3] == 0.0))
        ok = np.isfinite(host) & (host > 1e-300)
        lim = (F_SF_C_DEVICE + F_SF_C_HOST) * EPS * (1.0 + np.abs(np.log(host[ok])))
        assert (np.abs(out[ok] - host[ok]) <= lim * host[ok]).all()
    from pydeseq2_amd._lib import DeviceArray

    d = DeviceArray.from_host(ctx, np.ones(4))
    for bad in ((0, 5.0), (128, 5.0), (3, 0.0), (3, np.inf)):
        with pytest.raises(ValueError, match="d1|d2"):
            ctx.call("dsq_dev_f_sf", _vp(d.ptr), 4, bad[0], C.c_double(bad[1]), _vp(d.ptr))
    d.free()


def _dev_ql(ctx, counts, sf, X, Xr, disp, bf, br):
    """dsq_dev_ql_deviance on samples x genes counts -> (num, dev, s2), a guard value behind the outputs' end checked."""
    from pydeseq2_amd._design import pad16
    from pydeseq2_amd._lib import DeviceArray

    N, G = counts.shape
    ldn = pad16(N)
    y = np.zeros((G, ldn), np.int32)
    y[:, :N] = counts.T
    Xf, Xt = np.zeros((X.shape[1], ldn)), np.zeros((Xr.shape[1], ldn))
    Xf[:, :N], Xt[:, :N] = X.T, Xr.T
    d = [DeviceArray.from_host(ctx, np.ascontiguousarray(a)) for a in (y, sf, Xf, Xt, disp, bf, br)]
    d_o = DeviceArray.from_host(ctx, np.full(3 * G + 2, -7.0))
    ctx.call("dsq_dev_ql_deviance", _vp(d[0].ptr), ldn, _vp(d[1].ptr), _vp(d[2].ptr), ldn, X.shape[1], _vp(d[3].ptr), ldn,
             Xr.shape[1], N, G, _vp(d[4].ptr), _vp(d[5].ptr), _vp(d[6].ptr), _vp(d_o.ptr), _vp(d_o.ptr + 8 * G),
             _vp(d_o.ptr + 16 * G))
    o = d_o.to_host()
    for a in d + [d_o]:
        a.free()
    assert (o[3 * G:] == -7.0).all()
    return o[:G], o[G:2 * G], o[2 * G:3 * G]


def _kernel_inputs(N, Pf, Pr, G, seed):
    """Integer size factors and a first gene with zero coefficients (mu = sf exactly, y = mu on every other sample), rows
    with zeros, dispersions from 1e-3 to 10."""
    rng = np.random.default_rng(seed)
    X = np.column_stack([np.ones(N), rng.normal(0, 1, (N, Pf - 1))])
    Xr = np.ascontiguousarray(X[:, :Pr])
    sf = (np.arange(N) % 9 + 1).astype(float)
    bf = rng.normal(0, 0.4 / np.sqrt(Pf), (G, Pf))
    bf[:, 0] = rng.uniform(0.0, 5.0, G)
    bf[0] = 0.0
    br = bf[:, :Pr] + rng.normal(0, 0.05 / np.sqrt(Pr), (G, Pr))
    mu = sf[:, None] * np.exp(X @ bf.T)
    counts = rng.poisson(mu * rng.gamma(2.0, 0.5, (N, G))).astype(np.int64)
    counts[::5] = 0
    counts[::2, 0] = sf[::2].astype(np.int64)
    return counts, sf, X, Xr, 10 ** rng.uniform(-3, 1, G), bf, br


@pytest.mark.parametrize("Pf", [2, 12, 13, 48, 49, 128])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 129, 1000])
def test_ql_dev_kernel_vs_host_build_bit_for_bit(ctx, N, Pf):
    """Rows of 1 ... 1000 samples (below, at and above one and two sweeps of the 64 lanes), designs of 2 ... 128 columns
    with P_r = P_f - 1, G = 1, 3, 4, 5, 257 genes (four per block: a partial last block, gene indices beyond one block),
    rows containing y = 0 and y = mu: num, D_f and s2 equal the host build's wave-ordered instantiation EXACTLY (the sample
    loop is single IEEE operations and explicit fmas - nothing the compiler may contract - and the host adds the 64
    lane sums in the butterfly's order); N <= P_f included (s2 is then the plain quotient by N - P_f)."""
    counts, sf, X, Xr, disp, bf, br = _kernel_inputs(N, Pf, Pf - 1, 257, 1000 * N + Pf)
    for G in (1, 3, 4, 5, 257):
        a = (counts[:, :G], sf, X, Xr, disp[:G], bf[:G], br[:G])
        got, want = _dev_ql(ctx, *a), hq.deviance(*a, wave64=True)
        for g, w, name in zip(got, want, ("num", "deviance", "s2")):
            assert np.array_equal(g, w, equal_nan=True), (name, G, np.nanmax(np.abs(g - w)))
    one = hq.deviance(*a)
    assert_close(got[1], one[1], 1e-9, 1e-9, "one-lane order")


def test_ql_dev_kernel_intercept_only_reduced_design(ctx):
    a = _kernel_inputs(130, 13, 1, 6, 77)
    got, want = _dev_ql(ctx, *a), hq.deviance(*a, wave64=True)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    from pydeseq2_amd._lib import DeviceArray

    d = DeviceArray.from_host(ctx, np.ones(64))
    with pytest.raises(ValueError, match="P_reduced"):
        ctx.call("dsq_dev_ql_deviance", _vp(d.ptr), 16, _vp(d.ptr), _vp(d.ptr), 16, 2, _vp(d.ptr), 16, 2, 4, 1, _vp(d.ptr),
                 _vp(d.ptr), _vp(d.ptr), _vp(d.ptr), _vp(d.ptr), _vp(d.ptr))
    d.free()


def _dev_score(ctx, num, s2_post, df_test, df_total):
    from pydeseq2_amd._lib import DeviceArray

    n = len(num)
    d_in = DeviceArray.from_host(ctx, np.concatenate([num, s2_post]))
    d_o = DeviceArray.from_host(ctx, np.full(2 * n + 2, -7.0))
    ctx.call("dsq_dev_ql_score", _vp(d_in.ptr), _vp(d_in.ptr + 8 * n), n, int(df_test), C.c_double(df_total), _vp(d_o.ptr),
             _vp(d_o.ptr + 8 * n))
    o = d_o.to_host()
    d_in.free(); d_o.free()
    assert (o[2 * n:] == -7.0).all()
    return o[:n], o[n:2 * n]


@pytest.mark.parametrize("n", [1, 259])
def test_ql_score_branches(ctx, n):
    """df_total = inf: F's chi-square limit, the bits of dsq_dev_chisq_sf(df_test F, df_test); finite: the host build (F
    exactly - two IEEE operations -, p within the sum of the two f_sf bounds); a negative numerator gives F = 0, p = 1,
    NaN gives NaN."""
    from pydeseq2_amd._lib import DeviceArray

    rng = np.random.default_rng(n)
    num = np.concatenate([[-0.5, np.nan, 0.0], rng.chisquare(3, 256) * rng.choice([0.1, 1, 30], 256)])[:n]
    s2p = np.concatenate([[1.0, 1.0, 2.0], rng.uniform(0.3, 3.0, 256)])[:n]
    for df_test in (1, 3):
        F, p = _dev_score(ctx, num, s2p, df_test, np.inf)
        d_x, d_o = DeviceArray.from_host(ctx, df_test * F), DeviceArray(ctx, (n,), np.float64)
        ctx.call("dsq_dev_chisq_sf", _vp(d_x.ptr), n, df_test, _vp(d_o.ptr))
        assert np.array_equal(p, d_o.to_host(), equal_nan=True)
        d_x.free(); d_o.free()
        hF, _ = hq.score(num, s2p, df_test, np.inf)
        assert np.array_equal(F, hF, equal_nan=True)
        for df_total in (4.0, 57.3, 6e6):
            F, p = _dev_score(ctx, num, s2p, df_test, df_total)
            hF, hp = hq.score(num, s2p, df_test, df_total)
            assert np.array_equal(F, hF, equal_nan=True) and F[0] == 0.0 and p[0] == 1.0
            assert n < 2 or (np.isnan(F[1]) and np.isnan(p[1]))
            ok = np.isfinite(hp) & (hp > 1e-300)
            lim = (F_SF_C_DEVICE + F_SF_C_HOST) * EPS * (1.0 + np.abs(np.log(hp[ok])))
            assert (np.abs(p[ok] - hp[ok]) <= lim * hp[ok]).all()


@pytest.mark.parametrize("seed,df0_inf", [(10, True), (1, False)])
def test_pipeline_ql_without_gene_specific_variability(ctx, seed, df0_inf):
    """The data sets of tests/test_ql_host.py drawn at the trend (10 genes x 12 samples).  Seed 10: the moderation ends
    with df0 = infinity and DeseqPipeline.ql gives the chi-square limit, as the reference does - not F on the capped
    (1, 90) degrees of freedom; seed 1: df0 above the cap, F on (1, 90).  Fit tolerance of the likelihood-ratio tests."""
    import pydeseq2_amd
    from oracle import nbglm_oracle as orc
    from pydeseq2_amd.pipeline import DeseqResult
    from scipy.stats import f as f_dist

    counts, meta, X, Xr, c, trend = ql_scenario(12, G=10, seed=seed, spread=0.0)
    y = counts.to_numpy()
    sf = orc.size_factors_ratio(y)[0]
    ref = ql_ref.ql_reference(y, sf, X, Xr, trend, np.ones(10, bool))
    pipe = pydeseq2_amd.DeseqPipeline(y, X, ctx=ctx)
    r = pipe.ql(DeseqResult(size_factors=sf, non_zero=np.ones(10, bool), fitted_dispersions=trend,
                            refitted=np.zeros(10, bool), new_all_zeroes=np.zeros(10, bool)), Xr)
    pipe.close()
    assert np.isinf(r.df0) == df0_inf == np.isinf(ref["df0"])
    assert r.df_total == (np.inf if df0_inf else 90.0)
    assert_close(r.F, ref["F"], 1e-7, 1e-9, "F")
    assert_close(r.pvalue, ref["p"], 1e-6, 0, "p")
    assert_close(r.s02, ref["s02"], 1e-7, 0, "s02")
    if df0_inf:
        big = r.F > 10
        assert big.any() and (np.abs(r.pvalue / f_dist.sf(r.F, 1, 90.0) - 1) > 0.05)[big].all()


def test_facade_ql_end_to_end():
    """300 genes x 24 samples, ~batch + condition (two levels each), one gene refitted on its replaced counts.  test="QL"
    with the contrast and with reduced="~batch" are the same test here: F and p agree to the fit tolerance of the
    likelihood-ratio tests (stat rtol 1e-7, p rtol 1e-6); both agree at that tolerance with the CPU reference (oracle IRLS
    at the engine's trend dispersions and size factors, numpy deviances, ql_ref.squeeze_var, scipy.stats.f.sf); two calls
    give identical bits; every device buffer of the call is released."""
    from pydeseq2_amd.api import DeseqDataSet, DeseqStats

    counts, meta, X, Xr, c, _ = ql_scenario(24, G=300, seed=24, outlier=True)
    counts.iloc[:, 11] = 0  # a gene without counts
    dds = DeseqDataSet(counts=counts, metadata=meta, design="~batch + condition", min_replicates=4)
    dds.deseq2()
    eng = dds._res
    assert list(np.nonzero(eng.refitted)[0]) == [5] and not np.asarray(eng.new_all_zeroes).any()
    con = ["condition", "y", "x"]
    a = DeseqStats(dds, con, test="QL")
    a.run_ql_test()
    raw_p = a.p_values.to_numpy().copy()
    df_a = a.summary()
    b = DeseqStats(dds, con, test="QL", reduced="~batch")
    df_b = b.summary()
    wald = DeseqStats(dds, con).summary()

    # the CPU reference at the engine's size factors and trend dispersions, on the counts the final LFC was fitted on
    # (the layer itself is held to the reference's rebuilt counts by tests/test_gpu_lrt.py)
    fit_counts = np.asarray(dds.layers["replace_counts"])
    assert (fit_counts[:, 5] != counts.to_numpy()[:, 5]).sum() == 1
    ref = ql_ref.ql_reference(fit_counts, eng.size_factors, X, Xr, eng.fitted_dispersions, np.asarray(eng.non_zero, bool))
    assert np.isfinite(ref["df0"])
    for name, s in (("contrast", a), ("reduced", b)):
        F, p = s.statistics.to_numpy(), (raw_p if s is a else None)
        print(f"{name}: max rel F err {np.nanmax(np.abs(F - ref['F']) / np.maximum(ref['F'], 1e-2)):.3e}; df0 {s.ql_df0!r} "
              f"vs {ref['df0']!r}; s02 {s.ql_s02!r} vs {ref['s02']!r}")
        assert_close(F, ref["F"], 1e-7, 1e-9, f"{name}: F")
        assert_close(s.ql_dispersion.to_numpy(), ref["s2_post"], 1e-7, 0, f"{name}: s2_post")
        assert_close(s.ql_df0, ref["df0"], 1e-6, 0, f"{name}: df0")
        assert_close(s.ql_s02, ref["s02"], 1e-7, 0, f"{name}: s02")
        if p is not None:
            assert_close(p, ref["p"], 1e-6, 0, f"{name}: p")
    assert_close(b.statistics.to_numpy(), a.statistics.to_numpy(), 1e-7, 1e-9, "contrast vs reduced: F")
    co = np.asarray(eng.cooks_outlier, bool)
    assert_close(df_b["pvalue"].to_numpy()[~co], raw_p[~co], 1e-6, 0, "contrast vs reduced: p")
    assert np.isnan(a.statistics.to_numpy()[11]) and np.isnan(raw_p[11])
    # the refitted gene runs on its replaced counts: the reference on the ORIGINAL counts differs
    ref_o = ql_ref.ql_reference(counts.to_numpy(), eng.size_factors, X, Xr, eng.fitted_dispersions,
                                np.asarray(eng.non_zero, bool))
    assert abs(ref_o["num"][5] - ref["num"][5]) > 1e-3 * abs(ref["num"][5])
    # summary(): F in stat, the Cook's filter, a ql_dispersion column; the contrast's columns are the Wald run's
    assert np.array_equal(df_a["stat"].to_numpy(), a.statistics.to_numpy(), equal_nan=True)
    assert np.array_equal(df_a["pvalue"].to_numpy(), np.where(co, np.nan, raw_p), equal_nan=True)
    assert np.array_equal(df_a["ql_dispersion"].to_numpy(), a.ql_dispersion.to_numpy(), equal_nan=True)
    for col in ("baseMean", "log2FoldChange", "lfcSE"):
        assert np.array_equal(df_a[col].to_numpy(), wald[col].to_numpy(), equal_nan=True), col
    assert df_a["padj"].notna().sum() > 100 and (df_a["padj"].dropna() >= df_a["pvalue"][df_a["padj"].notna()] - 1e-15).all()
    with pytest.raises(ValueError, match="alt_hypothesis"):
        a.summary(alt_hypothesis="greater")
    assert a.alt_hypothesis is None and a.summary().equals(df_a)  # (refused before the object changed)
    assert a.ql_df_total == a.ql_df0 + 21 and a.ql_df_total < 299 * 21

    # two calls in a row: identical bits; and nothing of the call stays allocated
    pipe = dds._pipe
    ctx = pipe.ctx
    live, malloc, free = set(), ctx.malloc, ctx.free

    def tracked_malloc(nbytes):
        ptr = malloc(nbytes)
        live.add(ptr)
        return ptr

    def tracked_free(ptr):
        free(ptr)
        live.discard(ptr)

    hip = C.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value

    r1 = pipe.ql(eng, Xr)
    ctx.sync()
    before = free_bytes()
    ctx.malloc, ctx.free = tracked_malloc, tracked_free
    try:
        r2 = pipe.ql(eng, Xr)
    finally:
        ctx.malloc, ctx.free = malloc, free
    ctx.sync()
    assert not live, f"{len(live)} allocation(s) of ql() left"
    assert free_bytes() == before
    for u, v in zip(r1, r2):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    with pytest.raises(ValueError, match="test='QL' fits a reduced design per contrast"):
        DeseqStats.batch(dds, [con], test="QL")
    dds.close()

