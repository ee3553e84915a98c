"""Likelihood-ratio test of a reduced design on the GPU: dsq_dev_chisq_sf, DeseqPipeline.lrt on every case of the reference
fixture (kat_lrt.npz), the kernel's shapes against the host build (tests/hostlrt), reruns, the façade end to end against
oracle functions, and the release of the kept replaced counts."""
import ctypes as C

import numpy as np
import pytest

from oracle import nbglm_oracle as orc
from tests import hostlrt as hl
from tests.helpers import assert_close, load_kat
from tests.lrt_cases import CASES, chisq_check, chisq_grid, facade_scenario, lrt_case, oracle_lrt, rebuilt_counts
from tests.test_gpu_parity import _jobs

pytestmark = pytest.mark.gpu

_vp = C.c_void_p


@pytest.fixture(scope="module")
def ctx():
    from pydeseq2_amd._lib import Context

    return Context(0)


def _dev_chisq_sf(ctx, x, df):
    from pydeseq2_amd._lib import DeviceArray

    x = np.ascontiguousarray(x, dtype=np.float64)
    d_x, d_o = DeviceArray.from_host(ctx, x), DeviceArray(ctx, (x.size,), np.float64)
    ctx.call("dsq_dev_chisq_sf", _vp(d_x.ptr), int(x.size), int(df), _vp(d_o.ptr))
    out = d_o.to_host()
    d_x.free(); d_o.free()
    return out


def test_chisq_sf_device_against_50_digits(ctx):
    """The grid and the bound of tests/test_lrt_host.py::test_chisq_sf_against_50_digits, on the device build."""
    chisq_check(lambda x, df: _dev_chisq_sf(ctx, x, df), "device chisq_sf")


@pytest.mark.parametrize("n", [1, 65])
def test_chisq_sf_device_lengths_and_edges(ctx, n):
    """One element, and one more than a wavefront: every element written, none beyond (a guard value behind the end)."""
    from pydeseq2_amd._lib import DeviceArray

    x = np.concatenate([[0.0, -2.0, np.nan], np.geomspace(1e-3, 900.0, 62)])[:n]
    d_x = DeviceArray.from_host(ctx, x)
    d_o = DeviceArray.from_host(ctx, np.full(n + 3, -7.0))
    ctx.call("dsq_dev_chisq_sf", _vp(d_x.ptr), n, 3, _vp(d_o.ptr))
    out = d_o.to_host()
    assert (out[n:] == -7.0).all()
    host = hl.chisq_sf(x, 3)
    g = chisq_grid()
    assert_close(out[:n], host, 2 * g["bound"], 0, "device vs host chisq_sf")  # (each within the bound of the truth)
    assert out[0] == 1.0 and (n < 3 or (out[1] == 1.0 and np.isnan(out[2])))
    with pytest.raises(ValueError, match="df"):
        ctx.call("dsq_dev_chisq_sf", _vp(d_x.ptr), n, 128, _vp(d_o.ptr))


def _result(counts, sf, disp, beta):
    from pydeseq2_amd.pipeline import DeseqResult

    G = counts.shape[1]
    return DeseqResult(size_factors=sf, non_zero=np.ones(G, bool), dispersions=disp, LFC=beta,
                       refitted=np.zeros(G, bool), new_all_zeroes=np.zeros(G, bool))


@pytest.mark.parametrize("case", CASES)
def test_pipeline_lrt_vs_reference_fixture(ctx, case):
    """DeseqPipeline.lrt fits the reduced design itself: flags equal, reduced_LFC rtol 1e-8 / atol 1e-10, stat rtol 1e-7 +
    10 x the reference's cancellation error, p rtol 1e-6 (above 1e-300).  p65: the reduced fit (64 columns) runs in the
    kernel family of the designs wider than 48 columns."""
    import pydeseq2_amd

    counts, sf, X, Xr, fx = lrt_case(case)
    pipe = pydeseq2_amd.DeseqPipeline(counts, X, ctx=ctx)
    p, stat, beta_r, conv = pipe.lrt(_result(counts, sf, fx["disp"], fx["beta_full"]), Xr)
    pipe.close()
    assert (conv == fx["conv_reduced"]).all()
    assert_close(beta_r, fx["beta_reduced"], 1e-8, 1e-10, f"{case} reduced LFC")
    assert_close(stat, fx["stat"], 1e-7, 10 * float(fx["stat_ref_err"]), f"{case} stat")
    big = fx["p"] > 1e-300
    assert_close(p[big], fx["p"][big], 1e-6, 0, f"{case} p")
    assert (p[~big] <= 1e-299).all() and (p >= 0).all()


def _dev_lrt(ctx, counts, sf, X, Xr, disp, bf, br):
    """dsq_dev_lrt on samples x genes counts -> (stat, p), a guard value behind the outputs' end checked."""
    from pydeseq2_amd._design import pad16
    from pydeseq2_amd._lib import DeviceArray

    N, G = counts.shape
    ldn = pad16(N)
    y = np.zeros((G, ldn), np.int32)
    y[:, :N] = counts.T
    Xf, Xt = np.zeros((X.shape[1], ldn)), np.zeros((Xr.shape[1], ldn))
    Xf[:, :N], Xt[:, :N] = X.T, Xr.T
    d = [DeviceArray.from_host(ctx, np.ascontiguousarray(a)) for a in (y, sf, Xf, Xt, disp, bf, br)]
    d_o = DeviceArray.from_host(ctx, np.full(2 * G + 2, -7.0))
    ctx.call("dsq_dev_lrt", _vp(d[0].ptr), ldn, _vp(d[1].ptr), _vp(d[2].ptr), ldn, X.shape[1], _vp(d[3].ptr), ldn,
             Xr.shape[1], N, G, _vp(d[4].ptr), _vp(d[5].ptr), _vp(d[6].ptr), _vp(d_o.ptr), _vp(d_o.ptr + 8 * G))
    o = d_o.to_host()
    for a in d + [d_o]:
        a.free()
    assert (o[2 * G:] == -7.0).all()
    return o[:G], o[G:2 * G]


@pytest.mark.parametrize("G", [1, 5, 257])
@pytest.mark.parametrize("N,case", [(3, "p2"), (63, "p4"), (64, "p2"), (65, "p4"), (130, "p4")])
def test_kernel_shapes_vs_host_build(ctx, N, G, case):
    """Block remainders (G = 1, 5, 257 with four genes per block) and rows of 3 ... 130 samples (below, at and above one
    sweep of the 64 lanes), cut from - or tiled out of - the p2 / p4 inputs, coefficients drawn around the fixture's.
    The statistic is compared with the host build's wave-ordered instantiation by EXACT EQUALITY: the sample loop is
    written in single IEEE operations and explicit fmas, and the host adds the 64 lane sums in the butterfly's order.
    The p-value goes through the two platforms' erfc / sqrt: both are within the chisq_sf bound of the truth, hence
    within twice that bound of each other."""
    k, fx = load_kat(case), lrt_case(case)[4]
    rng = np.random.default_rng(1000 * N + G)
    rows = np.arange(N) % k["counts"].shape[0]
    genes = rng.integers(0, len(fx["genes"]), G)
    counts = k["counts"][rows][:, fx["genes"][genes]]
    X = k["X"][rows]
    if N == 3:  # (three rows of p2's design: both groups present)
        X = np.array([[1.0, 0.0], [1.0, 1.0], [1.0, 0.0]])
    Xr = np.ascontiguousarray(X[:, fx["cols"]])
    sf = np.resize(k["sf"], N)
    bf = fx["beta_full"][genes] + rng.normal(0, 0.05, (G, X.shape[1]))
    br = fx["beta_reduced"][genes] + rng.normal(0, 0.05, (G, Xr.shape[1]))
    disp = fx["disp"][genes]
    stat, p = _dev_lrt(ctx, counts, sf, X, Xr, disp, bf, br)
    h_stat, h_p = hl.lrt(counts, sf, X, Xr, disp, bf, br, wave64=True)
    assert np.array_equal(stat, h_stat), np.abs(stat - h_stat).max()
    assert_close(p, h_p, 2 * chisq_grid()["bound"], 0, "p")
    assert_close(stat, hl.lrt(counts, sf, X, Xr, disp, bf, br)[0], 1e-9, 1e-9, "one-lane order")


def test_reruns_are_bit_identical(ctx):
    import pydeseq2_amd

    counts, sf, X, Xr, fx = lrt_case("p8m")
    pipe = pydeseq2_amd.DeseqPipeline(counts, X, ctx=ctx)
    res = _result(counts, sf, fx["disp"], fx["beta_full"])
    a, b = pipe.lrt(res, Xr), pipe.lrt(res, Xr)
    pipe.close()
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def test_lrt_refuses_a_design_that_is_not_nested(ctx):
    import pydeseq2_amd

    counts, sf, X, Xr, fx = lrt_case("p4")
    pipe = pydeseq2_amd.DeseqPipeline(counts, X, ctx=ctx)
    res = _result(counts, sf, fx["disp"], fx["beta_full"])
    with pytest.raises(ValueError, match="not nested"):
        pipe.lrt(res, np.column_stack([np.ones(60), np.arange(60.0) ** 2]))
    with pytest.raises(ValueError, match="between 1 and 3"):
        pipe.lrt(res, X)
    pipe.close()


def test_facade_lrt_end_to_end_with_replaced_outliers():
    """300 genes x 24 samples, ~batch + condition (three levels) against ~batch, two injected Cook's outliers (one gene
    refitted on its replaced counts, one all zero after the replacement).  Expected values are composed from oracle
    functions: orc.deseq2, orc.irls on both designs over the counts rebuilt as dds.py:1329-1358 does, orc.nb_nll,
    chi2.sf, and orc.summary's filtering applied to the LRT p-values."""
    from pydeseq2_amd.api import DeseqDataSet, DeseqStats

    counts, meta, X = facade_scenario()
    cvec = np.array([0.0, 0.0, 1.0, 0.0])
    ref = orc.deseq2(counts.to_numpy(), X, contrast=cvec, min_replicates=4, n_jobs=_jobs())
    assert list(np.nonzero(ref.replaced)[0]) == [5, 9] and list(np.nonzero(ref.new_all_zeroes)[0]) == [9]
    assert list(np.nonzero(ref.refitted)[0]) == [5]
    rebuilt = rebuilt_counts(counts.to_numpy(), X, ref, 4)
    want_layer = rebuilt.copy()
    e_stat, e_p, e_beta, e_conv, ref_err = oracle_lrt(counts.to_numpy(), X, X[:, :2], ref, rebuilt)

    dds = DeseqDataSet(counts=counts, metadata=meta, design="~batch + condition", min_replicates=4)
    dds.deseq2()
    assert np.array_equal(dds.var["replaced"], ref.replaced) and np.array_equal(dds.var["refitted"], ref.refitted)
    assert "replace_counts" in dds.layers.available()
    got_layer = dds.layers["replace_counts"]
    assert got_layer.dtype == np.int64 and np.array_equal(got_layer, want_layer)
    ds = DeseqStats(dds, ["condition", "y", "x"], test="LRT", reduced="~batch")
    ds.run_lrt_test()
    raw_p = ds.p_values.to_numpy().copy()  # before summary()'s Cook's filter masks the outlier genes
    df = ds.summary()
    wald = DeseqStats(dds, ["condition", "y", "x"]).summary()

    stat, p = df["stat"].to_numpy(), df["pvalue"].to_numpy()
    # the issue's tolerances hold between the engine and the oracle functions at the SAME dispersions and size factors
    # (the engine's; those of the oracle's own pass differ by the ~1e-6 of the dispersion fits, checked further down)
    eng = dds._res
    s2, p2, b2, c2, err2 = oracle_lrt(counts.to_numpy(), X, X[:, :2], eng, rebuilt)
    b2[9] = 0.0
    co = np.asarray(eng.cooks_outlier, bool)
    assert_close(ds.reduced_LFC.to_numpy(), b2, 1e-8, 1e-10, "reduced LFC")
    keep = np.arange(len(c2)) != 9  # (the flag of the gene that became all zero is that of a discarded fit)
    assert (ds.reduced_converged.to_numpy()[keep] == c2[keep]).all()
    assert_close(stat, s2, 1e-7, 10 * err2, "stat")
    assert_close(raw_p, p2, 1e-6, 0, "pvalue of run_lrt_test()")
    assert np.array_equal(p, np.where(co, np.nan, raw_p), equal_nan=True)  # summary(): the Cook's filter, nothing else
    # the rules of the two replaced genes: the one that became all zero has stat 0 and p 1 - and, being a Cook's outlier
    # that was not refitted (dds.py:1066-1110), loses that p-value in summary() exactly as it does under the Wald test
    assert stat[9] == 0.0 and raw_p[9] == 1.0 and (ds.reduced_LFC.to_numpy()[9] == 0.0).all()
    assert co[9] and np.isnan(p[9]) and np.isnan(wald["pvalue"].to_numpy()[9]) and wald["stat"].to_numpy()[9] == 0.0
    y5 = rebuilt[:, [5]]
    st5 = hl.lrt(y5, eng.size_factors, X, X[:, :2], eng.dispersions[[5]], eng.LFC[[5]], ds.reduced_LFC.to_numpy()[[5]])[0]
    assert_close(stat[[5]], st5, 1e-12, 1e-12, "refitted gene: scored on its replaced counts")
    y5o = counts.to_numpy()[:, [5]]
    assert abs(hl.lrt(y5o, eng.size_factors, X, X[:, :2], eng.dispersions[[5]], eng.LFC[[5]],
                      ds.reduced_LFC.to_numpy()[[5]])[0][0] - stat[5]) > 1e-3 * abs(stat[5])
    # against the oracle's own pass (its dispersions): the pipeline tolerance of the Wald columns
    assert (np.abs(stat - e_stat) <= 1e-4 * np.maximum(np.abs(e_stat), 1.0)).mean() >= 0.99
    assert (ds.reduced_converged.to_numpy()[keep] == e_conv[keep]).all()
    assert ref_err < 1e-9 and np.abs(ds.reduced_LFC.to_numpy()[keep] - e_beta[keep]).max() < 1e-3
    # the summary tail over the LRT p-values: Cook's filter, independent filtering, BH
    eng_lrt = type("R", (), dict(pvalue=p2, cooks_outlier=eng.cooks_outlier, normed_means=eng.normed_means, LFC=eng.LFC,
                                 lfcSE=eng.lfcSE, stat=s2))
    want = orc.summary(eng_lrt, cvec)
    assert (np.isnan(df["padj"].to_numpy()) == np.isnan(want["padj"])).all()
    assert_close(df["padj"].to_numpy(), want["padj"], 1e-5, 0, "padj")
    # the contrast's columns are the Wald run's
    for col in ("baseMean", "log2FoldChange", "lfcSE"):
        assert np.array_equal(df[col].to_numpy(), wald[col].to_numpy(), equal_nan=True), col
    assert not np.array_equal(df["stat"].to_numpy(), wald["stat"].to_numpy(), equal_nan=True)
    with pytest.raises(ValueError, match="alt_hypothesis"):
        ds.summary(alt_hypothesis="greater")
    # lfc_shrink after an LRT: as after a Wald test
    ds.alt_hypothesis = None
    a = ds.lfc_shrink("condition[T.y]")
    b = DeseqStats(dds, ["condition", "y", "x"])
    b.summary()
    b = b.lfc_shrink("condition[T.y]")
    assert np.array_equal(a["log2FoldChange"].to_numpy(), b["log2FoldChange"].to_numpy(), equal_nan=True)
    assert np.array_equal(a["pvalue"].to_numpy(), df["pvalue"].to_numpy(), equal_nan=True)
    dds.close()


def test_close_releases_the_kept_replaced_counts():
    """The replaced rows live in a buffer of the pipeline's own: creating, running and closing pipelines over and over
    leaves the device's free memory where it was (as tests/test_gpu_wider_designs.py checks the wider slots)."""
    import gc

    import pydeseq2_amd
    from pydeseq2_amd._lib import Context

    hip = C.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value

    N, G = 4096, 512  # every gene carries an outlier: 512 kept rows of 16 KB, 8 MB a cycle
    X = np.column_stack([np.ones(N), np.arange(N) % 2]).astype(float)
    rng = np.random.default_rng(3)
    mean = 10 ** rng.uniform(1.7, 3.3, G)
    counts = rng.negative_binomial(20, 20 / (20 + mean[None, :]), (N, G)).astype(np.int64)
    counts[np.arange(G), np.arange(G)] = (3000 * mean).astype(np.int64)

    def cycle():
        ctx = Context(0)
        pipe = pydeseq2_amd.DeseqPipeline(counts, X, ctx=ctx)
        r = pipe.deseq2()
        assert r.replaced.sum() >= G // 2 and pipe._replace_buf is not None
        kept = pipe._replace_buf.nbytes
        pipe.close()
        assert pipe._replace_buf is None
        del r, pipe
        gc.collect()
        ctx.close()
        gc.collect()
        return kept

    kept = cycle()
    assert kept >= (G // 2) * 4 * N
    before = free_bytes()
    for _ in range(4):
        cycle()
    assert before - free_bytes() < 2 * kept, (before - free_bytes(), kept)  # (a leak: 4 x kept)
