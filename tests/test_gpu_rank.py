"""Rank-sum test on the device: dsq_dev_ranksum through the C ABI on the cases of tests/rank_cases.py
against the numpy / mpmath reference of tests/rank_ref.py and scipy.stats.mannwhitneyu; reruns and K comparisons bit for
bit; the refusals of the C ABI; DeseqPipeline.ranksum, DeseqStats(test="wilcoxon") and DeseqStats.batch."""
import ctypes as C
import pickle
import warnings

import numpy as np
import pandas as pd
import pytest

from tests import rank_cases as rc
from tests import rank_ref as rr

pytestmark = pytest.mark.gpu

SMALL = rc.small_cases()
FILL = -7.25  # what the outputs hold before the call: the row pitch's padding must keep it


@pytest.fixture(scope="module")
def ctx():
    from pydeseq2_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def _packed(case, rows=None):
    from pydeseq2_amd import ranktest as rt

    rows = range(case.K) if rows is None else rows
    return rt.pack_layouts([rt.build_layout(case.labels[k], case.strata) for k in rows], case.labels[list(rows)])


def _call(ctx, y, ldn, sf, N, P, alt, pad_g=3):
    """dsq_dev_ranksum through ctypes: outputs of pitch G + pad_g, their padding checked.  dict of K x G arrays."""
    from pydeseq2_amd._lib import DeviceArray, _vp

    G, K = y.shape[0], len(P.nstrata)
    ldg = G + pad_g
    held = [DeviceArray.from_host(ctx, np.ascontiguousarray(a)) for a in
            (y.ravel(), sf, P.order.ravel(), P.seg.ravel(), P.pad.ravel(), P.nstrata, P.labels.ravel(),
             np.full(4 * K * ldg, FILL))]
    d_y, d_sf, d_o, d_s, d_p, d_n, d_l, d_out = held
    try:
        o = d_out.ptr
        ctx.call("dsq_dev_ranksum", _vp(d_y.ptr), ldn, _vp(d_sf.ptr), N, G, K, _vp(d_o.ptr), P.ldo, _vp(d_s.ptr),
                 _vp(d_p.ptr), P.lds, _vp(d_n.ptr), _vp(d_l.ptr), P.ldl, alt, _vp(o), _vp(o + 8 * K * ldg),
                 _vp(o + 16 * K * ldg), _vp(o + 24 * K * ldg), ldg)
        out = d_out.to_host().reshape(4, K, ldg)
    finally:
        ctx.sync()
        for a in held:
            a.free()
    assert (out[:, :, G:] == FILL).all(), "the padding of an output row was written"
    return dict(zip(("stat", "pvalue", "usum", "ties"), (out[j, :, :G].copy() for j in range(4))))


def _run(ctx, case, alt, rows=None):
    return _call(ctx, case.y, case.ldn, case.sf, case.N, _packed(case, rows), rr.ALT_CODE[alt])


def _bits(o):
    return {k: v.view(np.int64).copy() for k, v in o.items()}


@pytest.fixture(scope="module")
def host_scipy_deviation():
    """The worst relative deviation of the HOST build's p-value from scipy.stats.mannwhitneyu's over the unstratified
    cases (measured here, held to its own derived bound in tests/test_rank_host.py): the device is held to it plus the
    bound of norm_sf."""
    from pydeseq2_amd import ranktest as rt
    from tests import hostrank

    worst = 0.0
    for case in SMALL:
        if case.strata is not None:
            continue
        P = rt.pack_layouts([rt.build_layout(case.labels[k]) for k in range(case.K)], case.labels)
        for alt in rc.ALTS:
            code, got = hostrank.ranksum(case.y, case.ldn, case.sf, case.N, P, rr.ALT_CODE[alt])
            assert code == 0
            worst = max(worst, rr.check_case(case, alt, got, "host")["scipy"])
    print(f"host build against scipy.stats.mannwhitneyu: worst relative deviation of the p-value {worst:.3g}")
    return worst


# ------------------------------------------------------------------------------------------------ C ABI against the reference
@pytest.mark.parametrize("alt", rc.ALTS, ids=["two-sided", "greater", "less"])
@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
def test_device_against_the_reference(ctx, host_scipy_deviation, case, alt):
    w = rr.check_case(case, alt, _run(ctx, case, alt), "device", scipy_extra=host_scipy_deviation)
    print(f"{case.name} alt={alt}: stat error {w['stat']:.2f} of its bound, p error {w['p']:.2g} of its bound, "
          f"worst deviation from scipy {w['scipy']:.3g}")


@pytest.mark.parametrize("case", rc.big_cases(), ids=["n16384", "n8192x2"])
def test_device_on_the_longest_rows(ctx, host_scipy_deviation, case):
    """L = 16 384: one wave per workgroup, 128 KiB of LDS, one stratum and two."""
    for alt in rc.ALTS:
        w = rr.check_case(case, alt, _run(ctx, case, alt), "device", scipy_extra=host_scipy_deviation)
        print(f"{case.name} alt={alt}: stat {w['stat']:.2f}, p {w['p']:.2g} of their bounds, scipy {w['scipy']:.3g}")


def test_reruns_and_k_comparisons_give_the_same_bits(ctx):
    for name in ("K3", "K3_strata"):
        case = [c for c in SMALL if c.name == name][0]
        for alt in rc.ALTS:
            a, b = _bits(_run(ctx, case, alt)), _bits(_run(ctx, case, alt))
            for key in a:
                assert np.array_equal(a[key], b[key]), (name, alt, key)
            for k in range(case.K):  # one launch of K = 3 against three launches of K = 1
                one = _bits(_run(ctx, case, alt, rows=[k]))
                for key in a:
                    assert np.array_equal(a[key][k], one[key][0]), (name, alt, k, key)
    big = rc.big_cases()[0]
    a, b = _bits(_run(ctx, big, None)), _bits(_run(ctx, big, None))
    assert all(np.array_equal(a[key], b[key]) for key in a)


def test_plan_of_the_library(ctx):
    from tests import hostrank

    for L in (0, 1, 1000, 5120, 5121, 10240, 10241, 16384, 16385):
        w, b = C.c_int(-1), C.c_size_t(1)
        code = ctx.lib.dsq_ranksum_plan(L, C.byref(w), C.byref(b))
        assert (code, w.value, b.value) == hostrank.plan(L), L


def test_c_abi_refusals(ctx):
    case = [c for c in SMALL if c.name == "left_out_ldn"][0]
    P = _packed(case)
    _call(ctx, case.y, case.ldn, case.sf, case.N, P, 0)
    for alt in (1, 2, 5):
        with pytest.raises(ValueError, match="alt: two-sided"):
            _call(ctx, case.y, case.ldn, case.sf, case.N, P, alt)
    with pytest.raises(ValueError, match="smaller than N"):
        _call(ctx, case.y, case.N - 1, case.sf, case.N, P, 0)
    with pytest.raises(ValueError, match="ldg is smaller"):
        _call(ctx, case.y, case.ldn, case.sf, case.N, P, 0, pad_g=-1)
    bad = _packed(case)
    bad.pad[0, 1] *= 2
    with pytest.raises(ValueError, match="prefix sums"):
        _call(ctx, case.y, case.ldn, case.sf, case.N, bad, 0)
    bad = _packed(case)
    bad.order[0, 5] = case.N
    with pytest.raises(ValueError, match="outside 0"):
        _call(ctx, case.y, case.ldn, case.sf, case.N, bad, 0)
    bad = _packed(case)
    bad.nstrata[0] = 2
    with pytest.raises(ValueError, match="n_strata"):
        _call(ctx, case.y, case.ldn, case.sf, case.N, bad, 0)
    # 8193 + 8191 samples in two strata: L = 24 576, packed by hand (the layout builder refuses it itself)
    from pydeseq2_amd import ranktest as rt

    r = rc.refused_case()
    with pytest.raises(ValueError, match="DSQ_RANK_MAX_L"):
        rt.build_layout(r.labels[0], r.strata)
    order = np.argsort(r.strata, kind="stable").astype(np.int32)[None, :]
    Pr = rt.PackedLayouts(order, np.array([[0, 8193, 16384]], np.int32), np.array([[0, 16384, 24576]], np.int32),
                          np.array([2], np.int32), r.labels.astype(np.int8))
    with pytest.raises(ValueError, match="DSQ_RANK_MAX_L = 16384"):
        _call(ctx, r.y, r.ldn, r.sf, r.N, Pr, 0)


def test_ranksum_of_the_python_layer_is_the_c_abi(ctx):
    from pydeseq2_amd import ranktest as rt
    from pydeseq2_amd._lib import DeviceArray

    case = [c for c in SMALL if c.name == "K3_strata"][0]
    d_y = DeviceArray.from_host(ctx, case.y.ravel())
    try:
        r = rt.ranksum(ctx, d_y.ptr, case.ldn, case.sf, case.G, case.labels, case.strata, "less")
    finally:
        d_y.free()
    want = _run(ctx, case, "less")
    for name, key in (("statistic", "stat"), ("pvalue", "pvalue"), ("usum", "usum"), ("ties", "ties")):
        assert np.array_equal(getattr(r, name).view(np.int64), want[key].view(np.int64)), name
    refs = rr.case_reference(case, "less")
    assert r.pairs.tolist() == [refs[k][0]["pairs"] for k in range(3)] and r.n_strata.tolist() == [4, 4, 3]
    assert np.array_equal(r.auc, r.usum / r.pairs[:, None]) and (r.n1 + r.n2).tolist() == [100, 60, int((case.labels[2] >= 0).sum())]


# ------------------------------------------------------------------------------------------------ the facade
def _scenario():
    """64 genes x 44 samples, ~batch + condition: condition A / B / C (20 / 18 / 6 samples), batch x / y; one gene
    without counts, one with a gross outlier, one heavily tied."""
    rng = np.random.default_rng(77)
    N, G = 44, 64
    cond = np.array(list("A" * 20 + "B" * 18 + "C" * 6))
    batch = np.array(["x", "y"])[rng.integers(0, 2, N)]
    perm = rng.permutation(N)
    meta = pd.DataFrame({"condition": cond[perm], "batch": batch}, index=[f"s{i}" for i in range(N)])
    mu = rng.uniform(5, 400, G)[None, :] * np.where((meta["condition"].to_numpy() == "B")[:, None], rng.uniform(0.4, 2.5, G), 1.0)
    mu = mu * np.exp(rng.normal(0, 0.25, N))[:, None]
    counts = rng.negative_binomial(5, 5 / (5 + mu)).astype(np.int64)
    counts[:, 7] = 0
    # (the data set is fitted with min_replicates = 30: no cell is that large, so the count is flagged and not replaced)
    counts[np.nonzero(meta["condition"].to_numpy() == "A")[0][0], 11] = 100 * counts[:, 11].max() + 1000
    counts[:, 20] = rng.poisson(0.2, N)
    return pd.DataFrame(counts, index=meta.index, columns=[f"g{j}" for j in range(G)]), meta


@pytest.fixture(scope="module")
def dds():
    from pydeseq2_amd import DeseqDataSet

    counts, meta = _scenario()
    d = DeseqDataSet(counts=counts, metadata=meta, design="~batch + condition", min_replicates=30)
    d.deseq2()
    yield d
    d.close()


def _facade_reference(dds, tested, ref, strata, alt):
    lv = dds.obs["condition"].astype(str).to_numpy()
    lab = np.where(lv == tested, 1, np.where(lv == ref, 0, -1))
    ids = None if strata is None else pd.factorize(dds.obs[strata].astype(str), sort=True)[0]
    y = np.asarray(dds.X, dtype=np.int64).T
    sf = np.asarray(dds.obs["size_factors"], dtype=float)
    return [rr.reference(y[g], sf, lab, ids, alt) for g in range(y.shape[0])]


@pytest.mark.parametrize("strata,alt", [(None, None), ("batch", None), (["batch"], "greater"), (None, "less")],
                         ids=["plain", "strata", "strata-greater", "less"])
def test_facade_summary(dds, strata, alt):
    from pydeseq2_amd import DeseqStats
    from pydeseq2_amd import summary as _summary

    ds = DeseqStats(dds, ["condition", "B", "A"], test="wilcoxon", strata=strata, alt_hypothesis=alt)
    df = ds.summary()
    assert list(df.columns) == ["baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "padj", "auc"]
    wald = DeseqStats(dds, ["condition", "B", "A"], alt_hypothesis=alt).summary()
    for col in ("baseMean", "log2FoldChange", "lfcSE"):  # the GLM fit's
        assert np.array_equal(df[col].to_numpy(), wald[col].to_numpy(), equal_nan=True), col
    refs = _facade_reference(dds, "B", "A", "batch" if strata is not None else None, alt)
    nz = np.asarray(dds.var["non_zero"], bool)
    assert not nz[7] and nz.sum() == 63
    got = dict(stat=df["stat"].to_numpy()[None, nz], pvalue=df["pvalue"].to_numpy()[None, nz],
               usum=ds.rank_usum.to_numpy()[None, nz], ties=ds.rank_ties.to_numpy()[None, nz])
    for j, g in enumerate(np.nonzero(nz)[0]):
        r = refs[g]
        assert got["usum"][0, j] == r["usum"] and got["ties"][0, j] == r["ties"], g
        assert abs(got["stat"][0, j] - float(r["stat"])) <= r["stat_tol"], g
        assert abs(got["pvalue"][0, j] - float(r["p"])) <= rr.p_tolerance(r), g
        assert df["auc"].to_numpy()[g] == r["usum"] / r["pairs"], g
    for col in ("stat", "pvalue", "padj", "auc"):  # a gene without counts: NaN, as every other test gives it
        assert np.isnan(df[col].to_numpy()[7]), col
    # no Cook's filter (the Wald summary drops the outlier gene's p-value, the rank test keeps it) ...
    co = dds.cooks_outlier().to_numpy()
    assert co[11] and np.isnan(wald["pvalue"].to_numpy()[co]).all()
    assert np.isfinite(df["pvalue"].to_numpy()[co]).all()
    # ... and padj = independent filtering and BH of exactly these p-values
    padj, _ = _summary.adjusted_pvalues(dds._pipe.ctx, ds.base_mean.to_numpy(), df["pvalue"].to_numpy(), ds.alpha, True)
    assert np.array_equal(df["padj"].to_numpy(), padj, equal_nan=True)
    ds2 = DeseqStats(dds, ["condition", "B", "A"], test="wilcoxon", strata=strata, alt_hypothesis=alt,
                     independent_filter=False)
    padj2, _ = _summary.adjusted_pvalues(dds._pipe.ctx, ds.base_mean.to_numpy(), df["pvalue"].to_numpy(), ds.alpha, False)
    assert np.array_equal(ds2.summary()["padj"].to_numpy(), padj2, equal_nan=True)
    # summary() with another alternative re-runs the rank test; an unsupported one is refused
    other = ds.summary(alt_hypothesis="less" if alt != "less" else "greater")
    assert not np.array_equal(other["pvalue"].to_numpy(), df["pvalue"].to_numpy(), equal_nan=True)
    with pytest.raises(ValueError, match="'greater' or 'less'"):
        ds.summary(alt_hypothesis="greaterAbs")
    with pytest.raises(ValueError, match="no lfc_null"):
        DeseqStats(dds, ["condition", "B", "A"], test="wilcoxon").summary(lfc_null=0.5)


def test_facade_batch_and_pickling(dds, monkeypatch):
    from pydeseq2_amd import DeseqStats, pairwise_contrasts

    calls = []
    monkeypatch.setattr(dds._pipe, "ranksum", lambda *a, _f=dds._pipe.ranksum, **kw: calls.append(1) or _f(*a, **kw))
    cons = pairwise_contrasts(dds, "condition")
    assert cons == [["condition", "B", "A"], ["condition", "C", "A"], ["condition", "C", "B"]]
    batch = DeseqStats.batch(dds, cons, test="wilcoxon", strata="batch")
    assert len(calls) == 1
    got = [b.summary() for b in batch]
    assert len(calls) == 1, "summary() of a batch member ran the rank test again"
    for c, b, g in zip(cons, batch, got):
        one = DeseqStats(dds, c, test="wilcoxon", strata="batch")
        want = one.summary()
        for col in ("stat", "pvalue", "auc"):  # one launch of K = 3: the bits of three launches
            assert np.array_equal(g[col].to_numpy().view(np.int64), want[col].to_numpy().view(np.int64)), (c, col)
        assert np.array_equal(g["padj"].to_numpy(), want["padj"].to_numpy(), equal_nan=True)
        assert np.allclose(g["lfcSE"].to_numpy(), want["lfcSE"].to_numpy(), rtol=1e-9, equal_nan=True)
    assert len(calls) == 4
    with pytest.raises(ValueError, match="must be .factor, tested, ref."):
        DeseqStats.batch(dds, [cons[0], np.array([0.0, 0.0, 1.0, 0.0])], test="wilcoxon")
    with pytest.raises(ValueError, match="does not depend on the contrast"):
        DeseqStats.batch(dds, cons, test="LRT", reduced="~batch")
    assert len(calls) == 4
    # pickles with its results and runs on after loading
    blob = pickle.dumps(batch[0])
    back = pickle.loads(blob)
    assert back.test == "wilcoxon" and back.strata == ["batch"]
    assert back.results_df.equals(got[0]) and back.auc.equals(batch[0].auc)
    again = back.summary(alt_hypothesis="greater")
    want = DeseqStats(dds, cons[0], test="wilcoxon", strata="batch", alt_hypothesis="greater").summary()
    assert np.array_equal(again["pvalue"].to_numpy(), want["pvalue"].to_numpy(), equal_nan=True)
    back.dds.close()


def test_facade_warning_and_refusals(dds):
    from pydeseq2_amd import DeseqStats

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        DeseqStats(dds, ["condition", "B", "A"], test="wilcoxon")  # 18 and 20 samples: no warning
    with pytest.warns(UserWarning, match="6 tested and 20 reference samples - below 8"):
        small = DeseqStats(dds, ["condition", "C", "A"], test="wilcoxon", strata="batch")
    assert np.isfinite(small.summary()["pvalue"].to_numpy()[0])
    with pytest.warns(UserWarning, match="18 tested and 6 reference"):
        DeseqStats(dds, ["condition", "B", "C"], test="wilcoxon")
    with pytest.raises(ValueError, match="must be .factor, tested, ref."):
        DeseqStats(dds, np.array([0.0, 0.0, 1.0, 0.0]), test="wilcoxon")
    with pytest.raises(ValueError, match="are the same"):
        DeseqStats(dds, ["condition", "B", "B"], test="wilcoxon")
    with pytest.raises(ValueError, match="should be levels of 'condition'"):
        DeseqStats(dds, ["condition", "B", "Z"], test="wilcoxon")
    with pytest.raises(ValueError, match=r"not found: \['site'\]"):
        DeseqStats(dds, ["condition", "B", "A"], test="wilcoxon", strata="site")
    with pytest.raises(ValueError, match="pass test='wilcoxon'"):
        DeseqStats(dds, ["condition", "B", "A"], strata="batch")
    with pytest.raises(ValueError, match="needs DeseqStats"):
        DeseqStats(dds, ["condition", "B", "A"]).run_ranksum_test()
    with pytest.raises(ValueError, match="'greater' or 'less'"):
        dds._pipe.ranksum(dds._res, np.where(dds.obs["condition"] == "B", 1, 0), alt_hypothesis="lessAbs")
    with pytest.raises(ValueError, match="K x N with N = 44"):
        dds._pipe.ranksum(dds._res, np.array([1, 0, 1]))
