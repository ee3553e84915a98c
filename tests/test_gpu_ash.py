"""Adaptive shrinkage on the GPU: dsq_dev_ash (k_ash_fit, k_ash_post) against the dense restatement (tests/ash_ref) and the
host build in the device's order (tests/hostash) over the seeded sets of tests/ash_cases - every chunk edge, unused genes,
the tile edges of the Gram matrix, several contrasts in one call -, guard values, reruns, the argument refusals, and the
facade: DeseqStats.lfc_shrink(type="ashr") on a contrast apeGLM cannot take, summary() afterwards, shrink_batch."""
import ctypes as C
import warnings

import numpy as np
import pytest

from tests import ash_cases as ac
from tests import ash_ref
from tests import hostash as ha
from tests.helpers import load_dataset

pytestmark = pytest.mark.gpu

_vp = C.c_void_p
GUARD = 3


@pytest.fixture(scope="module")
def ctx():
    from pydeseq2_amd._lib import Context

    return Context(0)


def _dev_ash(ctx, cases, grids=None, max_iter=100, ldg_extra=0):
    """dsq_dev_ash on K cases of equal G -> the dict tests/hostash.ash returns; guard values behind the end of all eight
    outputs, and the pad of every row, are checked untouched."""
    from pydeseq2_amd._lib import DeviceArray

    K, G = len(cases), len(cases[0].b)
    grids = [c.sd for c in cases] if grids is None else grids
    mk = np.array([len(g) for g in grids], np.int32)
    ldm, ldg = max(1, int(mk.max())) + 1, G + ldg_extra
    b, s, sd = np.zeros((K, ldg)), np.zeros((K, ldg)), np.zeros((K, ldm))
    for k, c in enumerate(cases):
        b[k, :G], s[k, :G], sd[k, :mk[k]] = c.b, c.s, grids[k]
    d_in = [DeviceArray.from_host(ctx, a.ravel()) for a in (b, s, sd, mk)]
    shapes = dict(pi=(K * ldm, np.float64), post_mean=(K * ldg, np.float64), post_sd=(K * ldg, np.float64),
                  lfsr=(K * ldg, np.float64), n_iter=(K, np.int32), converged=(K, np.uint8), kkt=(K, np.float64),
                  loglik=(K, np.float64))
    fill = {np.float64: -7.0, np.int32: -7, np.uint8: 0x5A}
    d_out = {k: DeviceArray.from_host(ctx, np.full(n + GUARD, fill[t], t)) for k, (n, t) in shapes.items()}
    try:
        ctx.call("dsq_dev_ash", _vp(d_in[0].ptr), _vp(d_in[1].ptr), G, ldg, K, _vp(d_in[2].ptr), _vp(d_in[3].ptr), ldm,
                 max_iter, *[_vp(d_out[k].ptr) for k in shapes])
        ctx.sync()
        o = {k: d_out[k].to_host() for k in shapes}
    finally:
        for a in d_in + list(d_out.values()):
            a.free()
    for k, (n, t) in shapes.items():
        assert (o[k][n:] == fill[t]).all(), f"{k}: the guard values behind the output were written"
        o[k] = o[k][:n]
    for k, ld in (("pi", ldm), ("post_mean", ldg), ("post_sd", ldg), ("lfsr", ldg)):
        o[k] = o[k].reshape(K, ld)
    for k in range(K):
        assert (o["pi"][k, mk[k]:] == -7.0).all()
        for key in ("post_mean", "post_sd", "lfsr"):
            assert (o[key][k, G:] == -7.0).all()
    o["skipped"] = mk == 0
    assert set(np.unique(o["converged"][~o["skipped"]])) <= {0, 1}
    return o


def _same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def _vs_host(c, got, k=0):
    """Against the host build in the device's order: the same pieces in the same order everywhere but inside a chunk of the
    Gram matrix, so the two may part by a step's rounding and, like any two fits, stop within the measured tolerance."""
    h = ha.ash(c.b[None], c.s[None], [c.sd], ha.WAVES4)
    u = ash_ref.used(c.b, c.s)
    for key in ("post_mean", "post_sd", "lfsr"):
        a, e = got[key][k][:len(c.b)][u], h[key][0][u]
        assert (np.abs(a - e) <= ac.POST_TOL * np.maximum(1.0, np.abs(e))).all(), f"{c.name}: {key} vs the host build"
    return h


@pytest.mark.parametrize("G", [1, 5, 63, 64, 65, 203, 3000])
@pytest.mark.parametrize("kind", ac.KINDS)
def test_sets_vs_restatement_and_host_build(ctx, kind, G):
    """The four constructions at every chunk edge (one lane, a partly filled chunk, exactly one, one gene into the second,
    three full chunks and a tail, 47 chunks over four waves); a second launch gives the same bits.  heavy at G = 3000
    lies outside the condition on the inputs (tests/ash_cases): there the device must say so, as the host build does."""
    if (kind, G) == ("heavy", 3000):
        c = ac.breakdown()
        got = _dev_ash(ctx, [c])
        h = ha.ash(c.b[None], c.s[None], [c.sd], ha.WAVES4)
        assert not got["converged"][0] and not h["converged"][0]
        pi = got["pi"][0][:c.M]
        assert (pi >= 0).all() and abs(pi.sum() - 1) <= 1e-12 and np.isfinite(got["post_mean"][0][:G]).all()
        L, _ = ash_ref.lik(c.b, c.s, c.sd)
        assert ash_ref.kkt_residual(L, pi) > 1e-8  # (the flag is truthful)
        return
    c = ac.case(kind, G)
    got = _dev_ash(ctx, [c])
    worst = ac.check(c, got, 0, "device")
    _vs_host(c, got)
    print(f"{c.name} M={c.M}: {got['n_iter'][0]} iterations, KKT {got['kkt'][0]:.3g}, largest difference from the "
          f"restatement {worst}")
    assert _same_bits(got, _dev_ash(ctx, [c]))


@pytest.mark.parametrize("M", ac.FORCED_M)
def test_forced_grids_at_the_tile_edges(ctx, M):
    c = ac.forced(M)
    got = _dev_ash(ctx, [c])
    ac.check(c, got, 0, "device")
    _vs_host(c, got)


def test_three_contrasts_one_unused_genes_one_skipped(ctx):
    """K = 3 in one call, row pitches larger than G and M: a plain set, the heavy set with unused genes (among them the
    first and the last gene and a whole chunk), and a contrast with m = 0, whose outputs stay untouched; the rows equal
    the single-contrast calls bit for bit."""
    cs = [ac.case("plain", 203), ac.nan_case("heavy", 203), ac.case("wide-se", 203)]
    grids = [cs[0].sd, cs[1].sd, np.zeros(0)]
    got = _dev_ash(ctx, cs, grids, ldg_extra=5)
    for k in (0, 1):
        ac.check(cs[k], got, k, "device K=3")
        one = _dev_ash(ctx, [cs[k]])
        for key in ("pi", "post_mean", "post_sd", "lfsr"):
            n = cs[k].M if key == "pi" else 203
            assert got[key][k][:n].tobytes() == one[key][0][:n].tobytes()
        assert got["n_iter"][k] == one["n_iter"][0] and got["loglik"][k] == one["loglik"][0]
    assert (got["post_mean"][2] == -7.0).all() and got["n_iter"][2] == -7 and got["converged"][2] == 0x5A
    assert got["kkt"][2] == -7.0 and got["loglik"][2] == -7.0
    big = ac.nan_case("wide-se", 3000)
    ac.check(big, _dev_ash(ctx, [big]), 0, "device")


def test_no_used_gene_and_the_iteration_cap(ctx):
    c = ac.case("plain", 65)
    dead = ac.Case.__new__(ac.Case)
    dead.b, dead.s, dead.sd, dead.M, dead.name = np.full(65, np.nan), c.s, c.sd, c.M, "no used gene"
    got = _dev_ash(ctx, [dead])
    assert np.isnan(got["pi"][0][:c.M]).all() and np.isnan(got["post_mean"][0][:65]).all()
    assert got["n_iter"][0] == 0 and got["converged"][0] == 0 and np.isnan(got["kkt"][0]) and np.isnan(got["loglik"][0])
    capped = _dev_ash(ctx, [c], max_iter=1)
    assert capped["n_iter"][0] == 1 and capped["converged"][0] == 0 and capped["kkt"][0] > 1e-8
    assert abs(capped["pi"][0][:c.M].sum() - 1) <= 1e-12


def test_argument_refusals(ctx):
    from pydeseq2_amd._lib import DeviceArray

    d = DeviceArray.from_host(ctx, np.full(256, -7.0))
    m_ok = DeviceArray.from_host(ctx, np.array([3, 0], np.int32))
    m_bad = [DeviceArray.from_host(ctx, np.array(v, np.int32)) for v in ([3, 49], [-1, 3])]
    p = _vp(d.ptr)
    ok = dict(G=4, ldg=8, K=2, m=_vp(m_ok.ptr), ldm=4, it=100, lfc=p, se=p, sd=p, o=[p] * 8)

    def call(**kw):
        a = {**ok, **kw}
        ctx.call("dsq_dev_ash", a["lfc"], a["se"], a["G"], a["ldg"], a["K"], a["sd"], a["m"], a["ldm"], a["it"], *a["o"])

    bad = [dict(K=0), dict(G=-1), dict(ldg=3), dict(m=_vp(m_bad[0].ptr)), dict(m=_vp(m_bad[1].ptr)), dict(ldm=2),
           dict(it=0), dict(lfc=None), dict(se=None), dict(sd=None), dict(m=None)]
    bad += [dict(o=[None if j == i else p for j in range(8)]) for i in range(8)]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
    call(G=0, ldg=0)  # nothing to do, nothing written
    ctx.sync()
    assert (d.to_host() == -7.0).all()
    for a in [d, m_ok] + m_bad:
        a.free()


# ------------------------------------------------------------------ the facade
@pytest.fixture(scope="module")
def synthetic():
    from pydeseq2_amd.api import DeseqDataSet

    counts, meta = load_dataset("synthetic")
    meta = meta.copy()
    meta["condition"] = np.array(["A", "B", "C"])[np.arange(len(meta)) % 3]  # three levels: B vs C is no design column
    dds = DeseqDataSet(counts=counts, metadata=meta, design="~condition")
    dds.deseq2()
    yield dds
    dds.close()


def test_lfc_shrink_ashr_on_a_contrast_that_is_no_column(synthetic):
    from pydeseq2_amd.api import DeseqStats
    from pydeseq2_amd.ash import mixsd_grid

    ds = DeseqStats(synthetic, contrast=["condition", "C", "B"], quiet=True)
    with pytest.raises(KeyError):
        ds.lfc_shrink("condition[T.C]_vs_B")  # apeGLM takes design columns only
    ds.summary()
    before = ds.results_df.copy()
    ds.lfc_shrink(type="ashr", svalue=True)
    after = ds.results_df
    assert ds.shrunk_LFCs and ds.ash_fit["converged"]
    u = np.isfinite(before["log2FoldChange"].to_numpy()) & (before["lfcSE"].to_numpy() > 0)
    assert u.sum() >= 8  # (the synthetic set has ten genes)
    a, b0 = after["log2FoldChange"].to_numpy(), before["log2FoldChange"].to_numpy()
    assert (np.abs(a[u]) <= np.abs(b0[u]) * (1 + 1e-12)).all() and (np.sign(a[u]) * np.sign(b0[u]) >= 0).all()
    assert (np.abs(a[u]) < np.abs(b0[u])).mean() > 0.9
    # against the restatement fed with the published unshrunk values (log2 scale: the statement is homogeneous)
    e = ash_ref.ash(b0, before["lfcSE"].to_numpy())
    assert np.allclose(mixsd_grid(b0, before["lfcSE"].to_numpy()), e["grid"], rtol=1e-12, atol=0)
    assert np.allclose(ds.ash_fit["grid"] / np.log(2), e["grid"], rtol=1e-9, atol=0)
    assert (np.abs(a[u] - e["post_mean"][u]) <= ac.POST_TOL * np.maximum(1, np.abs(e["post_mean"][u]))).all()
    assert (np.abs(after["lfcSE"].to_numpy()[u] - e["post_sd"][u]) <= ac.POST_TOL).all()
    assert (np.abs(ds.lfsr.to_numpy()[u] - e["lfsr"][u]) <= ac.POST_TOL).all()
    # s-values: monotone in lfsr, NaN exactly where lfsr is
    sv, fs = after["svalue"].to_numpy(), ds.lfsr.to_numpy()
    o = np.argsort(fs[u], kind="stable")
    assert (np.diff(sv[u][o]) >= 0).all() and np.array_equal(np.isnan(sv), np.isnan(fs))
    assert np.array_equal(sv[u], ash_ref.svalues(fs)[u])
    # the other columns are untouched, and a later summary() keeps the shrunk values
    for col in ("baseMean", "stat", "pvalue", "padj"):
        assert before[col].equals(after[col])
    ds.summary()
    assert np.array_equal(ds.results_df["log2FoldChange"].to_numpy(), a, equal_nan=True)
    assert np.array_equal(ds.results_df["lfcSE"].to_numpy(), after["lfcSE"].to_numpy(), equal_nan=True)
    # re-running the Wald test under another null drops them
    ds.summary(lfc_null=0.5, alt_hypothesis="greaterAbs")
    assert not ds.shrunk_LFCs and np.array_equal(ds.results_df["log2FoldChange"].to_numpy(), b0, equal_nan=True)


def test_shrink_batch_equals_the_single_calls(synthetic):
    from pydeseq2_amd.api import DeseqStats, pairwise_contrasts

    cons = pairwise_contrasts(synthetic, "condition")
    assert len(cons) == 3
    batch = DeseqStats.batch(synthetic, cons, quiet=True)
    DeseqStats.shrink_batch(batch, svalue=True)
    for con, bs in zip(cons, batch):
        one = DeseqStats(synthetic, contrast=con, quiet=True)
        one.summary()
        one.lfc_shrink(type="ashr", svalue=True)
        assert bs.shrunk_LFCs and bs.ash_fit["converged"]
        bs.summary()  # (a batch member has no results_df yet: the summary publishes the shrunk values)
        for col in ("log2FoldChange", "lfcSE", "svalue"):
            x, y = bs.results_df[col].to_numpy(), one.results_df[col].to_numpy()
            assert np.array_equal(np.isnan(x), np.isnan(y))
            ok = ~np.isnan(x)
            assert (np.abs(x[ok] - y[ok]) <= ac.POST_TOL * np.maximum(1, np.abs(y[ok]))).all(), (con, col)


def test_apeglm_path_is_what_it_was(synthetic):
    """lfc_shrink(coeff) with the default type: the values of the positional call and of type="apeglm" are the same bits,
    and ashr on the same column shrinks to something else."""
    from pydeseq2_amd.api import DeseqStats

    out = []
    for kw in (dict(), dict(type="apeglm")):
        ds = DeseqStats(synthetic, contrast=["condition", "B", "A"], quiet=True)
        ds.summary()
        ds.lfc_shrink("condition[T.B]", **kw)
        out.append(ds.results_df[["log2FoldChange", "lfcSE"]].to_numpy().copy())
        assert not hasattr(ds, "ash_fit") or ds.ash_fit is None
    assert out[0].tobytes() == out[1].tobytes()
    with pytest.raises(ValueError, match="apeglm.*ashr|ashr.*apeglm"):
        ds.lfc_shrink("condition[T.B]", type="normal")
    with pytest.raises(ValueError, match="coeff"):
        ds.lfc_shrink("condition[T.B]", type="ashr")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ds.lfc_shrink(type="ashr")
    assert np.nanmax(np.abs(ds.results_df["log2FoldChange"].to_numpy() - out[0][:, 0])) > 1e-6


def test_ashr_after_the_likelihood_ratio_test(synthetic):
    """test="LRT" has the contrast's LFC and SE too: shrinking before or after summary() gives the Wald path's shrunk values,
    and the statistic and p-value stay the likelihood-ratio test's."""
    from pydeseq2_amd.api import DeseqStats

    con = ["condition", "C", "B"]
    wald = DeseqStats(synthetic, contrast=con, quiet=True)
    wald.summary()
    wald.lfc_shrink(type="ashr")
    first = DeseqStats(synthetic, contrast=con, quiet=True, test="LRT", reduced="~1")
    first.lfc_shrink(type="ashr")  # (no SE yet: the Wald test runs for it)
    first.summary()
    after = DeseqStats(synthetic, contrast=con, quiet=True, test="LRT", reduced="~1")
    plain = after.summary().copy()
    after.lfc_shrink(type="ashr")
    after.summary()
    for ds in (first, after):
        for col in ("log2FoldChange", "lfcSE"):
            assert np.array_equal(ds.results_df[col].to_numpy(), wald.results_df[col].to_numpy(), equal_nan=True)
        for col in ("stat", "pvalue", "padj"):
            assert np.array_equal(ds.results_df[col].to_numpy(), plain[col].to_numpy(), equal_nan=True)
    assert not np.array_equal(plain["stat"].to_numpy(), wald.results_df["stat"].to_numpy(), equal_nan=True)
