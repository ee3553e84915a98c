"""Designs of 49 ... 128 columns on the GPU (the slot geometry of dsq_k_wide.hip: p x p matrices in device-memory slots, one
gene per workgroup): the reference KATs through the plug-in C ABI, deseq2() + Wald end to end against the oracle (the paired
`~subject + condition` design, a 72-level factor with outliers, 128 mixed columns), the façade, run-to-run bit equality
and two ranks sharing the genes."""
import threading

import numpy as np
import pandas as pd
import pytest

from oracle import nbglm_oracle as orc
from tests.helpers import assert_close, load_kat
from tests.test_gpu_parity import _compare, _jobs

pytestmark = pytest.mark.gpu


def _synth(X, G, seed, eff=0.3, min_mean=30.0, b0=6.0, d0=0.1):
    """NB counts of G expressed genes (mean count >= min_mean) on the design X (log2-scale coefficients, intercept
    around b0, dispersion 4 / mean + d0)."""
    rng = np.random.default_rng(seed)
    N, p = X.shape
    sf = np.exp(rng.normal(0, 0.2, N))
    out, have = [], 0
    while have < G:
        B = 4 * G
        beta = np.vstack([rng.normal(b0, 1.5 if b0 == 6.0 else 1.0, B)] + [rng.normal(0, eff, B) for _ in range(p - 1)])
        disp = 4 / np.maximum(2.0 ** beta[0], 1e-3) + d0
        mu = sf[:, None] * 2.0 ** (X @ beta)
        size = 1 / disp
        c = rng.negative_binomial(size[None, :], size[None, :] / (size[None, :] + mu)).astype(np.int64)
        c = c[:, c.mean(0) >= min_mean]
        out.append(c)
        have += c.shape[1]
    return np.ascontiguousarray(np.hstack(out)[:, :G])


def _paired(n_sub=64):
    i = np.arange(2 * n_sub)
    cols = [np.ones(2 * n_sub)] + [(i // 2 == s) for s in range(1, n_sub)] + [i % 2 == 1]
    return np.column_stack([np.asarray(v, dtype=float) for v in cols])


def _factor(levels, reps):
    lv = np.arange(levels * reps) // reps
    cols = [np.ones(levels * reps)] + [(lv == k) for k in range(1, levels)]
    return np.column_stack([np.asarray(v, dtype=float) for v in cols])


def _mixed(p, N, seed):
    rng = np.random.default_rng(seed)
    a, b = np.arange(N) % 2, (np.arange(N) // 2) % 4
    cols = [np.ones(N), (a == 1)] + [(b == k) for k in (1, 2, 3)]
    while len(cols) < p:
        cols.append(rng.normal(0, 0.6, N))
    return np.column_stack([np.asarray(v, dtype=float) for v in cols])


@pytest.fixture(scope="module")
def paired():
    """(a): 64 subjects x 2 conditions, P = 65, G = 400; the condition contrast and the oracle's result."""
    X = _paired(64)
    counts = _synth(X, 400, 65)
    c = np.zeros(X.shape[1])
    c[-1] = 1.0
    ref = orc.deseq2(counts, X, contrast=c, n_jobs=_jobs())
    return counts, X, c, ref


@pytest.mark.parametrize("case", ["p65", "p72", "p128"])
def test_wider_kats_through_the_plugin_abi(case):
    """Every per-gene stage of the wider family against the reference, at the tolerances of the p40 / p48 KATs."""
    from pydeseq2_amd import HipInference

    inf = HipInference(device=0)
    k = load_kat(case)
    P = k["X"].shape[1]
    maxd = float(max(10, k["X"].shape[0]))
    assert_close(inf.fit_rough_dispersions(k["normed"], k["X"]), k["rough"], 1e-9, 1e-13, "rough")
    assert_close(inf.fit_moments_dispersions(k["normed"], k["sf"]), k["moments"], 1e-10, 1e-14, "moments")
    assert_close(inf.lin_reg_mu(k["counts"], k["sf"], k["X"], 0.5), k["lin_mu"], 1e-10, 0, "lin_mu")
    b, mu, H, conv = inf.irls(k["counts"], k["sf"], k["X"], k["mom"], 0.5, 1e-8)
    assert (conv == k["irls_conv"]).all()
    assert_close(b, k["irls_beta"], 1e-8, 1e-10, "irls beta")
    assert_close(mu, k["irls_mu"], 1e-8, 1e-10, "irls mu")
    assert_close(H, k["irls_H"], 1e-8, 1e-12, "irls H")
    a, c = inf.alpha_mle(k["counts"], k["X"], k["mu_hat"], k["mom"], 1e-8, maxd)
    assert (c == k["gw_conv"]).all()
    assert_close(a, k["gw_alpha"], 2e-6, 0, "genewise alpha")
    a, c = inf.alpha_mle(k["counts"], k["X"], k["mu_hat"], k["fitted"], 1e-8, maxd,
                         prior_disp_var=float(k["prior_var"]), cr_reg=True, prior_reg=True)
    assert (c == k["map_conv"]).all()
    assert_close(a, k["map_alpha"], 2e-6, 0, "MAP alpha")
    ng = len(k["grid_alpha"])
    la = inf.grid_fit_alpha(k["counts"][:, :ng], k["X"], k["mu_hat"][:, :ng], 1e-8, maxd)
    assert np.abs(la - k["grid_alpha"]).max() < 1e-12
    disp = np.clip(k["map_alpha"], 1e-8, maxd)
    b, mu, H, conv = inf.irls(k["counts"], k["sf"], k["X"], disp, 0.5, 1e-8)
    assert (conv == k["lfc_conv"]).all()
    assert_close(b, k["lfc_beta"], 1e-8, 1e-10, "lfc beta")
    assert_close(H, k["lfc_H"], 1e-8, 1e-12, "lfc H")
    mu_w = np.exp(k["X"] @ k["lfc_beta"].T) * k["sf"][:, None]
    ridge = np.diag(np.repeat(1e-6, P))
    for alt, null in ((None, 0.0), ("greater", 0.5), ("less", -0.5), ("greaterAbs", 0.5), ("lessAbs", 0.5)):
        tag = alt or "none"
        p, s, se = inf.wald_test(k["X"], disp, k["lfc_beta"], mu_w, ridge, k["contrast"], np.log(2) * null, alt)
        assert_close(se, k[f"wald_se_{tag}"], 1e-10, 0, f"se {tag}")
        assert_close(s, k[f"wald_stat_{tag}"], 1e-9, 1e-13, f"stat {tag}")
        assert_close(p, k[f"wald_p_{tag}"], 1e-8, 1e-300, f"p {tag}")


def test_paired_design_of_64_subjects_end_to_end(paired):
    import pydeseq2_amd

    counts, X, c, ref = paired
    res = pydeseq2_amd.deseq2(counts, X, contrast=c, device=0)
    _compare(res, ref, frac_noise=0.01)


def test_72_level_factor_with_outliers_replaced_and_refitted():
    """72 design cells (the linear-model mu_hat beyond 64 cells), 8 replicates each: Cook's outliers are replaced and
    their genes refitted on the wider kernels."""
    import pydeseq2_amd

    X = _factor(72, 8)
    counts = _synth(X, 300, 72, b0=9.0, d0=0.005)  # low dispersions: an outlier's Cook's distance clears F(0.99, 72, 504)
    rng = np.random.default_rng(7)
    hit = rng.choice(300, 30, replace=False)
    counts[rng.integers(0, X.shape[0], 30), hit] *= 60
    c = np.zeros(X.shape[1])
    c[1] = 1.0
    res = pydeseq2_amd.deseq2(counts, X, contrast=c, device=0)
    ref = orc.deseq2(counts, X, contrast=c, n_jobs=_jobs())
    assert ref.refitted.sum() >= 10 and res.refitted.sum() >= 10
    _compare(res, ref, frac_noise=0.01)


def test_128_mixed_columns_end_to_end():
    import pydeseq2_amd

    X = _mixed(128, 512, 128)
    counts = _synth(X, 200, 128)
    c = np.zeros(X.shape[1])
    c[1] = 1.0
    res = pydeseq2_amd.deseq2(counts, X, contrast=c, device=0)
    ref = orc.deseq2(counts, X, contrast=c, n_jobs=_jobs())
    _compare(res, ref, frac_noise=0.01)


def test_facade_paired_design_summary_and_shrinkage_limit(paired):
    from pydeseq2_amd.api import DeseqDataSet, DeseqStats

    counts, X, c, ref = paired
    N, G = counts.shape
    idx = [f"s{i}" for i in range(N)]
    meta = pd.DataFrame({"subject": [f"p{i // 2:02d}" for i in range(N)], "condition": ["A", "B"] * (N // 2)}, index=idx)
    df = pd.DataFrame(counts, index=idx, columns=[f"g{j}" for j in range(G)])
    dds = DeseqDataSet(counts=df, metadata=meta, design="~subject + condition")
    assert np.array_equal(np.asarray(dds.obsm["design_matrix"], dtype=float), X)
    dds.deseq2()
    ds = DeseqStats(dds, contrast=["condition", "B", "A"])
    out = ds.summary()
    want = orc.summary(ref, c)["padj"]
    assert (np.isnan(out["padj"].to_numpy()) == np.isnan(want)).all()
    assert_close(out["padj"].to_numpy(), want, 1e-5, 1e-12, "padj")
    with pytest.raises(ValueError, match="at most 48"):
        ds.lfc_shrink(coeff="condition[T.B]")


def test_paired_design_runs_are_bit_identical(paired):
    import pydeseq2_amd

    counts, X, c, _ = paired
    a = pydeseq2_amd.deseq2(counts, X, contrast=c, device=0)
    b = pydeseq2_amd.deseq2(counts, X, contrast=c, device=0)
    for f in ("size_factors", "genewise_dispersions", "dispersions", "LFC", "lfcSE", "stat", "pvalue"):
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f


def test_paired_design_two_ranks_threads(paired):
    """Two gene shards as two ranks (threads, one context each) through DistDeseqPipeline: each rank reproduces its
    slice of the single-GPU result."""
    import pydeseq2_amd
    from pydeseq2_amd._lib import Context
    from pydeseq2_amd.distributed import DistDeseqPipeline

    counts, X, _, _ = paired
    W, cuts = 2, [0, 150, counts.shape[1]]
    res_full = pydeseq2_amd.DeseqPipeline(counts, X, device=0).deseq2()
    barrier = threading.Barrier(W)
    slots = [None] * W

    class ThreadComm:
        def __init__(self, ctx, rank):
            self.ctx, self.rank, self.world = ctx, rank, W

        def _exchange(self, host):
            slots[self.rank] = host
            barrier.wait()
            got = list(slots)
            barrier.wait()
            return got

        def allreduce_sum(self, darr):
            n = darr.nbytes // darr.dtype.itemsize
            host = np.empty(n, dtype=darr.dtype)
            self.ctx.d2h(host, darr.ptr)
            self.ctx.h2d(darr.ptr, np.sum(self._exchange(host), axis=0).astype(darr.dtype))
            return darr

        def allgather(self, dsend, drecv):
            host = np.empty(dsend.nbytes // 8, dtype=np.float64)
            self.ctx.d2h(host, dsend.ptr)
            self.ctx.h2d(drecv.ptr, np.concatenate(self._exchange(host)))
            return drecv

    out, errs = [None] * W, []

    def run(rank):
        try:
            ctx = Context(0)
            sl = slice(cuts[rank], cuts[rank + 1])
            pipe = DistDeseqPipeline(np.ascontiguousarray(counts[:, sl]), X, comm=ThreadComm(ctx, rank), ctx=ctx)
            out[rank] = pipe.deseq2()
        except Exception as e:  # pragma: no cover
            errs.append(e)
            barrier.abort()

    ts = [threading.Thread(target=run, args=(r,)) for r in range(W)]
    [t.start() for t in ts]
    [t.join(300) for t in ts]
    assert not errs, errs
    for rank in range(W):
        sl = slice(cuts[rank], cuts[rank + 1])
        r = out[rank]
        assert_close(r.size_factors, res_full.size_factors, 1e-14, 0, "sf")
        assert_close(r.trend_coeffs, res_full.trend_coeffs, 1e-9, 0, "trend")
        assert abs(r.prior_disp_var - res_full.prior_disp_var) < 1e-10
        assert np.array_equal(r.genewise_dispersions, res_full.genewise_dispersions[sl], equal_nan=True)
        # the trend's fitted values (the MAP fits' alpha_hat) agree to rounding only (the gathered order differs), and
        # the MAP L-BFGS-B runs stop within their own tolerance of each other on these flat objectives: the parity
        # tolerance of _compare (1e-5), and a run whose success flag flips on that noise is left out (at most two)
        noisy = r.MAP_converged != res_full.MAP_converged[sl]
        assert noisy.sum() <= 2
        ok = ~noisy
        assert_close(r.dispersions[ok], res_full.dispersions[sl][ok], 1e-5, 0, "disp")
        assert_close(r.LFC[ok], res_full.LFC[sl][ok], 1e-5, 1e-8, "LFC")
        stat = res_full.stat[sl][ok]
        perr = np.abs(r.pvalue[ok] - res_full.pvalue[sl][ok]) / np.maximum(res_full.pvalue[sl][ok], 1e-300)
        assert (perr / np.maximum(1.0, stat ** 2)).max() <= 1e-5


def test_irls_rescue_kernel_reuses_its_workspace_across_genes():
    """maxiter = 2 sends every gene through the L-BFGS-B rescue (utils.py:374-413), k_irls_rescue_wide<SlotGeom>.  600 genes
    are more than the resident workgroups, so later genes run on workgroups (LDS optimiser state, device-memory slot) that
    fitted an earlier gene: against the oracle at both ends, and bitwise equal to the same genes fitted alone."""
    from pydeseq2_amd import HipInference

    inf = HipInference(device=0)
    X = _paired(64)
    G = 600
    counts = _synth(X, G, 11)
    sf = np.exp(np.random.default_rng(1).normal(0, 0.2, X.shape[0]))
    disp = np.full(G, 0.1)
    b, mu, H, conv = inf.irls(counts, sf, X, disp, 0.5, 1e-8, maxiter=2)
    calls = [0]
    fallback = orc._irls_fallback

    def spy(*a, **kw):
        calls[0] += 1
        return fallback(*a, **kw)

    orc._irls_fallback = spy
    try:
        sel = np.r_[0:24, G - 24:G]
        start = np.linalg.qr(X)
        ref = [orc.irls_gene(counts[:, g], sf, X, disp[g], start, maxiter=2) for g in sel]
    finally:
        orc._irls_fallback = fallback
    assert calls[0] == len(sel)
    assert (conv[sel] == np.array([r[3] for r in ref])).all()
    assert_close(b[sel], np.array([r[0] for r in ref]), 1e-6, 1e-8, "rescue beta")
    assert_close(mu[:, sel], np.array([r[1] for r in ref]).T, 1e-6, 1e-10, "rescue mu")
    assert_close(H[:, sel], np.array([r[2] for r in ref]).T, 1e-6, 1e-10, "rescue H")
    b2, mu2, H2, conv2 = inf.irls(counts, sf, X, disp, 0.5, 1e-8, maxiter=2)
    assert np.array_equal(b, b2) and np.array_equal(mu, mu2) and np.array_equal(H, H2) and (conv == conv2).all()
    for g in (0, 300, G - 1):
        b1, mu1, H1, c1 = inf.irls(counts[:, [g]], sf, X, disp[[g]], 0.5, 1e-8, maxiter=2)
        assert np.array_equal(b1[0], b[g]) and np.array_equal(mu1[:, 0], mu[:, g]) and np.array_equal(H1[:, 0], H[:, g])
        assert c1[0] == conv[g]


def test_closing_contexts_releases_the_wider_slots():
    """The device-memory slots of the wider kernels belong to the streams of a context: creating, using and closing
    contexts over and over leaves the device's free memory where it was."""
    import ctypes
    import gc

    import pydeseq2_amd
    from pydeseq2_amd._lib import Context

    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = ctypes.c_size_t(), ctypes.c_size_t()
        assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value

    X = _paired(64)
    counts = _synth(X, 300, 3)

    def cycle():
        ctx = Context(0)
        r = pydeseq2_amd.DeseqPipeline(counts, X, ctx=ctx).deseq2()
        assert np.isfinite(r.dispersions).all()
        del r
        gc.collect()
        ctx.close()
        gc.collect()

    cycle()
    before = free_bytes()
    for _ in range(4):
        cycle()
    assert before - free_bytes() < 64 << 20, (before - free_bytes()) / 2**20
