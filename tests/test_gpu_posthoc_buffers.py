"""Lifetime of the device buffers of every post-hoc call on the GPU: the set of live allocations of the
context after a call equals the set before it - on a normal return, and when the call's launch raises - and an array the
caller owns is alive and readable afterwards.  One fitted pipeline (12 samples, 96 genes, two columns; six genes without
counts, so every gather runs; one injected Cook's outlier, so lrt() also gathers the replaced counts)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, G = 12, 96
ZERO = np.array([3, 17, 40, 41, 77, 95])
OUTLIER = 5


class Fitted:
    """The pipeline, its result, and the context's malloc / free wrapped to keep the set of live pointers."""

    def __init__(self):
        import pydeseq2_amd
        from pydeseq2_amd._lib import Context

        rng = np.random.default_rng(96)
        self.X = np.column_stack([np.ones(N), np.arange(N) % 2]).astype(float)
        base = rng.uniform(np.log(30.0), np.log(3000.0), G)
        mu = np.exp(base[None, :] + np.outer(self.X[:, 1], rng.normal(0, 0.7, G)))
        disp = 4.0 / np.exp(base) + 0.05
        counts = rng.negative_binomial(1 / disp[None, :], 1 / (1 + disp[None, :] * mu)).astype(np.int64)
        counts[:, ZERO] = 0
        counts[2, OUTLIER] = 400 * int(counts[:, OUTLIER].max() + 1)
        self.counts = counts
        self.ctx = ctx = Context(0)
        self.live = set()
        malloc, free = ctx.malloc, ctx.free

        def tracked_malloc(nbytes):
            p = malloc(nbytes)
            self.live.add(p)
            return p

        def tracked_free(p):
            free(p)
            self.live.discard(p)

        ctx.malloc, ctx.free = tracked_malloc, tracked_free
        self.pipe = pydeseq2_amd.DeseqPipeline(counts, self.X, ctx=ctx, min_replicates=5)  # (cells of six: replaceable)
        self.res = self.pipe.deseq2(contrast=np.array([0.0, 1.0]))
        self.x = np.log2(counts / np.asarray(self.res.size_factors)[:, None] + 1.0)  # a transformed matrix, N x G

    def calls(self):
        """name -> (the call, the dsq_dev_* entry point at which the error run raises)"""
        from pydeseq2_amd.summary import lfc_shrink

        pipe, res, x = self.pipe, self.res, self.x
        K3 = np.array([[0.0, 1.0], [1.0, 0.0], [1.0, -1.0]])
        lfc, se = np.asarray(res.LFC)[:, 1][None, :], np.asarray(res.lfcSE)[None, :]
        labels, strata = np.arange(N) % 2, np.arange(N) // 6
        nz, trend = np.asarray(res.non_zero, bool), (res.trend_coeffs, res.mean_disp)
        with np.errstate(all="ignore"):
            logmeans = np.log(np.asarray(res.normed_means, dtype=float))  # (any finite vector on the genes with counts)
        ctl = np.setdiff1d(np.arange(0, G, 3), np.append(ZERO, OUTLIER))
        return {
            "wald": (lambda: pipe.wald(res, [0.0, 1.0]), "dsq_dev_wald"),
            "wald_multi": (lambda: pipe.wald_multi(res, K3), "dsq_dev_wald_multi"),
            "lrt": (lambda: pipe.lrt(res, self.X[:, :1]), "dsq_dev_lrt"),
            "rlog": (lambda: pipe.rlog(res), "dsq_dev_rlog"),
            "ash": (lambda: pipe.ash(lfc, se), "dsq_dev_ash"),
            "ranksum": (lambda: pipe.ranksum(res, labels, strata=strata), "dsq_dev_ranksum"),
            "pca": (lambda: pipe.pca(x, ntop=50), "dsq_dev_sample_gram"),
            "sample_distances": (lambda: pipe.sample_distances(x), "dsq_dev_gram_dist"),
            "residuals": (lambda: pipe.residuals(res), "dsq_dev_nb_residuals"),
            "ruv_g": (lambda: pipe.ruv(res, 2, controls=ctl, return_counts=True, corrected=True), "dsq_dev_project_out"),
            "ruv_r": (lambda: pipe.ruv(res, 2, method="r"), "dsq_dev_sample_gram"),
            "remove_batch_effect": (lambda: pipe.remove_batch_effect(x, batch=np.arange(N) // 4), "dsq_dev_project_out"),
            "vst_transform": (lambda: pipe.vst_transform(res.size_factors, *trend), "dsq_dev_vst"),
            "vst_transform_new": (lambda: pipe.vst_transform_new(self.counts[:5], logmeans, nz, *trend), "dsq_dev_vst"),
            "lfc_shrink": (lambda: lfc_shrink(pipe, res, 1), "dsq_dev_lfc_shrink2"),
        }


@pytest.fixture(scope="module")
def fitted():
    f = Fitted()
    yield f
    f.pipe.close()


CALLS = ["wald", "wald_multi", "lrt", "rlog", "ash", "ranksum", "pca", "sample_distances", "residuals", "ruv_g", "ruv_r",
         "remove_batch_effect", "vst_transform", "vst_transform_new", "lfc_shrink"]


def test_fixture_runs_every_gather(fitted):
    res = fitted.res
    assert not np.asarray(res.non_zero, bool)[ZERO].any() and np.asarray(res.non_zero, bool).sum() == G - len(ZERO)
    assert np.asarray(res.refitted, bool)[OUTLIER] and set(fitted.calls()) == set(CALLS)


@pytest.mark.parametrize("name", CALLS)
def test_call_leaves_no_allocation(fitted, name):
    """No post-hoc call keeps a cache on the device, so the first call already leaves the set as it found it; so does the
    second."""
    fn, _ = fitted.calls()[name]
    before = set(fitted.live)
    for _ in range(2):
        fn()
        assert fitted.live == before, f"{name}: {len(fitted.live - before)} allocation(s) left, {len(before - fitted.live)} gone"


@pytest.mark.parametrize("name", CALLS)
def test_failing_launch_leaves_no_allocation(fitted, name):
    """The launch is refused in Python, before anything reaches the device."""
    fn, entry = fitted.calls()[name]
    ctx, seen = fitted.ctx, []
    real = ctx.call

    def call(cname, *args):
        if cname == entry:
            seen.append(cname)
            raise RuntimeError(f"{cname} refused by the test")
        return real(cname, *args)

    before = set(fitted.live)
    ctx.call = call
    try:
        with pytest.raises(RuntimeError, match="refused by the test"):
            fn()
    finally:
        del ctx.call  # (the instance attribute: the class's method is back)
    assert seen == [entry]
    assert fitted.live == before, f"{name}: {len(fitted.live - before)} allocation(s) left, {len(before - fitted.live)} gone"


def test_borrowed_arrays_stay_the_callers(fitted):
    from pydeseq2_amd import ruv
    from pydeseq2_amd._lib import GENE_MAJOR, DeviceArray

    ctx, pipe, x = fitted.ctx, fitted.pipe, fitted.x
    before = set(fitted.live)
    d_sm, d_gm = DeviceArray.from_host(ctx, x), DeviceArray.from_host(ctx, np.ascontiguousarray(x.T))
    mine = before | {d_sm.ptr, d_gm.ptr}
    assert np.array_equal(pipe.pca(d_sm, ntop=50).scores, pipe.pca(x, ntop=50).scores)
    assert fitted.live == mine and np.array_equal(d_sm.to_host(), x)
    P = np.linalg.qr(np.random.default_rng(1).normal(size=(N, 2)))[0]
    want = ruv.project_out(pipe, d_gm, P, P, layout=GENE_MAJOR)
    assert fitted.live == mine and np.array_equal(d_gm.to_host(), x.T)
    assert ruv.project_out(pipe, d_gm, P, P, layout=GENE_MAJOR, inplace=True) is None
    assert fitted.live == mine and np.array_equal(d_gm.to_host().T, want)
    d_sm.free(); d_gm.free()
    assert fitted.live == before
