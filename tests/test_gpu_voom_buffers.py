"""Lifetime of the device buffers of the voom calls on the GPU, after the pattern of
tests/test_gpu_posthoc_buffers.py: the set of live allocations of the context after a call equals the set before it - on a
normal return, when the second launch is refused, and when the trend is refused on the host between the launches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, G = 12, 96
ZERO = np.array([3, 17, 40, 41, 77, 95])


class Fitted:
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
        self.pipe = pydeseq2_amd.DeseqPipeline(counts, self.X, ctx=ctx)
        self.res = self.pipe.deseq2(contrast=np.array([0.0, 1.0]))

    def calls(self):
        pipe, res = self.pipe, self.res
        K3 = np.array([[0.0, 1.0], [1.0, 0.0], [1.0, -1.0]])
        return {
            "voom": lambda: pipe.voom(res, K3),
            "voom_colsums": lambda: pipe.voom(res, [0.0, 1.0], lib_size="colsums"),
            "voom_layers": lambda: pipe.voom_layers(res.size_factors),
        }


@pytest.fixture(scope="module")
def fitted():
    f = Fitted()
    yield f
    f.pipe.close()


CALLS = ["voom", "voom_colsums", "voom_layers"]


@pytest.mark.parametrize("name", CALLS)
def test_call_leaves_no_allocation(fitted, name):
    fn = fitted.calls()[name]
    before = set(fitted.live)
    for _ in range(2):
        out = fn()
        assert fitted.live == before, f"{name}: {len(fitted.live - before)} allocation(s) left, {len(before - fitted.live)} gone"
    if name == "voom":
        assert out.pvalue.shape == (3, G) and np.isnan(out.pvalue[:, ZERO]).all()
        assert np.isfinite(np.delete(out.pvalue, ZERO, axis=1)).all()


@pytest.mark.parametrize("name", CALLS)
@pytest.mark.parametrize("entry", ["dsq_dev_voom_fit1", "dsq_dev_voom_wls"])
def test_failing_launch_leaves_no_allocation(fitted, name, entry):
    """The launch is refused in Python, before anything reaches the device."""
    fn = fitted.calls()[name]
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


def test_refused_trend_leaves_no_allocation(fitted, monkeypatch):
    """The host refuses between the two launches (a trend that is not positive): the first launch's buffers are released
    and the second launch never happens."""
    from pydeseq2_amd import voom

    ctx, seen = fitted.ctx, []
    real = ctx.call

    def call(cname, *args):
        seen.append(cname)
        return real(cname, *args)

    monkeypatch.setattr(voom, "lowess_delta", lambda x, y, **kw: voom.Lowess(y, np.array([0.0, 1.0]), np.array([1.0, -1.0])))
    before = set(fitted.live)
    ctx.call = call
    try:
        with pytest.raises(ValueError, match="positive finite"):
            fitted.pipe.voom(fitted.res, [0.0, 1.0])
    finally:
        del ctx.call
    assert "dsq_dev_voom_fit1" in seen and "dsq_dev_voom_wls" not in seen
    assert fitted.live == before
