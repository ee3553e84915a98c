"""DeviceScope (pydeseq2_amd/_lib.py) on a fake context that records malloc / free / sync / copies / launches
and raises where it is told to: the order and the completeness of the release, which exception wins, adopted and borrowed
arrays - and three post-hoc calls whose launch fails must leave nothing but the caller's own array alive.  No GPU."""
import numpy as np
import pytest

from pydeseq2_amd import ash as _ash
from pydeseq2_amd import pca, ruv
from pydeseq2_amd._lib import GENE_MAJOR, DeviceArray, DeviceScope, gather_rows_i32, launch, split


class _Lib:
    @staticmethod
    def dsq_sample_gram_work_doubles(N, K):
        return 64


class FakeContext:
    """malloc / free keep the set of live pointers; ``log`` is the order of everything; ``fail_sync`` / ``fail_free`` (a set
    of pointers) / ``fail_call`` (an entry point's name, or True for every launch) / ``fail_h2d`` make the call raise."""

    lib = _Lib()

    def __init__(self):
        self.live, self.log, self._next = set(), [], 0x1000
        self.fail_sync, self.fail_free, self.fail_call, self.fail_h2d = False, set(), None, False

    def malloc(self, nbytes):
        p, self._next = self._next, self._next + int(nbytes) + 256
        self.live.add(p)
        self.log.append(("malloc", p))
        return p

    def free(self, p):
        self.log.append(("free", p))
        if p in self.fail_free:
            raise OSError(f"free of {p:#x} failed")
        self.live.remove(p)  # (KeyError: freed twice, or never allocated)

    def sync(self):
        self.log.append(("sync",))
        if self.fail_sync:
            raise OSError("sync failed")

    def h2d(self, p, arr):
        self.log.append(("h2d", p))
        if self.fail_h2d:
            raise OSError("h2d failed")

    def h2d_rows(self, p, arr, ld):
        self.h2d(p, arr)

    def d2h(self, arr, p):
        self.log.append(("d2h", p))
        arr[...] = 0
        return arr

    def d2h_rows(self, p, rows, cols, ld, dtype=np.float64):
        self.log.append(("d2h", p))
        return np.zeros((rows, cols), dtype)

    def call(self, name, *args):
        self.log.append(("call", name))
        if self.fail_call is True or self.fail_call == name:
            raise RuntimeError(f"{name} refused")

    def frees(self):
        return [e[1] for e in self.log if e[0] == "free"]


def _three(ctx, s):
    a = s.upload(np.arange(6.0))
    b = s.empty((4, 3), np.float64, ld=8)
    c = s.upload(np.ones((2, 3)), dtype=np.float32, ld=4)  # (pitched: goes through h2d_rows)
    assert (a.dtype, b.nbytes, c.dtype, c.ld) == (np.float64, 4 * 8 * 8, np.float32, 4)
    return [a.ptr, b.ptr, c.ptr]


def test_normal_exit_syncs_once_then_frees_in_reverse_order():
    ctx = FakeContext()
    with DeviceScope(ctx) as s:
        ptrs = _three(ctx, s)
        assert ctx.live == set(ptrs) and ("sync",) not in ctx.log
    assert ctx.live == set() and ctx.frees() == ptrs[::-1]
    assert ctx.log.count(("sync",)) == 1 and ctx.log.index(("sync",)) < ctx.log.index(("free", ptrs[-1]))


def test_body_exception_frees_everything_once_and_propagates():
    ctx = FakeContext()
    with pytest.raises(ZeroDivisionError):
        with DeviceScope(ctx) as s:
            ptrs = _three(ctx, s)
            1 / 0
    assert ctx.live == set() and ctx.frees() == ptrs[::-1] and ctx.log.count(("sync",)) == 1


def test_body_exception_wins_over_sync_and_free():
    ctx = FakeContext()
    ctx.fail_sync = True
    with pytest.raises(ZeroDivisionError):
        with DeviceScope(ctx) as s:
            ptrs = _three(ctx, s)
            ctx.fail_free = {ptrs[1]}
            1 / 0
    assert ctx.frees() == ptrs[::-1] and ctx.live == {ptrs[1]}  # (a failing sync or free stops none of the others)


def test_failing_free_does_not_stop_the_others_and_surfaces():
    ctx = FakeContext()
    with pytest.raises(OSError, match="free of") as e:
        with DeviceScope(ctx) as s:
            ptrs = _three(ctx, s)
            ctx.fail_free = {ptrs[2], ptrs[0]}
    assert f"{ptrs[2]:#x}" in str(e.value)  # the first error, in the order of the release
    assert ctx.frees() == ptrs[::-1] and ctx.live == {ptrs[0], ptrs[2]}
    ctx.fail_free = set()  # (the arrays' own __del__ may try again)


def test_failing_sync_surfaces_after_the_frees():
    ctx = FakeContext()
    ctx.fail_sync = True
    with pytest.raises(OSError, match="sync failed"):
        with DeviceScope(ctx) as s:
            _three(ctx, s)
    assert ctx.live == set()


def test_failed_upload_leaves_no_allocation():
    ctx = FakeContext()
    ctx.fail_h2d = True
    with pytest.raises(OSError, match="h2d failed"):
        with DeviceScope(ctx) as s:
            s.empty(5, np.int32)
            s.upload(np.arange(3))
    assert ctx.live == set()


def test_adopted_is_freed_and_borrowed_is_untouched():
    ctx = FakeContext()
    mine, made_elsewhere = DeviceArray.from_host(ctx, np.arange(4.0)), DeviceArray(ctx, (3,), np.int32)
    with DeviceScope(ctx) as s:
        assert s.adopt(made_elsewhere) is made_elsewhere
        own = s.upload(np.arange(2))
        assert mine.ptr and own.ptr
    assert ctx.live == {mine.ptr} and made_elsewhere.ptr == 0 and own.ptr == 0
    assert ("free", mine.ptr) not in ctx.log
    mine.free()
    assert ctx.live == set()


def test_second_exit_is_a_no_op():
    ctx = FakeContext()
    s = DeviceScope(ctx)
    with s:
        _three(ctx, s)
    n = len(ctx.log)
    s.__exit__(None, None, None)
    with s:
        pass
    assert len(ctx.log) == n and ctx.live == set()


def test_split_launch_and_gather():
    ctx = FakeContext()

    class Pipe:
        def __init__(self):
            self.ctx, self.seen = ctx, []

        def _k(self, name, genes, cname, *args):
            self.seen.append((name, genes, cname, args))

    pipe = Pipe()
    assert split(pipe) == (pipe, ctx) and split(ctx) == (None, ctx) and split(None) == (None, None)
    launch(pipe, "stage", 7, "dsq_dev_x", 1, 2)
    launch(ctx, "stage", 7, "dsq_dev_x", 1, 2)
    assert pipe.seen == [("stage", 7, "dsq_dev_x", (1, 2))] and ctx.log == [("call", "dsq_dev_x")]
    with DeviceScope(ctx) as s:
        d = gather_rows_i32(s, ctx, 0x10, 16, np.array([4, 0, 9]), 12)
        assert (d.shape, d.ld, d.dtype) == ((3, 12), 16, np.int32) and len(ctx.live) == 2
        assert ctx.log[-1] == ("call", "dsq_dev_gather_rows_i32")
    assert ctx.live == set()


# ---------------------------------------------------------------------------------------------------- post-hoc calls
RNG = np.random.default_rng(5)
X = RNG.normal(size=(6, 40))
PB = np.linalg.qr(RNG.normal(size=(6, 2)))[0]


def _run(ctx, fn, fail_call):
    ctx.fail_call = fail_call
    if fail_call is None:
        fn()
    else:
        with pytest.raises(RuntimeError, match="refused"):
            fn()
        assert ctx.log[-1][0] in ("sync", "free")  # (nothing ran after the launch that failed but the release)


@pytest.mark.parametrize("fail_call", [True, "dsq_dev_sample_gram", "dsq_dev_gram_dist", None])
@pytest.mark.parametrize("resident", [False, True])
def test_sample_distances_releases_everything(fail_call, resident):
    ctx = FakeContext()
    x = DeviceArray.from_host(ctx, X) if resident else X
    _run(ctx, lambda: pca.sample_distances(ctx, x, genes=[3, 1, 7]), fail_call)
    assert ctx.live == ({x.ptr} if resident else set())
    assert ("call", "dsq_dev_row_meanvar") in ctx.log and len(ctx.frees()) == len(set(ctx.frees()))


@pytest.mark.parametrize("fail_call", [True, "dsq_dev_project_out", None])
def test_project_out_releases_everything(fail_call):
    ctx = FakeContext()
    _run(ctx, lambda: ruv.project_out(ctx, X, PB, PB, return_coef=True), fail_call)  # (uploaded, transposed on the device)
    assert ctx.live == set() and ("call", "dsq_dev_f64_to_gene_major") in ctx.log
    d = DeviceArray.from_host(ctx, np.ascontiguousarray(X.T))
    _run(ctx, lambda: ruv.project_out(ctx, d, PB, PB, layout=GENE_MAJOR, return_coef=True, inplace=True), fail_call)
    assert ctx.live == {d.ptr} and ("free", d.ptr) not in ctx.log
    _run(ctx, lambda: ruv.project_out(ctx, d, PB, PB, layout=GENE_MAJOR), fail_call)
    assert ctx.live == {d.ptr} and ("free", d.ptr) not in ctx.log


@pytest.mark.parametrize("fail_call", [True, None])
def test_ash_releases_everything(fail_call):
    ctx = FakeContext()
    _run(ctx, lambda: _ash.ash(ctx, RNG.normal(size=(2, 30)), np.full((2, 30), 0.5)), fail_call)
    assert ctx.live == set() and ("call", "dsq_dev_ash") in ctx.log
    assert [e[0] for e in ctx.log].count("malloc") == 2 == len(ctx.frees())
