"""The workgroup medians of csrc/dsq_k_stats.hip at every branch, on the device, against numpy's sort-based median of
exactly the values the kernel sees (tests/select_cases.py has the cases, the reference and the path model; the host
tests prove which branch each case takes).

* block_median_values<256> / <1024> through k_sf_row (dsq_dev_size_factors, dsq_dev_size_factors_new): int32 and int64
  counts, with and without a gene mask, G on both sides of 8192 and up to the full register file;
* block_median_each (11-bit digits) through k_row_median_c: 32 769 and 40 000 usable genes;
* the per-pass kernels of the multi-GPU protocol (8-bit digits) through median_select_protocol, gene shards on one GPU;
* block_median_values<1024> twice through k_prior_mad (dsq_dev_prior_mad).

Tolerances: values on the dyadic grid have an exact median, the only rounding is the device `exp`: rtol 1e-13 on the
size factor (the bound of test_size_factors_register_and_key_matrix_paths; a pick that is off by one order statistic
misses by >= 9e-10).  An infinite or NaN reference median must give exactly 0, inf or NaN.  rtol 1e-12 on the squared
MAD (the bound of test_prior_mad_kernel_vs_numpy).  Every test prints its worst error in units of its tolerance."""
import ctypes as C

import numpy as np
import pytest

from tests import select_cases as sc

pytestmark = pytest.mark.gpu

RTOL_SF = 1e-13
RTOL_MAD = 1e-12
SENTINEL = 12345.0  # what d_size_factors holds before a launch: every sample must be written, exactly once
_vp = C.c_void_p

VALUE_CASES = sc.value_cases()
BIG = {c.name: c for c in sc.value_cases() + sc.big_value_cases()}
RADIX_CASES = sc.radix_cases()
ENTRY = {"default": "dsq_dev_size_factors", "new": "dsq_dev_size_factors_new"}
COUNT_TYPE = {"int32": 0, "int64": 1}


@pytest.fixture(scope="module")
def ctx():
    from pydeseq2_amd._lib import Context

    return Context(0)


class SfLaunch:
    """the device buffers of one (counts, logmeans, mask): both entry points, as often as asked"""

    def __init__(self, ctx, counts, lm, mask, dtype):
        from pydeseq2_amd._lib import DeviceArray

        self.ctx, (self.N, self.G), self.ct = ctx, counts.shape, COUNT_TYPE[dtype]
        assert counts.max() < 2 ** 31 or dtype == "int64"
        self.d_c = DeviceArray.from_host(ctx, counts.astype(dtype))
        self.d_lm = DeviceArray.from_host(ctx, lm)
        self.d_mask = DeviceArray.from_host(ctx, mask) if mask is not None else None
        self.d_work = DeviceArray(ctx, (ctx.lib.dsq_size_factors_work_doubles(self.N, self.G),), np.float64)
        self.d_sf = DeviceArray(ctx, (self.N,), np.float64)

    def run(self, mode):
        ctx = self.ctx
        # (keys left over from another launch would give the radix kernels something to select from: all ones = no key)
        ctx.memset(self.d_work.ptr, 0xff, self.d_work.nbytes)
        ctx.h2d(self.d_sf.ptr, np.full(self.N, SENTINEL))
        ctx.call(ENTRY[mode], _vp(self.d_c.ptr), self.ct, self.N, self.G, _vp(self.d_lm.ptr),
                 _vp(self.d_mask.ptr) if self.d_mask is not None else None, _vp(self.d_work.ptr), _vp(self.d_sf.ptr))
        return self.d_sf.to_host()


def sf_error(sf, ref_median, label):
    """worst |sf - exp(median)| in units of RTOL_SF * exp(median); infinite / NaN medians must be hit exactly"""
    with np.errstate(over="ignore"):
        want = np.exp(ref_median)
    worst = 0.0
    for n in range(sf.size):
        if np.isfinite(ref_median[n]):
            assert np.isfinite(sf[n]), (label, n, sf[n], want[n])
            worst = max(worst, abs(sf[n] - want[n]) / (RTOL_SF * want[n]))
        else:
            assert sc.same_bits(sf[n], want[n]), (label, n, sf[n], want[n])
    assert worst <= 1.0, (label, worst, sf, want)
    return worst


def run_case(ctx, case, Gs, masks=(False, True)):
    """every dtype x mask x entry point at every G of `Gs`, each launched twice (the compaction order of k_sf_compact
    differs between launches, the size factors must not); returns the worst error in units of the tolerance"""
    worst = 0.0
    for G in Gs:
        for with_mask in masks:
            if case.mask_only and not with_mask:
                continue
            counts, lm, mask = sc.layout(case, G, with_mask)
            for dtype in case.dtypes:
                launch = SfLaunch(ctx, counts, lm, mask, dtype)
                for mode in ("default", "new"):
                    label = (case.name, G, with_mask, dtype, mode)
                    sf = launch.run(mode)
                    again = launch.run(mode)
                    assert np.array_equal(sf.view(np.int64), again.view(np.int64)), (label, sf, again)
                    worst = max(worst, sf_error(sf, case.reference(mode), label))
    return worst


@pytest.mark.parametrize("case", VALUE_CASES, ids=lambda c: c.name)
def test_size_factors_at_every_branch(ctx, case):
    """k_sf_row<*, 256, 32> (G <= 8192) and k_sf_row<*, 1024, 32> (G = 8193) on every named case"""
    g_small = min(8192, case.Gu + 331)
    worst = run_case(ctx, case, (g_small, 8193))
    print(f"\n{case.name}: worst |sf - exp(median)| = {worst:.4f} x rtol {RTOL_SF}")


@pytest.mark.parametrize("name,G", [("full-32768", 32768), ("full-32768", 40000), ("descend2", 32768),
                                     ("descend-collapse", 40000), ("deep-two-ties", 40000), ("low-even", 40000),
                                     ("low-odd", 40000), ("no-usable-gene", 40000), ("empty-sample", 40000)])
def test_size_factors_full_register_file_and_wide_matrices(ctx, name, G):
    """k_sf_row<*, 1024, 32> with every register slot used (32 768 usable genes), and with G = 40 000 genes of which at
    most 32 768 are usable: k_sf_row takes them, the two radix kernels (launched, the number of usable genes is known on
    the device only) must leave without touching the size factors - their key matrix holds no key here."""
    worst = run_case(ctx, BIG[name], (G,))
    print(f"\n{name} at G = {G}: worst |sf - exp(median)| = {worst:.4f} x rtol {RTOL_SF}")


@pytest.mark.parametrize("case", RADIX_CASES, ids=lambda c: c.name)
def test_radix_select_above_the_register_file(ctx, case):
    """k_ratio_keys_c + k_row_median_c (block_median_each, 6 passes of 11/11/11/11/11/9 bits): 32 769 and 40 000 usable
    genes among G = 40 000"""
    worst = run_case(ctx, case, (40000,))
    print(f"\n{case.name}: worst |sf - exp(median)| = {worst:.4f} x rtol {RTOL_SF}")


# ------------------------------------------------------------------------------------------------ protocol
class ShardOps:
    """the local passes of median_select_protocol for one gene shard: the six dsq_dev_sf_* entry points"""

    def __init__(self, ctx, counts, lm, mask, dtype):
        from pydeseq2_amd._lib import DeviceArray

        self.ctx, (self.N, G) = ctx, counts.shape
        N = self.N
        d_c = DeviceArray.from_host(ctx, counts.astype(dtype))
        d_lm = DeviceArray.from_host(ctx, lm)
        d_mask = DeviceArray.from_host(ctx, mask) if mask is not None else None
        d_idx = DeviceArray(ctx, (G + 2,), np.int32)
        self.d_keys = DeviceArray(ctx, (N * G,), np.uint64)
        gu = C.c_int(-1)
        ctx.call("dsq_dev_sf_keys_compact", _vp(d_c.ptr), COUNT_TYPE[dtype], N, G, _vp(d_lm.ptr),
                 _vp(d_mask.ptr) if d_mask is not None else None, _vp(d_idx.ptr), _vp(self.d_keys.ptr), C.byref(gu))
        self.Gu = int(gu.value)
        self.d_cnt = DeviceArray(ctx, (N,), np.uint32)
        self.d_prefix = DeviceArray(ctx, (2 * N,), np.uint64)
        self.d_rank = DeviceArray(ctx, (2 * N,), np.uint32)
        self.d_hist = DeviceArray(ctx, (2 * N * 256,), np.uint32)
        self.d_sf = DeviceArray(ctx, (N,), np.float64)

    def count(self):
        self.ctx.call("dsq_dev_sf_count", _vp(self.d_keys.ptr), self.N, self.Gu, _vp(self.d_cnt.ptr))
        return self.d_cnt

    def init(self, total):
        self.ctx.call("dsq_dev_sf_init", _vp(total.ptr), self.N, _vp(self.d_prefix.ptr), _vp(self.d_rank.ptr))

    def hist(self, shift):
        self.ctx.call("dsq_dev_sf_hist", _vp(self.d_keys.ptr), self.N, self.Gu, _vp(self.d_prefix.ptr), int(shift),
                      _vp(self.d_hist.ptr))
        return self.d_hist

    def pick(self, hist, shift):
        self.ctx.call("dsq_dev_sf_pick", _vp(hist.ptr), self.N, int(shift), _vp(self.d_prefix.ptr), _vp(self.d_rank.ptr))

    def finish(self, total):
        self.ctx.h2d(self.d_sf.ptr, np.full(self.N, SENTINEL))
        self.ctx.call("dsq_dev_sf_finish", _vp(self.d_prefix.ptr), _vp(total.ptr), self.N, _vp(self.d_sf.ptr))
        return self.d_sf.to_host()


class AllShards:
    """the ranks of one protocol run in lock step: every pass on every shard, then the exchange"""

    def __init__(self, shards):
        self.shards = shards

    def count(self):
        return [s.count() for s in self.shards]

    def init(self, totals):
        [s.init(t) for s, t in zip(self.shards, totals)]

    def hist(self, shift):
        return [s.hist(shift) for s in self.shards]

    def pick(self, hists, shift):
        [s.pick(h, shift) for s, h in zip(self.shards, hists)]

    def finish(self, totals):
        return [s.finish(t) for s, t in zip(self.shards, totals)]


def host_allreduce_sum(ctx):
    def allreduce_sum(darrs):
        total = np.sum([d.to_host().astype(np.uint64) for d in darrs], axis=0)
        assert total.max() < 2 ** 32
        for d in darrs:
            ctx.h2d(d.ptr, total.astype(d.dtype))
        return darrs

    return allreduce_sum


PROTOCOL_CASES = [c for c in RADIX_CASES if c.mode == "default"] + [BIG["deep-two-ties"], BIG["hist-two"],
                                                                    BIG["empty-sample"]]


@pytest.mark.parametrize("n_shards", [2, 3])
@pytest.mark.parametrize("case", PROTOCOL_CASES, ids=lambda c: c.name)
def test_protocol_on_gene_shards_is_the_single_gpu_result(ctx, case, n_shards):
    """k_sf_count / init / hist / pick / finish under median_select_protocol: the genes in 2 and in 3 shards of unequal
    size - with 3, the middle one has no usable gene - give the bits of dsq_dev_size_factors on the unsplit matrix
    (k_row_median_c above 32 768 usable genes, k_sf_row below) and numpy's median of the union."""
    from pydeseq2_amd.distributed import median_select_protocol

    worst = 0.0
    for with_mask, dtype in ((False, "int32"), (True, "int64")):
        counts, lm, mask = sc.layout(case, case.Gu + 700, with_mask, seed=n_shards)
        G = lm.size
        if n_shards == 3:
            # the genes in the order: usable and unusable mixed | 700 unusable | mixed
            use = np.isfinite(lm) & (mask != 0 if mask is not None else True)
            dead = np.nonzero(~use)[0][:700]
            rest = np.setdiff1d(np.arange(G), dead)
            cut = int(0.23 * rest.size)
            order = np.concatenate([rest[:cut], dead, rest[cut:]])
            counts, lm = np.ascontiguousarray(counts[:, order]), lm[order]
            mask = mask[order] if mask is not None else None
            cuts = [0, cut, cut + 700, G]
        else:
            cuts = [0, int(0.37 * G), G]
        shards = [ShardOps(ctx, np.ascontiguousarray(counts[:, a:b]), lm[a:b], mask[a:b] if mask is not None else None,
                           dtype) for a, b in zip(cuts[:-1], cuts[1:])]
        assert sum(s.Gu for s in shards) == case.Gu
        if n_shards == 3:
            assert shards[1].Gu == 0
        sfs = median_select_protocol(AllShards(shards), host_allreduce_sum(ctx))
        single = SfLaunch(ctx, counts, lm, mask, dtype).run("default")
        for sf in sfs:
            assert np.array_equal(sf.view(np.int64), single.view(np.int64)), (case.name, with_mask, sf, single)
        worst = max(worst, sf_error(sfs[0], case.reference("default"), (case.name, n_shards, with_mask)))
    print(f"\n{case.name} in {n_shards} shards: worst |sf - exp(median)| = {worst:.4f} x rtol {RTOL_SF}")


# ------------------------------------------------------------------------------------------------ prior MAD
def prior_mad(ctx, case):
    from pydeseq2_amd._lib import DeviceArray

    d_gw, d_fit = DeviceArray.from_host(ctx, case.gw), DeviceArray.from_host(ctx, case.fit)
    d_work = DeviceArray(ctx, (ctx.lib.dsq_prior_mad_work_doubles(case.n),), np.float64)
    out = []
    for _ in range(2):
        ctx.memset(d_work.ptr, 0, d_work.nbytes)
        sq = C.c_double(SENTINEL)
        ctx.call("dsq_dev_prior_mad", _vp(d_gw.ptr), _vp(d_fit.ptr), case.n, C.c_double(case.MIN_DISP),
                 C.c_double(case.MAX_DISP), _vp(d_work.ptr), C.byref(sq))
        out.append(sq.value)
    assert sc.same_bits(out[0], out[1]), out
    return out[0]


def check_prior(ctx, case):
    got, want = prior_mad(ctx, case), case.reference()
    if np.isnan(want):
        assert np.isnan(got), (case.name, got)
        print(f"\n{case.name}: NaN, as the reference")
        return
    err = abs(got - want)
    assert err <= RTOL_MAD * want, (case.name, got, want)
    ratio = err / (RTOL_MAD * want) if want > 0 else 0.0
    print(f"\n{case.name}: |MAD^2 - ref| = {ratio:.4f} x rtol {RTOL_MAD} (paths {case.paths()})")


@pytest.mark.parametrize("n", sc.PRIOR_SIZES)
def test_prior_mad_around_the_eight_loads_walk(ctx, n):
    """k_prior_mad reads eight residuals per trip while i + 7 * 1024 < n, then one: sizes on both sides of 1024 (one
    value per thread), of 8192 (the first full trip) and of 16384"""
    check_prior(ctx, sc.prior_size_case(n))


@pytest.mark.parametrize("case", sc.prior_cases(), ids=lambda c: c.name)
def test_prior_mad_at_every_branch(ctx, case):
    """both medians of k_prior_mad (block_median_values<1024>) on the crafted residuals: exact ties from equal `fitted`"""
    check_prior(ctx, case)
