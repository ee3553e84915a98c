"""The product kernels of the trimmed statistics through the C ABI - dsq_dev_robust_disp / dsq_dev_robust_disp2,
dsq_dev_cooks, dsq_dev_replace_outliers - at the decision edges of their launchers (csrc/dsq_k_stats.hip), against the
oracle's sort-based restatements (robust_mom_disp, trimmed_mean) and the Python model of the Cook's bookkeeping.

Every count row is pitched (ldn > N) and its padding holds large garbage counts, so a read past N shows.  No gene is left
out of a comparison; NaN results are part of what is expected.

The tests not marked `gpu` check the inputs: at least three quarters of a case's genes have a reference robust dispersion
above the 0.04 floor, and in a design with several cells every cell holds the largest trimmed variance of at least one
gene - so an error in any cell's variance reaches an output.

Run as a module (python -m tests.test_gpu_trimmed_stats CASE OUT.npz) it computes one case's device outputs: what the
tests do in a fresh child process for the switches that the library reads once (DSQ_NO_SEG_CELLS, DSQ_REPLACE_LEAN)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import nbglm_oracle as orc
from tests import stats_cases as sc
from tests.helpers import assert_close

gpu = pytest.mark.gpu
_vp = C.c_void_p
GARBAGE = 1_000_000_007  # the padding of every count row
CUTOFF = 3.0        # outlier replacement
COOKS_CUTOFF = 0.05  # dsq_dev_cooks: a cutoff that a few samples of most genes pass


@pytest.fixture(scope="module")
def ctx():
    from pydeseq2_amd._lib import Context

    return Context(0)


# ------------------------------------------------------------------------------------------------ inputs
# BucketWork (dsq_stats.h) = 512 * 8 + 512 * 4 + 2 * 128 * 8 + 16 bytes = 8208 bytes = 1026 doubles.  A buffered wavefront
# holds cap + 1026 doubles with cap = (largest cell + 15) & ~15 from 129 samples on (trim_cap), next_pow2 below.
ROBUST_CASES = {
    # largest cell 64: next_pow2(64) = 64 <= kSegMaxCell -> batched segments; 65 -> one cell at a time (sorted)
    "seg64": dict(sizes=[64, 40, 17, 3], G=41),
    "one65": dict(sizes=[65, 40, 17, 3], G=41),
    # largest cell 128 < kTrimBucketMin = 129: every cell sorted, BIG = false, no BucketWork; 129: that cell takes the
    # bucket path, BIG = true, the cells of 100, 25 and 3 are sorted in the same wavefront's LDS in front of the BucketWork
    "sort128": dict(sizes=[128, 100, 25, 3], G=41),
    "bucket129": dict(sizes=[129, 100, 25, 3], G=41),
    # one pseudo-cell of all N samples (continuous covariate).  N = 1008: cap 1008, (1008 + 1026) * 8 = 16272 B, four of
    # them 65088 <= 65536 -> 4 waves per block; N = 1009: cap 1024, 16400 B, 65600 > 65536 -> 2 waves per block
    "wpb4_1008": dict(whole=1008, G=6),
    "wpb2_1009": dict(whole=1009, G=6),
    # N = 9200: cap 9200, (9200 + 1026) * 8 = 81808 B, two of them 163616 <= 163840 -> 2 waves; N = 9201: cap 9216,
    # 81936 B, 163872 > 163840 -> 1 wave per block.  (From 2048 samples on the buffer-less kernel takes such a design:
    # the tests run these two with it and, DSQ_NO_ROBUST_LEAN set, with the buffered kernel.)
    "wpb2_9200": dict(whole=9200, G=6),
    "wpb1_9201": dict(whole=9201, G=6),
    # buffer-less kernel: every cell >= 129 samples and the largest >= 2048
    "lean_129_2048": dict(sizes=[129, 2048], G=41),
    "buffered_128_2048": dict(sizes=[128, 2048], G=41),
    "buffered_129_2047": dict(sizes=[129, 2047], G=41),
    # (19600 + 1026) * 8 = 165008 B > 160 KB: no buffered kernel can hold the cell
    "huge_19600": dict(whole=19600, G=5),
}
LEAN = ("wpb2_9200", "wpb1_9201", "lean_129_2048", "huge_19600")        # the buffer-less kernel takes these ...
LEAN_AND_BUFFERED = ("wpb2_9200", "wpb1_9201", "lean_129_2048")        # ... and the buffered one can


def design(spec, rng):
    """(X, cell of every sample or None): cells of the given sizes in shuffled sample order, or no cell at all"""
    if "whole" in spec:
        N = spec["whole"]
        return np.column_stack([np.ones(N), rng.normal(0, 1, N)]), None
    lv = np.repeat(np.arange(len(spec["sizes"])), spec["sizes"])
    rng.shuffle(lv)
    return np.column_stack([np.ones(len(lv))] + [(lv == k).astype(float) for k in range(1, len(spec["sizes"]))]), lv


def gene_content(rng, N, G, sf, lv):
    """samples x genes.  With G >= 20 the first eight genes are those of the host test
    test_robust_dispersion_large_cells_bucket_path (constant, two values, all zero but one, one huge outlier, a zero block
    that ends at either trimming boundary, more than 128 ties in a boundary bucket); a short case keeps the zero-block
    gene.  The others are negative binomial over a wide range of means, each with one cell - gene g: cell g mod n_cells -
    spread out threefold, so that every cell is some gene's largest variance."""
    mean = np.exp(rng.uniform(np.log(2.0), np.log(3000), G))
    counts = rng.negative_binomial(5.0, 5.0 / (5.0 + mean[None, :] * sf[:, None])).astype(np.int64)
    if lv is not None:
        nc = int(lv.max()) + 1
        for g in range(G):
            rows = np.nonzero(lv == g % nc)[0]
            counts[rows, g] = (counts[rows, g] + 1) * 8 ** (np.arange(len(rows)) % 3)
    if G >= 20:
        counts[:, 0] = 7
        counts[:, 1] = np.where(rng.random(N) < 0.5, 3, 11)
        counts[:, 2] = 0; counts[5, 2] = 1
        counts[:, 3] = rng.poisson(100, N); counts[17, 3] = 2_000_000
        counts[:, 4] = np.where(rng.random(N) < 0.9, 0, rng.poisson(5, N))
        counts[:, 5] = np.where(rng.random(N) < 0.12, 0, rng.poisson(50, N))
        counts[:, 6] = np.where(rng.random(N) < 0.125, 0, 1 + rng.poisson(2, N))
        counts[:, 7] = 100000 + rng.poisson(2, N); counts[33, 7] = 2_000_000_000
    else:
        counts[:, 0] = np.where(rng.random(N) < 0.125, 0, 1 + rng.poisson(2, N))
    return counts


_cases = {}


def robust_case(name):
    if name not in _cases:
        spec = ROBUST_CASES[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        X, lv = design(spec, rng)
        N = X.shape[0]
        sf = np.exp(rng.normal(0, 0.3, N))
        sf[: N // 2] = 1.0  # equal size factors: exact ties among the normalised counts
        counts = gene_content(rng, N, spec["G"], sf, lv)
        _cases[name] = dict(counts=counts, sf=sf, X=X, lv=lv, ref=orc.robust_mom_disp(counts / sf[:, None], X))
    return _cases[name]


def cell_variances(normed, lv):
    """[cells][genes]: the scaled trimmed variances whose maximum robust_mom_disp takes (utils.py:602-650)"""
    ratios, scales = (1 / 3, 1 / 4, 1 / 8), (2.04, 1.86, 1.51)
    out = []
    for c in range(int(lv.max()) + 1):
        x = normed[lv == c]
        k = 2 if len(x) >= 24 else (1 if len(x) >= 4 else 0)
        d = x - orc.trimmed_mean(x, ratios[k], axis=0)[None, :]
        out.append(scales[k] * orc.trimmed_mean(d ** 2, ratios[k], axis=0))
    return np.array(out)


@pytest.mark.parametrize("name", list(ROBUST_CASES) + ["cooks:small", "cooks:bucket"])
def test_inputs_reach_the_outputs(name):
    k = cooks_case(name.split(":")[1]) if name.startswith("cooks:") else robust_case(name)
    G = k["counts"].shape[1]
    assert 5 <= G <= 70 and G % 4 != 0
    assert (k["ref"] > 0.04).sum() >= 0.75 * G
    if k["lv"] is not None:
        v = cell_variances(k["counts"] / k["sf"][:, None], k["lv"])
        assert set(np.argmax(v, axis=0).tolist()) == set(range(v.shape[0]))


# ------------------------------------------------------------------------------------------------ device calls
def pitched_counts(counts, extra=16):
    """genes x ldn int32 with ldn > N, the padding full of garbage"""
    from pydeseq2_amd._design import pad16

    N, G = counts.shape
    ldn = pad16(N) + extra
    y = np.full((G, ldn), GARBAGE, np.int32)
    y[:, :N] = counts.T
    return y, ldn


def dev_robust_disp(ctx, counts, sf, X, api="dsq_dev_robust_disp2"):
    from pydeseq2_amd._design import DesignPack
    from pydeseq2_amd._lib import DeviceArray

    D = DesignPack(X)
    N, G = counts.shape
    y, ldn = pitched_counts(counts)
    sfp = np.full(ldn, np.nan)
    sfp[:N] = sf
    d = [DeviceArray.from_host(ctx, a) for a in (y, sfp, D.cell_offsets, D.cell_index)]
    d_o = DeviceArray.from_host(ctx, np.full(G + 3, -7.0))
    args = [_vp(d[0].ptr), ldn, _vp(d[1].ptr), _vp(d[2].ptr), _vp(d[3].ptr), D.n_cells, int(D.whole), D.max_cell]
    if api == "dsq_dev_robust_disp2":
        args.append(D.min_cell)
    ctx.call(api, *args, N, G, _vp(d_o.ptr))
    ctx.sync()
    out = d_o.to_host()
    for a in d + [d_o]:
        a.free()
    assert (out[G:] == -7.0).all()
    return out[:G]


def check_robust(got, k, what):
    # 1e-10 relative: the bound tests/test_hostsim.py holds the host instantiation to.  The bucket paths' y * frcp_g(sf)
    # moves a normalised count by <= 4 u = 4.4e-16 relative (stats_cases.accessor_tolerance), a trimmed variance of values
    # whose spread is at least a fifth of their size (dispersion >= 0.04) by <= 2 * 5 * 4 u = 4.4e-15, and (v - m) / m^2
    # above the 0.04 floor amplifies that by v / (v - m) <= 1 + 1 / (0.04 m) <= 14 at the smallest mean used (2): six
    # orders inside the bound.
    assert_close(got, k["ref"], 1e-10, 0.0, what)


@gpu
@pytest.mark.parametrize("name", [n for n in ROBUST_CASES if n not in LEAN])
def test_robust_dispersion_at_the_buffered_launchers_edges(ctx, name):
    k = robust_case(name)
    check_robust(dev_robust_disp(ctx, k["counts"], k["sf"], k["X"]), k, name)
    check_robust(dev_robust_disp(ctx, k["counts"], k["sf"], k["X"], "dsq_dev_robust_disp"), k, name + " (robust_disp)")


@gpu
@pytest.mark.parametrize("name", LEAN)
def test_robust_dispersion_buffer_less_and_buffered_both_match_the_reference(ctx, name, monkeypatch):
    k = robust_case(name)
    check_robust(dev_robust_disp(ctx, k["counts"], k["sf"], k["X"]), k, name + " buffer-less")
    if name in LEAN_AND_BUFFERED:
        monkeypatch.setenv("DSQ_NO_ROBUST_LEAN", "1")  # (read on every launch)
        check_robust(dev_robust_disp(ctx, k["counts"], k["sf"], k["X"]), k, name + " buffered")


def handback_case(bad):
    """the buffer-less shape with one sample of each cell under a size factor of 0 or NaN; half of the genes have a zero
    count at those two samples (0 / 0, 0 / NaN), the others a positive one (inf, NaN)"""
    k = robust_case("lean_129_2048")
    counts, sf = k["counts"].copy(), k["sf"].copy()
    s = [int(np.nonzero(k["lv"] == c)[0][3]) for c in (0, 1)]
    sf[s] = bad
    counts[s, :] = 40
    counts[np.ix_(s, np.arange(0, counts.shape[1], 2))] = 0
    with np.errstate(all="ignore"):
        ref = orc.robust_mom_disp(counts / sf[:, None], k["X"])
    return dict(counts=counts, sf=sf, X=k["X"], ref=ref)


@pytest.mark.parametrize("bad", [0.0, np.nan])
def test_a_bad_size_factor_makes_every_reference_value_nan(bad):
    """Why the hand-back cases cannot carry the three-quarters condition: the reference divides by the mean of ALL
    normalised counts (utils.py:954), which is inf or NaN for every gene as soon as one size factor is 0 or NaN -
    np.maximum keeps the NaN.  What these cases can show, and did before the fixes, is a finite value or the 0.04 floor
    where the reference has NaN."""
    assert np.isnan(handback_case(bad)["ref"]).all()


@gpu
@pytest.mark.parametrize("bad", [0.0, np.nan])
def test_genes_the_buffer_less_kernel_hands_back(ctx, bad, monkeypatch):
    """One sample of each cell has the size factor 0 or NaN: every gene meets a normalised count that is not finite -
    inf or NaN under a positive count, NaN under a zero count - is handed back by the buffer-less kernel and redone by
    the buffered one, which orders them as numpy.sort does.  The unmodified oracle is the reference, NaN pattern
    included; the buffered kernel alone must say the same."""
    k = handback_case(bad)
    assert_close(dev_robust_disp(ctx, k["counts"], k["sf"], k["X"]), k["ref"], 1e-10, 0.0, "handed back and redone")
    monkeypatch.setenv("DSQ_NO_ROBUST_LEAN", "1")
    assert_close(dev_robust_disp(ctx, k["counts"], k["sf"], k["X"]), k["ref"], 1e-10, 0.0, "buffered kernel alone")


def _child(case, env):
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"trimmed_stats_{os.getpid()}_{case}.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        subprocess.run([sys.executable, "-m", "tests.test_gpu_trimmed_stats", case, out], check=True, cwd=root,
                       env={**os.environ, **env}, timeout=120)
        return dict(np.load(out))
    finally:
        if os.path.exists(out):
            os.remove(out)


@gpu
def test_small_cells_one_at_a_time_under_the_switch():
    """DSQ_NO_SEG_CELLS is read once per process: a fresh child runs the 64-sample design through the one-cell path."""
    check_robust(_child("seg64", {"DSQ_NO_SEG_CELLS": "1"})["robust"], robust_case("seg64"), "seg64 without segments")


# ------------------------------------------------------------------------------------------------ Cook's
COOKS_CASES = {"small": [40, 20, 10], "bucket": [170, 130]}  # N = 70, three cells; N = 300, two cells (bucket path)


def cooks_case(name):
    rng = np.random.default_rng(7 + len(name))
    X, lv = design(dict(sizes=COOKS_CASES[name]), rng)
    N, G, P = X.shape[0], 9, X.shape[1]
    sf = np.exp(rng.normal(0, 0.3, N))
    counts = gene_content(rng, N, G, sf, lv)
    mu = np.maximum(counts * np.exp(rng.normal(0, 0.4, (N, G))), 0.5)
    hat = rng.uniform(0.01, 0.5, (N, G))
    return dict(counts=counts, sf=sf, X=X, lv=lv, mu=mu, hat=hat, P=P, ref=orc.robust_mom_disp(counts / sf[:, None], X))


@gpu
@pytest.mark.parametrize("name", list(COOKS_CASES))
def test_cooks_kernel_all_five_outputs(ctx, name):
    from pydeseq2_amd._design import DesignPack
    from pydeseq2_amd._lib import DeviceArray

    k = cooks_case(name)
    D = DesignPack(k["X"], min_replicates=15)  # (the cell of 10 is not replaceable)
    N, G = k["counts"].shape
    y, ldn = pitched_counts(k["counts"])

    def pitch(a):
        o = np.full((G, ldn), np.nan)
        o[:, :N] = a.T
        return o

    sfp = np.full(ldn, np.nan)
    sfp[:N] = k["sf"]
    fl = np.full(ldn, 3, np.uint8)
    fl[:N] = D.flags
    d = [DeviceArray.from_host(ctx, a) for a in (y, sfp, pitch(k["mu"]), pitch(k["hat"]), D.cell_offsets, D.cell_index, fl)]
    d_ck = DeviceArray.from_host(ctx, np.full((G, ldn), -7.0))
    d_rd = DeviceArray.from_host(ctx, np.full(G + 3, -7.0))
    d_f = [DeviceArray.from_host(ctx, np.full(G + 3, 9, np.uint8)) for _ in range(4)]
    ctx.call("dsq_dev_cooks", _vp(d[0].ptr), ldn, _vp(d[1].ptr), _vp(d[2].ptr), _vp(d[3].ptr), _vp(d[4].ptr),
             _vp(d[5].ptr), D.n_cells, int(D.whole), D.max_cell, _vp(d[6].ptr), N, G, k["P"], COOKS_CUTOFF, _vp(d_ck.ptr),
             _vp(d_rd.ptr), *[_vp(a.ptr) for a in d_f])
    ctx.sync()
    ck, rd = d_ck.to_host(), d_rd.to_host()
    flags = [a.to_host() for a in d_f]
    for a in d + [d_ck, d_rd] + d_f:
        a.free()
    assert (ck[:, N:] == -7.0).all() and (rd[G:] == -7.0).all() and all((f[G:] == 9).all() for f in flags)
    assert_close(rd[:G], k["ref"], 1e-10, 0.0, "robust dispersion")
    for g in range(G):
        m = sc.cooks_model(k["counts"][:, g], k["mu"][:, g], k["hat"][:, g], D.flags, k["ref"][g], COOKS_CUTOFF, k["P"])
        ref = np.asarray(m["ck"], float)
        # the inputs decide every flag beyond rounding (a property of the reference alone)
        assert (np.abs(ref / COOKS_CUTOFF - 1) > 1e-6).all() and np.sort(ref)[-1] > np.sort(ref)[-2] * (1 + 1e-6)
        # V = mu + ar mu^2 carries the robust dispersion's 1e-10; the reciprocal form adds 17 u (stats_cases.COOKS_REL)
        assert_close(ck[g, :N], ref, 1e-10 + sc.COOKS_REL, 0.0, f"cooks gene {g}")
        assert [int(f[g]) for f in flags] == [m["any_all"], m["any_use"], m["any_use_nr"], m["few_above"]], g


# ------------------------------------------------------------------------------------------------ outlier replacement
# N = 128: next_pow2 room, no BucketWork, the row is sorted; 129: the bucket pass; "ties": size factors of 1 and counts of
# two values - more than 128 of them in a boundary bucket, the pass refuses and the sort behind it runs
# "nan_sf128": three size factors are NaN - the sorted row holds NaNs (one of them 0 / NaN), which numpy.sort and the LDS
# sorter put last, inside the trimmed fifth; those samples stay below the cutoff, so no replaced value is undefined
REPLACE_CASES = {"sort128": 128, "bucket129": 129, "ties300": 300, "nan_sf128": 128}


def replace_case(name):
    rng = np.random.default_rng(40 + len(name))
    N = REPLACE_CASES[name]
    X, lv = design(dict(sizes=[N - 3, 3]), rng)  # (the cell of three is not replaceable)
    G = 11
    sf = np.ones(N) if name == "ties300" else np.exp(rng.normal(0, 0.3, N))
    mean = np.exp(rng.uniform(np.log(5.0), np.log(3000), G))
    counts = rng.negative_binomial(5.0, 5.0 / (5.0 + mean[None, :] * sf[:, None])).astype(np.int64)
    if name == "ties300":
        counts = 20 + 7 * rng.integers(0, 2, (N, G))
    counts[:, 4] = 0
    counts[[2, 9, 50], 4] = [30, 7, 12]  # trimmed mean 0: whatever is replaced becomes 0
    cooks = np.where(rng.random((N, G)) < 0.08, 10.0, 0.1)
    cooks[:, 4] = 0.1
    cooks[[2, 9, 50], 4] = 10.0
    cooks[0, 6] = np.nan                 # (NaN > cutoff is false: kept)
    cooks[np.ix_(np.nonzero(lv == 1)[0], [0, 9])] = 10.0  # above the cutoff in the cell that is not replaceable: kept
    if name == "nan_sf128":
        sf[[5, 40, 77]] = np.nan
        cooks[[5, 40, 77], :] = 0.1
        counts[40, :] = 0
    sel = np.array([9, 4, 0, 6, 10, 2, 7], np.int32)  # 7 rows: one block of four and one of three
    return dict(counts=counts, sf=sf, X=X, cooks=cooks, sel=sel)


def replace_reference(k):
    from pydeseq2_amd._design import DesignPack

    D = DesignPack(k["X"], min_replicates=7)
    tbm = orc.trimmed_mean(k["counts"] / k["sf"][:, None], 0.2, axis=0)
    val = tbm[None, :] * k["sf"][:, None]
    with np.errstate(invalid="ignore"):
        repl = D.replaceable[:, None] & (k["cooks"] > CUTOFF)
    with np.errstate(invalid="ignore"):
        new = np.where(repl, np.where(repl, val, 0.0).astype(np.int64), k["counts"])
    zero = (new == 0).all(0)
    new[:, zero] = k["counts"][:, zero]  # k_replace: a row that became all zero keeps its original counts
    return new[:, k["sel"]], zero[k["sel"]], val[repl], repl


@pytest.mark.parametrize("name", list(REPLACE_CASES))
def test_replacement_inputs_are_decided_beyond_rounding(name):
    """int(tbm * sf) is compared exactly: no replaced value lies within 1e-9 of an integer (the trimmed mean is held to
    1e-12), the non-replaceable cell and the all-zero row are exercised"""
    k = replace_case(name)
    new, zero, val, repl = replace_reference(k)
    frac = val - np.floor(val)
    assert ((np.minimum(frac, 1 - frac) > 1e-9 * np.maximum(val, 1)) | (val == 0)).all()
    assert zero.tolist() == [False, True, False, False, False, False, False]
    with np.errstate(invalid="ignore"):
        assert ((k["cooks"] > CUTOFF) & ~repl).any() and repl[:, k["sel"]].sum() >= 20
    if name == "ties300":
        v = k["counts"][:, 0].astype(float)
        assert not sc.bucket_accepts(v, 60, 239)


def dev_replace(ctx, k):
    from pydeseq2_amd._design import DesignPack
    from pydeseq2_amd._lib import DeviceArray

    D = DesignPack(k["X"], min_replicates=7)
    N, G = k["counts"].shape
    y, ldn = pitched_counts(k["counts"])
    ck = np.full((G, ldn), 1e9)
    ck[:, :N] = k["cooks"].T
    sfp = np.full(ldn, np.nan)
    sfp[:N] = k["sf"]
    fl = np.full(ldn, 3, np.uint8)
    fl[:N] = D.flags
    n_sel = len(k["sel"])
    d = [DeviceArray.from_host(ctx, a) for a in (y, ck, sfp, fl, k["sel"])]
    d_out = DeviceArray.from_host(ctx, np.full((n_sel + 1, ldn), -7, np.int32))
    d_z = DeviceArray.from_host(ctx, np.full(n_sel + 3, 9, np.uint8))
    ctx.call("dsq_dev_replace_outliers", _vp(d[0].ptr), _vp(d[1].ptr), ldn, _vp(d[2].ptr), _vp(d[3].ptr), _vp(d[4].ptr),
             n_sel, N, CUTOFF, _vp(d_out.ptr), _vp(d_z.ptr))
    ctx.sync()
    out, z = d_out.to_host(), d_z.to_host()
    for a in d + [d_out, d_z]:
        a.free()
    assert (out[:n_sel, N:] == -7).all() and (out[n_sel] == -7).all() and (z[n_sel:] == 9).all()
    return out[:n_sel, :N].T, z[:n_sel]


@gpu
@pytest.mark.parametrize("name", list(REPLACE_CASES))
def test_replaced_counts_are_exact(ctx, name):
    k = replace_case(name)
    new, zero, _, _ = replace_reference(k)
    got, z = dev_replace(ctx, k)
    assert np.array_equal(got, new), np.argwhere(got != new)[:5]
    assert np.array_equal(z.astype(bool), zero)


@gpu
def test_replacement_through_the_buffer_less_kernel_is_exact():
    """DSQ_REPLACE_LEAN (read once per process): the 129-sample rows through k_replace_lean, in a fresh child"""
    k = replace_case("bucket129")
    new, zero, _, _ = replace_reference(k)
    r = _child("replace:bucket129", {"DSQ_REPLACE_LEAN": "1"})
    assert np.array_equal(r["counts"], new) and np.array_equal(r["zero"].astype(bool), zero)


if __name__ == "__main__":
    from pydeseq2_amd._lib import Context

    case, path = sys.argv[1], sys.argv[2]
    c = Context(0)
    if case.startswith("replace:"):
        got, z = dev_replace(c, replace_case(case.split(":")[1]))
        np.savez(path, counts=got, zero=z)
    else:
        k = robust_case(case)
        np.savez(path, robust=dev_robust_disp(c, k["counts"], k["sf"], k["X"]))
