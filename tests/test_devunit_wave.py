"""The wave policies of csrc/dsq_wave.h on the device: DeviceWave (64 lanes per gene: v_permlane32/16_swap + DPP
butterflies) and RowWave (16 lanes per gene, four genes per wavefront: the row-scoped last four stages).

The claims checked are the header's own: the butterflies are bit-identical to the xor butterfly of
tests/test_wave_butterfly.py and leave the same bits in every lane, sum_n<K> is bit-identical to sum() per value,
sum_comp follows the same partners with KSum::merge, slot_add hands out values in lane order, cell_add is
deterministic, and a RowWave row neither reads nor disturbs the other rows of its wavefront."""
import math

import numpy as np
import pytest

from tests.devunit import SUM_N_K
from tests.test_wave_butterfly import xor_butterfly

pytestmark = pytest.mark.gpu

WAVES = [64, 16]
N = 1024  # 16 DeviceWave genes / 64 RowWave genes
INT_MIN, INT_MAX = -(2**31), 2**31 - 1


@pytest.fixture(scope="module")
def du():
    from tests import devunit

    devunit.lib()
    return devunit


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def butterfly(v, op, wave):
    """The lane model per gene: DeviceWave = xor_butterfly (partners 32 ... 1), RowWave = its stages 8, 4, 2, 1."""
    if wave == 64:
        return xor_butterfly(v, op)
    v = list(v)
    for m in (8, 4, 2, 1):
        v = [op(v[i], v[i ^ m]) for i in range(16)]
    return v


def per_gene(x, wave, fn):
    x = list(x)
    out = []
    for g in range(0, len(x), wave):
        out += fn(x[g:g + wave])
    return out


def wide_data(rng, n=N):
    """wide dynamic range, both signs, signed zeros and a few exact cancellations; every RowWave row its own data"""
    x = rng.normal(size=n) * 10.0 ** rng.integers(-12, 12, n)
    x[rng.integers(0, n, n // 16)] = 0.0
    x[rng.integers(0, n, n // 16)] = -0.0
    i = rng.integers(0, n - 1, n // 32)
    x[i + 1] = -x[i]
    return x


def int_data(rng, n=N):
    x = rng.integers(-(10**6), 10**6, n).astype(np.int64)
    x[rng.integers(0, n, n // 16)] = INT_MIN
    x[rng.integers(0, n, n // 16)] = INT_MAX
    return x


def wrap32(v):
    return ((int(v) + 2**31) % 2**32) - 2**31


def fadd(p, q):
    return float(np.float64(p) + np.float64(q))


def fmax_sel(v, o):  # the device's `v > o ? v : o`, operands in the same order as shfl_xor's
    return v if v > o else o


def imax(p, q):
    return p if p > q else q


# ------------------------------------------------------------------------------------------------ reductions
@pytest.mark.parametrize("wave", WAVES)
@pytest.mark.parametrize("seed", range(3))
def test_sum_matches_xor_butterfly(du, wave, seed):
    x = wide_data(np.random.default_rng(seed))
    got, _ = du.wave(wave, "sum", x)
    ref = np.array(per_gene(x, wave, lambda v: butterfly(v, fadd, wave)))
    assert (bits(got[0]) == bits(ref)).all()
    g = bits(got[0]).reshape(-1, wave)
    assert (g == g[:, :1]).all()  # every lane holds the same bits


@pytest.mark.parametrize("wave", WAVES)
def test_sumi_maxi_match_xor_butterfly(du, wave):
    x = int_data(np.random.default_rng(11))
    _, s = du.wave(wave, "sumi", xi=x.astype(np.int32))
    _, m = du.wave(wave, "maxi", xi=x.astype(np.int32))
    rs = per_gene(x, wave, lambda v: butterfly(v, lambda p, q: wrap32(p + q), wave))
    rm = per_gene(x, wave, lambda v: butterfly(v, imax, wave))
    assert s[0].tolist() == rs
    assert m[0].tolist() == rm == np.repeat(x.reshape(-1, wave).max(axis=1), wave).tolist()


@pytest.mark.parametrize("wave", WAVES)
def test_max(du, wave):
    x = wide_data(np.random.default_rng(5))
    got, _ = du.wave(wave, "max", x)
    assert (got[0] == np.repeat(x.reshape(-1, wave).max(axis=1), wave)).all()
    ref = np.array(per_gene(x, wave, lambda v: butterfly(v, fmax_sel, wave)))
    assert (bits(got[0]) == bits(ref)).all()  # the signed zero that wins, too


@pytest.mark.parametrize("wave", WAVES)
def test_excl_scan(du, wave):
    x = int_data(np.random.default_rng(6))
    _, got = du.wave(wave, "excl_scan_i", xi=x.astype(np.int32))
    xr = x.astype(np.int32).reshape(-1, wave)
    with np.errstate(over="ignore"):
        ref = (np.cumsum(xr, axis=1, dtype=np.int32) - xr).ravel()  # int32 wrap-around, as the device adds
    assert (got[0] == ref).all()


# ------------------------------------------------------------------------------------------------ sum_n<K>
@pytest.mark.parametrize("wave", WAVES)
@pytest.mark.parametrize("K", SUM_N_K)  # K < 3, K not a multiple of 4, and the widths the kernels use
def test_sum_n_bitwise_equals_sum(du, wave, K):
    rng = np.random.default_rng(100 + K)
    x = np.stack([wide_data(rng) for _ in range(K)])
    o, r = du.sum_n(wave, x)
    assert (bits(o) == bits(r)).all()
    for k in (0, K // 2, K - 1):  # and sum() itself is the butterfly
        ref = np.array(per_gene(x[k], wave, lambda v: butterfly(v, fadd, wave)))
        assert (bits(r[k]) == bits(ref)).all()


# ------------------------------------------------------------------------------------------------ sum_comp / KSum
def two_sum_add(s, c, x):
    """KSum::add in float64 (Knuth TwoSum, no fused operations)"""
    s, c, x = np.float64(s), np.float64(c), np.float64(x)
    t = s + x
    bp = t - s
    c = c + ((s - (t - bp)) + (x - bp))
    return t, c


def merge(p, q):
    """KSum::merge(this = p, other = q)"""
    s, c = p
    os_, oc = q
    t = s + os_
    e = ((s - t) + os_) if abs(s) >= abs(os_) else ((os_ - t) + s)
    return (t, (c + oc) + e)


@pytest.mark.parametrize("wave", WAVES)
@pytest.mark.parametrize("T", [1, 9])
def test_sum_comp_matches_model(du, wave, T):
    # count-sized terms that cancel: each lane adds T terms ~ +-1e6 whose total is small; the compensated total must
    # match the model bitwise in every lane and be within a few ulps of the exact sum (math.fsum)
    rng = np.random.default_rng(40 + T)
    x = rng.integers(0, 10**6, (T, N)).astype(np.float64) * rng.choice([-1.0, 1.0], (T, N))
    x += rng.normal(size=(T, N)) * 1e-3
    x[:, ::2] = -x[:, 1::2] + rng.normal(size=(T, N // 2)) * 1e-9  # neighbours nearly cancel
    ls, lc, got = du.ksum(wave, x)
    ms, mc = np.zeros(N), np.zeros(N)
    for i in range(N):
        s, c = 0.0, 0.0
        for t in range(T):
            s, c = two_sum_add(s, c, x[t, i])
        ms[i], mc[i] = s, c
    # the per-lane KSum, compiled with -ffp-contract=fast, is still exactly TwoSum (it has no products to fuse)
    assert (bits(ls) == bits(ms)).all() and (bits(lc) == bits(mc)).all()
    pairs = per_gene(list(zip(ms, mc)), wave, lambda v: butterfly(v, merge, wave))
    ref = np.array([np.float64(s) + np.float64(c) for s, c in pairs])
    assert (bits(got) == bits(ref)).all()
    g = bits(got).reshape(-1, wave)
    assert (g == g[:, :1]).all()
    # error: s + c holds the exact total up to the roundings of c itself; c collects at most T + 6 error terms (one per
    # add / merge on a lane's path), each <= u (T + 6) sum|x|, and is rounded at most 2 (T + 6) times; value() rounds
    # once more.  |err| <= u |total| + 2 (T + 6)^2 u^2 sum|x|
    u = 2.0**-53
    for gi, row in enumerate(x.T.reshape(-1, wave, T)):
        exact = math.fsum(row.ravel())
        tol = u * abs(exact) + 2 * (T + 6) ** 2 * u * u * np.abs(row).sum() + 1e-300
        assert abs(got[gi * wave] - exact) <= tol, (gi, got[gi * wave], exact)


# ------------------------------------------------------------------------------------------------ lane helpers
@pytest.mark.parametrize("wave", WAVES)
def test_from_lane_every_source(du, wave):
    x = wide_data(np.random.default_rng(8))
    o, _ = du.wave(wave, "from_lane", x, nout=wave)
    xr = x.reshape(-1, wave)
    for s in range(wave):
        assert (bits(o[s]) == bits(np.repeat(xr[:, s], wave))).all(), s


def test_readlane_d_every_lane(du):
    x = wide_data(np.random.default_rng(9))
    o, _ = du.wave(64, "readlane_d", x, nout=64)
    xr = x.reshape(-1, 64)
    for s in range(64):
        assert (bits(o[s]) == bits(np.repeat(xr[:, s], 64))).all(), s


def test_row_bcast_every_lane(du):
    x = wide_data(np.random.default_rng(10))
    o, _ = du.wave(16, "row_bcast", x, nout=16)
    xr = x.reshape(-1, 16)
    for L in range(16):
        assert (bits(o[L]) == bits(np.repeat(xr[:, L], 16))).all(), L


@pytest.mark.parametrize("wave", WAVES)
def test_uniform(du, wave):
    rng = np.random.default_rng(12)
    v = np.repeat(wide_data(rng, N // wave), wave)  # identical within a gene, different across genes / rows
    o, _ = du.wave(wave, "uniform", v)
    assert (bits(o[0]) == bits(v)).all()


@pytest.mark.parametrize("wave", WAVES)
def test_any(du, wave):
    # DeviceWave: over the gene's 64 lanes; RowWave: over the whole wavefront's active lanes (its comment: conservative)
    xi = np.zeros(N, np.int32)
    xi[[5, 64 + 17, 64 + 33, 3 * 64 + 63, 9 * 64]] = 1
    _, o = du.wave(wave, "any", xi=xi)
    ref = np.repeat(xi.reshape(-1, 64).max(axis=1), 64)
    assert (o[0] == ref).all()


@pytest.mark.parametrize("wave", WAVES)
def test_hist_add(du, wave):
    xi = np.random.default_rng(13).integers(0, 8, N).astype(np.int32)
    _, o = du.wave(wave, "hist_add", xi=xi)
    for g, row in enumerate(xi.reshape(-1, wave)):
        counts = np.bincount(row, minlength=8)
        assert o[0][g * wave:(g + 1) * wave].tolist() == [int(counts[l & 7]) for l in range(wave)]


@pytest.mark.parametrize("wave", WAVES)
def test_slot_add_lane_order(du, wave):
    _, o = du.wave(wave, "slot_add", xi=np.zeros(N, np.int32))
    assert o[0].reshape(-1, wave).tolist() == [list(range(wave))] * (N // wave)
    _, o = du.wave(wave, "slot_add_third", xi=np.zeros(N, np.int32), ifill=-7)
    act = np.arange(wave) % 3 == 0
    for row in o[0].reshape(-1, wave):
        assert row[act].tolist() == list(range(int(act.sum())))
        assert (row[~act] == -7).all()


@pytest.mark.parametrize("wave", WAVES)
def test_cell_add_deterministic(du, wave):
    rng = np.random.default_rng(14)
    x = rng.normal(size=N) * 10.0 ** rng.integers(-6, 6, N)
    o1, _ = du.wave(wave, "cell_add", x)
    o2, _ = du.wave(wave, "cell_add", x)
    assert (bits(o1) == bits(o2)).all()
    xr = x.reshape(-1, wave)
    tot = o1[0].reshape(-1, wave)
    assert (bits(tot) == bits(tot[:, :1])).all()
    serial_equal = 0
    for g in range(xr.shape[0]):
        # any order of W - 1 rounded additions: |err| <= (W - 1) u sum|x|
        exact = math.fsum(xr[g])
        assert abs(tot[g, 0] - exact) <= (wave - 1) * 2.0**-53 * np.abs(xr[g]).sum()
        s = 0.0
        for v in xr[g]:
            s = fadd(s, v)
        serial_equal += bits(s) == bits(tot[g, 0])
    print(f"cell_add wave={wave}: {serial_equal} of {xr.shape[0]} genes equal the serial lane-order sum")


# ------------------------------------------------------------------------------------------------ RowWave rows
def test_row_wave_inactive_rows(du):
    """rows 1 and 3 of every wavefront leave before the reductions: rows 0 and 2 give the bits of the full run, and
    nothing is written for the inactive rows"""
    rng = np.random.default_rng(15)
    x, xi = wide_data(rng), int_data(rng).astype(np.int32)
    even = ((np.arange(N) >> 4) & 1) == 0
    for op, kw, dbl in (("sum", {"x": x}, True), ("max", {"x": x}, True), ("sumi", {"xi": xi}, False),
                        ("maxi", {"xi": xi}, False), ("excl_scan_i", {"xi": xi}, False)):
        full = du.wave(16, op, **kw)
        part = du.wave(16, op, even_only=True, **kw)
        f, p = (bits(full[0][0]), bits(part[0][0])) if dbl else (full[1][0], part[1][0])
        assert (f[even] == p[even]).all(), op
        assert (np.isnan(part[0][0][~even]) if dbl else (part[1][0][~even] == -7)).all(), op
    xs = np.stack([wide_data(rng) for _ in range(13)])
    fo, _ = du.sum_n(16, xs)
    po, _ = du.sum_n(16, xs, even_only=True)
    assert (bits(fo[:, even]) == bits(po[:, even])).all() and np.isnan(po[:, ~even]).all()
    t = np.stack([wide_data(rng) for _ in range(3)])
    _, _, fk = du.ksum(16, t)
    _, _, pk = du.ksum(16, t, even_only=True)
    assert (bits(fk[even]) == bits(pk[even])).all() and np.isnan(pk[~even]).all()
