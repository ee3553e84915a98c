"""Crafted inputs, the numpy reference and a float64 path model for the workgroup medians of csrc/dsq_k_stats.hip
(no GPU needed).

The selections under test: `block_median_values<NT>` (narrowing in value space: k_sf_row<*, 256, 32>,
k_sf_row<*, 1024, 32>, k_prior_mad), `block_median_each` (bitwise radix select, 11/11/11/11/11/9 bits: k_row_median_c
above 32 768 usable genes) and the per-pass kernels of the multi-GPU protocol (8-bit digits, k_sf_count ... k_sf_finish).

How a multiset is put in front of a selection: the log means are an INPUT of the size-factor entry points, the value
that enters a sample's median is log(count) - logmeans[g], and with count = 1 (kLogInt[1] == 0.0 exactly) that is
-logmeans[g] bit for bit.  A case is therefore a pool of float64 values (one per usable gene) and, per sample, the
subset of it that has count 1; the others have count 0, which `dsq_dev_size_factors` leaves out of the median and
`dsq_dev_size_factors_new` counts as -inf at the low end.

Value grid: every finite crafted value is a multiple of 2^-40 with |x| <= 16 (here: of 2^-30, so any two distinct
values are >= 2^-30 apart), hence the mean of the two middle values is exact and numpy's sort-based median is the
unambiguous reference; a selection that is off by one order statistic moves the size factor by >= 9e-10 relative.
Exempt (`grid=False`): the `flog` cases (counts >= 256, reference np.log(c) - lm, neighbours near the middle >= 1e-9
apart) and `radix-last9`, whose point is values that differ only in the nine bits of the last radix pass - no value on
the grid has a set bit there.  That case is held by the exact agreement of the two radix implementations (11-bit and
8-bit digits) and of both with numpy's median before `exp`.
"""
import numpy as np

GRID = 2.0 ** -40
SPACING = 2.0 ** -30
K_SEL_CAND = 1024  # kSelCand
N_BINS = 2048

ALL_TAGS = ("empty", "all-low", "high", "nan", "low0", "equal", "direct", "hist-same", "hist-two", "deep-two-bins",
            "descend", "collapse")


# ------------------------------------------------------------------------------------------------ reference
def ref_median(values):
    """numpy's sort-based median in float64 of exactly the values the kernel sees (NaN = not part of the median;
    infinities as numpy treats them; nothing left: NaN)."""
    v = np.asarray(values, dtype=np.float64)
    v = v[~np.isnan(v)]
    if v.size == 0:
        return np.nan
    with np.errstate(invalid="ignore"):
        return float(np.median(v))


def same_bits(a, b):
    a, b = np.float64(a), np.float64(b)
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    return a.view(np.int64) == b.view(np.int64) or (a == 0.0 and b == 0.0)


# ------------------------------------------------------------------------------------------------ path model
def model_median(values):
    """float64 model of block_median_values: (median, tags).  Same arithmetic as the kernel: scale = 2048 / (hi - lo),
    bin = min(int((x - lo) * scale), 2047), membership lo <= x <= hi, at most 1024 candidates are ranked, the ranks are
    re-based by the prefix of bin b0.  (A subtraction followed by a multiplication cannot be contracted, so numpy's
    float64 gives the device's bins bit for bit.)"""
    v = np.asarray(values, dtype=np.float64)
    v = v[~np.isnan(v)]
    n_low, n_high = int(np.sum(v == -np.inf)), int(np.sum(v == np.inf))
    fin = v[np.isfinite(v)]
    n_fin = fin.size
    M = n_fin + n_low + n_high
    if M == 0:
        return np.nan, ["empty"]
    r0, r1 = (M - 1) // 2, M // 2
    if r1 < n_low:
        return -np.inf, ["all-low"]
    if r1 >= n_low + n_fin:
        return (np.nan, ["nan"]) if r0 < n_low else (np.inf, ["high"])
    tags = []
    low0 = r0 < n_low
    if low0:
        tags.append("low0")
    q0, q1 = (r1 if low0 else r0) - n_low, r1 - n_low
    lo, hi, cnt = float(fin.min()), float(fin.max()), n_fin
    a0 = a1 = np.nan
    for level in range(64):
        if lo == hi:
            tags.append("collapse" if level else "equal")
            a0 = a1 = lo
            break
        scale = 2048.0 / (hi - lo)
        cur = fin[(fin >= lo) & (fin <= hi)]
        bins = np.minimum(((cur - lo) * scale).astype(np.int64), N_BINS - 1)
        if cnt <= K_SEL_CAND:
            tags.append("direct")
            cand = np.sort(cur)
        else:
            h = np.bincount(bins, minlength=N_BINS)
            excl = np.cumsum(h) - h
            b0 = int(np.nonzero((excl <= q0) & (q0 < excl + h))[0][0])
            b1 = int(np.nonzero((excl <= q1) & (q1 < excl + h))[0][0])
            pre0 = int(excl[b0])
            c0 = int(h[b0])
            csel = c0 + (int(h[b1]) if b1 != b0 else 0)
            q0 -= pre0
            q1 -= pre0
            if csel > K_SEL_CAND:
                if b0 != b1:
                    tags.append("deep-two-bins")
                    a0, a1 = float(cur[bins == b0].max()), float(cur[bins == b1].min())
                    break
                tags.append("descend")
                lo, hi, cnt = float(cur[bins == b0].min()), float(cur[bins == b0].max()), c0
                continue
            tags.append("hist-same" if b0 == b1 else "hist-two")
            cand = np.sort(cur[(bins == b0) | (bins == b1)])
        assert cand.size <= K_SEL_CAND
        a0, a1 = float(cand[q0]), float(cand[q1])
        break
    v0 = -np.inf if low0 else a0
    return (v0 if r0 == r1 else (v0 + a1) / 2.0), tags


# ------------------------------------------------------------------------------------------------ value builders
def _snap(x):
    return np.round(np.asarray(x, dtype=np.float64) / SPACING) * SPACING


def spread(rng, n, a, b):
    """n DISTINCT multiples of 2^-30 in [a, b], uniformly drawn, unsorted"""
    ia, ib = int(np.ceil(a / SPACING)), int(np.floor(b / SPACING))
    assert ib - ia + 1 >= n, (n, a, b)
    if ib - ia + 1 <= 8 * n:
        k = rng.choice(ib - ia + 1, n, replace=False) + ia
    else:
        k = np.unique(rng.integers(ia, ib + 1, 2 * n + 16))
        assert k.size >= n
        k = rng.permutation(k)[:n]
    return rng.permutation(k.astype(np.float64) * SPACING)


def _subset(rng, pool, drop_low=0, drop_high=0, drop_random=0):
    """boolean row: the pool minus its `drop_low` smallest, `drop_high` largest and `drop_random` random values"""
    order = np.argsort(pool, kind="stable")
    sel = np.ones(pool.size, dtype=bool)
    sel[order[:drop_low]] = False
    if drop_high:
        sel[order[-drop_high:]] = False
    if drop_random:
        left = np.nonzero(sel)[0]
        sel[rng.choice(left, drop_random, replace=False)] = False
    return sel


class Case:
    """pool [Gu] float64 (value of a gene whose count is 1), sel [N][Gu] bool (count 1 / 0), mode 'default' (a zero
    count leaves the gene out: dsq_dev_size_factors) or 'new' (a zero count is -inf: dsq_dev_size_factors_new): the
    entry point whose `expect` tags the host tests assert (the GPU tests run both entry points on every case).
    expect: per sample the model's tag list, or None.  decoys: values that the gene mask removes (None: the generic
    ones of layout()).  counts: explicit counts [N][Gu] instead of 0 / 1 (then pool holds the log means' negatives)."""

    def __init__(self, name, pool, sel, mode="default", expect=None, decoys=None, counts=None, grid=True,
                 mask_only=False, dtypes=("int32", "int64")):
        self.name, self.pool, self.sel, self.mode = name, np.asarray(pool, dtype=np.float64), np.asarray(sel), mode
        self.N, self.Gu = self.sel.shape
        assert self.pool.shape == (self.Gu,)
        self.expect = expect if expect is not None else [None] * self.N
        assert len(self.expect) == self.N
        self.decoys, self.counts, self.grid, self.mask_only, self.dtypes = decoys, counts, grid, mask_only, dtypes

    def count_matrix(self):
        return self.counts if self.counts is not None else self.sel.astype(np.int64)

    def values_seen(self, n, mode=None):
        """what the selection of sample n sees (NaN = left out), in pool order"""
        mode = mode or self.mode
        c = self.count_matrix()[n]
        with np.errstate(divide="ignore"):
            x = self.pool if self.counts is None else np.log(c.astype(np.float64)) + self.pool
        return np.where(c > 0, x, -np.inf if mode == "new" else np.nan)

    def reference(self, mode=None):
        """reference medians [N] of the entry point `mode`"""
        return np.array([ref_median(self.values_seen(n, mode)) for n in range(self.N)])


def layout(case, G, with_mask, seed=0):
    """The case as the size-factor entry points take it: (counts [N][G] int64, logmeans [G], mask [G] uint8 or None) in
    a shuffled gene order.  Genes beyond the pool have a log mean of -inf (not usable) or NaN (every 7th: not usable
    either) and random counts; with a mask, decoy genes - finite log mean, count 1 in every sample, values that would
    move every median - are masked out, and a few unusable genes are masked in."""
    rng = np.random.default_rng([seed, G, int(with_mask)])
    Gu, N = case.Gu, case.N
    assert G >= Gu
    decoys = np.zeros(0)
    if with_mask:
        if case.decoys is not None:
            decoys = np.asarray(case.decoys, dtype=np.float64)
        elif G > Gu:
            fin = case.pool[np.isfinite(case.pool)]
            base = (fin.min() if fin.size else 0.0) - 0.5
            decoys = np.full(min(64, G - Gu), base)
    nd = decoys.size
    assert Gu + nd <= G
    lm = np.full(G, -np.inf)
    lm[Gu + nd::7] = np.nan
    counts = rng.integers(0, 300, (N, G)).astype(np.int64)
    lm[:Gu] = -case.pool
    counts[:, :Gu] = case.count_matrix()
    lm[Gu:Gu + nd] = -decoys
    counts[:, Gu:Gu + nd] = 1
    mask = None
    if with_mask:
        mask = np.zeros(G, dtype=np.uint8)
        mask[:Gu] = 1
        mask[Gu + nd::3] = 1
    perm = rng.permutation(G)
    return (np.ascontiguousarray(counts[:, perm]), np.ascontiguousarray(lm[perm]),
            None if mask is None else np.ascontiguousarray(mask[perm]))


# ------------------------------------------------------------------------------------------------ named cases
def _rows(*rows):
    return np.stack(rows)


def case_direct():
    rng = np.random.default_rng(101)
    pool = spread(rng, 1024, -8.0, 8.0)
    sizes = [1, 2, 1023, 1024, 513, 3]
    sel = np.zeros((len(sizes), 1024), dtype=bool)
    for n, s in enumerate(sizes):
        sel[n, rng.choice(1024, s, replace=False)] = True
    return Case("direct", pool, sel, expect=[["equal"], ["direct"], ["direct"], ["direct"], ["direct"], ["direct"]])


def case_hist_1025():
    rng = np.random.default_rng(102)
    pool = spread(rng, 1026, -8.0, 8.0)
    # the two middle values of the full pool next to each other, so that the even sample has both ranks in one bin
    srt = np.sort(pool)
    pool[np.argmax(pool == srt[513])] = srt[512] + SPACING
    sel = _rows(_subset(rng, pool), _subset(rng, pool, drop_low=1), _subset(rng, pool, drop_high=1),
                _subset(rng, pool, drop_low=1, drop_high=1), _subset(rng, pool, drop_random=1))
    return Case("hist-1025", pool, sel, expect=[["hist-same"], ["hist-same"], ["hist-same"], ["direct"], ["hist-same"]])


def case_full(n):
    rng = np.random.default_rng(103 + n)
    pool = spread(rng, n, -4.0, 4.0)
    sel = _rows(_subset(rng, pool), _subset(rng, pool, drop_low=1), _subset(rng, pool, drop_random=n // 10),
                _subset(rng, pool, drop_random=n // 10 + 1), _subset(rng, pool, drop_high=n // 3))
    return Case(f"full-{n}", pool, sel)


def case_hist_two():
    rng = np.random.default_rng(104)
    pool = np.concatenate([spread(rng, 1500, -6.0, -1.0), spread(rng, 1500, 1.0, 6.0)])
    sel = _rows(_subset(rng, pool), _subset(rng, pool, drop_low=1), _subset(rng, pool, drop_low=1, drop_high=1),
                _subset(rng, pool, drop_low=200, drop_high=200), _subset(rng, pool, drop_high=1))
    return Case("hist-two", pool, sel,
                expect=[["hist-two"], ["hist-same"], ["hist-two"], ["hist-two"], ["hist-same"]])


def _two_groups(rng, a, b):
    """500 outliers, group a (1500), group b (1500), 500 outliers"""
    return np.concatenate([spread(rng, 500, -8.0, -2.0), a, b, spread(rng, 500, 2.0, 8.0)])


def _two_group_rows(rng, pool):
    return _rows(_subset(rng, pool), _subset(rng, pool, drop_low=1), _subset(rng, pool, drop_high=1),
                 _subset(rng, pool, drop_low=100, drop_high=100), _subset(rng, pool, drop_low=499, drop_high=499),
                 _subset(rng, pool, drop_low=3, drop_high=1))


def case_deep_two_ties():
    rng = np.random.default_rng(105)
    pool = _two_groups(rng, np.full(1500, -0.5), np.full(1500, 0.5))
    dc = ["descend", "collapse"]
    return Case("deep-two-ties", pool, _two_group_rows(rng, pool),
                expect=[["deep-two-bins"], dc, dc, ["deep-two-bins"], ["deep-two-bins"], dc])


def case_deep_two_clusters():
    rng = np.random.default_rng(106)
    w = 4000 * SPACING  # 3.7e-6: far inside one of the 2048 bins of [-8, 8]
    pool = _two_groups(rng, spread(rng, 1500, -0.5, -0.5 + w), spread(rng, 1500, 0.5, 0.5 + w))
    return Case("deep-two-clusters", pool, _two_group_rows(rng, pool),
                expect=[["deep-two-bins"], None, None, ["deep-two-bins"], ["deep-two-bins"], None])


def _outliers(rng, n):
    """n outliers on each side, the extremes exactly -8 and 8 (first / last), so that the level-0 bins are 2^-7 wide and
    bin 1024 starts at 0 in every sample that keeps both extremes"""
    return (np.concatenate([[-8.0], spread(rng, n - 1, -7.9, -1.0)]), np.concatenate([spread(rng, n - 1, 1.0, 7.9), [8.0]]))


def _outlier_rows(rng, n_out, n_mid, drops):
    """samples of a pool [n_out low outliers | n_mid values | n_out high outliers] that lack `drops[n]` = (low, high)
    random outliers, never an extreme"""
    Gu = 2 * n_out + n_mid
    sel = np.ones((len(drops), Gu), dtype=bool)
    for n, (dl, dh) in enumerate(drops):
        sel[n, rng.choice(np.arange(1, n_out), dl, replace=False)] = False
        sel[n, rng.choice(np.arange(n_out + n_mid, Gu - 1), dh, replace=False)] = False
    return sel


DROPS = [(0, 0), (1, 0), (0, 1), (120, 120), (400, 401), (37, 36)]


def case_descend1():
    rng = np.random.default_rng(107)
    # 1500 distinct values in 0.003, inside bin 1024 = [0, 2^-7) of the level-0 range, among 600 outliers on each side
    lo_out, hi_out = _outliers(rng, 600)
    pool = np.concatenate([lo_out, spread(rng, 1500, 0.0010, 0.0040), hi_out])
    return Case("descend1", pool, _outlier_rows(rng, 600, 1500, DROPS))


def _nested(rng, core):
    """500 outliers | 750 cluster values | core (1500) | 750 cluster values | 500 outliers: the cluster spans exactly
    [lo1, hi1] ~ [0.001, 0.006] (inside bin 1024 of the level-0 range), the core sits between 0.2 and 0.8 of bin 1000
    of the cluster's range"""
    lo1, hi1 = float(_snap(0.0010)), float(_snap(0.0060))
    w1 = (hi1 - lo1) / N_BINS
    c0 = float(_snap(lo1 + 1000.2 * w1))
    below = spread(rng, 749, lo1 + SPACING, c0 - 4 * w1)
    above = spread(rng, 749, c0 + 4 * w1, hi1 - SPACING)
    lo_out, hi_out = _outliers(rng, 500)
    return np.concatenate([lo_out, [lo1], below, core(c0, w1), above, [hi1], hi_out])


def case_descend2():
    rng = np.random.default_rng(108)
    # the core: 1500 values at >= 2^-30 in 0.6 of a level-1 bin (1.46e-6 = 1572 grid steps)
    pool = _nested(rng, lambda c0, w1: spread(rng, 1500, c0, c0 + 0.6 * w1))
    return Case("descend2", pool, _outlier_rows(rng, 500, 3000, DROPS))


def case_descend_collapse():
    rng = np.random.default_rng(109)
    pool = _nested(rng, lambda c0, w1: np.concatenate([spread(rng, 100, c0, c0 + 0.6 * w1),
                                                       np.full(1400, float(_snap(c0 + 0.3 * w1)))]))
    return Case("descend-collapse", pool, _outlier_rows(rng, 500, 3000, DROPS))


def case_all_equal():
    rng = np.random.default_rng(110)
    pool = np.full(3000, 1.25)
    sizes = [3000, 2999, 1025, 1024, 1, 2]
    sel = np.zeros((len(sizes), 3000), dtype=bool)
    for n, s in enumerate(sizes):
        sel[n, rng.choice(3000, s, replace=False)] = True
    return Case("all-equal", pool, sel, expect=[["equal"]] * 6)


def _zeros_rows(rng, Gu, n_zero):
    sel = np.ones((len(n_zero), Gu), dtype=bool)
    for n, z in enumerate(n_zero):
        sel[n, rng.choice(Gu, z, replace=False)] = False
    return sel


def case_low(Gu, name):
    """-inf at the low end (the new-samples entry point): exactly half (M even: `low0`, median (-inf + x) / 2 = -inf),
    one fewer than the middle rank (finite median), the middle rank itself, more than half, all, none"""
    rng = np.random.default_rng(111 + Gu)
    pool = spread(rng, Gu, -8.0, 8.0)
    h = Gu // 2
    n_zero = [h, (Gu - 1) // 2, h + 1, h - 1 if Gu % 2 == 0 else h - 2, Gu - Gu // 4, Gu, 0, 7]
    sel = _zeros_rows(rng, Gu, n_zero)
    first = ["low0", "direct" if Gu - h <= K_SEL_CAND else "hist-same"] if Gu % 2 == 0 else None
    expect = [first, None, ["all-low"], None, ["all-low"], ["all-low"], None, None]
    return Case(name, pool, sel, mode="new", expect=expect)


def case_empty():
    rng = np.random.default_rng(112)
    pool = spread(rng, 100, -8.0, 8.0)
    sel = _zeros_rows(rng, 100, [100, 99, 0, 50, 100])
    return Case("empty-sample", pool, sel, expect=[["empty"], ["equal"], ["direct"], ["direct"], ["empty"]])


def case_no_usable():
    return Case("no-usable-gene", np.zeros(0), np.zeros((4, 0), dtype=bool), expect=[["empty"]] * 4)


def case_mask_middle():
    rng = np.random.default_rng(113)
    full = np.sort(spread(rng, 3000, -8.0, 8.0))
    mid = np.zeros(3000, dtype=bool)
    mid[1400:1700] = True  # the 300 values around both middle ranks, more of them above: the median moves down
    pool = rng.permutation(full[~mid])
    sel = _rows(_subset(rng, pool), _subset(rng, pool, drop_low=1), _subset(rng, pool, drop_random=270),
                _subset(rng, pool, drop_high=1))
    return Case("mask-middle", pool, sel, decoys=full[mid], mask_only=True)


def case_flog(name, cmax, dtypes):
    """counts >= 256 (flog) next to table counts: log means chosen so that sample 0's values log(c) - lm are ~2^-29
    apart; sample n has (n + 1) times the counts, i.e. the same values shifted by log(n + 1)"""
    rng = np.random.default_rng(114 + int(np.log2(cmax)))
    Gu, N = 3001, 5
    c0 = np.where(rng.random(Gu) < 0.5, rng.integers(1, 256, Gu), (2.0 ** rng.uniform(8, np.log2(cmax), Gu)).astype(np.int64))
    t = rng.permutation((np.arange(Gu) - Gu // 2) * 2.0 * SPACING) + 0.37
    t[: Gu // 3] += rng.uniform(-3, 3, Gu // 3).round(3)  # and a third of them spread widely
    lm = np.log(c0.astype(np.float64)) - t
    counts = c0[None, :] * (np.arange(N)[:, None] + 1)
    assert counts.max() < (2 ** 31 if "int32" in dtypes else 2 ** 62)
    sel = _zeros_rows(rng, Gu, [0, 1, 300, 301, 2])
    return Case(name, -lm, sel, counts=np.where(sel, counts, 0).astype(np.int64), grid=False, dtypes=dtypes)


def value_cases():
    """the named cases of block_median_values (Gu <= 8192 unless named full-32768)"""
    return [case_direct(), case_hist_1025(), case_full(8192), case_hist_two(), case_deep_two_ties(),
            case_deep_two_clusters(), case_descend1(), case_descend2(), case_descend_collapse(), case_all_equal(),
            case_low(4000, "low-even"), case_low(3999, "low-odd"), case_low(1000, "low-even-direct"),
            case_low(999, "low-odd-direct"), case_empty(), case_no_usable(), case_mask_middle(),
            case_flog("flog", 2 ** 31 // 5, ("int32", "int64")), case_flog("flog-int64", 2 ** 40, ("int64",))]


def big_value_cases():
    """the full register file of k_sf_row<*, 1024, 32>"""
    return [case_full(32768)]


# ---- radix cases: the two middle values of every even sample have opposite signs (the top digit of the two tracked
# ranks differs from pass 0 on); M odd and even; one sample of every default-mode case has no value at all
def _balanced_rows(rng, bal, extra, inner=1000):
    """bal: as many negative as positive values; `extra` further genes (an odd Gu) enter no sample.  Samples: all (even),
    minus the lowest (odd: the first positive), minus the highest (odd: the last negative), minus `inner` at each end
    (even), nothing (M = 0), minus 2 at each end (even)"""
    rows = _rows(_subset(rng, bal), _subset(rng, bal, drop_low=1), _subset(rng, bal, drop_high=1),
                 _subset(rng, bal, drop_low=inner, drop_high=inner), np.zeros(bal.size, dtype=bool),
                 _subset(rng, bal, drop_low=2, drop_high=2))
    return np.concatenate([rows, np.zeros((rows.shape[0], extra), dtype=bool)], axis=1)


def radix_smooth(Gu):
    rng = np.random.default_rng(201 + Gu)
    h = Gu // 2
    bal = np.concatenate([spread(rng, h, -8.0, -SPACING), spread(rng, h, SPACING, 8.0)])
    pool = np.concatenate([bal, spread(rng, Gu - 2 * h, 9.0, 10.0)])
    return Case(f"radix-smooth-{Gu}", pool, _balanced_rows(rng, bal, Gu - 2 * h))


def radix_last9(Gu):
    """the values around both middle ranks differ only in the nine bits of the last pass: -(1 + k 2^-52) and
    +(1 + k 2^-52), k < 512, next to long runs of ties at +-(1 + 2^-40) and +-2; the fourth sample has nothing but
    values of the last pass"""
    rng = np.random.default_rng(202 + Gu)
    h = Gu // 2
    near = 1.0 + rng.choice(512, 300, replace=False).astype(np.float64) * 2.0 ** -52
    runs = (h - 300) // 2
    side = np.concatenate([near, np.full(runs, 1.0 + GRID), np.full(h - 300 - runs, 2.0)])
    bal = np.concatenate([-side, side])
    pool = np.concatenate([bal, np.full(Gu - 2 * h, 3.0)])
    return Case(f"radix-last9-{Gu}", pool, _balanced_rows(rng, bal, Gu - 2 * h, inner=h - 150), grid=False)


def radix_equal(Gu):
    rng = np.random.default_rng(203 + Gu)
    pool = np.full(Gu, -1.25)
    sel = _zeros_rows(rng, Gu, [0, 1, Gu, Gu - 1, Gu - 2, 5000])
    return Case(f"radix-equal-{Gu}", pool, sel)


def radix_low(Gu):
    """-inf keys at the low end (new samples): zeros + negatives = positives, so the middle is -x | +x; then exactly
    half zeros, more than half, all, none"""
    rng = np.random.default_rng(204 + Gu)
    h = Gu // 2
    pool = np.concatenate([spread(rng, h, -8.0, -SPACING), spread(rng, Gu - h, SPACING, 8.0)])
    neg, pos = np.arange(h), np.arange(h, Gu)
    sel = np.ones((6, Gu), dtype=bool)
    sel[0, rng.choice(neg, h // 2, replace=False)] = False
    sel[1, np.concatenate([neg, rng.choice(pos, (Gu + 1) // 2 - h, replace=False)])] = False
    sel[2, np.concatenate([neg, rng.choice(pos, 100, replace=False)])] = False
    sel[3] = False
    sel[5, rng.choice(Gu, 9, replace=False)] = False
    return Case(f"radix-low-{Gu}", pool, sel, mode="new")


RADIX_SIZES = (32769, 40000)  # usable genes on the radix side of kSfRegGenes = 32 768, odd and even


def radix_cases(sizes=RADIX_SIZES):
    return [f(Gu) for Gu in sizes for f in (radix_smooth, radix_last9, radix_equal, radix_low)]


# ------------------------------------------------------------------------------------------------ prior MAD
class PriorCase:
    """dsq_dev_prior_mad inputs: gw (raw genewise dispersions), fit (trend values).  A gene enters with the residual
    log(clip(gw)) - log(fit) if clip(gw) >= 100 * min_disp.  The crafted genes have gw = 1 (log exactly 0) and
    fit = exp(-x), so the residual is x to within the last bits of the two logarithms and equal `fit` give exact
    ties; every case keeps its MAD >= 0.01 |x|, so that those last bits stay below the tolerance."""
    MIN_DISP, MAX_DISP = 1e-8, 10.0

    def __init__(self, name, x, gw=None, fit=None):
        x = np.asarray(x, dtype=np.float64)
        self.name = name
        self.gw = np.ones(x.size) if gw is None else np.asarray(gw, dtype=np.float64)
        self.fit = np.exp(-x) if fit is None else np.asarray(fit, dtype=np.float64)
        self.n = x.size

    def residuals(self):
        """the numpy expression of test_prior_mad_kernel_vs_numpy on these inputs (NaN residuals dropped)"""
        g = np.clip(self.gw, self.MIN_DISP, self.MAX_DISP)
        ok = ~np.isnan(self.gw) & (g >= 100.0 * self.MIN_DISP)
        with np.errstate(divide="ignore", invalid="ignore"):
            res = np.log(g[ok]) - np.log(self.fit[ok])
        return res[~np.isnan(res)]

    def reference(self):
        """squared MAD / norm.ppf(0.75)^2, NaN if no gene passes"""
        res = self.residuals()
        if res.size == 0:
            return np.nan
        with np.errstate(invalid="ignore"):
            mad = np.median(np.abs(res - np.median(res))) / 0.67448975019608171
        return float(mad ** 2)

    def paths(self):
        """(tags of the first median, tags of the second) by the model, on numpy's residuals"""
        res = self.residuals()
        c, t1 = model_median(res)
        with np.errstate(invalid="ignore"):
            _, t2 = model_median(np.abs(res - c))
        return t1, t2


PRIOR_SIZES = (1, 2, 1024, 1025, 8191, 8192, 8193, 16385)  # around the eight-loads-per-trip walk of k_prior_mad


def prior_size_case(n):
    rng = np.random.default_rng(300 + n)
    return PriorCase(f"n{n}", _snap(rng.uniform(-1.0, 1.0, n)))


def _shuffled(rng, *parts):
    return rng.permutation(np.concatenate(parts))


def prior_cases():
    out = []
    rng = np.random.default_rng(301)
    # L 1000 | A 1000 | B 2000 || C 2000 | D 1000 | R 1000: the middle is B | C, the absolute deviations are 4000 x 0.1,
    # 2000 x 0.3 and the outliers: their middle is (0.1-group) | (0.3-group)
    x = _shuffled(rng, spread(rng, 1000, -1.0, -0.6), np.full(1000, -0.3), np.full(2000, -0.1), np.full(2000, 0.1),
                  np.full(1000, 0.3), spread(rng, 1000, 0.6, 1.0))
    out.append(PriorCase("both-deep-two-bins", x))
    # a cluster of 1500 around 0 in 1e-4 among 3250 values on each side: the first median descends into the cluster
    # (the extremes are -1 and 1: the cluster lies at 0.1 ... 0.2 of bin 1024 of the level-0 range)
    x = _shuffled(rng, [-1.0], spread(rng, 3249, -0.99, -0.05), spread(rng, 1500, 0.0001, 0.0002),
                  spread(rng, 3250, 0.05, 0.99), [1.0])
    out.append(PriorCase("descend", x))
    # 2000 ties in the middle of 5000
    x = _shuffled(rng, spread(rng, 1500, -1.0, -0.1), np.full(2000, 0.125), spread(rng, 1500, 0.3, 1.0))
    out.append(PriorCase("ties-2000", x))
    x = _shuffled(rng, spread(rng, 1499, -1.0, -0.1), np.full(2000, 0.125), spread(rng, 1500, 0.3, 1.0))
    out.append(PriorCase("ties-2000-odd", x))
    # a few +-inf residuals (fit = 0 / inf), genes below 100 * min_disp, NaN padding
    x = _snap(rng.uniform(-1.0, 1.0, 8200))
    gw, fit = np.ones(8200), np.exp(-x)
    fit[rng.choice(8200, 5, replace=False)] = 0.0
    fit[rng.choice(8200, 4, replace=False)] = np.inf
    out.append(PriorCase("infinite-residuals", x, gw, fit))
    gw, fit = np.ones(8200), np.exp(-x)
    gw[:3000] = 10.0 ** rng.uniform(-9.0, -6.01, 3000)  # left out
    gw[3000:3100] = 0.0
    fit[:3000] = np.exp(5.0)  # (would move both medians if they entered)
    out.append(PriorCase("below-threshold", x, gw, fit))
    gw, fit = np.ones(8200), np.exp(-x)
    pad = rng.random(8200) < 0.3
    gw[pad], fit[pad] = np.nan, np.nan
    gw[-1000:], fit[-1000:] = np.nan, np.nan
    out.append(PriorCase("nan-padding", x, gw, fit))
    gw = np.full(500, 1e-7)
    gw[::3] = np.nan
    out.append(PriorCase("no-gene-passes", x[:500], gw, np.exp(-x[:500])))
    # the infinity exits of the first median: the middle between -inf and +inf (NaN), inside the +inf / the -inf
    # residuals.  An infinite center makes the deviations of its own residuals inf - inf = NaN: the result is NaN
    fit = np.exp(-x[:2000])
    fit[:1000], fit[1000:] = np.inf, 0.0
    out.append(PriorCase("opposite-infinities", x[:2000], None, fit))
    fit = np.exp(-x[:2001])
    fit[:1001] = 0.0
    out.append(PriorCase("mostly-plus-inf", x[:2001], None, fit))
    fit = np.exp(-x[:2001])
    fit[:1001] = np.inf
    out.append(PriorCase("mostly-minus-inf", x[:2001], None, fit))
    return out
