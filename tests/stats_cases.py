"""Inputs and sort-based fp64 references shared by the tests of the trimmed statistics (csrc/dsq_stats.h): the host
instantiation (tests/test_hostsim.py), the 64-lane device unit (tests/test_devunit_stats.py) and the product kernels
through the C ABI (tests/test_gpu_trimmed_stats.py).

The row generators are those the host tests have always drawn from (same calls on the same random stream); the device
tests add the sizes and ranks at which 64 lanes can go wrong where one lane cannot.  Every reference is numpy.sort +
math.fsum over the kept slice - never a run of the code under test."""
import math

import numpy as np

# ------------------------------------------------------------------------------------------------ row generators
def heavy_ties(rng, n, lo=0, hi=6):
    return rng.integers(lo, hi, n) / 1.37


def mixed_signs(rng, n):
    return rng.normal(0, 1, n) * 10 ** rng.uniform(-3, 6)


def shared_leading_bytes(rng, n):
    return 1000.0 + rng.uniform(0, 1e-9, n)


def all_equal(n):
    return np.full(n, 3.25)


def nb_over_size_factors(rng, n, shift=0.0):
    return rng.negative_binomial(2, 0.01, n) / rng.uniform(0.5, 2, n) + shift


def with_inactive(rng, v, frac=0.3):
    """a float copy of v with a share of the entries turned into the inactive marker (-1: a zero count)"""
    v = np.asarray(v).astype(float)
    v[rng.random(len(v)) < frac] = -1.0
    return v


# ------------------------------------------------------------------------------------------------ shapes and ranks
# below / at / above one, two and four sweeps of the 64 lanes, around the bucket threshold (129) and the gather limit
# (128), rows of several sweeps, and 4097 = 64 * 64 + 1 (one lane makes one trip more than the others)
LANE_N = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4097)
FILLS = (0x00, 0xFF, 0x5A)
K_BUCKETS, K_GATHER = 512, 128  # kBuckets, kBucketGather of dsq_stats.h
U = 2.0 ** -53                  # unit roundoff of fp64


def trim_counts(n):
    return [nt for nt in sorted({0, n // 8, n // 4, n // 3, (n - 1) // 2}) if n - 2 * nt >= 1]


def rank_pairs(m):
    """(j_lo, j_hi) among m active entries: the trimming windows, single ranks, the empty window j_hi = j_lo - 1,
    ranks 0 and m - 1"""
    if m == 0:
        return [(0, -1)]
    out = {(nt, m - nt - 1) for nt in trim_counts(m)}
    out |= {(m // 3, m // 3), (m // 2, m // 2 - 1), (0, 0), (m - 1, m - 1), (0, m - 1)}
    return sorted((a, b) for a, b in out if a >= 0 and b < m and b >= a - 1)


def kept_sum(sorted_vals, a, b):
    return math.fsum(sorted_vals[a:b + 1]) if b >= a else 0.0


def detection_margin(sorted_vals, a, b):
    """What the smallest one-rank mistake costs: moving either end of the kept window [a, b] by one rank in either
    direction adds or drops one of sorted_vals[a - 1], [a], [b], [b + 1] (a tie block miscounted by one: the same, the
    block's value).  The smallest |value| among those that exist."""
    m = len(sorted_vals)
    idx = {i for i in (a - 1, a, b, b + 1) if 0 <= i < m}
    return min(abs(float(sorted_vals[i])) for i in idx) if idx else math.inf


def pos_keys(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def bucket_of(active):
    """bucket_rank_sum's bucket of every value: linear in the bit pattern between the smallest and the largest one"""
    k = pos_keys(active)
    kmin, kmax = int(k.min()), int(k.max())
    shift = 0
    while ((kmax - kmin) >> shift) >= K_BUCKETS:
        shift += 1
    return ((k - np.uint64(kmin)) >> np.uint64(shift)).astype(np.int64)


def bucket_accepts(active, a, b):
    """The rule in bucket_rank_sum's comment: not applicable with a non-finite value or with more than kBucketGather
    values in the bucket of either boundary rank."""
    active = np.asarray(active, dtype=np.float64)
    if len(active) == 0 or b < a:
        return True
    if not np.isfinite(active).all():
        return False
    s = np.sort(active)
    if s[0] == s[-1]:
        return True
    bk = bucket_of(s)
    return bool((bk == bk[a]).sum() <= K_GATHER and (bk == bk[b]).sum() <= K_GATHER)


def away_from_zero(v, margin=0.05):
    """mixed-sign rows for the detection condition: no value within margin * scale of zero (a boundary element of
    negligible size cannot show a one-rank mistake)"""
    s = np.abs(v).max()
    return v + np.where(v < 0, -margin, margin) * s


def _percent_apart(rng, n, base=1.0):
    """n distinct values, neighbours 1 % apart (a one-rank mistake moves a sum by at least a percent of an element),
    in random order"""
    v = base * 1.01 ** np.arange(n)
    rng.shuffle(v)
    return v


def select_rows():
    """(name, values) rows for trimmed_sum_select: the host generators at the lane sizes (negative and mixed signs
    included), plus the lane-specific rows."""
    rng = np.random.default_rng(101)
    rows = []
    for n in LANE_N:
        rows += [(f"ties n={n}", heavy_ties(rng, n, 1, 7)),
                 (f"mixed n={n}", away_from_zero(mixed_signs(rng, n))),
                 (f"negative n={n}", -nb_over_size_factors(rng, n, 1.0)),
                 (f"shared bytes n={n}", shared_leading_bytes(rng, n)),
                 (f"equal n={n}", all_equal(n)),
                 (f"nb n={n}", nb_over_size_factors(rng, n, 1.0))]
        if n <= 1000:  # (1.01^4097 leaves the smallest elements below the resolution of the sum)
            rows.append((f"percent n={n}", _percent_apart(rng, n)))
    return rows


def select_cases():
    """(name, values, nt)"""
    out = [(f"{name} nt={nt}", v, nt) for name, v in select_rows() for nt in trim_counts(len(v))]
    rng = np.random.default_rng(102)
    for n, nt in ((200, 25), (257, 64), (1000, 333)):
        # the boundary order statistics sit where only the last lane looks (k = 63 mod 64)
        v = np.sort(_percent_apart(rng, n))
        lo, hi = v[nt], v[n - nt - 1]
        rest = np.array([x for x in v if x != lo and x != hi])
        rng.shuffle(rest)
        row = np.empty(n)
        pos = np.ones(n, bool)
        pos[[63, 127]] = False
        row[63], row[127] = lo, hi
        row[pos] = rest
        out.append((f"last lane n={n}", row, nt))
        # a block of ties that straddles each boundary rank
        t = np.sort(_percent_apart(rng, n))
        t[nt - 2:nt + 3] = t[nt]
        t[n - nt - 3:n - nt + 2] = t[n - nt - 1]
        rng.shuffle(t)
        out.append((f"tie blocks n={n}", t, nt))
    return out


def rank_rows(accessor):
    """Rows for the rank sums.  accessor = False: (name, buffer of doubles with -1 markers).  True: (name, y, sf) whose
    normalised counts y / sf are the values (a zero count is the inactive marker)."""
    rng = np.random.default_rng(103 + int(accessor))
    rows = []
    for n in LANE_N:
        if not accessor:
            for name, v in ((f"ties n={n}", heavy_ties(rng, n, 1, 7)),
                            (f"nb n={n}", nb_over_size_factors(rng, n, 1e-3)),
                            (f"shared bytes n={n}", shared_leading_bytes(rng, n)),
                            (f"equal n={n}", all_equal(n)),
                            (f"percent n={n}", _percent_apart(rng, min(n, 1000)))):
                if len(v) == n:
                    rows.append((name, with_inactive(rng, v)))
        else:
            off = rng.random((4, n)) < 0.3  # 30 % inactive
            y_t = rng.integers(1, 7, n)
            y_nb = rng.negative_binomial(2, 0.01, n) + 1
            y_sh = (1 << 30) + rng.integers(0, 1024, n)
            y_eq = np.full(n, 13)
            for j, (name, y, sf) in enumerate(((f"ties n={n}", y_t, np.full(n, 1.37)),
                                               (f"nb n={n}", y_nb, rng.uniform(0.5, 2, n)),
                                               (f"shared bytes n={n}", y_sh, np.ones(n)),
                                               (f"equal n={n}", y_eq, np.full(n, 4.0)))):
                rows.append((name, np.where(off[j], 0, y).astype(np.int32), sf))
    return rows


def _active(v):
    v = np.asarray(v, dtype=np.float64)
    return v[v >= 0]


def rank_cases_buffer():
    """(name, buffer, j_lo, j_hi) over a plain buffer: every row x every rank pair, plus the engineered rows."""
    out = []
    for name, v in rank_rows(False):
        for a, b in rank_pairs(len(_active(v))):
            out.append((f"{name} [{a},{b}]", v, a, b))
    rng = np.random.default_rng(105)
    # two boundary ranks in one bucket, and in adjacent buckets (1000 values 1 % apart over 512 buckets)
    v = _percent_apart(rng, 1000)
    s = np.sort(v)
    bk = bucket_of(s)
    same = next(j for j in range(100, 900) if bk[j] == bk[j + 1])
    adj = next(j for j in range(100, 900) if bk[j + 1] == bk[j] + 1)
    out += [("same bucket", v, same, same + 1), ("adjacent buckets", v, adj, adj + 1)]
    for n, a, b in ((200, 25, 174), (257, 64, 192), (1000, 333, 666)):
        s = np.sort(_percent_apart(rng, n))
        row = np.empty(n)
        pos = np.ones(n, bool)
        pos[[63, 127]] = False
        row[63], row[127] = s[a], s[b]
        rest = np.delete(s, [a, b])
        rng.shuffle(rest)
        row[pos] = rest
        out.append((f"last lane n={n}", row, a, b))
        t = np.sort(_percent_apart(rng, n))
        t[a - 2:a + 3] = t[a]
        t[b - 2:b + 3] = t[b]
        rng.shuffle(t)
        out.append((f"tie blocks n={n}", t, a, b))
    # exactly kBucketGather and kBucketGather + 1 values in a boundary bucket: accepted and refused
    for cnt in (K_GATHER, K_GATHER + 1):
        base = 1.01 ** np.arange(60, 260)           # 1.8 ... 13: buckets of ~0.7 % at the low end
        row = np.concatenate([np.full(cnt, 1.5), [1.0], base])
        rng.shuffle(row)
        out.append((f"{cnt} in the lower boundary bucket", row, 40, len(row) - 41))
        row = np.concatenate([np.full(cnt, 1.5), [1.0], base])
        rng.shuffle(row)
        out.append((f"{cnt} in the only boundary bucket", row, 40, 40))
    return out


def nonfinite_cases():
    """rows with a non-finite value, bucket pass without `range`: refused"""
    rng = np.random.default_rng(106)
    out = []
    for bad in (np.inf, np.nan):
        v = _percent_apart(rng, 300)
        v[77] = bad
        out.append((f"{bad} among the values", v, 30, 250))
    return out


def rank_cases_accessor():
    """(name, y, sf, idx or None, tm, squared, j_lo, j_hi) over a NormedValues accessor.  Odd rows go through an index
    list (a permutation of the samples); the squared mode takes the trimming windows of the middle sizes."""
    out = []
    rng = np.random.default_rng(107)
    for r, (name, y, sf) in enumerate(rank_rows(True)):
        n = len(y)
        idx = rng.permutation(n).astype(np.int32) if r % 2 else None
        m = int((y != 0).sum())
        for a, b in rank_pairs(m):
            out.append((f"{name} [{a},{b}]", y, sf, idx, 0.0, False, a, b))
        if n in (65, 129, 257, 1000) and m >= 8 and not name.startswith(("equal", "shared")):
            v = np.sort(y[y != 0] / sf[y != 0])
            tm = float(np.round(v[(3 * m) // 10], 1))  # a short decimal near the 30 % quantile: (v - tm)^2 is not monotone
            for nt in (m // 8, m // 4, m // 3):
                out.append((f"{name} squared nt={nt}", y, sf, idx, tm, True, nt, m - nt - 1))
    # the engineered rows of the plain buffer over the accessor too (the buffer-less kernels' real input): counts
    # round(1024 v) over a size factor of 1024 - the order, the ties and the positions stay, the quotient is exact
    for name, v, a, b in rank_cases_buffer():
        if name.startswith(("last lane", "tie blocks", "128 in", "129 in")):
            y = np.round(np.asarray(v) * 1024).astype(np.int32)
            idx = rng.permutation(len(y)).astype(np.int32) if name.startswith("tie blocks") else None
            out.append((f"{name} (accessor)", y, np.full(len(y), 1024.0), idx, 0.0, False, a, b))
    return out


def accessor_values(y, sf, tm, squared):
    """the fp64 values the accessor stands for (IEEE division), active entries only, sorted; and v itself"""
    y = np.asarray(y)
    v = y[y != 0] / np.asarray(sf, dtype=np.float64)[y != 0]
    q = (v - tm) ** 2 if squared else v
    return np.sort(q), v


def accessor_tolerance(y, sf, tm, squared):
    """Bound on |device sum - reference| over an accessor.  The device forms y * frcp_g(sf): frcp_g is within 1 ulp
    (<= 2 u relative, u = 2^-53) of 1 / sf, the product rounds once more (u), and the reference's own y / sf carries u:
    every value is within delta = 4 u relative of the reference's.  Plain mode: the sum moves by at most
    delta * sum|v|; adding n terms in any order costs at most (n - 1) u sum|v|: (n + 3) u sum|v| <= 4.6e-13 sum|v| at
    n = 4097 - inside the 1e-12 sum|v| the host instantiation is held to, which therefore stays the bound.
    Squared mode: q = (v - tm)^2 moves by at most 2 |v - tm| |v| delta (+ second order) per value, which does not scale
    with q itself, so that term is added to 1e-12 sum q."""
    q, v = accessor_values(y, sf, tm, squared)
    tol = 1e-12 * max(1.0, float(np.abs(q).sum()))
    if squared:
        tol += 2.0 * (4 * U) * float((np.abs(v - tm) * np.abs(v)).sum()) * 1.01
    return tol


# ------------------------------------------------------------------------------------------------ sorter
def sort_rows():
    rng = np.random.default_rng(108)
    rows = []
    for n in list(range(1, 131)) + [255, 256, 257, 1000, 4096, 8191]:
        kind = n % 5
        if kind == 0:
            v = rng.normal(0, 1, n) * 10.0 ** rng.integers(-8, 8, n)
        elif kind == 1:
            v = rng.integers(-3, 4, n).astype(float)      # duplicates (no -0.0: its place among the zeros is not defined)
        elif kind == 2:
            v = np.sort(rng.normal(0, 1, n))               # already sorted
        elif kind == 3:
            v = np.sort(rng.normal(0, 1, n))[::-1].copy()  # reversed
        else:
            v = rng.normal(0, 1, n)
        if n >= 3 and n % 3 == 0:                          # NaNs and both infinities, anywhere
            pos = rng.choice(n, min(n, 3 + n // 50), replace=False)
            v[pos] = rng.choice([np.nan, np.inf, -np.inf], len(pos))
        rows.append(np.ascontiguousarray(v, dtype=np.float64))
    rows.append(np.full(70, np.nan))
    return rows


def sort_merge_rows():
    """rows for robust_disp_gene's sequence (sort, squared errors around the sorted row's element n // 3, merge), most
    of them with a few NaNs: they sort last, stay NaN when squared and must still be the row's last elements after the
    merge"""
    rng = np.random.default_rng(111)
    rows = []
    for n in list(range(3, 131)) + [255, 256, 257, 1000, 4096, 8191]:
        v = rng.gamma(2.0, 50.0, n)
        if n % 4:
            v[rng.choice(n, max(1, n // 8), replace=False)] = np.nan
        rows.append(v)
    return rows


def sort_merge_reference(v):
    s = np.sort(v)
    return np.sort((s - s[len(s) // 3]) ** 2)


def merge_rows():
    """decreasing-then-increasing rows: the squared errors of an ascending row around a value inside it, as
    robust_disp_gene hands them to LdsSorter::merge"""
    rng = np.random.default_rng(109)
    rows = []
    for n in list(range(1, 131)) + [255, 256, 257, 1000, 4096, 8191]:
        v = np.sort(rng.gamma(2.0, 50.0, n))
        if n % 4 == 1:
            v = np.floor(v)  # ties
        tm = float(v[n // 3]) if n % 7 else float(v[0]) - 1.0  # (every seventh: monotone - the turning point at the edge)
        rows.append(((v - tm) ** 2).astype(np.float64))
    return rows


# ------------------------------------------------------------------------------------------------ Cook's bookkeeping
def cooks_model(y, mu, hat, flags, ar, cutoff, P):
    """CooksAcc in plain Python over 80-bit reals: per-sample Cook's distances, the flags of dds.py:1066-1110 and the
    np.argmax winner (first NaN, else first maximum).  flags: bit 0 use_for_max, bit 1 replaceable."""
    ld = np.longdouble
    y_, mu_, h_ = np.asarray(y, ld), np.asarray(mu, ld), np.asarray(hat, ld)
    with np.errstate(all="ignore"):
        V = mu_ + ld(ar) * mu_ * mu_
        ck = (y_ - mu_) ** 2 / V / ld(P) * (h_ / (1 - h_) ** 2)
    best, nan_at = None, None
    for i in range(len(ck)):  # np.argmax semantics, spelled out
        if ck[i] != ck[i]:
            nan_at = i
            break
        if best is None or ck[i] > ck[best]:
            best = i
    win = nan_at if nan_at is not None else best
    gt = np.array([bool(c > cutoff) for c in ck])
    use, repl = (np.asarray(flags) & 1) != 0, (np.asarray(flags) & 2) != 0
    above = int((np.asarray(y) > np.asarray(y)[win]).sum())
    return dict(ck=ck, any_all=int(gt.any()), any_use=int((gt & use).any()), any_use_nr=int((gt & use & ~repl).any()),
                few_above=int(above < 3), win=int(win), above=above)


# (r^2 invP h) * frcp_g(V (1-h)^2), V = mu^2 ar + mu: roundings, each <= u relative (no cancellation: every sum has
# positive terms; y, mu, h are the exact inputs).  V: mu*mu, *ar, +mu = 3 u.  r = y - mu: u; r*r: 2 u + u = 3 u;
# invP = 1/P: u, the product: u -> 5 u; * h: u -> 6 u.  omh = 1 - h: u; omh^2: 3 u; V * omh^2: 3 + 3 + 1 = 7 u;
# frcp_g: 1 ulp <= 2 u -> 9 u; the last product: u.  6 + 9 + 1 = 16 u; contracted fmas only remove roundings.  17 u
# covers the second-order terms.
COOKS_REL = 17 * U


def cooks_cases():
    """(name, y, mu, hat, flags, ar, cutoff, P): per-sample values are built from a target Cook's distance so that ties,
    NaNs and the cutoff fall where each case wants them."""
    rng = np.random.default_rng(110)
    P, ar, cutoff = 3, 0.1, 4.0
    out = []

    def base(N, top=2.0):
        mu = np.exp(rng.uniform(1.5, 6, N))
        hat = rng.uniform(0.02, 0.4, N)
        y = np.maximum(rng.poisson(mu), 1).astype(np.int64)
        # raise or lower every sample's distance below `top` by moving the hat value only (y, mu stay a count and a mean)
        m = cooks_model(y, mu, hat, np.ones(N, np.uint8), ar, 1e300, P)
        big = np.asarray(m["ck"], float) >= top
        hat[big] = 1e-4
        return y, mu, hat

    def plant(y, mu, hat, i, yv, mv, hv):
        y[i], mu[i], hat[i] = yv, mv, hv

    for N in (1, 63, 64, 65, 200):
        y, mu, hat = base(N, top=math.inf)
        fl = rng.integers(0, 4, N).astype(np.uint8)
        out.append((f"random N={N}", y, mu, hat, fl, ar, 0.02, P))  # (a cutoff that a share of plain samples passes)
    # the maximum tied between two lanes (samples 70 and 5: the smaller index wins) and between two trips of one lane
    # (samples 7 and 71 = 7 + 64)
    for name, i, j in (("tie between lanes", 70, 5), ("tie between trips", 7, 71)):
        y, mu, hat = base(200)
        for k in (i, j):
            plant(y, mu, hat, k, 900, 100.0, 0.3)
        out.append((name, y, mu, hat, np.full(200, 1, np.uint8), ar, cutoff, P))
    # NaNs in several lanes (hat = NaN): the smallest index wins - also over a larger finite value
    y, mu, hat = base(200)
    hat[[150, 33, 97, 161]] = np.nan
    plant(y, mu, hat, 12, 5000, 50.0, 0.5)
    out.append(("NaNs in several lanes", y, mu, hat, np.full(200, 3, np.uint8), ar, cutoff, P))
    y, mu, hat = base(65)
    hat[64] = np.nan
    plant(y, mu, hat, 3, 5000, 50.0, 0.5)
    out.append(("NaN and a larger finite value", y, mu, hat, np.full(65, 1, np.uint8), ar, cutoff, P))
    # all below the cutoff
    y, mu, hat = base(200)
    out.append(("all below the cutoff", y, mu, hat, np.full(200, 3, np.uint8), ar, cutoff, P))
    # flags that separate the three any_gt: the only sample above the cutoff is (a) not use_for_max, (b) use_for_max and
    # replaceable, (c) use_for_max and not replaceable
    for name, f in (("above: not used", 0), ("above: used, replaceable", 3), ("above: used, not replaceable", 1),
                    ("above: replaceable only", 2)):
        y, mu, hat = base(130)
        plant(y, mu, hat, 99, 3000, 60.0, 0.4)
        fl = np.full(130, 1, np.uint8)
        fl[99] = f
        out.append((name, y, mu, hat, fl, ar, cutoff, P))
    # few_above flips between 2 and 3 samples whose count is above the winner's
    for k in (2, 3):
        y, mu, hat = base(200)
        y[:] = np.minimum(y, 400)
        plant(y, mu, hat, 140, 500, 20.0, 0.45)          # the winner: count 500
        for i in (3, 64, 199)[:k]:
            plant(y, mu, hat, i, 100000, 100000.0, 0.01)  # larger counts on their mean: no distance
        out.append((f"{k} samples above the winner", y, mu, hat, np.full(200, 1, np.uint8), ar, cutoff, P))
    return out


# ------------------------------------------------------------------------------------------------ batched cells
def seg_reference(y, sf, sizes):
    """scaled trimmed variance of every cell (cells laid out one after the other, `sizes` samples each)"""
    ratios, scales = (1 / 3, 1 / 4, 1 / 8), (2.04, 1.86, 1.51)
    out, beg = [], 0
    for n in sizes:
        v = np.sort(np.asarray(y[beg:beg + n], dtype=np.float64) / sf[beg:beg + n])
        cls = 2 if n >= 24 else (1 if n >= 4 else 0)
        nt = math.floor(n * ratios[cls])
        # (numpy.sort puts NaNs last: up to nt of them are trimmed away, one more makes the result NaN)
        tm = math.fsum(v[nt:n - nt]) / (n - 2 * nt)
        q = np.sort((v - tm) ** 2)
        out.append(scales[cls] * (math.fsum(q[nt:n - nt]) / (n - 2 * nt)))
        beg += n
    return np.array(out)
