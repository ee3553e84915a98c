"""The trimmed statistics and the Cook's bookkeeping of csrc/dsq_stats.h, and the LDS sorter of csrc/dsq_lds_sort.h, built
for the device with 64 lanes (tests/devunit/devunit_stats.hip) - against numpy.sort + math.fsum.

tests/test_hostsim.py holds the same routines to the same references with one lane.  What only 64 lanes have is checked
here: histogram bins split over the lanes and found again by a prefix scan, barriers between the LDS passes, boundary
buckets filled in atomic order, -inf defaults reduced over lanes that saw nothing, 128 elements of a batch spread over
64 lanes, the sorter's index arithmetic beyond 128 elements, the cross-lane argmax.  Every device result is computed
three times, on LDS pre-filled with 0x00, 0xFF and 0x5A, and must be the same bits each time.

The tests not marked `gpu` check the inputs: that every case can show a one-rank mistake (see detection_margin), and
that the engineered rows are what their names say."""
import math

import numpy as np
import pytest

from tests import stats_cases as sc
from tests.helpers import assert_close

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def du():
    from tests import devunit

    devunit.lib()
    return devunit


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def three_fills(run):
    """run(fill) on the three LDS fills: identical bits required; the first result"""
    ref = run(sc.FILLS[0])
    for fill in sc.FILLS[1:]:
        got = run(fill)
        for i, (a, b) in enumerate(zip(ref, got)):
            assert same_bits(a, b), f"output {i} depends on the LDS contents (fill {fill:#x})"
    return ref


def sum_tol(values):
    """the host instantiation's bound (tests/test_hostsim.py): 1e-12 of sum|v|.  64 partial sums reorder the additions
    without loosening it: any order of n additions is within (n - 1) u sum|v| = 4.6e-13 sum|v| at n = 4097."""
    return 1e-12 * max(1.0, float(np.abs(values).sum()))


# ------------------------------------------------------------------------------------------------ the inputs (CPU)
def test_every_selection_case_shows_a_one_rank_mistake():
    for name, v, nt in sc.select_cases():
        s, n = np.sort(v), len(v)
        assert sc.detection_margin(s, nt, n - nt - 1) >= 1000 * sum_tol(v), name


def test_every_rank_sum_case_shows_a_one_rank_mistake():
    for name, v, a, b in sc.rank_cases_buffer():
        act = np.sort(v[v >= 0])
        assert sc.detection_margin(act, a, b) >= 1000 * sum_tol(act), name
    for name, y, sf, idx, tm, squared, a, b in sc.rank_cases_accessor():
        q, _ = sc.accessor_values(y, sf, tm, squared)
        assert sc.detection_margin(q, a, b) >= 1000 * sc.accessor_tolerance(y, sf, tm, squared), name


def test_engineered_rows_are_what_their_names_say():
    cases = {name: (v, a, b) for name, v, a, b in sc.rank_cases_buffer()}
    v, a, b = cases["same bucket"]
    bk = sc.bucket_of(np.sort(v))
    assert bk[a] == bk[b] and b == a + 1
    v, a, b = cases["adjacent buckets"]
    bk = sc.bucket_of(np.sort(v))
    assert bk[b] == bk[a] + 1
    for cnt, accepted in ((128, True), (129, False)):
        for kind in ("lower", "only"):
            v, a, b = cases[f"{cnt} in the {kind} boundary bucket"]
            s = np.sort(v)
            bk = sc.bucket_of(s)
            assert (bk == bk[a]).sum() == cnt and (bk[b] == bk[a] or (bk == bk[b]).sum() <= 128)  # exactly cnt, no other cause
            assert sc.bucket_accepts(v, a, b) == accepted
    for name, (v, a, b) in cases.items():
        if name.startswith("last lane"):
            s = np.sort(v)
            assert v[63] == s[a] and v[127] == s[b] and (v == s[a]).sum() == 1 and (v == s[b]).sum() == 1
        if name.startswith("tie blocks"):
            s = np.sort(v)
            assert s[a - 2] == s[a + 2] and s[b - 2] == s[b + 2] and s[a - 3] < s[a] < s[a + 3]
    for name, v, nt in sc.select_cases():
        if name.startswith("last lane"):
            s = np.sort(v)
            assert v[63] == s[nt] and v[127] == s[len(v) - nt - 1]
        if name.startswith("tie blocks"):
            s, n = np.sort(v), len(v)
            assert s[nt - 2] == s[nt + 2] and s[n - nt - 3] == s[n - nt + 1]
    for name, y, sf, idx, tm, sq, a, b in sc.rank_cases_accessor():  # the same rows over the accessor
        if not name.endswith("(accessor)"):
            continue
        q, _ = sc.accessor_values(y, sf, tm, sq)
        if name.startswith("last lane"):
            assert y[63] / sf[63] == q[a] and y[127] / sf[127] == q[b] and (q == q[a]).sum() == 1 and (q == q[b]).sum() == 1
        if name.startswith("tie blocks"):
            assert q[a - 2] == q[a + 2] and q[b - 2] == q[b + 2] and q[a - 3] < q[a] < q[a + 3]
        if name[:3] in ("128", "129"):
            bk = sc.bucket_of(q)
            assert (bk == bk[a]).sum() == int(name[:3]) and (bk[b] == bk[a] or (bk == bk[b]).sum() <= 128)
    assert sum(n.endswith("(accessor)") for n, *_ in sc.rank_cases_accessor()) == 3 + 3 + 4
    # both outcomes of the bucket pass occur among the plain rows too
    acc = [sc.bucket_accepts(v[v >= 0], a, b) for _, v, a, b in sc.rank_cases_buffer()]
    assert sum(acc) >= 100 and len(acc) - sum(acc) >= 10


def test_cooks_cases_are_decided_beyond_rounding():
    """every distance is far from the cutoff and every winner far ahead of (or exactly tied with) the runner-up, so the
    17 u of the reciprocal form cannot move a flag or the argmax; the cases do what their names say"""
    seen = {}
    for name, y, mu, hat, fl, ar, cutoff, P in sc.cooks_cases():
        m = sc.cooks_model(y, mu, hat, fl, ar, cutoff, P)
        ck = np.asarray(m["ck"], float)
        fin = ck[~np.isnan(ck)]
        assert (np.abs(fin / cutoff - 1.0) > 1e-9).all(), name
        if not np.isnan(ck).any() and len(fin) > 1:
            top = np.sort(fin)[-2:]
            assert top[1] == top[0] or top[1] > top[0] * (1 + 1e-9), name
        seen[name] = m
    assert seen["tie between lanes"]["win"] == 5 and seen["tie between trips"]["win"] == 7
    assert seen["NaNs in several lanes"]["win"] == 33 and seen["NaN and a larger finite value"]["win"] == 64
    assert seen["all below the cutoff"]["any_all"] == 0
    assert [seen[f"above: {k}"][f] for k in ("not used", "used, replaceable", "used, not replaceable")
            for f in ("any_all", "any_use", "any_use_nr")] == [1, 0, 0, 1, 1, 0, 1, 1, 1]
    assert seen["2 samples above the winner"]["few_above"] == 1 and seen["2 samples above the winner"]["above"] == 2
    assert seen["3 samples above the winner"]["few_above"] == 0 and seen["3 samples above the winner"]["above"] == 3


# ------------------------------------------------------------------------------------------------ LdsSorter
@gpu
def test_sorter_equals_numpy_sort_bit_for_bit(du):
    rows = sc.sort_rows()
    (got,) = three_fills(lambda fill: (np.concatenate(du.lds_sort(rows, fill)),))
    want = np.concatenate([np.sort(r) for r in rows])
    # (any NaN is a NaN: the payload is the input's, and all inputs carry numpy's)
    assert same_bits(got, want), [len(r) for r, g in zip(rows, du.lds_sort(rows)) if not same_bits(g, np.sort(r))]


@gpu
def test_merge_sorts_a_decreasing_then_increasing_row(du):
    rows = sc.merge_rows()
    (got,) = three_fills(lambda fill: (np.concatenate(du.lds_sort(rows, fill, merge=True)),))
    assert same_bits(got, np.concatenate([np.sort(r) for r in rows]))


@gpu
def test_sort_then_merge_keeps_the_rows_nans_last(du):
    """the sequence robust_disp_gene runs on a sorted cell, on the device, with NaNs inside the row: the merge works on
    the tail that the sort itself left behind the row"""
    rows = sc.sort_merge_rows()
    (got,) = three_fills(lambda fill: (np.concatenate(du.lds_sort(rows, fill, merge="after sort")),))
    assert same_bits(got, np.concatenate([sc.sort_merge_reference(r) for r in rows]))


# ------------------------------------------------------------------------------------------------ selection, rank sums
@gpu
def test_trimmed_sum_select_against_the_sorted_slice(du):
    cases = sc.select_cases()
    rows, nts = [c[1] for c in cases], [c[2] for c in cases]
    (got,) = three_fills(lambda fill: (du.trimmed_select(rows, nts, fill),))
    for (name, v, nt), g in zip(cases, got):
        ref = sc.kept_sum(np.sort(v), nt, len(v) - nt - 1)
        assert abs(g - ref) <= sum_tol(v), (name, g, ref)


def _check_rank(cases_out, select):
    for name, act, a, b, tol, g, ok in cases_out:
        if select:
            assert ok == 1
        else:
            assert ok == int(sc.bucket_accepts(act, a, b)), (name, ok)
        if ok:
            ref = sc.kept_sum(np.sort(act), a, b)
            assert abs(g - ref) <= tol, (name, g, ref, tol)


@gpu
@pytest.mark.parametrize("use_range", [False, True])
def test_bucket_rank_sum_over_a_buffer(du, use_range):
    cases = sc.rank_cases_buffer()
    probs = [dict(v=v, j_lo=a, j_hi=b) for _, v, a, b in cases]
    got, ok = three_fills(lambda fill: du.rank_sum(probs, False, use_range, fill))
    _check_rank([(name, v[v >= 0], a, b, sum_tol(v[v >= 0]), g, o) for (name, v, a, b), g, o in zip(cases, got, ok)],
                False)
    assert 0 < ok.sum() < len(ok)


@gpu
def test_bucket_rank_sum_refuses_non_finite_values_without_a_range(du):
    cases = sc.nonfinite_cases()
    probs = [dict(v=v, j_lo=a, j_hi=b) for _, v, a, b in cases]
    got, ok = three_fills(lambda fill: du.rank_sum(probs, False, False, fill))
    assert (ok == 0).all()


@gpu
def test_select_rank_sum_over_a_buffer(du):
    cases = sc.rank_cases_buffer()
    probs = [dict(v=v, j_lo=a, j_hi=b) for _, v, a, b in cases]
    got, ok = three_fills(lambda fill: du.rank_sum(probs, True, True, fill))
    _check_rank([(name, v[v >= 0], a, b, sum_tol(v[v >= 0]), g, o) for (name, v, a, b), g, o in zip(cases, got, ok)],
                True)


@gpu
@pytest.mark.parametrize("select", [False, True])
def test_rank_sums_over_the_normalised_count_accessor(du, select):
    """NormedValues (y * frcp_g(sf), optional index list, squared errors around tm), bucket pass with the range and
    selection: the tolerance is derived in stats_cases.accessor_tolerance."""
    cases = sc.rank_cases_accessor()
    probs = [dict(y=y, sf=sf, idx=idx, tm=tm, squared=sq, j_lo=a, j_hi=b) for _, y, sf, idx, tm, sq, a, b in cases]
    got, ok = three_fills(lambda fill: du.rank_sum(probs, select, True, fill))
    out = []
    for (name, y, sf, idx, tm, sq, a, b), g, o in zip(cases, got, ok):
        q, _ = sc.accessor_values(y, sf, tm, sq)
        out.append((name, q, a, b, sc.accessor_tolerance(y, sf, tm, sq), g, o))
    _check_rank(out, select)
    if not select:  # the bucket pass without a range finds the same range itself
        got2, ok2 = du.rank_sum(probs, False, False)
        assert same_bits(got2[ok == 1], got[ok == 1]) and same_bits(ok2, ok)


# ------------------------------------------------------------------------------------------------ batched cells
def _seg_case(L, nan_cell=None):
    """2 * (128 / L) - 1 cells (the last pass partly filled) of 3 ... L samples mixed (L = 2: 1 ... 2 - a segment of
    two holds no more), scattered over the samples; gene 0 all zero, gene 1 constant on cell 1 (equal size factors
    there), the others negative binomial over a wide range of means."""
    rng = np.random.default_rng(200 + L)
    per = 128 // L
    nc = 2 * per - 1
    lo = min(3, L - 1) if L > 2 else 1
    sizes = rng.integers(lo, L + 1, nc)
    sizes[0], sizes[-1] = L, lo
    N = int(sizes.sum()) + 5
    index = rng.permutation(N)[: sizes.sum()]
    sf = np.exp(rng.normal(0, 0.3, N))
    beg = np.concatenate([[0], np.cumsum(sizes)])
    sf[index[beg[1]:beg[2]]] = 1.0
    G = 6
    mean = np.exp(rng.uniform(np.log(0.5), np.log(3000), G))
    y = rng.negative_binomial(2.0, 2.0 / (2.0 + mean[:, None] * sf[None, :])).astype(np.int32)
    y[0] = 0
    y[1] = 9
    if nan_cell is not None:  # one NaN more than the cell's trim count: numpy.sort puts them last, one stays in the kept slice
        n = int(sizes[nan_cell])
        nt = math.floor(n * (1 / 8 if n >= 24 else (1 / 4 if n >= 4 else 1 / 3)))
        sf[index[beg[nan_cell]:beg[nan_cell] + nt + 1]] = np.nan
    return y, sf, sizes, index


@gpu
@pytest.mark.parametrize("L", [2, 4, 8, 16, 32, 64])
def test_batched_cells_give_every_cells_trimmed_variance(du, L):
    for nan_cell in (None, 2):
        y, sf, sizes, index = _seg_case(L, nan_cell)
        cells, rest = three_fills(lambda fill: du.seg_variances(y, sf, sizes, index, L, fill))
        ref = np.array([sc.seg_reference(yg[index], sf[index], sizes) for yg in y])
        assert (rest == -np.inf).all()           # lanes without a cell, and cells beyond the last one
        if nan_cell is not None:
            assert np.isnan(ref[:, nan_cell]).all() and np.isnan(ref).sum() == len(y)  # only that lane's result is NaN
        assert_close(cells, ref, 1e-11, 0.0, f"batched cells L={L}")
        assert (cells[0] == 0.0)[~np.isnan(ref[0])].all() and (cells[1, 1] == 0.0 or nan_cell == 1)


# ------------------------------------------------------------------------------------------------ CooksAcc
@gpu
@pytest.mark.parametrize("counted", [False, True])
def test_cooks_bookkeeping_against_the_python_model(du, counted):
    for name, y, mu, hat, fl, ar, cutoff, P in sc.cooks_cases():
        m = sc.cooks_model(y, mu, hat, fl, ar, cutoff, P)
        ck, io = three_fills(lambda fill: du.cooks_acc(y[None, :], mu[None, :], hat[None, :], fl, ar, cutoff, P,
                                                       counted, fill))
        want = [m["any_all"], m["any_use"], m["any_use_nr"], m["few_above"], m["win"], int(y[m["win"]])]
        assert io[0].tolist() == want, (name, io[0].tolist(), want)
        ref = np.asarray(m["ck"], np.longdouble)
        nan = np.isnan(np.asarray(ref, float))
        assert (np.isnan(ck[0]) == nan).all(), name
        # |ck - ref| <= 17 u |ref|: the derivation stands next to stats_cases.COOKS_REL
        err = np.abs(ck[0][~nan].astype(np.longdouble) - ref[~nan])
        assert (err <= sc.COOKS_REL * np.abs(ref[~nan])).all(), (name, float(np.max(err / np.abs(ref[~nan]))))
