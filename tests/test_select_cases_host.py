"""CPU checks of tests/select_cases.py: the path model of block_median_values gives numpy's median bit for bit on every
crafted case, every branch of the selection is reached by a named case (and the data of the existing size-factor test
reach two of them), the value grid holds, and the table entry that makes a count of 1 contribute exactly -logmean is 0."""
import math

import mpmath
import numpy as np
import pytest

from tests import select_cases as sc

VALUE_CASES = sc.value_cases() + sc.big_value_cases()
RADIX_CASES = sc.radix_cases()
PRIOR_CASES = sc.prior_cases() + [sc.prior_size_case(n) for n in sc.PRIOR_SIZES]


def _paths(case, mode=None):
    out = []
    for n in range(case.N):
        v = case.values_seen(n, mode)
        med, tags = sc.model_median(v)
        out.append((med, tags, sc.ref_median(v)))
    return out


@pytest.mark.parametrize("case", VALUE_CASES + RADIX_CASES, ids=lambda c: c.name)
def test_model_is_numpys_median_bit_for_bit(case):
    for mode in ("default", "new"):
        for n, (med, tags, ref) in enumerate(_paths(case, mode)):
            assert sc.same_bits(med, ref), (case.name, mode, n, tags, med, ref)


@pytest.mark.parametrize("case", PRIOR_CASES, ids=lambda c: c.name)
def test_model_is_numpys_median_on_the_prior_residuals(case):
    res = case.residuals()
    c, _ = sc.model_median(res)
    assert sc.same_bits(c, sc.ref_median(res))
    with np.errstate(invalid="ignore"):
        dev = np.abs(res - c)
    m, _ = sc.model_median(dev)
    assert sc.same_bits(m, sc.ref_median(dev))
    ref = case.reference()
    assert np.isnan(ref) if not np.isfinite(c) else sc.same_bits((m / 0.67448975019608171) ** 2, ref)


@pytest.mark.parametrize("case", VALUE_CASES, ids=lambda c: c.name)
def test_named_case_takes_its_branch(case):
    got = [tags for _, tags, _ in _paths(case)]
    for n, want in enumerate(case.expect):
        if want is not None:
            assert got[n] == want, (case.name, n, got[n], want)


def _tags_by_case():
    by = {c.name: [tags for _, tags, _ in _paths(c)] for c in VALUE_CASES}
    for p in sc.prior_cases():
        by["prior:" + p.name] = list(p.paths())
    return by


def test_every_branch_is_reached_by_a_named_case():
    by = _tags_by_case()
    reached = {t for paths in by.values() for tags in paths for t in tags}
    assert reached == set(sc.ALL_TAGS), set(sc.ALL_TAGS) ^ reached

    def some(name, pred):
        return any(pred(tags) for tags in by[name])

    def every(name, pred):
        return all(pred(tags) for tags in by[name])

    # one descent, two descents, descents that end in lo == hi - in every sample of the case, at odd and even M
    assert every("descend1", lambda t: t[:-1] == ["descend"] and t[-1].startswith("hist-"))
    assert every("descend2", lambda t: t[:-1] == ["descend", "descend"] and t[-1].startswith("hist-"))
    assert every("descend-collapse", lambda t: t.count("descend") >= 3 and t[-1] == "collapse")
    # deep / two bins by ties and by clusters that are no ties
    assert some("deep-two-ties", lambda t: t == ["deep-two-bins"])
    assert some("deep-two-clusters", lambda t: t == ["deep-two-bins"])
    assert np.unique(sc.case_deep_two_clusters().pool).size == 4000
    # -inf at the low end: half (low0) with a ranking and with a histogram, more than half, fewer
    assert some("low-even", lambda t: t == ["low0", "hist-same"]) and some("low-even-direct", lambda t: t == ["low0", "direct"])
    for name in ("low-even", "low-odd", "low-even-direct", "low-odd-direct"):
        assert some(name, lambda t: t == ["all-low"]) and some(name, lambda t: t[0] not in ("low0", "all-low"))
    # the prior's medians: both through deep / two bins; one through a descent; ties above 1024; the infinity exits
    assert by["prior:both-deep-two-bins"] == [["deep-two-bins"], ["deep-two-bins"]]
    assert by["prior:descend"][0][0] == "descend"
    assert by["prior:ties-2000"][0] == ["descend", "collapse"] and by["prior:ties-2000-odd"][0] == ["descend", "collapse"]
    assert by["prior:opposite-infinities"][0] == ["nan"]
    assert by["prior:mostly-plus-inf"][0] == ["high"] and by["prior:mostly-minus-inf"][0] == ["all-low"]
    assert by["prior:no-gene-passes"] == [["empty"], ["empty"]]


def test_odd_and_even_counts_in_the_branches_that_allow_both():
    """(deep / two bins, one level / two bins and low0 need two different middle ranks: even M only)"""
    seen = {}
    for c in VALUE_CASES:
        for n in range(c.N):
            v = c.values_seen(n)
            M = int(np.sum(~np.isnan(v)))
            _, tags = sc.model_median(v)
            for t in set(tags):
                seen.setdefault(t, set()).add(M % 2)
    for t in ("equal", "direct", "hist-same", "descend", "collapse", "all-low"):
        assert seen[t] == {0, 1}, (t, seen[t])
    for t in ("hist-two", "deep-two-bins", "low0"):
        assert seen[t] == {0}, (t, seen[t])


@pytest.mark.parametrize("G,N,zero_frac", [(3000, 7, 0.0), (32768, 5, 0.0), (32769, 5, 0.0), (50000, 6, 0.0),
                                           (50000, 9, 0.5)])
def test_the_existing_size_factor_data_reach_two_branches(G, N, zero_frac):
    """the gap: the data of test_size_factors_register_and_key_matrix_paths (same generator, same seeds), the usable
    genes through the model - the first sample reaches nothing but `direct` / `hist-same`, and no sample anything beyond
    one histogram level (an even sample whose middle values straddle a bin edge is `hist-two`)"""
    rng = np.random.default_rng(G + N)
    counts = rng.poisson(rng.gamma(2.0, 20.0, G)[None, :] * rng.uniform(0.5, 2.0, N)[:, None]).astype(np.int64) + 1
    zero_genes = rng.random(G) < zero_frac
    counts[rng.integers(0, N, G)[zero_genes], np.nonzero(zero_genes)[0]] = 0
    usable = (counts > 0).all(axis=0)
    logc = np.log(counts[:, usable].astype(np.float64))
    ratios = logc - logc.mean(axis=0)
    reached = set()
    for n in range(N):
        med, tags = sc.model_median(ratios[n])
        assert sc.same_bits(med, sc.ref_median(ratios[n]))
        reached |= set(tags)
        if n == 0:
            assert set(tags) <= {"direct", "hist-same"}, tags
    assert reached <= {"direct", "hist-same", "hist-two"}, reached


def _near_middle(v, width=3):
    """the distinct finite values within `width` ranks of the two middle ranks"""
    v = np.sort(v[~np.isnan(v)])
    if v.size == 0:
        return v
    r0, r1 = (v.size - 1) // 2, v.size // 2
    w = v[max(r0 - width, 0):r1 + width + 1]
    return np.unique(w[np.isfinite(w)])


@pytest.mark.parametrize("case", VALUE_CASES + RADIX_CASES, ids=lambda c: c.name)
def test_value_grid_and_spacing(case):
    if case.grid:
        assert case.counts is None
        assert (np.abs(case.pool) <= 16.0).all()
        assert (case.pool / sc.GRID == np.round(case.pool / sc.GRID)).all()
        if case.decoys is not None:
            assert (case.decoys / sc.GRID == np.round(case.decoys / sc.GRID)).all()
    gap = sc.SPACING if case.grid else 1e-9
    for mode in ("default", "new"):
        for n in range(case.N):
            w = _near_middle(case.values_seen(n, mode))
            if case.name.startswith("radix-last9"):
                # its point: the neighbours of the middle values agree in the top 55 bits
                if w.size > 1 and n != 4:
                    for side in (w[w < 0], w[w > 0]):
                        assert (side.view(np.uint64) >> np.uint64(9)).max() - (side.view(np.uint64) >> np.uint64(9)).min() <= 1
                continue
            assert w.size < 2 or np.diff(w).min() >= gap, (case.name, mode, n, np.diff(w).min())


@pytest.mark.parametrize("case", RADIX_CASES, ids=lambda c: c.name)
def test_radix_cases_have_their_conditions(case):
    assert case.Gu > 32768
    parities = set()
    opposite = 0
    for n in range(case.N):
        v = case.values_seen(n)
        v = np.sort(v[~np.isnan(v)])
        parities.add(v.size % 2 if v.size else None)
        if v.size and v.size % 2 == 0:
            a, b = v[v.size // 2 - 1], v[v.size // 2]
            opposite += bool(a < 0 < b)
    if "equal" not in case.name and not (case.mode == "new" and case.Gu % 2):  # (new samples: M = Gu in every sample)
        assert opposite >= 1, case.name
    if case.mode == "default":
        assert {0, 1, None} <= parities, (case.name, parities)  # even, odd and a sample with M = 0
    # a size on either parity for the new-samples entry point, where M is the number of usable genes
    assert {c.Gu % 2 for c in RADIX_CASES if c.name.startswith("radix-low")} == {0, 1}
    if case.name.startswith("radix-low"):
        v = [case.values_seen(n) for n in range(case.N)]
        assert any(np.isneginf(x).sum() * 2 > x.size for x in v) and any(np.isneginf(x).all() for x in v)


def test_layout_is_the_case():
    """layout() puts exactly the case's values in front of the selection: usable genes, counts and mask recombine to
    values_seen(), in both entry points, with the decoys masked out"""
    for case in (sc.case_hist_two(), sc.case_mask_middle(), sc.case_flog("flog", 2 ** 31 // 5, ("int32",)),
                 sc.case_no_usable()):
        for with_mask in (False, True):
            if case.mask_only and not with_mask:
                continue
            counts, lm, mask = sc.layout(case, case.Gu + 300, with_mask, seed=5)
            use = np.isfinite(lm) & (np.ones_like(lm, dtype=bool) if mask is None else mask != 0)
            assert use.sum() == case.Gu
            for n in range(case.N):
                c = counts[n, use].astype(np.float64)
                with np.errstate(divide="ignore"):
                    x = np.where(c > 0, np.log(c) - lm[use], np.nan)
                want = case.values_seen(n)
                assert np.array_equal(np.sort(x[~np.isnan(x)]), np.sort(want[~np.isnan(want)]))


def test_log_table_entries_the_cases_rely_on():
    """kLogInt[1] == 0.0 exactly (count 1 contributes -logmean bit for bit), kLogInt[255] = log(255) correctly rounded"""
    from tests.test_devunit_build import parse_table

    tab = parse_table("dsq_lgamma_int.h", "kLogInt")
    assert tab[1] == 0.0 and not np.signbit(tab[1])
    mpmath.mp.prec = 120
    exact = mpmath.log(255)
    ulp = math.ulp(float(exact))
    assert abs(mpmath.mpf(float(tab[255])) - exact) <= mpmath.mpf(ulp) / 2
