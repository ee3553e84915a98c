"""Rank-sum test, CPU side: the launch plan and the layout of a comparison at their edges, the host build of
csrc/dsq_rank.h (tests/hostrank: the code the device runs, one lane) against the numpy / mpmath reference of
tests/rank_ref.py and against scipy.stats.mannwhitneyu, and every refusal of the host side."""
import numpy as np
import pytest

from tests import rank_cases as rc
from tests import rank_ref as rr

SMALL = rc.small_cases()


@pytest.fixture(scope="module")
def hr():
    from tests import hostrank

    hostrank.lib()
    return hostrank


def _packed(case):
    from pydeseq2_amd import ranktest as rt

    return rt.pack_layouts([rt.build_layout(case.labels[k], case.strata) for k in range(case.K)], case.labels)


def _run(hr, case, alt):
    code, got = hr.ranksum(case.y, case.ldn, case.sf, case.N, _packed(case), rr.ALT_CODE[alt])
    assert code == 0
    return got


# ------------------------------------------------------------------------------------------------ plan and layout
def test_plan_is_a_function_of_L(hr):
    assert hr.plan(0) == (-2, 0, 0) and hr.plan(-5) == (-2, 0, 0) and hr.plan(16385) == (-2, 0, 0)
    for L, waves in ((1, 4), (1024, 4), (5120, 4), (5121, 2), (8192, 2), (10240, 2), (10241, 1), (16384, 1)):
        assert hr.plan(L) == (0, waves, 8 * L * waves), L
        assert 8 * L * waves <= 160 * 1024
    assert hr.plan(16384)[2] == 128 * 1024


def test_layout_of_a_comparison():
    from pydeseq2_amd import ranktest as rt

    assert [rt.next_pow2(n) for n in (0, 1, 2, 3, 4, 5, 64, 65, 16384)] == [1, 1, 2, 4, 4, 8, 64, 128, 16384]
    lab = np.array([1, -1, 0, 0, 1, 0, -1, 1, 0])
    q = rt.build_layout(lab)
    assert q.order.tolist() == [0, 2, 3, 4, 5, 7, 8] and q.seg.tolist() == [0, 7] and q.pad.tolist() == [0, 8]
    assert (q.n_strata, q.L, q.pairs, q.n1.tolist(), q.n2.tolist()) == (1, 8, 12, [3], [4])
    # strata ids are any integers; the used samples' ids in ascending order; a stratum of left-out samples vanishes
    q = rt.build_layout(lab, np.array([9, 9, -4, 9, -4, 9, 0, 9, 9]))
    assert q.order.tolist() == [2, 4, 0, 3, 5, 7, 8] and q.seg.tolist() == [0, 2, 7] and q.pad.tolist() == [0, 2, 10]
    assert q.n1.tolist() == [1, 2] and q.n2.tolist() == [1, 3] and q.pairs == 7
    case = [c for c in SMALL if c.name == "strata_1_2_3_64_65"][0]
    q = rt.build_layout(case.labels[0], case.strata)
    assert np.diff(q.seg).tolist() == [1, 2, 3, 64, 65] and q.pad.tolist() == [0, 1, 3, 7, 71, 199]
    assert sorted(q.order.tolist()) == np.nonzero(case.labels[0] >= 0)[0].tolist()
    big = rc.big_cases()
    assert rt.build_layout(big[0].labels[0]).L == 16384 and rt.build_layout(big[1].labels[0], big[1].strata).L == 16384
    P = _packed([c for c in SMALL if c.name == "K3_strata"][0])
    assert P.order.shape[0] == 3 and P.seg.shape == P.pad.shape and P.labels.dtype == np.int8
    assert P.lds == P.nstrata.max() + 1 and P.order.dtype == P.seg.dtype == P.pad.dtype == P.nstrata.dtype == np.int32


def test_layout_check_of_the_launcher(hr):
    order, seg, pad = [4, 1, 0, 3], [0, 1, 4], [0, 1, 5]
    assert hr.check_layout(order, seg, pad, 2, N=5) is None
    assert "n_strata" in hr.check_layout(order, seg, pad, 0, N=5) and "n_strata" in hr.check_layout(order, seg, pad, 3, N=5)
    assert "first offset" in hr.check_layout(order, [1, 1, 4], pad, 2, N=5)
    assert "first offset" in hr.check_layout(order, seg, [1, 2, 6], 2, N=5)
    assert "at least one sample" in hr.check_layout(order, [0, 0, 4], pad, 2, N=5)
    assert "ldo or N" in hr.check_layout(order, seg, pad, 2, N=3) and "ldo or N" in hr.check_layout(order, seg, pad, 2, N=5, cap_order=3)
    assert "prefix sums" in hr.check_layout(order, seg, [0, 1, 4], 2, N=5)  # 3 samples need 4 doubles
    assert "prefix sums" in hr.check_layout(order, seg, [0, 2, 6], 2, N=5)
    assert "outside 0" in hr.check_layout([4, 1, 5, 3], seg, pad, 2, N=5) and "outside 0" in hr.check_layout([4, -1, 0, 3], seg, pad, 2, N=5)
    n = 8193
    assert "DSQ_RANK_MAX_L" in hr.check_layout(np.arange(2 * n), [0, n, 2 * n], [0, 16384, 32768], 2, N=2 * n)


def test_the_host_entry_refuses_what_the_c_abi_refuses(hr):
    case = SMALL[3]
    P = _packed(case)
    assert hr.ranksum(case.y, case.ldn, case.sf, case.N, P, 0)[0] == 0
    for alt in (1, 2, 5, -1):  # greaterAbs, lessAbs
        assert hr.ranksum(case.y, case.ldn, case.sf, case.N, P, alt)[0] == -2
    assert hr.ranksum(case.y, case.N - 1, case.sf, case.N, P, 0)[0] == -2
    bad = _packed(case)
    bad.pad[0, 1] = 32
    assert hr.ranksum(case.y, case.ldn, case.sf, case.N, bad, 0)[0] == -2


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("alt", rc.ALTS, ids=["two-sided", "greater", "less"])
@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
def test_host_build_against_the_reference(hr, case, alt):
    w = rr.check_case(case, alt, _run(hr, case, alt), "host")
    print(f"{case.name} alt={alt}: stat error {w['stat']:.2f} of its bound, p error {w['p']:.2g} of its bound, "
          f"worst deviation from scipy {w['scipy']:.3g}")


@pytest.mark.parametrize("case", rc.big_cases(), ids=["n16384", "n8192x2"])
def test_host_build_on_the_longest_rows(hr, case):
    for alt in rc.ALTS:
        w = rr.check_case(case, alt, _run(hr, case, alt), "host")
        print(f"{case.name} alt={alt}: stat {w['stat']:.2f}, p {w['p']:.2g} of their bounds, scipy {w['scipy']:.3g}")


def test_clamped_numerator_and_degenerate_rows(hr):
    case = [c for c in SMALL if c.name == "W_zero"][0]
    got = _run(hr, case, None)
    assert got["usum"][0].tolist() == [2.0, 2.5] and got["ties"][0].tolist() == [0.0, 6.0]
    assert got["stat"][0].tolist() == [0.0, 0.0] and got["pvalue"][0].tolist() == [1.0, 1.0]  # |W| - 1/2 clamped at 0
    g, l = _run(hr, case, "greater"), _run(hr, case, "less")
    assert g["stat"][0, 0] < 0 < l["stat"][0, 0] and g["stat"][0, 0] == -l["stat"][0, 0]
    assert g["pvalue"][0, 0] == l["pvalue"][0, 0] > 0.5 and g["stat"][0, 1] == 0.0 and g["pvalue"][0, 1] == 0.5
    case = [c for c in SMALL if c.name == "W_zero_strata"][0]
    for alt, p in ((None, 1.0), ("greater", 0.5), ("less", 0.5)):
        got = _run(hr, case, alt)
        assert got["stat"][0, 0] == 0.0 and got["pvalue"][0, 0] == p and got["usum"][0, 0] == 4.0
    # all values tied: V == 0 -> stat 0, p 1, whatever the alternative
    y = np.full((1, 10), 3, np.int32)
    tied = rc.Case("tied", y, np.ones(10), np.array([[1, 0] * 5], np.int8), None, 10, 10)
    for alt in rc.ALTS:
        got = _run(hr, tied, alt)
        assert (got["stat"][0, 0], got["pvalue"][0, 0], got["usum"][0, 0], got["ties"][0, 0]) == (0.0, 1.0, 12.5, 990.0)


def test_the_values_are_ieee_quotients(hr):
    """Ties are decided by (double)y / sf: 2/1 and 4/2 tie; 1/3 * 3 style near-ties do not merge or split."""
    sf = np.array([1.0, 2.0, 3.0, 0.1, 0.3, 49.0, 7.0, 98.0])
    y = np.array([[2, 4, 6, 1, 3, 7, 1, 14]], np.int32)  # 2, 2, 2, 10, 10, 1/7, 1/7, 1/7
    lab = np.array([[1, 0, 1, 0, 1, 0, 1, 0]], np.int8)
    v = y[0] / sf
    assert v[0] == v[1] == v[2] and v[5] == v[6] == v[7]
    case = rc.Case("quotients", y, sf, lab, None, 8, 8)
    rr.check_case(case, None, _run(hr, case, None), "host")
    _, cnt = np.unique(v, return_counts=True)
    assert _run(hr, case, None)["ties"][0, 0] == float(sum(int(t) ** 3 - int(t) for t in cnt))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_of_the_layout():
    from pydeseq2_amd import ranktest as rt

    with pytest.raises(ValueError, match="1 .tested., 0 .reference. or -1"):
        rt.build_layout([1, 0, 2])
    with pytest.raises(ValueError, match="1 .tested., 0 .reference. or -1"):
        rt.build_layout([[1, 0], [0, 1]])
    with pytest.raises(ValueError, match="at least one tested and one reference"):
        rt.build_layout([1, 1, -1])
    with pytest.raises(ValueError, match="at least one tested and one reference"):
        rt.build_layout([0, -1, 0])
    with pytest.raises(ValueError, match="one id per sample"):
        rt.build_layout([1, 0, 0], [0, 1])
    case = rc.refused_case()
    with pytest.raises(ValueError, match=r"24576 doubles.*16384 \(DSQ_RANK_MAX_L\)"):
        rt.build_layout(case.labels[0], case.strata)
    with pytest.raises(ValueError, match="DSQ_RANK_MAX_L"):
        rt.build_layout(np.tile([1, 0], 8193))  # 16 386 samples in one stratum
    assert rt.build_layout(case.labels[0]).L == 16384  # the same samples without strata fit


def test_refusals_of_the_alternative():
    from pydeseq2_amd import ranktest as rt

    for alt in rt.RANK_ALT:
        rt.check_alternative(alt)
    for alt in ("greaterAbs", "lessAbs", "two-sided"):
        with pytest.raises(ValueError, match="two-sided .None., 'greater' or 'less'"):
            rt.check_alternative(alt)
    with pytest.raises(ValueError, match="no lfc_null"):
        rt.check_alternative(None, lfc_null=0.5)


class _NoDevice:
    """Stands where a context would: any use of the device fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched ({name}) before the refusal")


def test_ranksum_refuses_before_the_device():
    from pydeseq2_amd import ranktest as rt

    sf, lab = np.ones(6), np.array([1, 1, 0, 0, -1, 0])
    bad = [
        (dict(labels=lab, size_factors=np.ones(5)), "K x N with N = 5"),
        (dict(labels=lab, size_factors=np.array([1, 1, 0, 1, 1, 1.0])), "finite and positive"),
        (dict(labels=lab, size_factors=np.array([1, 1, np.inf, 1, 1, 1.0])), "finite and positive"),
        (dict(labels=lab, size_factors=sf, alt_hypothesis="greaterAbs"), "'greater' or 'less'"),
        (dict(labels=np.array([lab, [1, 1, 1, 1, 1, 1]]), size_factors=sf), "at least one tested and one reference"),
        (dict(labels=lab, size_factors=sf, strata=[0, 1]), "one id per sample"),
        (dict(labels=lab, size_factors=sf, ldn=4), "row pitch"),
    ]
    for kw, match in bad:
        kw.setdefault("ldn", 6)
        with pytest.raises(ValueError, match=match):
            rt.ranksum(_NoDevice(), 0, G=3, **kw)


def test_facade_refusals_need_no_device():
    """DeseqStats(test="wilcoxon") refuses a numeric contrast, an LFC threshold, the *Abs alternatives, unknown strata and
    strata without the test before it looks at the data set's state."""
    from pydeseq2_amd import DeseqStats

    dds = _NoDevice()
    with pytest.raises(ValueError, match="must be .factor, tested, ref."):
        DeseqStats(dds, np.array([0.0, 1.0]), test="wilcoxon")
    with pytest.raises(ValueError, match="must be .factor, tested, ref."):
        DeseqStats(dds, [0.0, 1.0], test="wilcoxon")
    with pytest.raises(ValueError, match="no lfc_null"):
        DeseqStats(dds, ["condition", "B", "A"], test="wilcoxon", lfc_null=1.0)
    for alt in ("greaterAbs", "lessAbs"):
        with pytest.raises(ValueError, match="'greater' or 'less'"):
            DeseqStats(dds, ["condition", "B", "A"], test="wilcoxon", alt_hypothesis=alt)
    with pytest.raises(ValueError, match="pass test='wilcoxon'"):
        DeseqStats(dds, ["condition", "B", "A"], strata="batch")
    with pytest.raises(ValueError, match="pass test='wilcoxon'"):
        DeseqStats(dds, ["condition", "B", "A"], test="LRT", reduced="~1", strata=["batch"])
    with pytest.raises(ValueError, match="or 'wilcoxon' for the rank-sum test"):
        DeseqStats(dds, ["condition", "B", "A"], test="ranksum")

    class _Obs:
        obs = __import__("pandas").DataFrame({"condition": list("AABB"), "batch": list("xyxy")})

    with pytest.raises(ValueError, match=r"not found: \['site'\]"):
        DeseqStats(_Obs(), ["condition", "B", "A"], test="wilcoxon", strata=["batch", "site"])
    with pytest.raises(ValueError, match="reduced is the reduced design"):
        DeseqStats(_Obs(), ["condition", "B", "A"], test="wilcoxon", reduced="~1")
    with pytest.raises(ValueError, match="does not depend on the contrast"):
        DeseqStats.batch(_Obs(), [["condition", "B", "A"]], test="LRT", reduced="~1")


def test_exports_and_header():
    import os

    from pydeseq2_amd import _lib, ranktest

    assert {"dsq_dev_ranksum", "dsq_ranksum_plan"} <= set(_lib.EXPORTS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "deseq_hip.h")).read()
    assert f"#define DSQ_RANK_MAX_L {ranktest.RANK_MAX_L}" in hdr
    assert "DSQ_ABI_VERSION 5" in hdr
