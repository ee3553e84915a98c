"""Regularized-log transformation without a GPU: the per-gene fit of csrc/dsq_rlog.h in its host instantiations
(tests/hostrlog: one lane, and 64 lanes in the device's order with the samples in registers or in the output row) against
the dense QR restatement (tests/rlog_ref), two limits that rest on no restatement at all, the host estimate of the prior
variance against a direct construction, the edges, and the host-only argument checks of the façade."""
import numpy as np
import pytest

from tests import hostrlog as hr
from tests import rlog_ref
from tests.rlog_cases import check_hard, check_plain, hard_set, plain_set

MODES = [hr.ONE_LANE, hr.WAVE64, hr.WAVE64_ROW]


def _run(s, mode, **kw):
    return hr.rlog(s.counts, s.sf, s.disp, s.base_mean, kw.get("beta_prior_var", s.beta_prior_var), mode)


@pytest.mark.parametrize("N", [1, 2, 3, 12, 63, 64, 65, 130, 257, 512, 513])
def test_plain_sets_against_the_dense_restatement(N):
    """Every samples-per-lane count of the register path (R = 1, 2, 4, 8: N <= 64, 128, 256, 512), lane groups partly
    filled, and the row path (N = 513, and every N through WAVE64_ROW and ONE_LANE).  Largest difference seen over all
    of them: 1.4e-13 (rlog), 4.4e-14 (intercept), in log2 units."""
    s = plain_set(N, k=40)  # every gene restated
    host = _run(s, hr.WAVE64)
    worst = [check_plain(s, _run(s, m), f"N={N} mode={m}", host=host) for m in MODES]
    print(f"N={N}: largest |difference| from the restatement (rlog, intercept) = {np.max(worst, axis=0)}")


def _positive_set(N=12, G=30, seed=5, near=None, lo=None):
    """Positive counts whose fitted means stay far above the clamp at 0.5.  near=None: NB counts + 1 around means of 20 and
    more; near=sd: counts within a log-normal factor of sd of s_j m (means of 10^lo = 100 and more), rounded."""
    rng = np.random.default_rng(seed)
    sf = np.exp(rng.normal(0.0, 0.3, N))
    m = 10.0 ** rng.uniform(lo if lo is not None else 1.3 if near is None else 2.0, 4.0, G)
    a = 0.05 + 2.0 / m
    mu = sf[:, None] * m[None, :]
    if near is None:
        counts = 1 + rng.negative_binomial(1.0 / a, 1.0 / (1.0 + a * mu))
    else:
        counts = np.maximum(np.rint(mu * np.exp(rng.normal(0.0, near, (N, G)))), 1).astype(np.int64)
    return counts, sf, a, (counts / sf[:, None]).mean(0)


@pytest.mark.parametrize("mode", MODES)
def test_a_flat_prior_saturates_the_fit(mode):
    """beta_prior_var = 1e8: one free coefficient per sample, and the FULLY converged fit reproduces every count:
    rlog = log2(y / s).  The fit stops by the deviance rule, not at full convergence: Newton's error e_t squares per
    iteration (e_{t+1} ~ e_t^2 / 2), and the rule is met as soon as sum w e_t^2 < 1e-4 |dev|, i.e. at e_t ~ 1e-2, leaving
    e_{t+1} ~ 1e-4: with NB-scattered counts (_positive_set()) the difference is 6e-4 at the stop, in this build and in
    the dense restatement alike.  The 1e-6 of this test therefore needs counts that start close: within 1 % (sd) of
    s_j m, so e_0 <= 0.04, e_1 <= 1e-3 and the rule cannot be met before e_2 <= 5e-7 (natural log; 7e-7 in log2)."""
    counts, sf, a, bm = _positive_set(near=0.01)
    r, b0, conv, it = hr.rlog(counts, sf, a, bm, 1e8, mode)
    assert conv.all()
    print("largest |rlog - log2(y / s)|:", np.abs(r - np.log2(counts / sf[:, None])).max())
    assert np.abs(r - np.log2(counts / sf[:, None])).max() <= 1e-6


def _holds_the_restatement(counts, sf, a, bm, bpv, got, what):
    """Ordinary (NB-scattered) counts under an extreme prior: the stop comes before either limit is reached, so the values
    are held against the restatement's own - equal iteration counts (none borderline), rtol 1e-8 / atol 1e-10."""
    from tests.helpers import assert_close

    e = rlog_ref.rlog(counts, sf, a, bm, bpv)
    assert e[3].all() and not any(rlog_ref.borderline(c) for c in e[4]), "the seeded inputs are unsuitable"
    r, b0, conv, it = got
    assert conv.all() and np.array_equal(np.asarray(it, int), e[2])
    print(f"{what}: largest |difference| from the restatement (rlog, intercept) = "
          f"{np.abs(r - e[0]).max():.3g}, {np.abs(b0 - e[1]).max():.3g}")
    assert_close(r, e[0], 1e-8, 1e-10, f"{what} rlog")
    assert_close(b0, e[1], 1e-8, 1e-10, f"{what} intercept")
    return e


@pytest.mark.parametrize("mode", MODES)
def test_a_flat_prior_with_scattered_counts_stops_where_the_restatement_stops(mode):
    """The ordinary-counts regime under beta_prior_var = 1e8: NB-scattered positive counts.  The rule stops the fit one
    Newton step short of log2(y / s) (6e-4 seen, see above), in the restatement alike: the values are the restatement's,
    and they are within 1e-2 of the saturated fit (e_t ~ 1e-2 is what the rule lets pass, and the last step squares it)."""
    counts, sf, a, bm = _positive_set()
    got = hr.rlog(counts, sf, a, bm, 1e8, mode)
    _holds_the_restatement(counts, sf, a, bm, 1e8, got, f"flat prior, mode={mode}")
    assert np.abs(got[0] - np.log2(counts / sf[:, None])).max() <= 1e-2


def _common_mean_score(counts, sf, a, b0):
    """(|U| / sum y, |U| / sum w) per gene at mu_j = s_j 2^intercept: U = sum (y - mu) / (1 + a mu), w = mu / (1 + a mu).
    U / sum w is the Fisher scoring step the intercept would still take (natural log), the larger of the two (w <= mu)."""
    mu = sf[:, None] * 2.0 ** b0[None, :]
    U = ((counts - mu) / (1.0 + a[None, :] * mu)).sum(0)
    return np.abs(U) / counts.sum(0), np.abs(U) / (mu / (1.0 + a[None, :] * mu)).sum(0)


@pytest.mark.parametrize("mode", MODES)
def test_a_tight_prior_leaves_the_common_mean(mode):
    """beta_prior_var = 1e-10: b_j = q_j (z_j - beta0) with q_j <= w_j / lambda <= 1e-10 ln^2 2 / a, below 1e-8 here, so
    every sample sits at the intercept, and the intercept solves the common-mean score equation U = sum (y - mu) /
    (1 + a mu) = 0, mu_j = s_j 2^intercept.

    How close, worked out for these inputs: means of 1000 and more, every y_j / s_j within rho = 0.01 (relative) of
    their mean bm (asserted below).  The solution m* lies between the smallest and the largest y_j / s_j, so the start
    ln bm is off by e_0 <= rho and the relative residuals rho_j at the solution are at most 2 rho.  The fit is Fisher
    scoring in beta0 alone: its error (natural log) obeys e_{t+1} = e_t (1 - J / I) + O(e_t^2) with I = sum w and
    J - I = sum w rho_j u / (1 + u), u = a mu, so |1 - J / I| <= 2 rho and e_{t+1} <= e_t (2 rho + e_t): e_1 <= 3e-4 and,
    as the rule cannot stop before the second iteration, e_2 <= 6.1e-6.  The fixed point itself has U = lambda0 beta0
    (the ridge on the intercept): 2.1e-6 * 10 over sum w >= 12 * 18 is 1e-7.  Together a residual step |U| / sum w of
    1e-5 at the most, and |U| / sum y is smaller still (w <= mu).  Seen: 8e-8 (the ridge)."""
    counts, sf, a, bm = _positive_set(near=0.001, lo=3.0)
    assert np.abs(counts / sf[:, None] / bm[None, :] - 1.0).max() <= 0.01 and bm.min() >= 900.0
    r, b0, conv, it = hr.rlog(counts, sf, a, bm, 1e-10, mode)
    assert conv.all()
    assert np.abs(r - b0[None, :]).max() <= 1e-6
    rel_y, rel_w = _common_mean_score(counts, sf, a, b0)
    print("largest |score| / sum y, |score| / sum w:", rel_y.max(), rel_w.max())
    assert rel_y.max() <= 1e-5 and rel_w.max() <= 1e-5


@pytest.mark.parametrize("mode", MODES)
def test_a_tight_prior_with_scattered_counts_stops_where_the_restatement_stops(mode):
    """The ordinary-counts regime under beta_prior_var = 1e-10: NB-scattered positive counts (means of 20 and more).  The
    stopping rule bounds the score U before the last step: that step lowers the deviance by about U^2 / sum w <
    1e-4 (|dev| + 0.1); with sum w <= sum mu ~ sum y >= 20 N and |dev| ~ 10 N this is |U| / sum y < sqrt(1e-3 N / sum y)
    < 1e-2, and the last (Fisher scoring) step only shrinks it.  That bound is loose (3.4e-7 seen), so the values are
    also held against the restatement's own."""
    counts, sf, a, bm = _positive_set()
    got = hr.rlog(counts, sf, a, bm, 1e-10, mode)
    _holds_the_restatement(counts, sf, a, bm, 1e-10, got, f"tight prior, mode={mode}")
    assert np.abs(got[0] - got[1][None, :]).max() <= 1e-6
    assert _common_mean_score(counts, sf, a, got[1])[0].max() <= 1e-2


def test_weighted_upper_quantile_by_hand_and_against_the_direct_construction():
    from pydeseq2_amd.rlog import beta_prior_var, weighted_upper_quantile

    # n = 5, equal weights: order 4.8 -> 0.2 Q(4) + 0.8 Q(5) with the running weights 1 ... 5; a tie in the middle
    assert weighted_upper_quantile([1, 2, 2, 3, 10], np.ones(5)) == pytest.approx(0.2 * 3 + 0.8 * 10, rel=1e-15)
    # n = 4, order 3.85.  Weights (1, 1, 1, 5) scale to (.5, .5, .5, 2.5): running (.5, 1, 1.5, 4): Q(3) = Q(4) = 4
    assert weighted_upper_quantile([1, 2, 3, 4], [1, 1, 1, 5]) == pytest.approx(4.0, rel=1e-15)
    # weights (5, 1, 1, 1) -> running (2.5, 3, 3.5, 4): Q(3) = 2, Q(4) = 4
    assert weighted_upper_quantile([1, 2, 3, 4], [5, 1, 1, 1]) == pytest.approx(0.15 * 2 + 0.85 * 4, rel=1e-15)
    assert weighted_upper_quantile([7.0], [3.0]) == 7.0
    rng = np.random.default_rng(11)
    for n in (2, 3, 20, 21, 400):
        x = np.round(rng.exponential(1.0, n), 1)  # (one decimal: many ties)
        w = rng.uniform(0.1, 10.0, n)
        assert weighted_upper_quantile(x, w) == pytest.approx(rlog_ref.weighted_upper_quantile(x, w), rel=1e-14, abs=0)
        assert weighted_upper_quantile(x[::-1], w[::-1]) == pytest.approx(weighted_upper_quantile(x, w), rel=1e-14)
    s = plain_set(12)
    assert beta_prior_var(s.counts, s.sf, s.disp) == pytest.approx(rlog_ref.prior_var(s.counts, s.sf, s.disp), rel=1e-12)
    assert 0.05 < s.beta_prior_var < 0.6  # (these sets: 0.18 ... 0.30)


@pytest.mark.parametrize("mode", MODES)
def test_edges(mode):
    sf = np.array([0.8, 1.1, 1.3, 0.9, 1.0])
    counts = np.array([[0, 0, 0, 0, 0], [0, 0, 7, 0, 0], [3, 1, 4, 1, 5]]).T  # all zero; one count; an ordinary gene
    disp = np.array([0.3, 0.3, 0.2])
    bm = (counts / sf[:, None]).mean(0)
    r, b0, conv, it = hr.rlog(counts, sf, disp, bm, 0.3, mode)
    # a gene without counts is not fitted: zeros, no iteration, not converged
    assert (r[:, 0] == 0.0).all() and b0[0] == 0.0 and it[0] == 0 and not conv[0]
    ref = rlog_ref.rlog(counts[:, 1:], sf, disp[1:], bm[1:], 0.3)
    assert ref[3].all() and np.array_equal(it[1:], ref[2]) and conv[1:].all()
    np.testing.assert_allclose(r[:, 1:], ref[0], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(b0[1:], ref[1], rtol=1e-8, atol=1e-10)
    assert r[2, 1] > r[0, 1] and np.ptp(r[[0, 1, 3, 4], 1]) < 0.5  # the one count stands out, the zeros lie together


@pytest.mark.parametrize("mode", MODES)
def test_a_coefficient_beyond_30_ends_the_fit_unconverged(mode):
    """2e9 reads at a size factor of 1e-7 under a flat prior: that sample's eta heads for ln 2e16 = 37.6, so a sample
    coefficient passes 30 - checked on the restatement first.  Count 100, flag false, finite outputs; the ordinary gene
    next to it is untouched by its neighbour."""
    sf = np.array([1e-7, 1.0, 1.0])
    counts = np.array([[2_000_000_000, 5, 5], [40, 50, 60]]).T
    disp = np.array([0.1, 0.1])
    bm = (counts / sf[:, None]).mean(0)
    ref = rlog_ref.rlog(counts, sf, disp, bm, 1e8)
    assert ref[2][0] == 100 and not ref[3][0] and len(ref[4][0]) < 99 and ref[3][1]  # (left through the exit, not the cap)
    r, b0, conv, it = hr.rlog(counts, sf, disp, bm, 1e8, mode)
    assert it[0] == 100 and not conv[0] and np.isfinite(r[:, 0]).all() and np.isfinite(b0[0])
    assert conv[1] and it[1] == ref[2][1]
    np.testing.assert_allclose(r[:, 1], ref[0][:, 1], rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("mode", MODES)
def test_hard_set(mode):
    s = hard_set()
    easy, capped, same_row = check_hard(s, _run(s, mode), f"hard mode={mode}")
    print(f"hard set: {easy:.0%} of the genes converge within 30 iterations, {capped:.0%} run to 100")
    assert capped > 0.05 and same_row > 0  # (the set does exercise the cap, and the intercept at the cap)


def test_host_build_refuses_bad_arguments():
    import ctypes as C

    z = np.zeros(4)
    args = lambda N, G, v: (z.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int(max(N, 1)), hr._p(z, C.c_double), C.c_int(N),  # noqa: E731
                            C.c_int(G), hr._p(z, C.c_double), hr._p(z, C.c_double), C.c_double(v), C.c_int(0),
                            hr._p(z, C.c_double), hr._p(z, C.c_double), z.ctypes.data_as(C.POINTER(C.c_uint8)),
                            z.ctypes.data_as(C.POINTER(C.c_int32)))
    assert hr.lib().hr_rlog(*args(0, 1, 1.0)) == -1 and hr.lib().hr_rlog(*args(1, -1, 1.0)) == -1
    assert hr.lib().hr_rlog(*args(1, 1, 0.0)) == -1 and hr.lib().hr_rlog(*args(1, 1, float("nan"))) == -1
    assert hr.lib().hr_rlog(*args(1, 0, 1.0)) == 0


def test_facade_argument_checks_need_no_gpu():
    from pydeseq2_amd.api import DeseqDataSet
    from tests.lrt_cases import facade_scenario

    counts, meta, _ = facade_scenario()
    dds = DeseqDataSet(counts=counts, metadata=meta, design="~batch + condition", min_replicates=4)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="beta_prior_var"):
            dds.rlog(beta_prior_var=bad)
    with pytest.raises(NotImplementedError, match="fit_type"):
        dds.rlog(fit_type="local")
    assert dds._pipe_obj is None  # nothing above has touched the GPU


def test_rlog_entry_point_is_declared_and_the_abi_version_stays():
    import os
    import re

    from pydeseq2_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "deseq_hip.h")).read()
    assert re.search(r"int dsq_dev_rlog\(", hdr) and "dsq_dev_rlog" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "dsq_dev_rlog") and lib.dsq_abi_version() == 5
