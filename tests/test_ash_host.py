"""Adaptive shrinkage without a GPU: the templates of csrc/dsq_ash.h in their host instantiation (tests/hostash: one wave
that walks every chunk, and four waves in the device's order) against the dense restatement (tests/ash_ref) over the seeded
sets of tests/ash_cases; the restatement's posterior against mpmath; the host side of pydeseq2_amd.ash (grid, s-values) and
the argument checks of the facade that need no device."""
import re

import numpy as np
import pytest

from tests import ash_cases as ac
from tests import ash_ref
from tests import hostash as ha

ALL = ac.all_cases()


def test_the_sets_meet_the_condition_on_the_inputs():
    """Checked on the restatement alone, before anything is compared: every set converges (min grad >= -1e-13) within 30
    iterations, the constructions give the grids the tests are meant to walk (the sigma_max = 8 sigma_min branch, 20 to
    48 components, M = 48 itself), and the set that lies outside the condition is known to."""
    assert all(c.ref["converged"] and c.ref["n_iter"] <= ac.MAX_REF_ITER for c in ALL)
    assert ac.case("null", 5).M == 7 and ac.case("plain", 203).M == 21 and ac.case("heavy", 203).M == 30
    assert ac.case("wide-se", 203).M == 44 and ac.case("wide-se", 3000).M == 48
    assert [ac.forced(M).M for M in ac.FORCED_M] == list(ac.FORCED_M)
    c = ac.nan_case("wide-se", 3000)
    u = ash_ref.used(c.b, c.s)
    assert not u[0] and not u[-1] and not u[64:128].any() and 0.85 <= u.mean() <= 0.92
    assert not ac.breakdown().ref["converged"]


@pytest.mark.parametrize("nw", [ha.ONE_WAVE, ha.WAVES4])
@pytest.mark.parametrize("c", ALL, ids=lambda c: c.name.replace(" ", "_"))
def test_host_builds_vs_restatement(c, nw):
    """converged; the KKT residual recomputed from the returned pi and a dense L at most 1e-8; sum pi = 1, pi >= 0; loglik;
    posterior mean, standard deviation and lfsr within ac.POST_TOL (ten times the largest difference measured, 1.74e-9:
    the builds stop at the 1e-8 rule, the restatement at 1e-13)."""
    got = ha.ash(c.b[None], c.s[None], [c.sd], nw)
    worst = ac.check(c, got, 0, f"host build, {nw} wave(s)")
    print(f"{c.name} M={c.M} waves={nw}: {got['n_iter'][0]} iterations in {got['passes'][0]} passes, KKT "
          f"{got['kkt'][0]:.3g}; largest difference from the restatement {worst}")
    assert got["passes"][0] >= got["n_iter"][0] + 1


def test_breakdown_is_reported_not_hidden():
    """heavy at G = 3000 (outside the condition on the inputs, tests/ash_cases): neither the restatement nor the builds
    converge; the builds say so and still return proportions and finite posteriors."""
    c = ac.breakdown()
    L, _ = ash_ref.lik(c.b, c.s, c.sd)
    for nw in (ha.ONE_WAVE, ha.WAVES4):
        got = ha.ash(c.b[None], c.s[None], [c.sd], nw)
        pi = got["pi"][0]
        assert not got["converged"][0] and ash_ref.kkt_residual(L, pi) > 1e-8
        assert (pi >= 0).all() and abs(pi.sum() - 1) <= 1e-12
        assert all(np.isfinite(got[k][0]).all() for k in ("post_mean", "post_sd", "lfsr"))


def test_several_contrasts_a_skipped_one_and_one_without_used_genes():
    cs = [ac.case("plain", 203), ac.nan_case("heavy", 203), ac.case("null", 203)]
    b, s = np.stack([c.b for c in cs]), np.stack([c.s for c in cs])
    b[2] = np.nan
    got = ha.ash(b, s, [cs[0].sd, cs[1].sd, cs[2].sd])
    for k in (0, 1):
        ac.check(cs[k], got, k, "K=3")
    assert np.isnan(got["pi"][2][:cs[2].M]).all() and np.isnan(got["post_mean"][2]).all()
    assert got["n_iter"][2] == 0 and not got["converged"][2] and np.isnan(got["kkt"][2]) and np.isnan(got["loglik"][2])
    skipped = ha.ash(b[:1], s[:1], [np.zeros(0)])
    assert np.isnan(skipped["post_mean"]).all() and skipped["n_iter"][0] == 0


def test_iteration_cap():
    c = ac.case("plain", 65)
    got = ha.ash(c.b[None], c.s[None], [c.sd], max_iter=1)
    assert got["n_iter"][0] == 1 and not got["converged"][0] and got["kkt"][0] > 1e-8


def test_restatement_posterior_vs_mpmath():
    """A handful of genes of three sets, the outlying ones among them: relative 1e-12 on the mean and the standard
    deviation (plus, for the latter, the rounding of the subtraction under the root, which an outlying gene with a
    posterior mean a thousand times its standard deviation magnifies), and on an lfsr down to 1e-130 (both tails are
    computed directly)."""
    for c in (ac.case("plain", 203), ac.case("heavy", 203), ac.case("wide-se", 65)):
        z = np.abs(c.b / c.s)
        for g in {0, 1, int(z.argmax()), int(z.argmin()), len(c.b) - 1}:
            e = ash_ref.posterior_mp(c.b[g], c.s[g], c.sd, c.ref["pi"])
            a = [c.ref[k][g] for k in ("post_mean", "post_sd", "lfsr")]
            for x, y, k in zip(a, e, ("mean", "sd", "lfsr")):
                tol = 1e-12 * max(abs(y), 1e-3 if k != "lfsr" else 0.0) + 1e-300
                if k == "sd":  # sqrt(E x^2 - mean^2), as the statement writes it: the subtraction rounds at 4 ulp of E x^2
                    tol += 4 * 2.3e-16 * (y * y + e[0] * e[0]) / (2 * y)
                assert abs(x - y) <= tol, (c.name, g, k, x, y)


def test_mixsd_grid_hand_computed():
    from pydeseq2_amd.ash import mixsd_grid

    r2 = np.sqrt(2.0)
    # sigma_min = 0.1, b^2 - s^2 = 3 -> sigma_max = 2 sqrt 3; npoint = ceil(2 log2(20 sqrt 3)) = 11
    g = mixsd_grid(np.array([2.0, 0.0]), np.array([1.0, 1.0]))
    assert len(g) == 12 and np.allclose(g, [r2 ** e * 2 * np.sqrt(3.0) for e in range(-11, 1)], rtol=1e-15)
    # no b^2 above s^2: sigma_max = 8 sigma_min, npoint = 6, M = 7
    g = mixsd_grid(np.array([0.5, -0.1]), np.array([1.0, 2.0]))
    assert np.allclose(g, [r2 ** e * 0.8 for e in range(-6, 1)], rtol=1e-15)
    # sigma_max below sigma_min: b^2 - s^2 = 1e-6 -> sigma_max = 2e-3, sigma_min = 0.1, npoint = ceil(2 log2 0.02) = -11:
    # R's (-npoint):0 counts DOWN, 11, 10, ..., 0: twelve components from 2e-3 2^5.5 to 2e-3
    b = np.array([np.sqrt(1.0 + 1e-6)])
    g = mixsd_grid(b, np.array([1.0]))
    sm = 2 * np.sqrt(b[0] ** 2 - 1.0)
    assert len(g) == 12 and np.allclose(g, [r2 ** e * sm for e in range(11, -1, -1)], rtol=1e-15) and g[0] > g[-1]
    # unused genes take no part; none used: no grid
    g2 = mixsd_grid(np.array([2.0, 0.0, 50.0, np.nan, 9.0]), np.array([1.0, 1.0, 0.0, 1e-9, np.inf]))
    assert np.array_equal(g2, mixsd_grid(np.array([2.0, 0.0]), np.array([1.0, 1.0])))
    assert len(mixsd_grid(np.array([np.nan]), np.array([1.0]))) == 0
    for c in ALL[:12]:
        assert np.allclose(mixsd_grid(c.b, c.s), ash_ref.grid(c.b, c.s)[1], rtol=1e-14, atol=0)


def test_mixsd_grid_refuses_more_than_48_components():
    from pydeseq2_amd.ash import mixsd_grid

    c = ac.case("wide-se", 3000)
    assert len(ash_ref.grid(c.b, c.s)[1]) > 48
    with pytest.raises(ValueError, match="48"):
        mixsd_grid(c.b, c.s)
    # sigma_min = 1e-4, sigma_max = 2e4 (to 1e-14): npoint = ceil(2 log2 2e8) = ceil(55.15) = 56
    assert len(mixsd_grid(np.array([1e4, 0.0]), np.array([1e-3, 1.0]), max_m=64)) == 57
    with pytest.raises(ValueError, match="DSQ_ASH_MAX_M"):
        mixsd_grid(np.array([1e4, 0.0]), np.array([1e-3, 1.0]))


def test_svalues_vs_direct_loop():
    from pydeseq2_amd.ash import svalues

    rng = np.random.default_rng(5)
    f = rng.random(300) * 0.5
    f[rng.choice(300, 40, replace=False)] = np.nan
    f[[3, 17, 200]] = f[5]  # ties: stable order
    sv = svalues(f)
    assert np.array_equal(np.isnan(sv), np.isnan(f))
    ok = ~np.isnan(f)
    assert np.allclose(sv[ok], ash_ref.svalues(f)[ok], rtol=1e-14, atol=0)
    o = np.argsort(f[ok], kind="stable")
    assert (np.diff(sv[ok][o]) >= 0).all() and sv[ok][o][0] == f[ok].min()
    assert np.isnan(svalues(np.full(4, np.nan))).all() and len(svalues(np.zeros(0))) == 0


class _FakeDds:
    """What DeseqStats.lfc_shrink touches before it reaches the device."""


def _stats_without_device():
    import pandas as pd

    from pydeseq2_amd.api import DeseqStats

    ds = DeseqStats.__new__(DeseqStats)
    ds.LFC = pd.DataFrame(np.zeros((3, 2)), columns=["Intercept", "condition[T.B]"])
    ds.contrast_vector = np.array([0.0, 1.0])
    ds.dds = _FakeDds()
    return ds


def test_facade_argument_checks_need_no_device():
    ds = _stats_without_device()
    with pytest.raises(ValueError, match="'apeglm' or 'ashr'"):
        ds.lfc_shrink("condition[T.B]", type="normal")
    with pytest.raises(ValueError, match="coeff must be None"):
        ds.lfc_shrink("condition[T.B]", type="ashr")
    for coeff in (None, "condition[T.C]", "nonsense"):  # the apeGLM path's KeyError, None included
        with pytest.raises(KeyError, match="should be one the LFC columns"):
            ds.lfc_shrink(coeff)
        with pytest.raises(KeyError):
            ds.lfc_shrink(coeff, True, type="apeglm")
    from pydeseq2_amd.api import DeseqStats

    with pytest.raises(ValueError, match="at least one"):
        DeseqStats.shrink_batch([])
    other = _stats_without_device()
    with pytest.raises(ValueError, match="one DeseqDataSet"):
        DeseqStats.shrink_batch([ds, other])


def test_ash_refuses_grids_beyond_the_limit_before_the_device():
    from pydeseq2_amd.ash import ash

    with pytest.raises(ValueError, match="48"):
        ash(None, np.zeros((1, 4)), np.ones((1, 4)), grids=[np.ones(49)])
    with pytest.raises(ValueError, match="same K x G shape"):
        ash(None, np.zeros((1, 4)), np.ones((1, 5)))
    r = ash(None, np.full((2, 4), np.nan), np.ones((2, 4)))  # no used gene anywhere: nothing is launched
    assert np.isnan(r.post_mean).all() and not r.converged.any() and all(len(g) == 0 for g in r.grid)


def test_entry_point_is_declared_and_the_abi_version_stays():
    import os

    from pydeseq2_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "deseq_hip.h")).read()
    assert re.search(r"int dsq_dev_ash\(", hdr) and "dsq_dev_ash" in _lib.EXPORTS
    assert re.search(r"#define DSQ_ABI_VERSION 5\b", hdr) and re.search(r"#define DSQ_ASH_MAX_M 48\b", hdr)
    assert "dsq_k_ash.hip" in open(os.path.join(root, "pydeseq2_amd", "csrc", "Makefile")).read()
