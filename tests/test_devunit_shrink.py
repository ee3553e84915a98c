"""The apeGLM objective and its gradient as the device evaluates them (tests/devunit/devunit_shrink.hip) against mpmath
(tests/shrink_cases.py): shrink_fn<DeviceWave, P> at P = 1, 2, 3, 4, 5, 8, 9, 12 and shrink_fn_wide<DeviceWave, PMAX, PB> in
the launcher's five instantiations at p == PB and at p == the previous block + 1, where the `j < p` masks work.

A fitted coefficient cannot see an error of the loss that is constant in beta, nor a lane's share that the wave sum
drops near the optimum where it is small; these tests look at f and g themselves at caller-given points - near an
optimum, the optimiser's start, 0, points on the `d > 0` switch of the log-add-exp, and the grid corners where
exp(-|d|) underflows - in units of EPS S (shrink_cases) with the bounds K_f = 16 and K_g = 256: four times the
reference's own error (numpy against mpmath, measured and asserted in tests/test_shrink_cases_host.py), rounded up to a
power of two.

Xt, the coefficients and the gradient have their full PB rows and entries; those at index >= p hold NaN, so a read beyond
p poisons a result and a write beyond p loses a sentinel.  Every test prints its worst ratios."""
import numpy as np
import pytest

from tests import shrink_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def du():
    from tests import devunit

    devunit.lib()
    return devunit


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("p", sc.NARROW_P + sc.WIDE_P)
def test_objective_and_gradient_against_mpmath(du, p):
    wf = wg = 0.0
    for c, refs in zip(sc.objective_cases(p), sc.objective_refs(p)):
        f0, f1, g = du.shrink_fn(c["y"], c["offset"], c["X"], c["size"], sc.SIGMA0, c["sigma"], c["sidx"], c["b"], c["inst"])
        what = f"p = {p}, N = {c['N']}, G = {c['G']}"
        # every lane holds the same values; the loss-only call returns the bits of the call with a gradient
        assert (bits(f1) == bits(f1[:, :1])).all() and (bits(g) == bits(g[:, :1])).all(), what
        assert (bits(f0) == bits(f1)).all(), what
        # entries >= p keep their sentinel, no result is NaN (nor infinite: objective_ratios)
        assert np.isnan(g[:, :, p:]).all() and not np.isnan(g[:, :, :p]).any() and not np.isnan(f1).any(), what
        a, b = sc.objective_ratios(c, refs, f1[:, 0], g[:, 0])
        print(f"shrink_fn {what}: f {a:.4f}, g {b:.4f}")
        wf, wg = max(wf, a), max(wg, b)
    print(f"shrink_fn p = {p} {c['inst'] or ''}: worst f {wf:.4f} (K_f = {sc.K_F:g}), g {wg:.4f} (K_g = {sc.K_G:g})")
    assert wf <= sc.K_F and wg <= sc.K_G


def test_the_entry_points_refuse_what_the_templates_would_walk_past(du):
    """(the front-end sizes every buffer by PB; a p beyond the block, a shrink index beyond p or an unknown pair never
    reaches a kernel)"""
    c = sc.objective_cases(13)[0]
    args = (c["y"], c["offset"], c["X"], c["size"], sc.SIGMA0, c["sigma"])
    with pytest.raises(du.DevunitError):
        du.shrink_fn(*args, c["sidx"], c["b"], (16, 24))
    with pytest.raises(du.DevunitError):
        du.shrink_fn(*args, np.full(c["G"], 13), c["b"], c["inst"])
    with pytest.raises(ValueError):
        du.shrink_fn(*args, c["sidx"], c["b"], (8, 8))
