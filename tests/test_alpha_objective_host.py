"""The mpmath reference of the dispersion objective and its error scale (tests/alpha_cases.py), shown to be right on the
host instantiation of dsq_alpha.h's alpha_eval (tests/hostsim) before any device result is judged by them
(tests/test_devunit_alpha.py), and the row-kernel cases checked with the host optimiser.  No GPU."""
import math

import mpmath as mp
import numpy as np
import pytest

from tests import alpha_cases as ac
from tests import hostsim as hs
from tests.devunit.ref import MP_PREC

WIDTHS = (1, 2, 3, 4, 8, 9, 12)
COMBOS = ((True, False), (True, True), (False, True), (False, False))  # (cr_reg, prior_reg)


def test_reference_gradient_is_the_derivative_of_the_reference_loss():
    """g is written down from dnb_nll and the trace formula, f from nb_nll and the log-determinant: two restatements
    that a sign or a factor alpha would separate.  mpmath differentiates f numerically at 120 bits."""
    for P in (1, 3, 8):
        for name, y, mu, X, _, _, la, lah, pv in ac.eval_cases(P)[::7]:
            _, g, _, _ = ac.objective(y, mu, X, la, lah, pv, True, True)
            with mp.workprec(MP_PREC):
                def f_at(t):
                    p = ac.parts(y, mu, X, float(t))
                    return p["nll"][0] + p["cr"][0] + p["prior"](lah, pv)[0]
                h = 2.0 ** -14  # (la + h is a double: the reference takes doubles)
                d = (f_at(la + h) - f_at(la - h)) / (2 * h)
                assert abs(d - g) <= 1e-6 * max(1.0, abs(g)), (name, la, d, g)


def test_host_alpha_eval_against_mpmath():
    """hs.alpha_eval (HostWave, libm's log / exp, the general formula for every count) within K_h EPS S of mpmath for every
    case of alpha_cases.eval_cases and every combination of the Cox-Reid and the prior term.  K_h is the smallest power
    of two that covers the worst ratio measured here: f 0.91 (a one-sample gene; 0.86 beyond it), g 4.14 (N = 257 at
    alpha = N: 257 terms of a plain running sum) -> K_H_F = 1, K_H_G = 8.  With the Stirling differences counted as single
    terms the same evaluations are 1e4 - 1e5 units off at alpha = 1e-8: this shows the scale, not only the values."""
    worst_f, worst_g = (0.0, None), (0.0, None)
    for P in WIDTHS:
        for name, y, mu, X, _, _, la, lah, pv in ac.eval_cases(P):
            for cr, pr in COMBOS:
                f, g = hs.alpha_eval(y.astype(np.int32), mu, X, la, la_hat=lah, prior_var=pv, cr_reg=cr, prior_reg=pr)
                fr, gr, Sf, Sg = ac.objective(y, mu, X, la, lah, pv, cr, pr)
                rf, rg = ac.ratio(f, fr, Sf), ac.ratio(g, gr, Sg)
                if rf > worst_f[0]:
                    worst_f = (rf, (name, la, cr, pr))
                if rg > worst_g[0]:
                    worst_g = (rg, (name, la, cr, pr))
    print(f"host alpha_eval: worst |f - ref| = {worst_f[0]:.3f} EPS S_f at {worst_f[1]}, "
          f"worst |g - ref| = {worst_g[0]:.3f} EPS S_g at {worst_g[1]}")
    assert worst_f[0] <= ac.K_H_F, worst_f
    assert worst_g[0] <= ac.K_H_G, worst_g
    # the constants follow from the recorded figures: the smallest powers of two over them, and 4 x for the device
    assert ac.K_H_F == ac.pow2_ceil(ac.HOST_WORST_F) and ac.K_H_G == ac.pow2_ceil(ac.HOST_WORST_G)
    assert ac.K_D_F == ac.pow2_ceil(4 * ac.HOST_WORST_F) and ac.K_D_G == ac.pow2_ceil(4 * ac.HOST_WORST_G)


def test_eval_cases_hold_the_edges():
    """what the device tests rely on: every memo size on both sides of its boundaries, the BIG path mixed with every
    memo block, one-count genes, the clamp, sample counts around the wave width"""
    for P in WIDTHS:
        cases = ac.eval_cases(P)
        maxima = {int(c[1].max()) for c in cases}
        assert {63, 64, 127, 128, 255, 256, 257, 513, 65533} <= maxima
        big = next(c for c in cases if "big" in c[0])
        blocks = {min(int(v) >> 6, 4) for v in big[1]}
        assert blocks == {0, 1, 2, 3, 4} or len(big[1]) < 16
        assert any((c[2] == ac.MIN_MU).sum() > len(c[2]) // 2 for c in cases)
        assert any(c[1].sum() in (1, 9, 10) and (c[1] > 0).sum() == 1 for c in cases)
        assert {len(c[1]) % 64 for c in cases} - {0} and {len(c[1]) % 16 for c in cases} - {0}
    assert {len(c[1]) for P in WIDTHS for c in ac.eval_cases(P)} >= set(ac.NS)


@pytest.mark.parametrize("run", ac.ROW_RUNS, ids=ac.row_run_id)
def test_row_cases_start_off_the_optimum_and_restore_no_iterate(run):
    """alpha_hat is chosen by the reference alone with |g(log alpha_hat)| > 1e-3 (pgtol is 1e-5: no gene ends at its
    first evaluation, all of them park at eval_cap = 1), and the host optimiser on the host objective restores no
    earlier iterate in its first ten evaluations: no loss value occurs twice."""
    spec, prior = run
    case = ac.row_case(*spec, n_genes=ac.row_genes(spec))
    ah = ac.choose_alpha_hat(case, prior, ac.ROW_PRIOR_VAR)
    t = case["tail"]
    assert any({t - 1, t, t + 1} <= set(y.tolist()) for y in case["y"])
    assert any(y.max() >= t for y in case["y"]) and any(y.max() < t for y in case["y"])
    assert (case["y"] <= 65533).all() and (case["mu"] > 0).all()
    lo, hi = math.log(case["min_disp"]), math.log(case["max_disp"])
    for g in range(case["G"]):
        y, mu = case["y"][g].astype(np.int32), case["mu"][g]
        fs = []

        def fg(x):
            f, gr = hs.alpha_eval(y, mu, case["X"], x, la_hat=math.log(ah[g]), prior_var=ac.ROW_PRIOR_VAR, prior_reg=prior)
            fs.append(f)
            return f, gr

        _, _, _, nfev, _, _ = hs.lbfgsb1d(fg, math.log(ah[g]), lo, hi)
        assert nfev >= 2, (g, nfev)
        first = fs[:10]
        assert len(set(first)) == len(first), (g, first)
