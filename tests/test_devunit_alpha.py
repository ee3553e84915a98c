"""The dispersion objective as the device evaluates it (tests/devunit/devunit_alpha.hip) against mpmath
(tests/alpha_cases.py): dsq_alpha.h's alpha_eval in its 64-lane instantiations - the count memo with 1, 2 and 4 blocks,
the LDS-staged padded rows, the per-cell accumulation, the split second sweep from p = 9 - and the restatements of the
same objective in the row kernels (k_alpha_rows, k_alpha_rows_c) and in k_alpha_wg, evaluation by evaluation.

A fitted alpha cannot see an error of the loss that is constant in alpha, nor one of 1e-6 in the gradient; these tests
look at f and g themselves, in units of EPS S (the sum of the absolute terms, alpha_cases) with the bounds K_D_F = 4 and
K_D_G = 32 derived from the host's measured error (tests/test_alpha_objective_host.py).  A row kernel launched with an
evaluation cap k parks every unfinished gene with its optimiser's state, which holds f and g of the k-th evaluation and
the point of the next: caps 1 ... 10 give the kernel's own trace without restating the optimiser.

Every test prints its worst ratios; the docstrings hold what an MI355X gave (DESIGN section 7c has the table)."""
import math

import numpy as np
import pytest

from tests import alpha_cases as ac

gpu = pytest.mark.gpu
COMBOS = ((True, False), (True, True), (False, True), (False, False))  # (cr_reg, prior_reg)


@pytest.fixture(scope="module")
def du():
    from tests import devunit

    devunit.lib()
    return devunit


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def by_gene(cases):
    """eval_cases grouped: [(name, y, mu, X, cell_of, Xc, [la], la_hat, prior_var)]"""
    out = {}
    for name, y, mu, X, cell_of, Xc, la, lah, pv in cases:
        out.setdefault(name, (name, y, mu, X, cell_of, Xc, [], lah, pv))[6].append(la)
    return list(out.values())


# ------------------------------------------------------------------------------------------------ (a) alpha_eval
def _inst_id(i):
    return f"P{i[0]}-grad{i[1]}-pad{i[2]}-nb{i[3]}-cell{i[4]}"


def _all_inst():
    from tests.devunit import EVAL_INST

    return EVAL_INST


@gpu
@pytest.mark.parametrize("inst", _all_inst(), ids=_inst_id)
def test_alpha_eval_device_against_mpmath(du, inst):
    """alpha_eval<DeviceWave, P, GRAD, PAD, NB, CELL> on every gene of alpha_cases.eval_cases that the memo of NB blocks
    covers (NB = 4: all of them, the counts >= 256 on the BIG path), at four values of la each and with every combination
    of the Cox-Reid and the prior term: the 64 lanes return one bit pattern, f and g lie within K_D EPS S of mpmath.
    Measured over the 39 instantiations: worst f 0.91 EPS S_f (a one-sample gene whose loss is one product; 0.86 beyond
    it), worst g 1.22 EPS S_g (N = 150 at alpha = N)."""
    P, grad, pad, nb, cell = inst
    worst_f, worst_g = (0.0, None), (0.0, None)
    n_genes = 0
    for name, y, mu, X, cell_of, Xc, las, lah, pv in by_gene(ac.eval_cases(P, cells=bool(cell))):
        if nb < 4 and ac.required_nb(y) > nb:
            continue
        n_genes += 1
        G = len(las)
        yy, mm = np.tile(y, (G, 1)), np.tile(mu, (G, 1))
        for cr, pr in COMBOS:
            if cell and not cr:
                continue  # (without the Cox-Reid term the cell path has nothing of its own)
            f, g, cst = du.alpha_eval(inst, yy, mm, X, las, lah, pv, cr, pr, cell_of=cell_of, Xc=Xc)
            for k, la in enumerate(las):
                assert (bits(f[k]) == bits(f[k, 0])).all() and (bits(g[k]) == bits(g[k, 0])).all(), (name, la, cr, pr)
                fr, gr, Sf, Sg = ac.objective(y, mu, X, la, lah, pv, cr, pr)
                rf = ac.ratio(f[k, 0], fr, Sf)
                if rf > worst_f[0]:
                    worst_f = (rf, (name, la, cr, pr))
                if grad:
                    rg = ac.ratio(g[k, 0], gr, Sg)
                    if rg > worst_g[0]:
                        worst_g = (rg, (name, la, cr, pr))
                else:
                    assert g[k, 0] == 0.0
    print(f"alpha_eval{inst}: {n_genes} genes, worst f {worst_f[0]:.3f} EPS S_f at {worst_f[1]}, "
          f"worst g {worst_g[0]:.3f} EPS S_g at {worst_g[1]}")
    assert n_genes >= 3
    assert worst_f[0] <= ac.K_D_F, worst_f
    assert worst_g[0] <= ac.K_D_G, worst_g


# ------------------------------------------------------------------------------------------------ (b) alpha_const
@gpu
def test_alpha_const_and_alpha_const_max(du):
    """alpha_const and alpha_const_max agree bit for bit in every lane (the header's claim), the largest count is right
    and the constant is within K_D_F EPS (sum |lgamma(y+1)| + |y log mu|) of mpmath; counts up to 65 533 included.
    Measured: worst 0.36 EPS S."""
    worst = (0.0, None)
    seen_big = False
    for name, y, mu, *_ in by_gene(ac.eval_cases(1) + ac.eval_cases(4)):
        c, cm, mx = du.alpha_const(y[None, :], mu[None, :])
        assert same_bits(c, cm), name
        assert (bits(c) == bits(c[0, 0])).all(), name
        assert (mx == int(y.max())).all(), (name, mx[0, :4], y.max())
        ref, S = ac.nll_constant(y, mu)
        r = ac.ratio(c[0, 0], ref, S) if S > 0 else abs(c[0, 0])
        seen_big |= y.max() >= 256
        if r > worst[0]:
            worst = (r, name)
    print(f"alpha_const: worst {worst[0]:.3f} EPS S at {worst[1]}")
    assert seen_big
    assert worst[0] <= ac.K_D_F, worst


# ------------------------------------------------------------------------------------------------ (c) row kernels
def _row_kw(case, ah):
    kw = dict(route=case["route"], y=case["y"], sf=case["sf"], cell_of=case["cell_of"], Xc=case["Xc"], alpha_hat=ah,
              min_disp=case["min_disp"], max_disp=case["max_disp"], min_mu=case["min_mu"])
    if case["route"] == "cell_mu":
        kw["cell_mu"] = case["cell_mu"]
    else:
        kw["coef"] = case["coef"]
    return kw


def _whole(r, G):
    """an uncapped launch wrote every gene, parked none, and listed exactly the unconverged genes"""
    assert r["park_count"] == 0
    assert (bits(r["alpha"]) != bits(np.float64(-7.0))).all() and (r["conv"] <= 1).all() and (r["nfev"] >= 1).all()
    assert r["grid_count"] == int((r["conv"] == 0).sum())
    assert sorted(r["grid"].tolist()) == np.flatnonzero(r["conv"] == 0).tolist()


@gpu
@pytest.mark.parametrize("run", ac.ROW_RUNS, ids=ac.row_run_id)
def test_row_kernels_evaluation_by_evaluation(du, run):
    """k_alpha_rows<P> / k_alpha_rows_c<P> uncapped, then with eval_cap = 1 ... 10:
      * the genes parked at cap k are exactly those whose uncapped fit took more than k evaluations, and every other gene
        has the uncapped run's alpha, conv and nfev bit for bit (parking leaves the sequence of iterates unchanged);
      * the state parked at cap k holds f and g of the k-th evaluation, made at the point the state of cap k - 1 holds
        (cap 1: the clipped log alpha_hat): both within K_D EPS S of mpmath at that point;
      * the stored NLL constant against mpmath; a run that loads it reproduces the run that computes it bit for bit.
    Evaluations after which the optimiser holds an earlier loss value again (it restored an iterate, or evaluated a point
    twice) are left out: at most 1 % of the pairs, none expected.
    Measured over the 13 runs: worst f 0.75 EPS S_f, worst g 2.88 EPS S_g (always the second evaluation, at the upper
    bound alpha = max(10, N)), constant 0.47 EPS S, no evaluation left out."""
    spec, prior = run
    case = ac.row_case(*spec, n_genes=ac.row_genes(spec))
    G = case["G"]
    if spec[0] == "rows":
        assert du.row_tail() == ac.ROW_TAIL
    else:
        assert du.rowsc_tail(spec[3], spec[1], spec[2]) == case["tail"]
    ah = ac.choose_alpha_hat(case, prior, ac.ROW_PRIOR_VAR)
    kw = dict(_row_kw(case, ah), prior_reg=prior, prior_var=ac.ROW_PRIOR_VAR)
    full = du.rows_trace(**kw, const_mode=du.CONST_STORE)
    _whole(full, G)
    worst_c = 0.0
    for g in range(G):
        ref, S = ac.nll_constant(case["y"][g], case["mu"][g])
        worst_c = max(worst_c, ac.ratio(full["nll_const"][g], ref, S))
    comp = du.rows_trace(**kw, const_mode=du.CONST_COMPUTE)
    load = du.rows_trace(**kw, const_mode=du.CONST_LOAD, nll_const=full["nll_const"])
    for r in (comp, load):
        _whole(r, G)
        for key in ("alpha", "conv", "nfev"):
            assert same_bits(r[key], full[key]), key
    assert np.isnan(comp["nll_const"]).all() and same_bits(load["nll_const"], full["nll_const"])

    lo, hi = math.log(case["min_disp"]), math.log(case["max_disp"])
    x_prev = np.minimum(np.maximum(np.log(ah), lo), hi)
    seen_f = [[] for _ in range(G)]
    worst_f, worst_g = (0.0, None), (0.0, None)
    pairs = left_out = 0
    for k in range(1, 11):
        r = du.rows_trace(**kw, eval_cap=k)
        expect = np.flatnonzero(full["nfev"] > k)
        assert sorted(r["parked"].tolist()) == expect.tolist(), (k, r["parked"], full["nfev"])
        if k == 1:
            assert expect.size == G  # |g(log alpha_hat)| > 1e-3 by the reference: nobody stops at the first evaluation
        rest = np.setdiff1d(np.arange(G), expect)
        for key in ("alpha", "conv", "nfev"):
            assert same_bits(r[key][rest], full[key][rest]), (k, key)
            assert (r[key][expect] == {"alpha": du.SENT_D, "conv": du.SENT_U8, "nfev": du.SENT_I}[key]).all(), (k, key)
        assert sorted(r["grid"].tolist()) == [g for g in rest.tolist() if full["conv"][g] == 0]
        st = r["state"]
        for g in expect.tolist():
            assert st["nfev"][g] == k and st["done"][g] == 0, (k, g, st["nfev"][g])
            fk, gk = st["f"][g], st["g"][g]
            pairs += 1
            if any(bits(fk) == bits(v) for v in seen_f[g]):
                left_out += 1
            else:
                fr, gr, Sf, Sg = ac.objective(case["y"][g], case["mu"][g], case["X"], x_prev[g], math.log(ah[g]),
                                              ac.ROW_PRIOR_VAR, True, prior)
                rf, rg = ac.ratio(fk, fr, Sf), ac.ratio(gk, gr, Sg)
                if rf > worst_f[0]:
                    worst_f = (rf, (g, k, x_prev[g]))
                if rg > worst_g[0]:
                    worst_g = (rg, (g, k, x_prev[g]))
            seen_f[g].append(fk)
            x_prev[g] = st["x"][g]
    print(f"{ac.row_run_id(run)}: {pairs} evaluations, {left_out} left out, "
          f"worst f {worst_f[0]:.3f} EPS S_f at (gene, evaluation, la) "
          f"{worst_f[1]}, worst g {worst_g[0]:.3f} EPS S_g at {worst_g[1]}, worst constant {worst_c:.3f} EPS S")
    assert pairs >= 3 * G
    assert left_out <= 0.01 * pairs
    assert worst_c <= ac.K_D_F
    assert worst_f[0] <= ac.K_D_F, worst_f
    assert worst_g[0] <= ac.K_D_G, worst_g


# ------------------------------------------------------------------------------------------------ (d) slots and queue
@gpu
def test_row_slots_refilled_from_the_queue_are_independent_of_their_history(du):
    """More genes than the persistent grid of k_alpha_rows has slots (16 per workgroup, two workgroups per compute
    unit): rows refill from the queue, and the list alternates high-count genes (second sweep, long tail table) with genes
    that are zero but for one small count.  Every gene is written exactly once, all replicas of a gene are bitwise equal
    and equal to its result in a launch of the 50 distinct genes alone, and the grid list holds exactly the genes whose
    fit did not converge."""
    case = ac.queue_case()
    D = case["G"]
    base = du.rows_trace("rows", case["y"], case["sf"], case["cell_of"], case["Xc"], case["alpha_hat"], case["min_disp"],
                         case["max_disp"], case["min_mu"], coef=case["coef"])
    _whole(base, D)
    G = 32 * du.cus() + 37
    idx = np.arange(G) % D
    r = du.rows_trace("rows", case["y"][idx], case["sf"], case["cell_of"], case["Xc"], case["alpha_hat"][idx],
                      case["min_disp"], case["max_disp"], case["min_mu"], coef=case["coef"][idx])
    _whole(r, G)
    assert np.unique(r["grid"]).size == r["grid"].size
    for key in ("alpha", "conv", "nfev"):
        assert same_bits(r[key], base[key][idx]), key
    assert (base["nfev"] > 1).sum() >= D // 2 and (case["y"].max(1) >= 512).sum() == D // 2


# ------------------------------------------------------------------------------------------------ (e) k_alpha_wg
@gpu
@pytest.mark.parametrize("N", [100, 1025, 2049])
@pytest.mark.parametrize("P", [2, 4])
def test_alpha_wg_continues_the_parked_fits(du, P, N):
    """k_alpha_wg (256, 512 and 1024 threads at N = 100, 1025, 2049) on the states k_alpha_rows<P> parked at caps 1, 2
    and 8: every parked gene is written once and no other, the grid list is {conv = 0}, nfev > cap; against the uncapped
    row kernel the rule for two summation orders of one objective holds (conv equal for > 97 % of the genes, relative
    alpha difference > 1e-6 for <= 3 % of them and < 5e-3 for all); and by mpmath the loss at the returned alpha is not
    above the loss at alpha_hat by more than K_D_F EPS S_f."""
    n_genes = 12 if N == 100 else 8
    case = ac.row_case("rows", P, P, N, n_genes=n_genes)
    G = case["G"]
    s = np.where(np.arange(G) % 2 == 0, 1.0, -1.0)
    ah = np.clip(case["alpha_true"] * np.exp(s), 2 * case["min_disp"], case["max_disp"] / 2)
    args = (case["y"], case["sf"], case["cell_of"], case["Xc"], ah, case["min_disp"], case["max_disp"], case["min_mu"])
    full = du.rows_trace("rows", *args, coef=case["coef"])
    _whole(full, G)
    n_checked = 0
    for cap in (1, 2, 8):
        r = du.alpha_wg(*args, case["coef"], cap)
        parked = np.sort(r["parked"])
        assert parked.tolist() == np.flatnonzero(full["nfev"] > cap).tolist()
        rest = np.setdiff1d(np.arange(G), parked)
        assert (r["wg_alpha"][rest] == du.SENT_D).all() and (r["wg_conv"][rest] == du.SENT_U8).all() and \
            (r["wg_nfev"][rest] == du.SENT_I).all()
        assert (r["wg_alpha"][parked] > 0).all() and (r["wg_conv"][parked] <= 1).all()
        assert (r["wg_nfev"][parked] > cap).all()
        assert r["wg_grid_count"] == r["wg_grid"].size
        assert sorted(r["wg_grid"].tolist()) == [g for g in parked.tolist() if r["wg_conv"][g] == 0]
        if parked.size:
            a, b = r["wg_alpha"][parked], full["alpha"][parked]
            rel = np.abs(a - b) / b
            assert (r["wg_conv"][parked] == full["conv"][parked]).mean() > 0.97
            assert (rel > 1e-6).mean() <= 0.03 and (rel < 5e-3).all(), rel
        for g in parked.tolist():
            y, mu, X = case["y"][g], case["mu"][g], case["X"]
            f0, _, S0, _ = ac.objective(y, mu, X, float(np.log(ah[g])))
            f1, _, S1, _ = ac.objective(y, mu, X, float(np.log(r["wg_alpha"][g])))
            assert float(f1 - f0) <= ac.K_D_F * ac.EPS * max(S0, S1), (cap, g, float(f1 - f0))
            n_checked += 1
    assert n_checked >= G
