"""The shrinkage cases are what they claim, the references' own error, and the host build of dsq_shrink.h against mpmath
(tests/shrink_cases.py).  Needs no GPU.

The KAT fixtures hardly ever exchange a row in the hand-written Gauss-Jordan inverse and never evaluate the objective at its
edges; the cases of tests/shrink_cases.py do, and the first tests here prove it with a plain model on the oracle's fit.
The bounds the DEVICE tests assert (tests/test_devunit_shrink.py, tests/test_gpu_shrink_hessian.py) are derived from the
reference's own error, which is measured and asserted here."""
import functools

import numpy as np
import pytest

from tests import hostsim as hs
from tests import shrink_cases as sc


# ------------------------------------------------------------------------------------------------ the cases
def _exchanges(p):
    """per gene of hessian_cases(p): (launch, gene, exchanges, the shrink row moved)"""
    out = []
    for c, (b, ih, cv, H) in zip(sc.hessian_cases(p), sc.oracle_fits(p)):
        for g in range(c["G"]):
            sw = sc.gauss_jordan(H[g])[1]
            out.append((c, g, sw, sc.moves_row(sw, c["sidx"])))
    return out


def test_gauss_jordan_model():
    """the model inverts, reports the exchanges it makes and breaks ties towards the diagonal"""
    H = np.array([[1.0, 2.0, 0.0], [4.0, 1.0, 1.0], [-4.0, 0.0, 3.0]])
    inv, sw = sc.gauss_jordan(H)
    np.testing.assert_allclose(inv @ H, np.eye(3), atol=1e-15)
    assert sw[0] == (0, 1)  # |-4| is not strictly greater than |4|
    assert sc.gauss_jordan(np.diag([3.0, 2.0, 1.0]))[1] == []
    assert sc.moves_row([(0, 1)], 1) and sc.moves_row([(0, 1)], 0) and not sc.moves_row([(0, 1)], 2)


@pytest.mark.parametrize("p", [q for q in sc.HESS_P if q > 1])
def test_every_width_exchanges_rows_and_moves_the_shrink_row(p):
    """(a 1 x 1 matrix has no row to exchange: P = 1 is left out of this claim alone)"""
    ex = _exchanges(p)
    assert any(sw for _, _, sw, _ in ex)
    assert any(mv for _, _, _, mv in ex)
    assert {c["sidx"] for c, _, _, _ in ex} == {0, p - 1, p // 2}
    assert {c["sigma"] for c, _, _, _ in ex} == set(sc.HESS_SIGMAS)


def test_every_elimination_column_of_the_register_widths_is_exchanged():
    cols = {}
    for p in range(2, 13):
        for _, _, sw, _ in _exchanges(p):
            for c, _ in sw:
                cols.setdefault(c, set()).add(p)
    assert sorted(cols) == list(range(11)), cols  # columns 0 ... P - 2 of the widest register design
    assert len({c for _, _, sw, _ in _exchanges(12) for c, _ in sw}) >= 5  # (many columns within one width, too)
    assert {c["N"] for p in sc.HESS_P for c in sc.hessian_cases(p)} == {5, 64, 65, 130}


@pytest.mark.parametrize("p", sc.HESS_P)
def test_hessian_cases_are_fitted_and_conditioned(p):
    for c, (b, ih, cv, H) in zip(sc.hessian_cases(p), sc.oracle_fits(p)):
        assert np.isfinite(b).all() and cv.all()
        for g in range(c["G"]):
            kappa = np.linalg.norm(H[g], np.inf) * np.linalg.norm(np.linalg.inv(H[g]), np.inf)
            assert kappa <= 1e6, (p, c["N"], g, kappa)


def test_objective_cases_cover_their_claims():
    kinds, narrow_idx, wide_idx, shapes = set(), {}, {}, set()
    dlo, dhi, near = 0.0, 0.0, False
    for p in sc.NARROW_P + sc.WIDE_P:
        for c, refs in zip(sc.objective_cases(p), sc.objective_refs(p)):
            shapes.add((c["N"], c["G"]))
            for k in range(c["G"]):
                f, g, Sf, Sg, dmin, dmax = refs[k]
                assert np.isfinite(float(f)) and np.isfinite([float(v) for v in g]).all() and np.isfinite(Sf)
                kinds.add((c["counts"][k], c["beta"][k]))
                kinds.add(("size", float(c["size"][k]), float(c["sigma"][k])))
                (narrow_idx if p <= 12 else wide_idx).setdefault(p, set()).add(int(c["sidx"][k]))
                dlo, dhi = min(dlo, dmin), max(dhi, dmax)
                if c["beta"][k] == "switch":
                    eta = c["X"][k] @ c["b"][k]
                    d = eta + c["offset"][k] - np.log(c["size"][k])
                    near |= bool((np.abs(d) <= 1.0001e-9).sum() >= 1 and (d > 0).any() and (d < 0).any())
    assert {(ck, bk) for ck in sc.COUNT_KINDS for bk in sc.BETA_KINDS} <= kinds
    assert {("size", s, g) for s in sc.SIZES for g in sc.SIGMAS} <= kinds
    assert all(narrow_idx[p] == set(range(p)) for p in sc.NARROW_P)
    assert all(wide_idx[p] == {0, p // 2, p - 1} for p in sc.WIDE_P)
    assert {n for n, _ in shapes} == {3, 63, 64, 65, 130} and {g for _, g in shapes} == {1, 5, 9}
    assert dlo < -746 and dhi > 746 and near
    ys = np.concatenate([c["y"].ravel() for p in sc.NARROW_P for c in sc.objective_cases(p)])
    assert {0, 1, 255, 256, 65535, 65536, sc.INT_MAX} <= set(ys.tolist())


# ------------------------------------------------------------------------------------------------ the references' error
def _oracle_fn(c):
    r = [sc.oracle_objective(c, k) for k in range(c["G"])]
    return np.array([x[0] for x in r]), np.array([x[1] for x in r])


def _host_fn(c):
    f0, f1, g = hs.shrink_fn(c["y"], c["offset"], c["X"], c["size"], sc.SIGMA0, c["sigma"], c["sidx"], c["b"], c["inst"])
    assert f0.view(np.int64).tolist() == f1.view(np.int64).tolist()  # the loss-only call returns the same bits
    assert np.isnan(g[:, c["p"]:]).all() and not np.isnan(g[:, :c["p"]]).any() and not np.isnan(f0).any()
    return f1, g


@functools.lru_cache(maxsize=None)
def objective_worst(which, p):
    """worst (f, g) ratio of the oracle ("oracle") or of the host build ("host") over the launches of width p"""
    wf = wg = 0.0
    for c, refs in zip(sc.objective_cases(p), sc.objective_refs(p)):
        f, g = (_oracle_fn if which == "oracle" else _host_fn)(c)
        a, b = sc.objective_ratios(c, refs, f, g)
        wf, wg = max(wf, a), max(wg, b)
    return wf, wg


@pytest.mark.parametrize("p", sc.NARROW_P + sc.WIDE_P)
def test_objective_against_mpmath(p):
    """numpy's evaluation of the reference's formulas (R_f, R_g), and the host build: shrink_fn<HostWave, P> and the
    run-time-p shrink_fn_wide<HostWave, PMAX, PB> at p < PB and p == PB, every value finite"""
    (rf, rg), (hf, hg) = objective_worst("oracle", p), objective_worst("host", p)
    print(f"objective p = {p:2d}: oracle f {rf:.4f}, g {rg:.4f}; host f {hf:.4f}, g {hg:.4f}")
    assert rf <= sc.R_F and rg <= sc.R_G and hf <= sc.K_H_F and hg <= sc.K_H_G


def test_recorded_objective_constants():
    """the recorded worst ratios are upper bounds of those measured, within a few percent, and the bounds follow from them"""
    ps = sc.NARROW_P + sc.WIDE_P
    rf, rg = (max(objective_worst("oracle", p)[i] for p in ps) for i in (0, 1))
    hf, hg = (max(objective_worst("host", p)[i] for p in ps) for i in (0, 1))
    print(f"objective: R_f = {rf:.4f}, R_g = {rg:.4f}; host f {hf:.4f}, g {hg:.4f}")
    assert rf <= sc.R_F <= 1.05 * rf and rg <= sc.R_G <= 1.05 * rg
    assert hf <= sc.HOST_F <= 1.05 * hf and hg <= sc.HOST_G <= 1.05 * hg
    assert sc.K_F == sc.pow2_ceil(4 * sc.R_F) and sc.K_G == sc.pow2_ceil(4 * sc.R_G)
    assert sc.K_H_F == sc.pow2_ceil(sc.HOST_F) and sc.K_H_G == sc.pow2_ceil(sc.HOST_G)


@functools.lru_cache(maxsize=None)
def host_fits(p):
    """hostsim.shrink on the Hessian cases of width p: [(beta, invh, conv) per launch]"""
    return [hs.shrink(c["counts"], c["X"], c["size"], c["offset"], sc.SIGMA0, c["sigma"], c["sidx"])
            for c in sc.hessian_cases(p)]


@pytest.mark.parametrize("p", sc.HESS_P)
def test_host_fit_matches_the_oracle(p):
    """beta and flags at the tolerance tests/test_hostsim.py holds the KAT fixtures to"""
    for c, (b, ih, cv), (rb, rih, rcv, _) in zip(sc.hessian_cases(p), host_fits(p), sc.oracle_fits(p)):
        assert (cv == rcv).all()
        np.testing.assert_allclose(b, rb, rtol=1e-6, atol=1e-9)
        scale = np.abs(rih).max(axis=(1, 2), keepdims=True)
        assert np.max(np.abs(ih - rih) / scale) < 1e-8


@functools.lru_cache(maxsize=None)
def inverse_ratios(p):
    """worst ratio of numpy.linalg.inv of the oracle's Hessian and of the host build's Gauss-Jordan, each against mpmath's
    inverse at its own coefficients; and the largest condition number at the host's coefficients"""
    r_ref = r_host = kappa = 0.0
    for c, (b, ih, cv), (rb, rih, rcv, H) in zip(sc.hessian_cases(p), host_fits(p), sc.oracle_fits(p)):
        for g in range(c["G"]):
            r_ref = max(r_ref, sc.inverse_ratio(np.linalg.inv(H[g]), sc.hessian_ref(c, g, rb[g])))
            ref = sc.hessian_ref(c, g, b[g])
            kappa = max(kappa, ref[2])
            r_host = max(r_host, sc.inverse_ratio(ih[g], ref))
    return r_ref, r_host, kappa


@pytest.mark.parametrize("p", sc.HESS_P)
def test_inverses_against_mpmath(p):
    """R_inv, and the host build's inverse: the Wv::W == 1 version up to 12 columns, the run-time-p one beyond"""
    r_ref, r_host, kappa = inverse_ratios(p)
    print(f"inverse p = {p:2d}: numpy.linalg.inv {r_ref:.4f}, host {r_host:.4f}, kappa {kappa:.3g}")
    assert kappa <= 1e8 and r_ref <= sc.R_INV and r_host <= sc.K_H_INV


def test_recorded_inverse_constants():
    """the recorded worst ratios are those measured, and the bounds follow from them"""
    r = [inverse_ratios(p) for p in sc.HESS_P]
    r_ref, r_host = max(v[0] for v in r), max(v[1] for v in r)
    print(f"inverse: R_inv = {r_ref:.4f}, host {r_host:.4f}")
    assert r_ref <= sc.R_INV <= 1.05 * r_ref and r_host <= sc.HOST_INV <= 1.05 * r_host
    assert sc.K_INV == sc.pow2_ceil(8 * sc.R_INV) and sc.K_H_INV == sc.pow2_ceil(sc.HOST_INV)
