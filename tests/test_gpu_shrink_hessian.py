"""The Hessian and its hand-written Gauss-Jordan inverse as the product's shrinkage kernels compute them, against mpmath
(tests/shrink_cases.py): dsq_dev_lfc_shrink3 -> k_shrink<P, false> for P = 1 ... 12 (one row of
[H | I] per lane, logical positions exchanged), the five k_shrink_wide launches at p == PB and p == previous block + 1
(rows exchanged in LDS between barriers; the odd-p tail of the two-rows-per-pass Hessian), and k_shrink<P, true> with
Newton-CG at P = 2 and 12.

The KAT fixtures hold the inverse to 1e-6 of its largest entry and hardly ever exchange a row; the designs here exchange
rows at every width and move the row of the shrink index (proved on the CPU, tests/test_shrink_cases_host.py).  At the
device's own coefficients the reference's Hessian - with its prior curvature broadcast over the rows - is formed and
inverted in mpmath, and

    ||invh_dev - H^-1||_inf <= K_inv EPS kappa_inf ||H^-1||_inf,   K_inv = 32

eight times what numpy.linalg.inv of the oracle's float64 Hessian gives (R_inv = 2.26, measured and asserted in
tests/test_shrink_cases_host.py), rounded up to a power of two: the margin covers the device Hessian's own summation and
exponential, and Gauss-Jordan against LAPACK's LU.  Every test prints its worst ratio."""
import ctypes as C

import numpy as np
import pytest

from oracle import nbglm_oracle as orc
from tests import shrink_cases as sc

pytestmark = pytest.mark.gpu
_vp = C.c_void_p
U8_SENTINEL = 0xEE


@pytest.fixture(scope="module")
def ctx():
    from pydeseq2_amd._lib import Context

    return Context(0)


def launch(ctx, c, inv=True, entry=False, optimizer=0, sidx=None):
    """One dsq_dev_lfc_shrink3 call on a launch of hessian_cases: (beta [G][p], invh [G][p][p] or None, ih_entry [G] or
    None, conv [G]); the outputs hold NaN / 0xEE before the call."""
    from pydeseq2_amd._lib import DeviceArray

    N, G, p = c["N"], c["G"], c["p"]
    d_y = DeviceArray.from_host(ctx, np.ascontiguousarray(c["counts"].T, dtype=np.int32))
    d_off = DeviceArray.from_host(ctx, np.ascontiguousarray(c["offset"]))
    d_Xt = DeviceArray.from_host(ctx, np.ascontiguousarray(c["X"].T))
    d_size = DeviceArray.from_host(ctx, np.ascontiguousarray(c["size"]))
    d_beta = DeviceArray.from_host(ctx, np.full((G, p), np.nan))
    d_ih = DeviceArray.from_host(ctx, np.full((G, p * p), np.nan)) if inv else None
    d_e = DeviceArray.from_host(ctx, np.full(G, np.nan)) if entry else None
    d_conv = DeviceArray.from_host(ctx, np.full(G, U8_SENTINEL, np.uint8))
    ctx.call("dsq_dev_lfc_shrink3", _vp(d_y.ptr), N, _vp(d_off.ptr), _vp(d_Xt.ptr), N, N, G, p, _vp(d_size.ptr),
             C.c_double(sc.SIGMA0), C.c_double(c["sigma"]), int(c["sidx"] if sidx is None else sidx), _vp(d_beta.ptr),
             _vp(d_ih.ptr) if inv else None, _vp(d_conv.ptr), _vp(d_e.ptr) if entry else None, int(optimizer))
    conv = d_conv.to_host()
    assert set(conv.tolist()) <= {0, 1}  # every gene was written
    return (d_beta.to_host(), d_ih.to_host().reshape(G, p, p) if inv else None, d_e.to_host() if entry else None,
            conv.astype(bool))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def inverse_worst(c, b, ih):
    """worst ratio of a launch's inverses against mpmath at the device's coefficients; no gene is left out"""
    assert np.isfinite(b).all() and np.isfinite(ih).all()
    worst = 0.0
    for g in range(c["G"]):
        ref = sc.hessian_ref(c, g, b[g])
        assert ref[2] <= 1e8, (c["p"], c["N"], g, ref[2])
        worst = max(worst, sc.inverse_ratio(ih[g], ref))
    return worst


def against_oracle(b, ih, cv, rb, rih, rcv):
    """the tolerances of tests/test_gpu_summary.py::test_lfc_shrink_inference_vs_reference_kats"""
    assert (cv == rcv).all()
    np.testing.assert_allclose(b, rb, rtol=1e-5, atol=1e-8)
    scale = np.abs(rih).max(axis=(1, 2), keepdims=True)
    assert np.max(np.abs(ih - rih) / scale) < 1e-6


@pytest.mark.parametrize("p", sc.HESS_P)
def test_inverse_hessian_against_mpmath(ctx, p):
    worst = 0.0
    for c, (rb, rih, rcv, _) in zip(sc.hessian_cases(p), sc.oracle_fits(p)):
        b, ih, _, cv = launch(ctx, c)
        b2, ih2, _, cv2 = launch(ctx, c)
        assert same_bits(b, b2) and same_bits(ih, ih2) and same_bits(cv, cv2)  # two consecutive runs
        if p <= 12:
            # the three forms of the launch: the whole inverse, the one entry the pipeline uses, both
            be, _, ee, cve = launch(ctx, c, inv=False, entry=True)
            bb, ihb, eb, cvb = launch(ctx, c, inv=True, entry=True)
            assert same_bits(b, be) and same_bits(b, bb) and same_bits(cv, cve) and same_bits(cv, cvb)
            assert same_bits(ih, ihb) and same_bits(ee, eb)
            assert same_bits(ee, np.ascontiguousarray(ih[:, c["sidx"], c["sidx"]]))
        r = inverse_worst(c, b, ih)
        print(f"k_shrink p = {p}, N = {c['N']}, G = {c['G']}, index {c['sidx']}, scale {c['sigma']}: inverse {r:.4f}")
        worst = max(worst, r)
        against_oracle(b, ih, cv, rb, rih, rcv)
    print(f"k_shrink p = {p}: worst inverse ratio {worst:.4f} (K_inv = {sc.K_INV:g})")
    assert worst <= sc.K_INV


@pytest.mark.parametrize("p", range(1, 13))
def test_ih_entry_is_the_diagonal_entry_for_every_shrink_index(ctx, p):
    """ih_entry is written by the lane whose row ends at the position of the shrink index: every index, on the launch of
    the width whose design starts the saw-tooth at its largest scale"""
    c = sc.hessian_cases(p)[0]
    for s in range(p):
        b, ih, e, cv = launch(ctx, c, inv=True, entry=True, sidx=s)
        assert np.isfinite(b).all() and np.isfinite(ih).all()
        assert same_bits(e, np.ascontiguousarray(ih[:, s, s])), (p, s)


@pytest.mark.parametrize("p", [2, 12])
def test_newton_cg_inverse_against_mpmath(ctx, p):
    """k_shrink<P, true>: the same inverse behind the other optimiser's workspace"""
    worst = 0.0
    for c in sc.hessian_cases(p):
        b, ih, _, cv = launch(ctx, c, optimizer=2)
        b2, ih2, _, cv2 = launch(ctx, c, optimizer=2)
        assert same_bits(b, b2) and same_bits(ih, ih2) and same_bits(cv, cv2)
        worst = max(worst, inverse_worst(c, b, ih))
        r = [orc.nbinom_glm_gene(c["X"], c["counts"][:, g].astype(np.float64), c["size"][g], c["offset"], sc.SIGMA0,
                                 c["sigma"], c["sidx"], optimizer="Newton-CG") for g in range(c["G"])]
        against_oracle(b, ih, cv, np.array([x[0] for x in r]), np.array([x[1] for x in r]), np.array([x[2] for x in r], bool))
    print(f"k_shrink<{p}, Newton-CG>: worst inverse ratio {worst:.4f} (K_inv = {sc.K_INV:g})")
    assert worst <= sc.K_INV
