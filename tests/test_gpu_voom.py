"""limma-voom on the GPU: k_voom_fit1 and the per-sample part of k_voom_wls against the host build bit for bit, beta,
sigma2, est and u against the host build and the reference within the measured bounds, guards behind every output, reruns,
the C entry's refusals, and the façade end to end against tests/voom_ref.py."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import hostvoom as hv
from tests import voom_ref as vr
from tests.ql_cases import F_SF_C_DEVICE
from tests.voom_cases import (EPS, KERNEL_G, KERNEL_K, KERNEL_P, VOOM_C_DEVICE, VOOM_C_E, VOOM_C_HOST, VOOM_C_REL_DEVICE,
                              VOOM_C_REL_HOST, check_against_reference, kernel_case, kernel_N, scenario_design,
                              voom_scenario)

pytestmark = pytest.mark.gpu

_vp = C.c_void_p
GUARD = -7.0


@pytest.fixture(scope="module")
def ctx():
    from pydeseq2_amd._lib import Context

    return Context(0)


class Dev:
    """The inputs of one kernel case on the device (G genes), outputs with a guard value behind their end."""

    def __init__(self, ctx, kc, G, K):
        from pydeseq2_amd._design import pad16
        from pydeseq2_amd._lib import DeviceArray

        self.ctx, self.G, self.K = ctx, G, K
        counts = kc["counts"][:, :G]
        self.N, self.P = N, P = counts.shape[0], kc["X"].shape[1]
        self.ldn = ldn = pad16(N)
        y = np.zeros((G, ldn), np.int32)
        y[:, :N] = counts.T
        Xt, pinv = np.zeros((P, ldn)), np.zeros((P, ldn))
        Xt[:, :N], pinv[:, :N] = kc["X"].T, kc["pinv"]
        up = lambda a: DeviceArray.from_host(ctx, np.ascontiguousarray(a))  # noqa: E731
        self.nk = len(kc["kx"])
        self.d = dict(y=up(y), off=up(kc["off"]), Xt=up(Xt), pinv=up(pinv), kx=up(kc["kx"]), ky=up(kc["ky"]),
                      c=up(kc["contrasts"][:K]))
        self.n1 = G * P + 2 * G
        self.o1 = up(np.full(self.n1 + 3, GUARD))
        self.n2 = G * P + G + 2 * G * K
        self.o2 = up(np.full(self.n2 + 3, GUARD))
        self.lay = up(np.full((2 * G + 1) * ldn, GUARD))

    def fit1(self):
        d, G, P = self.d, self.G, self.P
        p = self.o1.ptr
        self.ctx.call("dsq_dev_voom_fit1", _vp(d["y"].ptr), self.ldn, _vp(d["off"].ptr), _vp(d["Xt"].ptr), _vp(d["pinv"].ptr),
                      self.ldn, P, self.N, G, _vp(p), _vp(p + 8 * G * P), _vp(p + 8 * (G * P + G)))
        o = self.o1.to_host()
        assert (o[self.n1:] == GUARD).all()
        return o[:G * P].reshape(G, P), o[G * P:G * P + G], o[G * P + G:self.n1]

    def wls(self, layers):
        d, G, P, K, ldn = self.d, self.G, self.P, self.K, self.ldn
        p, q = self.o2.ptr, self.lay.ptr
        off = [0, G * P, G * P + G, G * P + G + G * K]
        self.ctx.call("dsq_dev_voom_wls", _vp(d["y"].ptr), ldn, _vp(d["off"].ptr), _vp(d["Xt"].ptr), ldn, P, self.N, G,
                      _vp(self.o1.ptr), _vp(d["kx"].ptr), _vp(d["ky"].ptr), self.nk, _vp(d["c"].ptr), K, *(_vp(p + 8 * o) for o in off),
                      _vp(q) if layers else None, _vp(q + 8 * G * ldn) if layers else None, ldn if layers else 0)
        o = self.o2.to_host()
        assert (o[self.n2:] == GUARD).all()
        lay = self.lay.to_host()
        assert (lay[2 * G * ldn:] == GUARD).all()
        E = w = None
        if layers:
            lay = lay[:2 * G * ldn].reshape(2, G, ldn)
            assert (lay[:, :, self.N:] == GUARD).all()  # the padding of every row is left alone
            E, w = lay[0, :, :self.N].copy(), lay[1, :, :self.N].copy()
        else:
            assert (lay == GUARD).all()
        return (o[:off[1]].reshape(G, P), o[off[1]:off[2]], o[off[2]:off[3]].reshape(G, K), o[off[3]:self.n2].reshape(G, K),
                E, w)

    def free(self):
        for a in list(self.d.values()) + [self.o1, self.o2, self.lay]:
            a.free()


_host_cache = {}


def _host(N, P):
    if (N, P) not in _host_cache:
        kc = kernel_case(N, P)
        b1, am, s1 = hv.fit1(kc["counts"], kc["off"], kc["X"], kc["pinv"])
        host = (b1, am, s1) + hv.wls(kc["counts"], kc["off"], kc["X"], b1, kc["kx"], kc["ky"], kc["contrasts"], layers=True)
        _host_cache[(N, P)] = host, vr.wls(kc["counts"], kc["X"], kc["L"], b1, kc["kx"], kc["ky"], kc["contrasts"])
    return _host_cache[(N, P)]


@pytest.mark.parametrize("P", KERNEL_P)
@pytest.mark.parametrize("Nk", range(6))
def test_kernels_against_host_build_and_reference(ctx, Nk, P):
    """Every combination of N in {P + 1, 63, 64, 65, 129, 1000}, P, G in {1, 3, 4, 5, 257} and K in {1, 3}; rows containing
    zeros and one gene without counts.  k_voom_fit1 (beta1, Abar, sigma1) and the layers E and w of k_voom_wls equal the
    host build EXACTLY; beta, sigma2, est, u agree with the host build within the sum of both bounds and with the reference
    within the device bound; a guard value behind every output is untouched, with and without the layers; a rerun into
    the same buffers gives identical bits."""
    N = kernel_N(P)[Nk]
    kc = kernel_case(N, P)
    (hb1, ham, hs1, hbeta, hs2, hest, hu, hE, hw), full_ref = _host(N, P)
    eq = lambda a, b: np.array_equal(a, b, equal_nan=True)  # noqa: E731
    for G in KERNEL_G:
        for K in KERNEL_K:
            dv = Dev(ctx, kc, G, K)
            try:
                b1, am, s1 = dv.fit1()
                assert eq(b1, hb1[:G]) and eq(am, ham[:G]) and eq(s1, hs1[:G]), (G, K, "fit1")
                assert G == 1 or np.isnan(b1[1]).all()
                plain = dv.wls(False)
                got = dv.wls(True)
                again = dv.wls(True)
                for a, b, c in zip(plain[:4], got[:4], again[:4]):
                    assert eq(a, b) and eq(b, c), (G, K, "layers on / off / rerun")
                assert eq(got[4], again[4]) and eq(got[5], again[5])
                assert eq(got[4], hE[:G]) and eq(got[5], hw[:G]), (G, K, "layers against the host build")
                beta, s2, est, u = got[:4]
                live = ~np.isnan(hs2[:G])
                assert eq(np.isnan(s2), ~live) and np.isnan(beta[~live]).all() and np.isnan(est[~live]).all()
                _, ref = check_against_reference(kc, (b1, am, s1) + got, VOOM_C_DEVICE, VOOM_C_REL_DEVICE,
                                                 f"device N={N} P={P} G={G} K={K}", G=G, K=K, ref=full_ref)
                kap, nb = ref["kappa"][live], np.linalg.norm(ref["beta"][live], axis=1)
                both = (VOOM_C_DEVICE + VOOM_C_HOST) * EPS
                assert (np.linalg.norm(beta[live] - hbeta[:G][live], axis=1) <= both * kap * nb).all()
                cn = np.linalg.norm(kc["contrasts"][:K], axis=1)
                assert (np.abs(est[live] - hest[:G, :K][live]) <= both * (kap * nb)[:, None] * cn[None, :]).all()
                assert (np.abs(u[live] - hu[:G, :K][live]) <= both * kap[:, None] * hu[:G, :K][live]).all()
                assert (np.abs(s2[live] - hs2[:G][live]) <= (VOOM_C_REL_DEVICE + VOOM_C_REL_HOST) * EPS * hs2[:G][live]).all()
            finally:
                dv.free()


@pytest.mark.parametrize("nk", [2, 256])
def test_knot_tables_of_2_and_256(ctx, nk):
    """The smallest and the largest table: the layers equal the host build's bits."""
    kc = dict(kernel_case(65, 2))
    kc["kx"] = np.linspace(-1.0, 13.0, nk)
    kc["ky"] = 0.5 + 1.0 / (1.0 + np.exp(0.5 * (kc["kx"] - 5.0)))
    dv = Dev(ctx, kc, 5, 1)
    try:
        b1, _, _ = dv.fit1()
        got = dv.wls(True)
        want = hv.wls(kc["counts"][:, :5], kc["off"], kc["X"], b1, kc["kx"], kc["ky"], kc["contrasts"][:1], layers=True)
        assert np.array_equal(got[4], want[4], equal_nan=True) and np.array_equal(got[5], want[5], equal_nan=True)
        check_against_reference(kc, (b1, None, None) + got, VOOM_C_DEVICE, VOOM_C_REL_DEVICE, f"device nk={nk}", G=5, K=1)
    finally:
        dv.free()


def test_c_entry_refusals(ctx):
    """P = 49, N = P, K = 0, 1 and 257 knots, unsorted knots, one layer pointer without the other: DSQ_ERR_ARG, nothing
    launched."""
    from pydeseq2_amd._lib import DeviceArray

    d = DeviceArray.from_host(ctx, np.zeros(49 * 64 + 600))
    kx = DeviceArray.from_host(ctx, np.concatenate([[0.0, 2.0, 1.0, 3.0], np.arange(4.0, 300.0)]))
    p, k = _vp(d.ptr), _vp(kx.ptr)

    def fit1(P, N):
        ctx.call("dsq_dev_voom_fit1", p, 64, p, p, p, 64, P, N, 1, p, p, p)

    def wls(P, N, nk, K=1, knots=None, E=None, w=None):
        ctx.call("dsq_dev_voom_wls", p, 64, p, p, 64, P, N, 1, p, knots or _vp(kx.ptr + 8 * 3), k, nk, p, K, p, p, p, p, E, w, 64)

    for P, N in ((49, 60), (0, 10), (5, 5), (48, 48)):
        with pytest.raises(ValueError, match="P:|N:"):
            fit1(P, N)
        with pytest.raises(ValueError, match="P:|N:"):
            wls(P, N, 5)
    for nk in (1, 257, 0):
        with pytest.raises(ValueError, match="n_knots"):
            wls(2, 10, nk)
    with pytest.raises(ValueError, match="K:"):
        wls(2, 10, 5, K=0)
    with pytest.raises(ValueError, match="strictly increasing"):
        wls(2, 10, 4, knots=k)  # 0, 2, 1, 3
    with pytest.raises(ValueError, match="both or neither"):
        wls(2, 10, 5, E=p)
    with pytest.raises(ValueError, match="leading dimension"):
        ctx.call("dsq_dev_voom_fit1", p, 8, p, p, p, 64, 2, 10, 1, p, p, p)
    assert (d.to_host() == 0.0).all()
    d.free(); kx.free()


# ------------------------------------------------------------------------------------------------------------ façade
@pytest.fixture(scope="module")
def fitted():
    from pydeseq2_amd.api import DeseqDataSet

    counts, meta, formula = voom_scenario()
    dds = DeseqDataSet(counts=counts, metadata=meta, design=formula)
    dds.deseq2()
    X = np.asarray(dds.obsm["design_matrix"], dtype=float)
    assert np.array_equal(X, scenario_design(meta)), list(dds.obsm["design_matrix"].columns)
    cs = counts.to_numpy().sum(1).astype(float)
    L = vr.effective_lib_sizes(np.asarray(dds.obs["size_factors"], float), cs)
    contrasts = np.array([[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, -1.0], [0.0, 1.0, 0.5, 0.5]])
    ref = vr.voom_reference(counts.to_numpy(), X, L, contrasts)
    return dds, counts, X, L, contrasts, ref


W_TOL = 5e-12  # the weights of the two routes: the knots agree to 1e-12 (test_voom_host.py), f^-4 makes that 4e-12


def _p_bound(ref, k, d_s2, d_df):
    """Bound on |p - p_ref| per gene for contrast k: the f_sf bound of tests/ql_cases.py plus the bound on t propagated
    through the t distribution (mean-value theorem: the density at the end of the interval nearer zero) plus the change of
    p with the degrees of freedom over [df - d_df, df + d_df].  The bound on t: |dt / t| <= d_est / |est| + d_u + d_s2 / 2
    with d_est = (C eps + W_TOL) kappa ||c|| ||beta||, d_u = (C eps + W_TOL) kappa, C = VOOM_C_DEVICE."""
    from scipy import stats

    t, p, df = ref["t"][k], ref["p"][k], ref["df_total"]
    rel = (VOOM_C_DEVICE * EPS + W_TOL) * ref["kappa"]
    with np.errstate(invalid="ignore", divide="ignore"):
        amp = ref["cnorm"][k] * np.linalg.norm(ref["beta"], axis=1) / np.abs(ref["est"][:, k])
    rt = rel * amp + rel + 0.5 * d_s2
    lo = np.abs(t) * np.maximum(0.0, 1.0 - rt)
    dens = stats.t.pdf(lo, df) if np.isfinite(df) else stats.norm.pdf(lo)
    b = F_SF_C_DEVICE * EPS * (1.0 + np.abs(np.log(p))) * p + 2.0 * dens * np.abs(t) * rt
    if np.isfinite(df) and d_df > 0:
        b = b + np.maximum(np.abs(vr.t_pvalue(t, df + d_df) - p), np.abs(vr.t_pvalue(t, df - d_df) - p))
    return b, rt


def _prior_bounds(ref, N, P, d):
    """How far s2_post (relative) and df_total move when every sigma2 moves by up to d (relative), from the reference
    alone: ebar moves by <= d, var(e) by <= 2 sd(e) d n / (n - 1) + d^2, df0 = 2 trigammaInverse(v) by |d v| 2 /
    |psi''(df0 / 2)|, log s0^2 by d + |psi'(df0 / 2) / 2 - 1 / df0| |d df0|."""
    from scipy.special import polygamma

    df, df0 = N - P, ref["df0"]
    if not np.isfinite(df0):
        return 2.0 * d, 0.0
    s2 = ref["sigma2"][np.isfinite(ref["sigma2"]) & (ref["sigma2"] > 0)]
    e = np.log(s2)
    dv = 2.0 * e.std(ddof=1) * d * len(e) / (len(e) - 1) + d * d
    ddf0 = 2.0 * dv / abs(float(polygamma(2, df0 / 2)))
    dlog_s02 = d + abs(float(polygamma(1, df0 / 2)) / 2 - 1 / df0) * ddf0
    # s2_post = (df0 s02 + df s2) / (df0 + df): each part moves by its own relative amount, the weights by ddf0 / (df0 + df)
    return dlog_s02 + d + 2.0 * ddf0 / (df0 + df), ddf0


def test_facade_end_to_end(fitted):
    """DeseqStats(test='voom'), batch() and dds.voom() at G = 400, N = 24, ~condition + batch (p = 4) against the
    reference: column names, NaN rows for the genes without counts, padj present; estimates, standard errors, variances,
    the prior, t and the p-values within the propagated bounds."""
    from pydeseq2_amd.api import DeseqStats

    dds, counts, X, L, contrasts, ref = fitted
    N, P = X.shape
    G = counts.shape[1]
    zero = counts.to_numpy().sum(0) == 0
    assert zero.sum() == 5
    ref["cnorm"] = np.linalg.norm(contrasts, axis=1)
    d_s2 = VOOM_C_REL_DEVICE * EPS + W_TOL
    d_post, d_df = _prior_bounds(ref, N, P, d_s2)
    print(f"df0 {ref['df0']:.4g}, bounds: sigma2 {d_s2:.3g}, s2_post {d_post:.3g}, df {d_df:.3g}")

    E, w = dds.voom()
    assert E.shape == (N, G) and w.shape == (N, G) and "voom_E" in dds.layers and "voom_weights" in dds.layers
    assert np.isnan(E[:, zero]).all() and np.isnan(w[:, zero]).all() and np.isfinite(E[:, ~zero]).all()
    # |log2(y + .5)| + |off| < 40; the two routes' offsets are each within an eps of |off| of the exact one
    assert np.allclose(E[:, ~zero], ref["E"][:, ~zero], rtol=0, atol=(VOOM_C_E + 2) * EPS * 40)
    assert np.allclose(w[:, ~zero], ref["w"][:, ~zero], rtol=W_TOL, atol=0)
    kx, ky = dds.uns["voom_knots"]
    assert np.allclose(kx, ref["knots"][0], rtol=1e-12) and np.allclose(ky, ref["knots"][1], rtol=1e-12)

    one = DeseqStats(dds, ["condition", "b", "a"], test="voom")
    df1 = one.summary()
    assert list(df1.columns) == ["baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "padj", "voom_sigma2"]
    many = DeseqStats.batch(dds, [c for c in contrasts], test="voom")
    assert len(many) == 3
    for k, o in enumerate(many):
        df = o.summary()
        if k == 0:  # the single call and the batch run the same kernels on the same inputs
            for col in df.columns:
                assert np.array_equal(df[col].to_numpy(), df1[col].to_numpy(), equal_nan=True), col
        for col in ("log2FoldChange", "lfcSE", "stat", "pvalue", "voom_sigma2"):
            assert np.isnan(df[col].to_numpy()[zero]).all() and np.isfinite(df[col].to_numpy()[~zero]).all(), col
        assert np.isnan(df["padj"].to_numpy()[zero]).all() and np.isfinite(df["padj"].to_numpy()).sum() > 100
        live = ~zero
        rel = (VOOM_C_DEVICE * EPS + W_TOL) * ref["kappa"][live]
        nb = np.linalg.norm(ref["beta"][live], axis=1)
        assert (np.abs(df["log2FoldChange"].to_numpy()[live] - ref["est"][live, k]) <= rel * ref["cnorm"][k] * nb).all()
        assert (np.abs(df["voom_sigma2"].to_numpy()[live] - ref["s2_post"][live]) <= d_post * ref["s2_post"][live]).all()
        se_ref = ref["lfcSE"][k][live]
        assert (np.abs(df["lfcSE"].to_numpy()[live] - se_ref) <= (rel + 0.5 * d_post) * se_ref).all()
        assert abs(o.voom_df0 - ref["df0"]) <= max(d_df, 1e-9 * ref["df0"]) or not np.isfinite(ref["df0"])
        assert math.isinf(o.voom_df_total) == math.isinf(ref["df_total"])
        pb, rt = _p_bound(ref, k, d_post, d_df)
        t, p = df["stat"].to_numpy()[live], df["pvalue"].to_numpy()[live]
        assert (np.abs(t - ref["t"][k][live]) <= rt[live] * np.abs(ref["t"][k][live]) + 4 * EPS).all()
        worst = np.max(np.abs(p - ref["p"][k][live]) / pb[live])
        print(f"contrast {k}: largest |p - p_ref| / bound = {worst:.3g}; smallest p {p.min():.3g}")
        assert (np.abs(p - ref["p"][k][live]) <= pb[live]).all()
        assert np.array_equal(np.sign(t), np.sign(df["log2FoldChange"].to_numpy()[live]))
    assert many[0].voom_knots[0].shape[0] <= 202 and many[0].voom_LFC.shape == (G, P)
    # lib_size: the column sums and an explicit vector that equals them give the same bits
    a = DeseqStats(dds, contrasts[0], test="voom", lib_size="colsums").summary()
    b = DeseqStats(dds, contrasts[0], test="voom", lib_size=counts.to_numpy().sum(1).astype(float)).summary()
    assert np.array_equal(a["pvalue"].to_numpy(), b["pvalue"].to_numpy(), equal_nan=True)
    assert not np.array_equal(a["pvalue"].to_numpy(), df1["pvalue"].to_numpy(), equal_nan=True)
    with pytest.raises(ValueError, match="voom"):
        one.summary(lfc_null=1.0)
