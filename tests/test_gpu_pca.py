"""Sample PCA / sample distances on the GPU: dsq_dev_row_meanvar, dsq_dev_sample_gram (k_gram_pack, k_sample_gram,
k_gram_reduce) and dsq_dev_gram_dist against the restatement (tests/pca_ref) over the seeded sets of tests/pca_cases -
both layouts, poisoned padding, guard values, every edge of the fragments, the macro tile, the chunk and the slices, exact
integer Grams, the entrywise bound on real data, position independence, an input beyond 2^31 bytes, the argument refusals -
and the module functions and the DeseqDataSet facade end to end."""
import ctypes as C

import numpy as np
import pytest

from tests import hostgram as hg
from tests import pca_cases as cases
from tests import pca_ref as ref
from tests.helpers import assert_close, load_dataset

pytestmark = pytest.mark.gpu

_vp = C.c_void_p
GUARD, PAD, POISON = 3, 3, -7.0
SM, GM = 0, 1
CHUNK, T = hg.consts()["chunk"], hg.consts()["T"]


@pytest.fixture(scope="module")
def ctx():
    from pydeseq2_amd._lib import Context

    return Context(0)


def several_slices_k(N):
    """The smallest K (no multiple of the chunk) whose plan has at least three slices, the last one shorter."""
    for K in range(2 * CHUNK + 1, 400 * CHUNK, CHUNK // 2 + 1):
        p = hg.plan(N, K)
        if p["slices"] >= 3 and p["chunks"] % p["cps"] != 0 and K % CHUNK != 0:
            return K
    raise AssertionError("no such K")


def upload(ctx, x, layout, pad=PAD):
    """N x G host matrix -> (DeviceArray in `layout` with `pad` NaN columns behind every row, ld)"""
    from pydeseq2_amd._lib import DeviceArray

    a = x if layout == SM else x.T
    return DeviceArray.from_host(ctx, cases.poisoned(a, pad).ravel()), a.shape[1] + pad


def dev_meanvar(ctx, d_x, layout, N, G, ld, want_var=True):
    from pydeseq2_amd._lib import DeviceArray

    d_m = DeviceArray.from_host(ctx, np.full(G + GUARD, POISON))
    d_v = DeviceArray.from_host(ctx, np.full(G + GUARD, POISON))
    ctx.call("dsq_dev_row_meanvar", _vp(d_x.ptr), layout, N, G, ld, _vp(d_m.ptr), _vp(d_v.ptr) if want_var else None)
    ctx.sync()
    m, v = d_m.to_host(), d_v.to_host()
    d_m.free(); d_v.free()
    assert (m[G:] == POISON).all() and (v[G:] == POISON).all(), "the guard values behind an output were written"
    if not want_var:
        assert (v == POISON).all()
    return m[:G], v[:G]


def dev_gram(ctx, d_x, layout, N, G, ld, sel=None, mean=None, K=None, keep=False):
    """dsq_dev_sample_gram -> S [N][N]; the lds padding and the guard values behind S and behind the workspace are checked
    untouched.  keep: also return the device copy of S ([N][N + PAD]; the caller frees it)."""
    from pydeseq2_amd._lib import DeviceArray

    K = (G if sel is None else len(sel)) if K is None else K
    lds = N + PAD
    nw = int(ctx.lib.dsq_sample_gram_work_doubles(N, K))
    assert nw == hg.work_doubles(N, K)
    d_S = DeviceArray.from_host(ctx, np.full(N * lds + GUARD, POISON))
    d_w = DeviceArray.from_host(ctx, np.full(nw + GUARD, POISON))
    d_sel = DeviceArray.from_host(ctx, np.ascontiguousarray(sel, dtype=np.int32)) if sel is not None and len(sel) else None
    d_mean = DeviceArray.from_host(ctx, np.ascontiguousarray(mean)) if mean is not None else None
    try:
        ctx.call("dsq_dev_sample_gram", _vp(d_x.ptr) if d_x is not None else None, layout, N, G, ld,
                 _vp(d_sel.ptr) if d_sel is not None else None, K, _vp(d_mean.ptr) if d_mean is not None else None,
                 _vp(d_w.ptr), _vp(d_S.ptr), lds)
        ctx.sync()
        S, w = d_S.to_host(), d_w.to_host()
    finally:
        for d in (d_w, d_sel, d_mean) + (() if keep else (d_S,)):
            if d is not None:
                d.free()
    assert (S[N * lds:] == POISON).all() and (w[nw:] == POISON).all(), "guard values were written"
    S = S[:N * lds].reshape(N, lds)
    assert (S[:, N:] == POISON).all(), "the lds padding was written"
    S = np.ascontiguousarray(S[:, :N])
    return (S, d_S) if keep else S


# ------------------------------------------------------------------ row means and variances
@pytest.mark.parametrize("layout", (SM, GM))
def test_row_meanvar(ctx, layout):
    """Within the bounds of tests/pca_ref.meanvar_bounds of the fsum reference, derived there for any order of the sums:
    |mean - m| <= gamma_{N+1} mean|x|;  |var - rv| <= gamma_{N+4} (rv + c) + c with c = N e_m^2 / (N - 1)."""
    worst = 0.0
    for N in (1, 2, 63, 64, 65, 130, 513):
        for G in (1, 5, 203):
            x = cases.real_set(N, G)
            d_x, ld = upload(ctx, x, layout)
            m, v = dev_meanvar(ctx, d_x, layout, N, G, ld)
            m2, _ = dev_meanvar(ctx, d_x, layout, N, G, ld, want_var=False)
            d_x.free()
            em, ev = ref.meanvar_bounds(x)
            assert (m == m2).all()
            hm, hv = hg.row_meanvar(x, SM)  # the host build: the same order of the sums, so the same bits in both layouts
            assert (m == hm).all() and (v == hv)[~np.isnan(hv)].all()
            assert (np.abs(m - ref.row_means(x)) <= em).all(), (N, G)
            if N == 1:
                assert np.isnan(v).all()
            else:
                assert (np.abs(v - ref.row_vars(x)) <= ev).all(), (N, G)
                worst = max(worst, float(np.max(np.abs(v - ref.row_vars(x)) / ev)))
    print(f"row_meanvar layout {layout}: largest |var - ref| / bound = {worst:.3g}")


# ------------------------------------------------------------------ the Gram on integers: exact
@pytest.mark.parametrize("N", (1, 2, 15, 16, 17, 63, 64, 65, 130, T + 1))
def test_gram_exact_on_integers(ctx, N):
    """Uncentred integer data: both triangles bit for bit equal to the int64 Gram, for G = K without a list and for an
    unsorted list out of G > K genes that holds gene 0 and gene G - 1; the two layouts and a second launch give the same
    bits."""
    for K in (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, several_slices_k(N)):
        G = K + 5
        x = cases.int_set(N, G)
        sel = cases.unsorted_list(G, K)
        if K > 1:
            assert 0 in sel and G - 1 in sel and (np.diff(sel) < 0).any()
        want_all, want_sel = cases.int_gram(x[:, :K]), cases.int_gram(x, sel)
        got = {}
        for layout in (SM, GM):
            d_x, ld = upload(ctx, x, layout)
            d_k, ldk = upload(ctx, x[:, :K], layout)
            got[layout] = (dev_gram(ctx, d_k, layout, N, K, ldk), dev_gram(ctx, d_x, layout, N, G, ld, sel=sel))
            if K in (5, CHUNK + 1) or K > 2 * CHUNK:
                again = dev_gram(ctx, d_x, layout, N, G, ld, sel=sel)
                assert (again == got[layout][1]).all()
            d_x.free(); d_k.free()
            assert (got[layout][0] == want_all).all(), (N, K, layout)
            assert (got[layout][1] == want_sel).all(), (N, K, layout)
        assert (got[SM][0] == got[GM][0]).all() and (got[SM][1] == got[GM][1]).all()


def test_gram_of_no_gene_is_zero(ctx):
    x = cases.int_set(5, 7)
    d_x, ld = upload(ctx, x, SM)
    assert (dev_gram(ctx, d_x, SM, 5, 7, ld, sel=np.zeros(0, np.int32)) == 0).all()  # K = 0
    assert (dev_gram(ctx, None, SM, 5, 0, 0) == 0).all()  # G = 0
    d_x.free()


# ------------------------------------------------------------------ the Gram on real data: the entrywise bound
@pytest.mark.parametrize("N,K", [(3, 40), (17, 100), (33, 257), (130, 70), (20, 10 * CHUNK - 5)])
def test_gram_centred_within_the_bound(ctx, N, K):
    """Real data over twelve decades, centred with the means of dsq_dev_row_meanvar passed in: |S - S_ref| <= the entrywise
    bound of tests/pca_ref.gram_bound against the fsum Gram of the exactly centred data, in both layouts."""
    x = cases.decades_set(N, K)
    Sr, B = ref.gram_ref(x), ref.gram_bound(x)
    for layout in (SM, GM):
        d_x, ld = upload(ctx, x, layout)
        mean, _ = dev_meanvar(ctx, d_x, layout, N, K, ld)
        S = dev_gram(ctx, d_x, layout, N, K, ld, mean=mean)
        d_x.free()
        assert (S == S.T).all()
        print(f"centred Gram N={N} K={K} layout {layout}: largest |S - ref| / bound = {float(np.max(np.abs(S - Sr) / B)):.3g}")
        assert (np.abs(S - Sr) <= B).all()


# ------------------------------------------------------------------ position independence
def test_the_same_sample_gives_the_same_bits_wherever_it_stands(ctx):
    """Sample 0 copied to index 17 (the same macro tile, another fragment) and to an index of the second macro tile: the
    three rows (and columns) of S are bit-identical, S is exactly symmetric, and the copies are at distance exactly 0."""
    from pydeseq2_amd._lib import DeviceArray

    N, K = T + 22, several_slices_k(T + 22)
    x = cases.real_set(N, K)
    other = T + 12
    x[17] = x[0]
    x[other] = x[0]
    for layout in (SM, GM):
        d_x, ld = upload(ctx, x, layout)
        mean, _ = dev_meanvar(ctx, d_x, layout, N, K, ld)
        S, d_S = dev_gram(ctx, d_x, layout, N, K, ld, mean=mean, keep=True)
        d_D = DeviceArray.from_host(ctx, np.full(N * N, POISON))
        ctx.call("dsq_dev_gram_dist", _vp(d_S.ptr), N, N + PAD, _vp(d_D.ptr), N)
        ctx.sync()
        D = d_D.to_host().reshape(N, N)
        for d in (d_x, d_S, d_D):
            d.free()
        assert (S == S.T).all()
        for c in (17, other):
            keep = np.ones(N, bool)
            keep[[0, 17, other]] = False
            assert (S[c, keep] == S[0, keep]).all() and (S[keep, c] == S[keep, 0]).all()
            assert S[c, c] == S[0, 0] == S[c, 0] == S[0, c] == S[17, other]
            assert D[0, c] == 0.0 and D[c, 0] == 0.0
        assert D[17, other] == 0.0 and (np.diag(D) == 0).all() and (D == D.T).all()


# ------------------------------------------------------------------ beyond 2^31 bytes
def test_gene_major_input_beyond_two_gigabytes(ctx):
    """Gene-major, N = 16, ld = 16, G = 2^24 + 5: 2.1 GB of zeros with integers in the first gene and the last three;
    uncentred; exact.  (Byte offsets of the last genes lie beyond 2^31.)"""
    from pydeseq2_amd._lib import DeviceArray

    N, G = 16, 2 ** 24 + 5
    xt = np.zeros((G, N))
    rng = np.random.default_rng(5)
    rows = np.array([0, G - 3, G - 2, G - 1])
    xt[rows] = rng.integers(-15, 16, (4, N))
    d_x = DeviceArray.from_host(ctx, xt.ravel())
    nw = int(ctx.lib.dsq_sample_gram_work_doubles(N, G))
    d_w = DeviceArray(ctx, nw + GUARD, np.float64)
    d_S = DeviceArray.from_host(ctx, np.full(N * N + GUARD, POISON))
    d_mv = DeviceArray(ctx, 2 * G, np.float64)
    try:
        ctx.call("dsq_dev_sample_gram", _vp(d_x.ptr), GM, N, G, N, None, G, None, _vp(d_w.ptr), _vp(d_S.ptr), N)
        ctx.call("dsq_dev_row_meanvar", _vp(d_x.ptr), GM, N, G, N, _vp(d_mv.ptr), _vp(d_mv.ptr + 8 * G))
        ctx.sync()
        S = d_S.to_host()
        tail = np.empty(3)
        ctx.d2h(tail, d_mv.ptr + 8 * (G - 3))
    finally:
        for d in (d_x, d_w, d_S, d_mv):
            d.free()
    xi = xt[rows].astype(np.int64)
    assert (S[N * N:] == POISON).all()
    assert (S[:N * N].reshape(N, N) == (xi.T @ xi).astype(np.float64)).all()
    assert_close(tail, xt[rows[1:]].mean(1), 1e-15, 1e-15)


# ------------------------------------------------------------------ distances
def test_gram_dist(ctx):
    """Against explicit differences: |D^2 - D_ref^2| <= B_ii + B_jj + 2 B_ij (the entries' bounds; plus the rounding of
    the three-term sum and of the square of the reference, 4 u D^2); the diagonal exactly 0; a negative argument of the
    root gives 0, never NaN; the padding and the guard values behind D stay."""
    from pydeseq2_amd._lib import DeviceArray

    N, K = 41, 300
    x = cases.real_set(N, K)
    x[30] = x[4] * (1 + 2.0 ** -40)  # near-duplicates
    d_x, ld = upload(ctx, x, SM)
    mean, _ = dev_meanvar(ctx, d_x, SM, N, K, ld)
    S, d_S = dev_gram(ctx, d_x, SM, N, K, ld, mean=mean, keep=True)
    ldd = N + PAD
    d_D = DeviceArray.from_host(ctx, np.full(N * ldd + GUARD, POISON))
    Sneg = np.array([[1.0, 1.0 + 2.0 ** -40], [1.0 + 2.0 ** -40, 1.0]])
    d_Sn = DeviceArray.from_host(ctx, Sneg.ravel())
    d_Dn = DeviceArray.from_host(ctx, np.full(4, POISON))
    ctx.call("dsq_dev_gram_dist", _vp(d_S.ptr), N, N + PAD, _vp(d_D.ptr), ldd)
    ctx.call("dsq_dev_gram_dist", _vp(d_Sn.ptr), 2, 2, _vp(d_Dn.ptr), 2)
    ctx.sync()
    D, Dn = d_D.to_host(), d_Dn.to_host()
    for d in (d_x, d_S, d_D, d_Sn, d_Dn):
        d.free()
    assert (D[N * ldd:] == POISON).all()
    D = D[:N * ldd].reshape(N, ldd)
    assert (D[:, N:] == POISON).all()
    D = D[:, :N]
    assert (Dn == 0).all()
    assert (np.diag(D) == 0).all() and (D == D.T).all() and not np.isnan(D).any() and (D >= 0).all()
    B = ref.gram_bound(x)
    bound = np.add.outer(np.diag(B), np.diag(B)) + 2 * B
    Dr = ref.distances(x)
    assert (np.abs(D ** 2 - Dr ** 2) <= bound + 4 * ref.U * Dr ** 2).all()
    assert (D == hg.gram_dist(S)).all()  # (the same three-term formula on the host)


# ------------------------------------------------------------------ refusals
def test_argument_refusals(ctx):
    from pydeseq2_amd._lib import DeviceArray

    d = DeviceArray.from_host(ctx, np.full(256, POISON))
    p = _vp(d.ptr)
    ok = dict(x=p, layout=SM, N=4, G=6, ld=8, sel=None, K=6, mean=p, var=p, work=p, S=p, lds=4, D=p, ldd=4)

    def meanvar(**kw):
        a = {**ok, **kw}
        ctx.call("dsq_dev_row_meanvar", a["x"], a["layout"], a["N"], a["G"], a["ld"], a["mean"], a["var"])

    def gram(**kw):
        a = {**ok, **kw}
        ctx.call("dsq_dev_sample_gram", a["x"], a["layout"], a["N"], a["G"], a["ld"], a["sel"], a["K"], a["mean"], a["work"],
                 a["S"], a["lds"])

    def dist(**kw):
        a = {**ok, **kw}
        ctx.call("dsq_dev_gram_dist", a["S"], a["N"], a["lds"], a["D"], a["ldd"])

    for bad in (dict(N=0), dict(G=-1), dict(layout=2), dict(layout=-1), dict(ld=5), dict(layout=GM, ld=3), dict(mean=None),
                dict(x=None)):
        with pytest.raises(ValueError):
            meanvar(**bad)
    for bad in (dict(N=0), dict(G=-1), dict(K=-1), dict(K=7), dict(layout=2), dict(ld=5), dict(layout=GM, ld=3),
                dict(lds=3), dict(S=None), dict(x=None), dict(work=None)):
        with pytest.raises(ValueError):
            gram(**bad)
    for bad in (dict(N=0), dict(lds=3), dict(ldd=3), dict(S=None), dict(D=None)):
        with pytest.raises(ValueError):
            dist(**bad)
    meanvar(G=0, x=None)  # nothing to do, nothing written
    ctx.sync()
    assert (d.to_host() == POISON).all()
    d.free()
    assert int(ctx.lib.dsq_sample_gram_work_doubles(0, 5)) == 0 and int(ctx.lib.dsq_sample_gram_work_doubles(5, -1)) == 0


# ------------------------------------------------------------------ end to end
def leading(lam, most=3):
    """How many leading components the restatement defines up to rounding: relative gaps of at least 0.1."""
    k = 0
    while k < min(most, len(lam) - 1) and (ref.relative_gaps(lam, k + 1) >= 0.1).all():
        k += 1
    return k


def check_pca(r, want, N, k, scores=None):
    s1 = np.sqrt(want["lam"][0])
    sc = np.asarray(r.scores if scores is None else scores)
    assert_close(r.variance[:k], want["variance"][:k], 1e-8, 1e-10)
    assert_close(r.variance_ratio[:k], want["variance_ratio"][:k], 1e-8, 1e-10)
    assert_close(sc[:, :k] / s1, want["scores"][:, :k] / s1, 1e-8, 1e-10)
    assert_close(r.total_variance, want["total_variance"], 1e-8, 1e-10)


@pytest.mark.parametrize("N,G,ntop", cases.PCA_CASES)
def test_module_pca_and_distances(ctx, N, G, ntop):
    from pydeseq2_amd import pca as P
    from pydeseq2_amd._lib import DeviceArray

    x = cases.real_set(N, G)
    want = ref.pca_svd(x, ntop)
    k = min(3, N - 1)
    assert (ref.relative_gaps(want["lam"], k) >= 0.1).all()
    r = P.pca(ctx, x, ntop=ntop)
    assert r.scores.shape == (N, N) and np.asarray(r.genes).tolist() == want["genes"].tolist()
    check_pca(r, want, N, k)
    rk = P.pca(ctx, x, ntop=ntop, n_components=k)
    assert rk.scores.shape == (N, k)
    check_pca(rk, want, N, k)
    rv = P.row_variances(ctx, x)
    assert (np.abs(rv - ref.row_vars(x)) <= ref.meanvar_bounds(x)[1]).all()
    # a DeviceArray input in each layout: bit for bit the host input's result
    d_sm = DeviceArray.from_host(ctx, x)
    d_gm = DeviceArray.from_host(ctx, np.ascontiguousarray(x.T), ld=N + 5)
    try:
        for d, lay in ((d_sm, SM), (d_gm, GM)):
            rd = P.pca(ctx, d, ntop=ntop, layout=lay)
            assert (rd.scores == r.scores).all() and (rd.variance == r.variance).all() and (rd.genes == r.genes).all()
            assert (P.row_variances(ctx, d, layout=lay) == rv).all()
        if N <= 20:
            D = P.sample_distances(ctx, x)
            assert (P.sample_distances(ctx, d_gm, layout=GM) == D).all()
            B = ref.gram_bound(x)
            Dr = ref.distances(x)
            assert (np.abs(D ** 2 - Dr ** 2) <= np.add.outer(np.diag(B), np.diag(B)) + 2 * B + 4 * ref.U * Dr ** 2).all()
            sel = want["genes"][:7]
            S = P.sample_gram(ctx, x, genes=sel)
            assert (np.abs(S - ref.gram_ref(x[:, sel])) <= ref.gram_bound(x[:, sel])).all()
            assert (P.sample_gram(ctx, cases.int_set(N, 50), center=False) == cases.int_gram(cases.int_set(N, 50))).all()
    finally:
        d_sm.free(); d_gm.free()
    with pytest.raises(ValueError, match="not finite"):
        bad = x.copy()
        bad[0, 3] = np.inf
        P.pca(ctx, bad)


def test_dataset_pca_and_sample_distances(ctx):
    import pandas as pd

    from pydeseq2_amd import pca as P
    from pydeseq2_amd.api import DeseqDataSet

    counts, meta = load_dataset("synthetic")
    dds = DeseqDataSet(counts=counts, metadata=meta, design="~condition")
    try:
        with pytest.raises(KeyError, match="vst_counts"):
            dds.pca()
        with pytest.raises(KeyError, match="nope"):
            dds.sample_distances(layer="nope")
        dds.vst()
        x = np.asarray(dds.layers["vst_counts"], dtype=np.float64)
        N, G = x.shape
        want = ref.pca_svd(x, 500)  # ntop larger than G: every gene
        k = leading(want["lam"])
        assert k >= 2, ref.relative_gaps(want["lam"], 2)
        r = dds.pca()
        assert isinstance(r.scores, pd.DataFrame) and list(r.scores.index) == list(dds.obs_names)
        assert list(r.scores.columns) == [f"PC{i + 1}" for i in range(N)]
        assert list(r.genes) == list(dds.var_names[want["genes"]])
        check_pca(r, want, N, k)
        r2 = dds.pca(n_components=2)
        assert list(r2.scores.columns) == ["PC1", "PC2"]
        check_pca(r2, want, N, 2)
        assert_close(r2.scores.to_numpy(), r.scores.to_numpy()[:, :2], 1e-8, 1e-10 * np.sqrt(want["lam"][0]))
        r3 = dds.pca(ntop=4)
        assert list(r3.genes) == list(dds.var_names[ref.order_by_variance(ref.row_vars(x), 4)])
        m = P.pca(ctx, x)  # the module function on the same layer
        assert_close(m.scores[:, :k], r.scores.to_numpy()[:, :k], 1e-8, 1e-10 * np.sqrt(want["lam"][0]))
        D = dds.sample_distances()
        assert isinstance(D, pd.DataFrame) and list(D.index) == list(dds.obs_names) == list(D.columns)
        B = ref.gram_bound(x)
        Dr = ref.distances(x)
        Dv = D.to_numpy()
        assert (np.abs(Dv ** 2 - Dr ** 2) <= np.add.outer(np.diag(B), np.diag(B)) + 2 * B + 4 * ref.U * Dr ** 2).all()
        assert (np.diag(Dv) == 0).all() and (Dv == Dv.T).all()
        assert (Dv == dds._pipe.sample_distances(x)).all()
        # refusals of the facade
        for kw in (dict(ntop=0), dict(n_components=0), dict(n_components=N + 1), dict(ntop=3, n_components=4)):
            with pytest.raises(ValueError):
                dds.pca(**kw)
        dds.layers["odd"] = x[:, :3]
        with pytest.raises(ValueError, match="shape"):
            dds.pca(layer="odd")
        bad = x.copy()
        bad[1, 2] = np.nan
        dds.layers["bad"] = bad
        with pytest.raises(ValueError, match="not finite"):
            dds.pca(layer="bad")
        assert "pca" not in dds.uns and not any("pca" in str(key).lower() for key in dds.obsm)  # nothing is stored
    finally:
        dds.close()
