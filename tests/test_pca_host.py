"""Sample PCA / sample distances without a device: the launch plan of the Gram kernel, the host build of its shared code
(tests/hostgram: pack + Gram + reduce, row variances, distances), the selection's stable tie order, the sign rule and
the ratios, PcaResult through a Gram against the SVD route, and every refusal that needs no device."""
import numpy as np
import pytest

from tests import hostgram as hg
from tests import pca_cases as cases
from tests import pca_ref as ref
from tests.helpers import assert_close

C = hg.consts()
T, CHUNK = C["T"], C["chunk"]
PLAN_N = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300)


def several_slices_k(N):
    """A K that gives several slices with a remainder: chunks = 3 cps + 1 for some cps >= 2 is not always reachable, so
    search the plan itself for the smallest K with >= 3 slices whose last slice is shorter than the others."""
    for K in range(2 * CHUNK + 1, 200 * CHUNK, CHUNK // 2 + 1):
        p = hg.plan(N, K)
        if p["slices"] >= 3 and p["chunks"] % p["cps"] != 0 and K % CHUNK != 0:
            return K
    raise AssertionError("no such K")


def plan_ks(N):
    return (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, several_slices_k(N))


def test_constants():
    assert T % 16 == 0 and CHUNK % 4 == 0
    assert C["ld"] >= T and C["ld"] % 32 == 16  # (the bank argument of dsq_gram.h)


@pytest.mark.parametrize("N", PLAN_N)
def test_launch_plan_covers_every_pair_and_gene_once(N):
    for K in plan_ks(N):
        p = hg.plan(N, K)
        assert p["pad"] == (N + 15) // 16 * 16 and p["nt"] == -(-N // T) and p["ntiles"] == p["nt"] * (p["nt"] + 1) // 2
        # every pair i >= j lies in exactly one tile
        hits = np.zeros((N, N), np.int32)
        seen = set()
        for t in range(p["ntiles"]):
            ti, tj = hg.tile_rc(t)
            assert 0 <= tj <= ti < p["nt"] and (ti, tj) not in seen
            seen.add((ti, tj))
            i = np.arange(ti * T, min(N, ti * T + T))[:, None]
            j = np.arange(tj * T, min(N, tj * T + T))[None, :]
            hits[i, j] += (j <= i)
        assert (hits == np.tril(np.ones((N, N), np.int32))).all()
        # every gene lies in exactly one chunk of one slice; the boundaries do not depend on the tile (the plan has one
        # list of slices for all tiles: they are functions of p alone)
        assert p["chunks"] == -(-K // CHUNK) and 1 <= p["slices"] <= p["chunks"]
        assert p["slices"] == -(-p["chunks"] // p["cps"])
        count = np.zeros(K, np.int32)
        for s in range(p["slices"]):
            c0, c1 = s * p["cps"], min((s + 1) * p["cps"], p["chunks"])
            assert c0 < c1
            for c in range(c0, c1):
                count[c * CHUNK:min(K, c * CHUNK + CHUNK)] += 1
        assert (count == 1).all()
        assert p["slices"] * p["ntiles"] <= max(C["target"], p["ntiles"])
        want = K * p["pad"] + (p["slices"] * p["ntiles"] * T * T if p["slices"] > 1 else 0)
        assert hg.work_doubles(N, K) == want


def test_plan_of_nothing_and_of_many_samples():
    p = hg.plan(30, 0)
    assert p["chunks"] == 0 and p["slices"] == 0 and hg.work_doubles(30, 0) == 0
    assert hg.plan(30, 60000)["slices"] > 100  # three fragments, 60 000 genes: the gene dimension is split
    assert hg.plan(5000, 60000)["slices"] == 1  # tiles enough


@pytest.mark.parametrize("N", (1, 2, 17, 65, 129, 300))
@pytest.mark.parametrize("layout", (hg.SAMPLE_MAJOR, hg.GENE_MAJOR))
def test_host_gram_exact_on_integers(N, layout):
    for K in plan_ks(N):
        G = K + 5
        x = cases.int_set(N, G)
        xl = x if layout == hg.SAMPLE_MAJOR else np.ascontiguousarray(x.T)
        S = hg.sample_gram(xl[:, :K] if layout == hg.SAMPLE_MAJOR else xl[:K], layout)  # G == K, no list
        assert (S == cases.int_gram(x[:, :K])).all()
        if K >= 2 or G - 1 == 0:
            sel = cases.unsorted_list(G, K)
            S = hg.sample_gram(xl, layout, sel=sel)
            assert (S == cases.int_gram(x, sel)).all()


def test_host_gram_of_no_gene_is_zero():
    S = hg.sample_gram(np.zeros((5, 0)), hg.SAMPLE_MAJOR)
    assert (S == 0).all()
    S = hg.sample_gram(np.ones((5, 7)), hg.SAMPLE_MAJOR, sel=np.zeros(0, np.int32))
    assert (S == 0).all()


@pytest.mark.parametrize("N,K", [(3, 40), (17, 100), (33, 257), (130, 70)])
def test_host_gram_centred_within_the_bound(N, K):
    x = cases.decades_set(N, K)
    mean, _ = hg.row_meanvar(x, hg.SAMPLE_MAJOR)
    S = hg.sample_gram(x, hg.SAMPLE_MAJOR, mean=mean)
    Sr, B = ref.gram_ref(x), ref.gram_bound(x)
    assert (S == S.T).all()
    assert (np.abs(S - Sr) <= B).all(), float(np.max(np.abs(S - Sr) / B))
    # the bound is not vacuous: it is far below the entries' natural size
    assert (B <= 1e-11 * np.sqrt(np.outer(np.diag(Sr), np.diag(Sr))) + 1e-300).all()


@pytest.mark.parametrize("layout", (hg.SAMPLE_MAJOR, hg.GENE_MAJOR))
@pytest.mark.parametrize("N", (1, 2, 63, 130))
def test_host_row_meanvar(N, layout):
    x = cases.real_set(N, 23)
    m, v = hg.row_meanvar(x if layout == hg.SAMPLE_MAJOR else np.ascontiguousarray(x.T), layout)
    em, ev = ref.meanvar_bounds(x)
    m0, v0 = hg.row_meanvar(x, hg.SAMPLE_MAJOR)  # one order of the sums for both layouts: the same bits
    assert (m == m0).all() and (v == v0)[~np.isnan(v0)].all() and (np.isnan(v) == np.isnan(v0)).all()
    assert (np.abs(m - ref.row_means(x)) <= em).all()
    if N == 1:
        assert np.isnan(v).all()
    else:
        assert (np.abs(v - ref.row_vars(x)) <= ev).all()


def test_host_distances():
    x = cases.real_set(12, 300)
    x[7] = x[2]  # two identical samples
    mean, _ = hg.row_meanvar(x, hg.SAMPLE_MAJOR)
    S = hg.sample_gram(x, hg.SAMPLE_MAJOR, mean=mean)
    D = hg.gram_dist(S)
    assert (np.diag(D) == 0).all() and (D == D.T).all() and D[7, 2] == 0.0 and not np.isnan(D).any()
    B = ref.gram_bound(x)
    d2_bound = np.add.outer(np.diag(B), np.diag(B)) + 2 * B
    assert (np.abs(D ** 2 - ref.distances(x) ** 2) <= d2_bound * (1 + 1e-9) + 4 * ref.U * D ** 2).all()
    # a negative argument of the root (rounding) gives 0, not NaN
    Sneg = np.array([[1.0, 1.0 + 2.0 ** -40], [1.0 + 2.0 ** -40, 1.0]])
    assert (hg.gram_dist(Sneg) == 0).all()


# ------------------------------------------------------------------ host side of pydeseq2_amd/pca.py
def test_selection_is_stable_on_ties():
    from pydeseq2_amd.pca import select_genes

    rv = np.array([1.0, 5.0, 3.0, 5.0, 3.0, 3.0, 0.5, 3.0])
    # equal variances (3.0 at 2, 4, 5, 7) on both sides of the cut at 4
    assert select_genes(rv, 4).tolist() == [1, 3, 2, 4]
    assert select_genes(rv, 5).tolist() == [1, 3, 2, 4, 5]
    assert select_genes(rv, 500).tolist() == [1, 3, 2, 4, 5, 7, 0, 6]
    assert select_genes(rv, None).tolist() == list(range(8))
    assert select_genes(rv, 4).tolist() == ref.order_by_variance(rv, 4).tolist()
    rng = np.random.default_rng(3)
    rv = rng.integers(0, 5, 200).astype(float)
    assert select_genes(rv, 77).tolist() == ref.order_by_variance(rv, 77).tolist()
    for bad in (np.nan, np.inf):
        rv2 = rv.copy()
        rv2[11] = bad
        with pytest.raises(ValueError, match="not finite"):
            select_genes(rv2, 10)


def test_sign_rule_and_ratios():
    from pydeseq2_amd.pca import pca_from_gram

    x = cases.real_set(17, 300)
    xc = x - x.mean(0)
    r = pca_from_gram(xc @ xc.T)
    assert r.scores.shape == (17, 17)
    top = np.argmax(np.abs(r.scores), axis=0)
    lead = r.scores[top, np.arange(17)]
    assert (lead[:16] > 0).all() and lead[16] >= 0  # (centred data: the last eigenvalue is 0 up to rounding)
    assert abs(r.variance_ratio.sum() - 1.0) <= 1e-12
    assert (np.diff(r.variance) <= 0).all() and (r.variance >= 0).all()
    assert abs(r.total_variance - r.variance.sum()) <= 1e-12 * r.total_variance
    # a tie in magnitude: the FIRST of the two largest entries is the positive one
    S = np.array([[1.0, -1.0], [-1.0, 1.0]])  # scores +-1 in the one component
    r2 = pca_from_gram(S, n_components=1)
    assert r2.scores[0, 0] > 0 > r2.scores[1, 0]
    assert r2.variance_ratio[0] == pytest.approx(1.0)


@pytest.mark.parametrize("N,G,ntop", cases.PCA_CASES)
def test_pca_through_the_gram_against_svd(N, G, ntop):
    from pydeseq2_amd.pca import pca_from_gram, select_genes

    x = cases.real_set(N, G)
    want = ref.pca_svd(x, ntop)
    k = min(3, N - 1)
    assert (ref.relative_gaps(want["lam"], k) >= 0.1).all(), ref.relative_gaps(want["lam"], k)  # the case itself
    sel = select_genes(ref.row_vars(x), ntop)
    assert sel.tolist() == want["genes"].tolist()
    xc = x[:, sel] - ref.row_means(x[:, sel])
    S = xc @ xc.T
    full = pca_from_gram(S, None, sel)
    part = pca_from_gram(S, k, sel)
    s1 = np.sqrt(want["lam"][0])
    for r in (full, part):
        assert_close(r.variance[:k], want["variance"][:k], 1e-8, 1e-10)
        assert_close(r.variance_ratio[:k], want["variance_ratio"][:k], 1e-8, 1e-10)
        assert_close(r.scores[:, :k] / s1, want["scores"][:, :k] / s1, 1e-8, 1e-10)
        assert_close(r.total_variance, want["total_variance"], 1e-8, 1e-10)
    assert part.scores.shape == (N, k)
    # the host build's Gram (means from its own row pass) gives the same PCA
    mean, _ = hg.row_meanvar(x, hg.SAMPLE_MAJOR)
    r = pca_from_gram(hg.sample_gram(x, hg.SAMPLE_MAJOR, sel=sel, mean=mean), k, sel)
    assert_close(r.scores / s1, want["scores"][:, :k] / s1, 1e-8, 1e-10)
    assert_close(r.variance, want["variance"][:k], 1e-8, 1e-10)


def test_refusals_without_a_device():
    from pydeseq2_amd import pca as P

    x = cases.real_set(6, 20)
    with pytest.raises(ValueError, match="two samples"):
        P.pca(None, x[:1])
    with pytest.raises(ValueError, match="ntop"):
        P.pca(None, x, ntop=0)
    for bad in (0, 7, 21):
        with pytest.raises(ValueError, match="n_components"):
            P.pca(None, x, n_components=bad)
    with pytest.raises(ValueError, match="n_components"):
        P.pca(None, x, ntop=4, n_components=5)  # min(N, K) = 4
    with pytest.raises(ValueError, match="two-dimensional"):
        P.pca(None, x[0])
    with pytest.raises(ValueError, match="genes"):
        P.sample_distances(None, x, genes=[0, 20])
    with pytest.raises(ValueError, match="genes"):
        P.sample_gram(None, x, genes=[-1])
    with pytest.raises(ValueError, match="n_components"):
        P.pca_from_gram(np.eye(3), 4)
