"""WideGram (csrc/dsq_wide.h) as the DEVICE builds it: the three v_mfma_f64_16x16x4_f64 layouts.

tests/hostwide runs the plain-sum host branch of WideGram; only whole-pipeline parity at 1e-5 .. 1e-8 reaches the MFMA
fragments, the tile indices, the fragment-to-entry map of finish() and the first-chunk / later-chunk switch of the
device-memory accumulators.  Here tests/devunit (devunit_linalg.hip) runs the product's call sequence per gene - begin,
wide_zero_pad_rows, per chunk wide_stage_x / weights / add_chunk, finish - on workspaces bound as the product binds
them (MP = 48: DeviceWave on wave-private LDS; MP = 128: SlotWave on LDS plus a slot of device memory), every workspace
filled with NaN first, and compares

* bit for bit with the int64 Gram of integer data (every product and partial sum is an integer below 2^53, so exact in
  any order and with any fusing), both triangles.  Entries of the P x ld arrays outside the P x P block (the pad column of
  an even P) and the whole of dM without TWO are asserted to STILL HOLD THE POISON: the kernel writes nothing there;
* with the inner-product bound gamma_{N+2} sum_n |x_ni x_nj w_n| for data spread over twelve decades (N terms, one more
  rounding for x w; holds for any order and for fused accumulation; u = 2^-53), against tests/devunit/ref.py;
* the same gene at another place of the launch (another wave of a block, another block, another slot) bit for bit."""
import numpy as np
import pytest

from tests.devunit import ref

pytestmark = pytest.mark.gpu

P48 = (1, 5, 8, 9, 12, 13, 15, 16, 17, 31, 32, 33, 47, 48)
P128 = (49, 63, 64, 65, 80, 81, 96, 97, 112, 113, 127, 128)
SHAPES = [(48, p) for p in P48] + [(128, p) for p in P128]
NS = (1, 63, 64, 65, 130, 200)
G = 8
PAD = 3  # ldx = N + PAD, the padding holds a value that would show
BLOCKS = 3  # MP = 128: three workgroups (slots) take the eight genes, so a slot serves several genes in turn


@pytest.fixture(scope="module")
def du():
    from tests import devunit

    devunit.lib()  # builds on first use
    return devunit


def xt_of(X, fill):
    """[G][N][P] samples -> the kernels' [G][P][ldx]"""
    g, n, p = X.shape
    Xt = np.full((g, p, n + PAD), fill, dtype=np.float64)
    Xt[:, :, :n] = np.swapaxes(X, 1, 2)
    return Xt


def int_data(P, N, seed):
    rng = np.random.default_rng([seed, P, N])
    X = rng.integers(-15, 16, (G, N, P))
    X[:, :, rng.integers(0, P, max(1, P // 7))] = 0  # all-zero columns
    X[:, rng.integers(0, N, max(1, N // 9)), :] = 0  # all-zero samples
    w0 = rng.integers(0, 256, (G, N))
    w1 = rng.integers(0, 256, (G, N))
    w0[:, rng.integers(0, N, max(1, N // 8))] = 0
    w1[:, rng.integers(0, N, max(1, N // 8))] = 0
    w1 = np.where(w1 == w0, (w1 + 1) % 256, w1)  # different from each other, sample by sample
    return X, w0, w1


def int_gram(X, w):
    X = X.astype(np.int64)
    return np.einsum("gni,gn,gnj->gij", X, w.astype(np.int64), X, optimize=True)


def check_exact(du, mp, P, N, two):
    X, w0, w1 = int_data(P, N, 1)
    M, dM = du.gram(mp, two, xt_of(X, 7777.0), w0, w1 if two else None, blocks=BLOCKS)
    ref0 = int_gram(X, w0)
    assert np.abs(ref0).max() < 1.2e7
    assert ref.same_bits(M[:, :, :P], ref0.astype(np.float64)), np.argwhere(M[:, :, :P] != ref0)[:5]
    assert np.isnan(M[:, :, P:]).all()  # the pad column keeps the poison
    if two:
        ref1 = int_gram(X, w1)
        assert ref.same_bits(dM[:, :, :P], ref1.astype(np.float64)), np.argwhere(dM[:, :, :P] != ref1)[:5]
        assert np.isnan(dM[:, :, P:]).all()
    else:
        assert np.isnan(dM).all()  # never written


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("mp,P", SHAPES)
def test_gram_exact(du, mp, P, two):
    # two and P <= 8: the stacked layout; two and P >= 9: two accumulators per tile
    for N in NS:
        check_exact(du, mp, P, N, two)


# ------------------------------------------------------------------------------------------------ rounding
def real_data(P, N, seed):
    rng = np.random.default_rng([seed, P, N])
    X = rng.standard_normal((G, N, P)) * 10.0 ** rng.uniform(-3, 3, (G, N, P))
    w0 = 10.0 ** rng.uniform(-6, 6, (G, N))
    w1 = 10.0 ** rng.uniform(-6, 6, (G, N))
    return X, w0, w1


def sample_entries(P, rng, k=6):
    """corners, tile edges and a few random entries (i >= j)"""
    e = {(0, 0), (P - 1, 0), (P - 1, P - 1)}
    for t in range(16, P, 16):
        e |= {(t, t - 1), (t, t), (P - 1, t)}
    for _ in range(k):
        i = int(rng.integers(0, P))
        e.add((i, int(rng.integers(0, i + 1))))
    return sorted(e)


def check_rounding(du, mp, P, N):
    X, w0, w1 = real_data(P, N, 2)
    Xt = xt_of(X, 7777.0)
    M, dM = du.gram(mp, True, Xt, w0, w1, blocks=BLOCKS)
    M1, _ = du.gram(mp, False, Xt, w0, None, blocks=BLOCKS)
    g = ref.gamma(N + 2)
    rng = np.random.default_rng([3, P, N])
    for name, w, got_all in (("M", w0, (M, M1)), ("dM", w1, (dM,))):
        hi, lo, ab, (ii, jj) = ref.dd_gram_tri(X, w)
        k_of = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(ii, jj))}
        for got in got_all:
            got = got[:, :, :P]
            assert ref.same_bits(got, np.swapaxes(got, 1, 2)), name  # both triangles hold the same bits
            err = ref.err_vs_dd(got[:, ii, jj], hi, lo)
            bad = ~(err <= g * ab)
            assert not bad.any(), (name, np.argwhere(bad)[:5], err[bad][:5], (g * ab)[bad][:5])
        gene = int(rng.integers(0, G))  # sampled entries against mpmath itself
        for i, j in sample_entries(P, rng):
            s, a = ref.mp_dot(X[gene, :, i], X[gene, :, j], w[gene])
            k = k_of[(i, j)]
            assert ref.dd_agrees_with_mp(hi[gene, k], lo[gene, k], s, a), (name, gene, i, j)
            for got in got_all:
                assert ref.mp_err(got[gene, i, j], s) <= g * float(a), (name, gene, i, j)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("mp,P", SHAPES)
def test_gram_rounding(du, mp, P, N):
    # derived bound, nothing measured: gamma_{N+2} sum |x_ni x_nj w_n|
    check_rounding(du, mp, P, N)


# ------------------------------------------------------------------------------------------------ determinism, privacy
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("mp,P", SHAPES)
def test_gram_same_bits_wherever_the_gene_runs(du, mp, P, two):
    for N in (65, 200):
        X, w0, w1 = real_data(P, N, 4)
        M, dM = du.gram(mp, two, xt_of(X, 7777.0), w0, w1 if two else None, blocks=BLOCKS)
        assert not np.isnan(M[:, :, :P]).any()  # the poison shows nowhere in a result
        assert not two or not np.isnan(dM[:, :, :P]).any()
        # gene 0 goes to the last place (another wave, block and slot), every gene moves, six keep other neighbours
        order = np.array([3, 1, 2, 6, 5, 4, 7, 0])
        M2, dM2 = du.gram(mp, two, xt_of(X[order], 7777.0), w0[order], w1[order] if two else None, blocks=BLOCKS)
        assert ref.same_bits(M2[:, :, :P], M[order][:, :, :P])
        if two:
            assert ref.same_bits(dM2[:, :, :P], dM[order][:, :, :P])
