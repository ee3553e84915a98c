"""Seeded data sets of the sample-PCA tests (tests/test_pca_host.py, tests/test_gpu_pca.py)."""
import numpy as np

# (N, G, ntop) of the PCA cases; each is held to the gap rule on the restatement before anything is compared
PCA_CASES = [(3, 40, 500), (17, 300, 100), (65, 2000, 500), (130, 3000, 500), (12, 3000, 500)]


def real_set(N, G, seed=1):
    """Transformed-count-like values: a base level U(4, 14) per gene, three groups and two batches with sparse effects of
    different strength (so that the leading eigenvalues are well separated), noise of standard deviation 0.25."""
    rng = np.random.default_rng([seed, N, G])
    base = rng.uniform(4.0, 14.0, G)
    group, batch = np.arange(N) % 3, (np.arange(N) // 3) % 2
    ge = np.where(rng.random((3, G)) < 0.10, rng.normal(0.0, 1.0, (3, G)), 0.0) * np.array([[2.5], [1.2], [0.0]])
    be = np.where(rng.random((2, G)) < 0.05, rng.normal(0.0, 0.7, (2, G)), 0.0)
    return base + ge[group] + be[batch] + rng.normal(0.0, 0.25, (N, G))


def int_set(N, G, seed=1):
    """Integers in -15 ... 15 with all-zero genes and all-zero samples planted: every product and every partial sum of a
    Gram over them is exact in fp64, so any order of summation gives the int64 result bit for bit."""
    rng = np.random.default_rng([seed, N, G, 7])
    x = rng.integers(-15, 16, (N, G))
    x[:, rng.integers(0, G, max(1, G // 7))] = 0
    x[rng.integers(0, N, max(1, N // 9)), :] = 0
    return x.astype(np.float64)


def int_gram(x, sel=None):
    xi = np.asarray(x).astype(np.int64)
    if sel is not None:
        xi = xi[:, np.asarray(sel)]
    return (xi @ xi.T).astype(np.float64)


def unsorted_list(G, K, seed=1):
    """K distinct genes of 0 ... G-1 in no order, gene 0 and gene G-1 among them (K >= 2; K == 1: gene G-1)."""
    rng = np.random.default_rng([seed, G, K, 11])
    if K == 1:
        return np.array([G - 1], dtype=np.int32)
    mid = rng.permutation(np.arange(1, G - 1))[:K - 2]
    sel = rng.permutation(np.concatenate([[0, G - 1], mid]))
    if K > 2 and (np.diff(sel) > 0).all():
        sel = sel[::-1]
    return sel.astype(np.int32)


def decades_set(N, K, seed=1):
    """Real data over twelve decades: per gene a scale 10^U(-6, 6), a level of a few scales and unit noise."""
    rng = np.random.default_rng([seed, N, K, 13])
    scale = 10.0 ** rng.uniform(-6.0, 6.0, K)
    return scale * (rng.uniform(-3.0, 3.0, K) + rng.normal(0.0, 1.0, (N, K)))


def poisoned(a, pad, fill=np.nan):
    """The rows of `a` with `pad` extra columns of `fill` (the caller's ld padding)."""
    out = np.full((a.shape[0], a.shape[1] + pad), fill, dtype=np.float64)
    out[:, :a.shape[1]] = a
    return out
