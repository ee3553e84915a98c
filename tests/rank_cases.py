"""Cases of the rank-sum tests (tests/test_rank_host.py, tests/test_gpu_rank.py): a few genes each, G in {1, 5, 67}.

A case: name, y [G][ldn] int32 (gene-major, the pitch's padding filled with a count that must never be read), sf [N],
labels [K][N] in {1, 0, -1}, strata [N] or None, N, ldn.  The rows mix what can go wrong in a rank: Poisson rows of mean
0.2 (heavily tied), all values tied, all zero but one, ties between different (y, sf) pairs such as 2/1 and 4/2, size
factors that make y / sf inexact, and rows without ties."""
from dataclasses import dataclass

import numpy as np

PAD_COUNT = 2_000_000_000  # in the row pitch's padding: reading it would move every rank


@dataclass
class Case:
    name: str
    y: np.ndarray
    sf: np.ndarray
    labels: np.ndarray
    strata: object
    N: int
    ldn: int

    @property
    def G(self):
        return self.y.shape[0]

    @property
    def K(self):
        return self.labels.shape[0]


def _size_factors(rng, N):
    """Half of them powers of two (so that 2/1 and 4/2 tie), half of them such that y / sf is inexact."""
    exact = rng.choice([0.5, 1.0, 2.0, 4.0], N)
    return np.where(rng.random(N) < 0.5, exact, np.exp(rng.normal(0, 0.3, N)))


def _rows(rng, G, N, sf):
    kinds = ("pois02", "pois30", "tied", "one", "pairs", "big", "pois3")
    out = np.zeros((G, N), np.int64)
    for g in range(G):
        kind = kinds[g % len(kinds)] if G > 1 else "pois3"
        if kind == "pois02":
            out[g] = rng.poisson(0.2, N)
        elif kind == "pois30":
            out[g] = rng.poisson(30 * sf)
        elif kind == "tied":  # every quotient equal to 6 where sf is a power of two, all zero otherwise
            out[g] = np.where(np.isin(sf, (0.5, 1.0, 2.0, 4.0)), 6 * sf, 0)
            if g % 2:
                out[g] = 0
        elif kind == "one":
            out[g, int(rng.integers(N))] = 7
        elif kind == "pairs":  # 2/1, 4/2, 8/4, 1/0.5 ...: equal quotients of different pairs
            out[g] = np.rint(rng.integers(1, 4, N) * 2 * np.where(np.isin(sf, (0.5, 1.0, 2.0, 4.0)), sf, 1.0))
        elif kind == "big":
            out[g] = rng.negative_binomial(2, 2 / (2 + 3000.0 * sf))
        else:
            out[g] = rng.poisson(3, N)
    return out


def _case(name, seed, G, labels, strata=None, ldn=None, y=None, sf=None):
    rng = np.random.default_rng(seed)
    labels = np.atleast_2d(np.asarray(labels, np.int8))
    N = labels.shape[1]
    sf = _size_factors(rng, N) if sf is None else np.asarray(sf, float)
    rows = _rows(rng, G, N, sf) if y is None else np.atleast_2d(np.asarray(y))
    ldn = N if ldn is None else ldn
    ym = np.full((rows.shape[0], ldn), PAD_COUNT, np.int32)
    ym[:, :N] = rows
    return Case(name, ym, sf, labels, None if strata is None else np.asarray(strata, np.int64), N, ldn)


def _two_groups(rng, n_used, n1, n_left=0):
    """n1 tested and n_used - n1 reference samples in random order, n_left left-out samples interleaved."""
    lab = np.concatenate([np.ones(n1, np.int8), np.zeros(n_used - n1, np.int8), -np.ones(n_left, np.int8)])
    return rng.permutation(lab)


def small_cases():
    """Every case but the two rows of 16 384 values."""
    rng = np.random.default_rng(20)
    cs = []
    for n, n1, G in ((2, 1, 5), (3, 1, 5), (63, 20, 5), (64, 32, 67), (65, 40, 5), (127, 3, 5), (128, 64, 5), (129, 100, 1)):
        cs.append(_case(f"n{n}", 100 + n, G, _two_groups(rng, n, n1)))
    cs.append(_case("n1000_unequal", 7, 5, _two_groups(rng, 1000, 137)))
    cs.append(_case("left_out_ldn", 8, 5, _two_groups(rng, 90, 31, n_left=47), ldn=144))
    # K = 3: three comparisons with their own labels (other groups, other samples left out), one with one sample a side
    l3 = np.stack([_two_groups(rng, 70, 30, 30), _two_groups(rng, 100, 9), _two_groups(rng, 2, 1, 98)])
    cs.append(_case("K3", 9, 5, l3, ldn=112))
    # strata of sizes 1, 2, 3, 64, 65 in one row (the stratum of one sample holds one group only), left-out samples
    lab = np.concatenate([[1], [1, 0], [0, 1, 0], _two_groups(rng, 64, 30), _two_groups(rng, 65, 11), [-1] * 9])
    ids = np.concatenate([[0], [1] * 2, [2] * 3, [3] * 64, [4] * 65, [5] * 9])
    perm = rng.permutation(len(lab))
    cs.append(_case("strata_1_2_3_64_65", 10, 67, lab[perm], ids[perm]))
    # a stratum of 20 samples that holds only tested samples, between two that hold both
    lab = np.concatenate([_two_groups(rng, 30, 12), np.ones(20, np.int8), _two_groups(rng, 41, 20)])
    ids = np.concatenate([[7] * 30, [3] * 20, [11] * 41])
    cs.append(_case("stratum_one_group", 11, 5, lab, ids))
    # K = 3 with strata (shared ids; the used samples of a comparison may miss a stratum altogether)
    ids = rng.integers(0, 4, 120)
    l3 = np.stack([_two_groups(rng, 100, 50, 20), _two_groups(rng, 60, 25, 60), np.where(ids == 2, -1, _two_groups(rng, 120, 60))])
    cs.append(_case("K3_strata", 12, 5, l3, ids, ldn=128))
    # W exactly 0 with V > 0: tested {1, 4} against {2, 3}; and W = 1/2 ({2, 16} against {2, 6}), which the continuity
    # correction takes to a numerator of exactly 0
    cs.append(_case("W_zero", 13, 1, [1, 1, 0, 0], y=[[1, 4, 2, 3], [2, 16, 2, 6]], sf=[1.0, 1.0, 1.0, 1.0]))
    cs.append(_case("W_zero_strata", 14, 1, [1, 1, 0, 0, 1, 0, 0, 1], [0, 0, 0, 0, 1, 1, 1, 1],
                    y=[[1, 4, 2, 3, 5, 6, 7, 8], [1, 4, 2, 3, 9, 6, 7, 8]], sf=[1.0] * 8))
    return cs


def big_cases():
    """One stratum of 16 384 samples (L = 16 384, one wave per workgroup) and 8192 + 8192 in two strata."""
    rng = np.random.default_rng(21)
    cs = [_case("n16384", 15, 5, _two_groups(rng, 16384, 5000))]
    lab = np.concatenate([_two_groups(rng, 8192, 4000), _two_groups(rng, 8192, 100)])
    ids = np.repeat([0, 1], 8192)
    perm = rng.permutation(16384)
    cs.append(_case("n8192x2", 16, 5, lab[perm], ids[perm]))
    return cs


def refused_case():
    """8193 + 8191 in two strata: L = 16 384 + 8192 = 24 576."""
    rng = np.random.default_rng(22)
    lab = np.concatenate([_two_groups(rng, 8193, 4000), _two_groups(rng, 8191, 100)])
    return _case("n8193_8191", 17, 1, lab, np.concatenate([np.zeros(8193, int), np.ones(8191, int)]))


ALTS = (None, "greater", "less")
