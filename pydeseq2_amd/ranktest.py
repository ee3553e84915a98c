"""Wilcoxon rank-sum test (Mann-Whitney; with strata: van Elteren) of comparisons on the normalised counts: host side.

The layout of each comparison - the used samples ordered by stratum, the strata's offsets and their places in the gene's
LDS row - and every refusal are decided here; the ranking runs on the device (csrc/dsq_rank.h, dsq_dev_ranksum), one gene
per wavefront.  DESIGN.md 6k is the statement of the test."""
from dataclasses import dataclass

import numpy as np

from ._lib import ALT, DeviceScope, _vp, launch, split

RANK_MAX_L = 16384  # DSQ_RANK_MAX_L: LDS doubles per gene
RANK_ALT = (None, "greater", "less")


def next_pow2(n: int) -> int:
    L = 1
    while L < n:
        L <<= 1
    return L


def check_alternative(alt_hypothesis, lfc_null=0.0):
    """The rank-sum test is two-sided, "greater" or "less", and has no LFC threshold."""
    if lfc_null != 0:
        raise ValueError("The rank-sum test has no lfc_null: it compares the distributions of two groups "
                         f"(got lfc_null={lfc_null}; use test='wald' for a thresholded test).")
    if alt_hypothesis not in RANK_ALT:
        raise ValueError(f"The rank-sum test is two-sided (None), 'greater' or 'less' (got {alt_hypothesis!r}; "
                         "'greaterAbs' / 'lessAbs' need an LFC threshold: use test='wald').")


@dataclass
class RankLayout:
    """One comparison.  ``order[seg[s]:seg[s+1]]``: the used samples of stratum s; ``pad``: prefix sums of
    next_pow2(N_s), ``pad[-1]`` = L; ``n1`` / ``n2``: tested / reference samples per stratum."""
    order: np.ndarray
    seg: np.ndarray
    pad: np.ndarray
    n1: np.ndarray
    n2: np.ndarray

    @property
    def n_strata(self):
        return len(self.seg) - 1

    @property
    def L(self):
        return int(self.pad[-1])

    @property
    def pairs(self):
        """Sum over the strata of n1_s n2_s: what ``usum`` is divided by for the AUC."""
        return int(np.sum(self.n1.astype(np.int64) * self.n2.astype(np.int64)))


def build_layout(labels, strata=None) -> RankLayout:
    """``labels`` (N): 1 tested, 0 reference, -1 left out.  ``strata`` (N, optional): any integers, one id per sample;
    the distinct ids among the used samples become the strata 0 ... S-1 in ascending order.  ValueError: other labels, a
    group without samples, lengths that differ, a padded row above DSQ_RANK_MAX_L."""
    lab = np.asarray(labels)
    if lab.ndim != 1 or not np.isin(lab, (-1, 0, 1)).all():
        raise ValueError("ranksum: labels are 1 (tested), 0 (reference) or -1 (left out), one per sample.")
    used = np.nonzero(lab >= 0)[0]
    if not (lab == 1).any() or not (lab == 0).any():
        raise ValueError("ranksum: a comparison needs at least one tested and one reference sample.")
    if strata is None:
        sid = np.zeros(len(used), np.int64)
    else:
        st = np.asarray(strata)
        if st.shape != lab.shape:
            raise ValueError(f"ranksum: strata must have one id per sample (got {st.shape} for {lab.shape[0]} samples).")
        _, sid = np.unique(st[used], return_inverse=True)
    o = np.argsort(sid, kind="stable")
    order = used[o].astype(np.int32)
    sizes = np.bincount(sid).astype(np.int64)
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pad = np.concatenate([[0], np.cumsum([next_pow2(int(n)) for n in sizes])]).astype(np.int64)
    if pad[-1] > RANK_MAX_L:
        raise ValueError(f"ranksum: the strata of this comparison need {int(pad[-1])} doubles per gene (the sum of "
                         f"next_pow2 of their sizes {sizes.tolist() if len(sizes) <= 8 else '...'}); at most {RANK_MAX_L} "
                         f"(DSQ_RANK_MAX_L) are supported.")
    n1 = np.bincount(sid, weights=(lab[used] == 1)).astype(np.int32)
    return RankLayout(order, seg, pad.astype(np.int32), n1, (sizes - n1).astype(np.int32))


@dataclass
class PackedLayouts:
    """K layouts as dsq_dev_ranksum takes them: rows of pitch ldo / lds / ldl."""
    order: np.ndarray
    seg: np.ndarray
    pad: np.ndarray
    nstrata: np.ndarray
    labels: np.ndarray

    @property
    def ldo(self):
        return self.order.shape[1]

    @property
    def lds(self):
        return self.seg.shape[1]

    @property
    def ldl(self):
        return self.labels.shape[1]


def pack_layouts(layouts, labels) -> PackedLayouts:
    labels = np.atleast_2d(np.asarray(labels))
    K = len(layouts)
    ldo = max(1, max(len(q.order) for q in layouts))
    lds = max(q.n_strata for q in layouts) + 1
    order, seg, pad = np.zeros((K, ldo), np.int32), np.zeros((K, lds), np.int32), np.zeros((K, lds), np.int32)
    for k, q in enumerate(layouts):
        order[k, :len(q.order)] = q.order
        seg[k, :len(q.seg)] = q.seg
        pad[k, :len(q.pad)] = q.pad
    return PackedLayouts(order, seg, pad, np.array([q.n_strata for q in layouts], np.int32),
                         np.ascontiguousarray(labels, dtype=np.int8))


@dataclass
class RankSumResult:
    """Row k: comparison k.  ``usum`` = sum over the strata of U_s (exact half-integers), ``ties`` = sum of t^3 - t over
    the tie runs (exact integers), ``auc`` = usum / pairs: the probability that a tested sample lies above a reference
    sample of its stratum (ties count half).  ``n1`` / ``n2`` / ``n_strata`` / ``pairs``: per comparison."""
    statistic: np.ndarray
    pvalue: np.ndarray
    usum: np.ndarray
    ties: np.ndarray
    auc: np.ndarray
    n1: np.ndarray
    n2: np.ndarray
    n_strata: np.ndarray
    pairs: np.ndarray


def ranksum(pipe, d_y, ldn, size_factors, G, labels, strata=None, alt_hypothesis=None) -> RankSumResult:
    """Rank-sum tests of K comparisons (``labels``: K x N, or one vector) on the gene-major int32 counts at the device
    pointer ``d_y`` (G rows of pitch ``ldn``) normalised by ``size_factors``, on the device of ``pipe`` (a DeseqPipeline,
    or a ``_lib.Context``): one packed upload, one launch of dsq_dev_ranksum, one download.  ``strata``: one id per
    sample, shared by the comparisons.  Every refusal is raised before anything touches the device."""
    check_alternative(alt_hypothesis)
    lab = np.atleast_2d(np.asarray(labels))
    sf = np.ascontiguousarray(size_factors, dtype=np.float64)
    K, N = lab.shape
    if sf.shape != (N,):
        raise ValueError(f"ranksum: labels are K x N with N = {sf.shape[0]} samples (got {lab.shape}).")
    if N < 2 or ldn < N:
        raise ValueError("ranksum: at least two samples, and a row pitch of at least N.")
    if not (np.isfinite(sf) & (sf > 0)).all():
        raise ValueError("ranksum: the size factors must be finite and positive.")
    layouts = [build_layout(lab[k], strata) for k in range(K)]
    P = pack_layouts(layouts, lab)
    nan = np.full((K, G), np.nan)
    res = RankSumResult(nan.copy(), nan.copy(), nan.copy(), nan.copy(), nan.copy(),
                        np.array([q.n1.sum() for q in layouts]), np.array([q.n2.sum() for q in layouts]),
                        P.nstrata.copy(), np.array([q.pairs for q in layouts], np.int64))
    if G == 0:
        return res
    ints = np.concatenate([P.order.ravel(), P.seg.ravel(), P.pad.ravel(), P.nstrata])
    h_in = np.concatenate([sf.view(np.uint8), ints.view(np.uint8), P.labels.ravel().view(np.uint8)])
    with DeviceScope(split(pipe)[1]) as s:
        d_in = s.upload(h_in)
        d_out = s.empty((4 * K * G,), np.float64)
        i0 = d_in.ptr + 8 * N
        o_seg = i0 + 4 * P.order.size
        o_pad = o_seg + 4 * P.seg.size
        o_ns = o_pad + 4 * P.pad.size
        o_lab = o_ns + 4 * K
        launch(pipe, "ranksum", K * G, "dsq_dev_ranksum", _vp(d_y), int(ldn), _vp(d_in.ptr), N, G, K, _vp(i0), P.ldo,
               _vp(o_seg), _vp(o_pad), P.lds, _vp(o_ns), _vp(o_lab), P.ldl, ALT[alt_hypothesis], _vp(d_out.ptr),
               _vp(d_out.ptr + 8 * K * G), _vp(d_out.ptr + 16 * K * G), _vp(d_out.ptr + 24 * K * G), G)
        o = d_out.to_host().reshape(4, K, G)
    res.statistic, res.pvalue, res.usum, res.ties = (o[j].copy() for j in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):  # (no stratum with both groups: no pair, NaN)
        res.auc = res.usum / res.pairs[:, None].astype(np.float64)
    return res
