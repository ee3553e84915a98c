"""Wald tests of many contrasts in one launch on the GPU: dsq_dev_wald_multi (k_wald_multi<P> up to 12 columns,
k_wald_multi_wide over both geometries beyond) against the oracle, the reference's fixture outputs and K calls of
dsq_dev_wald; DeseqPipeline.wald_multi and DeseqStats.batch against the single-contrast path."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

from tests.wald_multi_cases import ALT_CODE, ALTS, TOL, check, excess, kat, oracle_ref

pytestmark = pytest.mark.gpu

_vp = C.c_void_p
CASES = ["p1", "p2", "p8m", "p12", "p16", "p48", "p65", "p128"]
KS = (1, 2, 63, 64, 65, 130)  # the boundaries of "lane l takes the contrasts l, l + 64, ..."
GUARD = 8


@pytest.fixture(scope="module")
def ctx():
    from pydeseq2_amd._lib import Context

    return Context(0)


class _Dev:
    """The device copies of one fixture's Wald inputs (gene-major mu with ldn = N, the transposed design with ldx = N)."""

    def __init__(self, ctx, case):
        from pydeseq2_amd._lib import DeviceArray

        k, disp, mu, ridge, cons = kat(case)
        self.ctx, self.N, self.P, self.G = ctx, *k["X"].shape, len(disp)
        up = lambda a: DeviceArray.from_host(ctx, np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
        self.sf, self.Xt, self.disp, self.beta = up(k["sf"]), up(k["X"].T), up(disp), up(k["lfc_beta"])
        self.mu, self.ridge, self.up = up(mu.T), np.ascontiguousarray(ridge), up

    def multi(self, cons, null_ln, alt, with_mu, G=None, K=None):
        """dsq_dev_wald_multi -> (p, stat, se), each K x G.  The outputs start as NaN with a guard block behind each:
        nothing in range stays NaN, the guards stay."""
        G = self.G if G is None else G
        K = len(cons) if K is None else K
        d_c = self.up(cons)
        host = np.full((3, G * K + GUARD), np.nan)
        host[:, G * K:] = -7.0
        d_o = self.up(host.ravel())
        ptr = [_vp(d_o.ptr + 8 * i * (G * K + GUARD)) for i in range(3)]
        self.ctx.call("dsq_dev_wald_multi", _vp(self.mu.ptr) if with_mu else None, self.N, _vp(self.sf.ptr),
                      _vp(self.Xt.ptr), self.N, self.N, G, self.P, _vp(self.disp.ptr), _vp(self.beta.ptr),
                      _vp(self.ridge.ctypes.data), _vp(d_c.ptr), K, C.c_double(null_ln), ALT_CODE[alt], *ptr)
        o = d_o.to_host().reshape(3, G * K + GUARD)
        assert (o[:, G * K:] == -7.0).all(), "guard block behind [G][K] overwritten"
        assert not np.isnan(o[:, :G * K]).any(), "an output in range was not written"
        return tuple(np.ascontiguousarray(o[i, :G * K].reshape(G, K).T) for i in range(3))

    def single(self, c, null_ln, alt, with_mu):
        d_o = self.up(np.full(3 * self.G, np.nan))
        c = np.ascontiguousarray(c, dtype=np.float64)
        self.ctx.call("dsq_dev_wald", _vp(self.mu.ptr) if with_mu else None, self.N, _vp(self.sf.ptr), _vp(self.Xt.ptr),
                      self.N, self.N, self.G, self.P, _vp(self.disp.ptr), _vp(self.beta.ptr), _vp(self.ridge.ctypes.data),
                      _vp(c.ctypes.data), C.c_double(null_ln), ALT_CODE[alt], _vp(d_o.ptr), _vp(d_o.ptr + 8 * self.G),
                      _vp(d_o.ptr + 16 * self.G))
        return d_o.to_host().reshape(3, self.G)


@pytest.mark.parametrize("alt,null", ALTS, ids=[a or "none" for a, _ in ALTS])
@pytest.mark.parametrize("case", CASES)
def test_kernel_vs_oracle_fixture_and_single_launches(ctx, case, alt, null):
    """K in {1, 2, 63, 64, 65, 130} contrasts (the set of tests/wald_multi_cases.py, cycled) x {all genes, 1, 5} x {mu
    given, mu = sf exp(X beta)}: every (gene, contrast) against orc.wald_test and against dsq_dev_wald of that contrast
    at SE 1e-10, statistic 1e-9 + 1e-13, p 1e-8 + 1e-300; the fixture's own contrast against the unmodified reference's
    outputs; two calls give the same bits.  Largest difference between one multi launch and the single launches
    measured on the MI355X, over all fixtures and alternatives: see DESIGN.md ("Wald tests of many contrasts")."""
    k, disp, mu, ridge, cons = kat(case)
    ref = oracle_ref(case, alt)
    tag, null_ln = alt or "none", np.log(2) * null
    fix = tuple(k[f"wald_{q}_{tag}"][None, :] for q in ("p", "stat", "se"))
    D = _Dev(ctx, case)
    worst = dict(p=0.0, stat=0.0, se=0.0)
    bits_equal = True
    for with_mu in (True, False):
        one = np.stack([D.single(c, null_ln, alt, with_mu) for c in cons], axis=1)  # [3][K_set][G]
        for K in KS:
            idx = np.arange(K) % len(cons)
            for G in (D.G, 1, 5):
                got = D.multi(cons[idx], null_ln, alt, with_mu, G=G)
                what = f"{case} {tag} mu={'given' if with_mu else 'NULL'} K={K} G={G}"
                check(got, tuple(a[idx][:, :G] for a in ref), what + " vs oracle")
                check(tuple(a[:1] for a in got), tuple(a[:, :G] for a in fix), what + " vs fixture")
                for i, name in enumerate(("p", "stat", "se")):
                    worst[name] = max(worst[name], excess(got[i], one[i][idx][:, :G], *TOL[name]))
                    bits_equal &= np.array_equal(got[i], one[i][idx][:, :G])
                if G == D.G:
                    again = D.multi(cons[idx], null_ln, alt, with_mu, G=G)
                    assert all(np.array_equal(a, b) for a, b in zip(got, again)), what + ": two calls differ"
    print(f"[wald_multi vs dsq_dev_wald] {case} {tag}: fractions of the tolerances {worst}, bits equal: {bits_equal}")
    assert max(worst.values()) <= 1.0, f"{case} {tag}: multi vs K single launches, fractions of the tolerances {worst}"


def test_argument_checks(ctx):
    from pydeseq2_amd import _lib

    D = _Dev(ctx, "p2")
    cons = kat("p2")[4]
    lib, d_c, d_o = _lib.load(), D.up(cons), D.up(np.full(3 * D.G * len(cons), -7.0))

    def rc(P, K, alt):
        return lib.dsq_dev_wald_multi(ctx.h, None, D.N, _vp(D.sf.ptr), _vp(D.Xt.ptr), D.N, D.N, D.G, P, _vp(D.disp.ptr),
                                      _vp(D.beta.ptr), _vp(D.ridge.ctypes.data), _vp(d_c.ptr), K, C.c_double(0.0), alt,
                                      _vp(d_o.ptr), _vp(d_o.ptr + 8 * D.G * len(cons)),
                                      _vp(d_o.ptr + 16 * D.G * len(cons)))

    for bad in ((2, 0, 0), (2, -3, 0), (0, 1, 0), (129, 1, 0), (2, 1, 5), (2, 1, -1)):
        assert rc(*bad) == -2, bad  # DSQ_ERR_ARG
        assert lib.dsq_last_error(ctx.h).decode()
    assert (d_o.to_host() == -7.0).all()  # a refused call writes nothing
    with pytest.raises(ValueError, match="at least one contrast"):
        D.multi(cons, 0.0, None, True, K=0)
    assert rc(2, len(cons), 0) == 0


# ------------------------------------------------------------------ pipeline and façade
def _scenario():
    """300 genes x 64 samples, ~batch + group (2 x 4 cells of 8 replicates): gene 5 carries one huge count (replaced and
    refitted), gene 9 a single count on an otherwise empty gene (all zero after the replacement), gene 11 is empty."""
    N, G = 64, 300
    i = np.arange(N)
    meta = pd.DataFrame({"batch": np.where(i % 2 == 0, "a", "b"), "group": np.array(["g0", "g1", "g2", "g3"])[(i // 2) % 4]},
                        index=[f"s{k}" for k in i])
    X = np.column_stack([np.ones(N), i % 2 == 1] + [(i // 2) % 4 == q for q in (1, 2, 3)]).astype(float)
    rng = np.random.default_rng(64)
    beta = np.vstack([rng.normal(6.0, 1.0, G), rng.normal(0, 0.4, G)] + [rng.normal(0, 0.6, G) for _ in range(3)])
    beta[2:, ::3] = 0.0
    disp = 4 / 2.0 ** beta[0] + 0.05
    sf = np.exp(rng.normal(0, 0.2, N))
    mu = sf[:, None] * 2.0 ** (X @ beta)
    counts = rng.negative_binomial(1 / disp[None, :], (1 / disp[None, :]) / (1 / disp[None, :] + mu)).astype(np.int64)
    counts[7, 5] = 400 * counts[:, 5].max()
    counts[:, 9] = 0
    counts[3, 9] = 5000
    counts[:, 11] = 0
    return pd.DataFrame(counts, index=meta.index, columns=[f"g{j}" for j in range(G)]), meta


@pytest.fixture(scope="module")
def dds():
    from pydeseq2_amd import DeseqDataSet

    counts, meta = _scenario()
    d = DeseqDataSet(counts=counts, metadata=meta, design="~batch + group")
    d.deseq2()
    assert list(np.nonzero(np.asarray(d._res.new_all_zeroes, bool))[0]) == [9] and not d.var["non_zero"].iloc[11]
    yield d
    d.close()


def _counted(dds, monkeypatch):
    pipe, n = dds._pipe, dict(wald=0, wald_multi=0)
    for name in n:
        def wrapped(*a, _f=getattr(pipe, name), _n=name, **kw):
            n[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(pipe, name, wrapped)
    return n


def _same_summary(a, b, what):
    for col in ("baseMean", "log2FoldChange"):
        assert np.array_equal(a[col].to_numpy(), b[col].to_numpy(), equal_nan=True), f"{what} {col}"
    for col, name in (("lfcSE", "se"), ("stat", "stat"), ("pvalue", "p")):
        assert excess(a[col].to_numpy(), b[col].to_numpy(), *TOL[name]) <= 1.0, f"{what} {col}"
    x, y = a["padj"].to_numpy(), b["padj"].to_numpy()  # as tests/test_gpu_summary.py::_same
    assert (np.isnan(x) == np.isnan(y)).all(), f"{what} padj"
    np.testing.assert_allclose(x[~np.isnan(y)], y[~np.isnan(y)], rtol=1e-12, atol=0, err_msg=f"{what} padj")


@pytest.mark.parametrize("kwargs", [dict(), dict(prior_LFC_var=np.array([4.0, 1.0, 0.5, 0.5, 2.0])),
                                    dict(alt_hypothesis="greaterAbs", lfc_null=0.4, independent_filter=False)],
                         ids=["default", "prior_LFC_var", "greaterAbs"])
def test_batch_equals_one_deseqstats_per_contrast(dds, monkeypatch, kwargs):
    from pydeseq2_amd import DeseqStats, pairwise_contrasts

    contrasts = pairwise_contrasts(dds, "group") + [np.array([0.0, 1.0, 0.0, 0.0, 0.0])]
    assert len(contrasts) == 7 and contrasts[0] == ["group", "g1", "g0"] and contrasts[5] == ["group", "g3", "g2"]
    n = _counted(dds, monkeypatch)
    batch = DeseqStats.batch(dds, contrasts, **kwargs)
    assert n == dict(wald=0, wald_multi=1) and len(batch) == 7
    got = [b.summary() for b in batch]
    assert n == dict(wald=0, wald_multi=1), "summary() of a batch member ran a Wald kernel"
    for c, b, g in zip(contrasts, batch, got):
        assert isinstance(b, DeseqStats) and np.array_equal(b.contrast_vector, DeseqStats(dds, c).contrast_vector)
        want = DeseqStats(dds, c, **kwargs).summary()
        _same_summary(g, want, f"{c}")
        for z in (9,):  # all zero after the replacement (ds.py:357-360), for every contrast
            assert b.SE.iloc[z] == 0.0 and b.statistics.iloc[z] == 0.0 and g["stat"].iloc[z] == 0.0
        assert np.isnan(g["lfcSE"].iloc[11])  # empty from the start: no fit, as on the single-contrast path
        if kwargs.get("alt_hypothesis") is None:  # (the one-sided statistics drop NaN terms: numpy.fmax, utils.py:778-806)
            assert np.isnan(g["pvalue"].iloc[11]) and np.isnan(g["stat"].iloc[11])
    assert n["wald"] == 7 and n["wald_multi"] == 1
    # new hypothesis on a batch member: the single-contrast path, as on any DeseqStats
    s = batch[2].summary(alt_hypothesis="less", lfc_null=-0.2)
    assert n["wald"] == 8
    _same_summary(s, DeseqStats(dds, contrasts[2], **{**kwargs, "alt_hypothesis": "less", "lfc_null": -0.2}).summary(),
                  "re-run")


def test_all_zero_rule_and_pipeline_wald_multi(dds):
    pipe, res = dds._pipe, dds._res
    rng = np.random.default_rng(5)
    cons = np.vstack([np.eye(5), rng.normal(size=(66, 5))])  # 71: more than one pass of the lanes
    pv, st, se = pipe.wald_multi(res, cons, lfc_null=0.3, alt_hypothesis="lessAbs")
    assert pv.shape == st.shape == se.shape == (71, 300)
    assert (pv[:, 9] == 1.0).all() and (st[:, 9] == 0.0).all() and (se[:, 9] == 0.0).all()
    assert np.isnan(se[:, 11]).all()  # empty from the start (its lessAbs statistic is numpy.fmax's: checked below)
    for k in (0, 4, 63, 64, 70):
        check((pv[k], st[k], se[k]), pipe.wald(res, cons[k], lfc_null=0.3, alt_hypothesis="lessAbs"), f"contrast {k}")
    with pytest.raises(ValueError, match=r"wald\(\)"):
        pipe.wald_multi(res, cons[0])
    with pytest.raises(ValueError, match="K x 5"):
        pipe.wald_multi(res, cons[:, :4])
    with pytest.raises(ValueError, match="positive lfc_null"):
        pipe.wald_multi(res, cons, lfc_null=-1.0, alt_hypothesis="greaterAbs")
    with pytest.raises(KeyError):
        pipe.wald_multi(res, cons, alt_hypothesis="two-sided")


def test_batch_refuses_before_anything_is_launched(dds, monkeypatch):
    from pydeseq2_amd import DeseqStats

    n = _counted(dds, monkeypatch)
    good = ["group", "g1", "g0"]
    with pytest.raises(ValueError, match="at least one contrast"):
        DeseqStats.batch(dds, [])
    with pytest.raises(ValueError, match="does not depend on the contrast"):
        DeseqStats.batch(dds, [good], test="LRT", reduced="~batch")
    with pytest.raises(ValueError, match="should be levels of 'group'"):
        DeseqStats.batch(dds, [good, ["group", "g9", "g0"]])
    with pytest.raises(ValueError, match="same length as the design matrix"):
        DeseqStats.batch(dds, [good, np.ones(3)])
    with pytest.raises(ValueError, match="should be one of the design factors"):
        DeseqStats.batch(dds, [["dose", "a", "b"], good])
    assert n == dict(wald=0, wald_multi=0)
