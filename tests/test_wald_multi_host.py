"""Wald tests of many contrasts without a GPU: the host instantiation (tests/hostwald) of wald_gene_multi (register path)
and wald_gene_multi_wide (run-time-P path, both workspaces) against the oracle and the reference's fixture outputs, and
pairwise_contrasts."""
import numpy as np
import pandas as pd
import pytest

from tests import hostwald as hw
from tests.wald_multi_cases import ALTS, check, kat, oracle_ref

REG = ["p1", "p2", "p8m", "p12"]
CASES = [(c, False) for c in REG] + [(c, True) for c in ("p2", "p12", "p16", "p65")]


@pytest.mark.parametrize("alt,null", ALTS, ids=[a or "none" for a, _ in ALTS])
@pytest.mark.parametrize("case,wide", CASES, ids=[c + ("_wide" if w else "") for c, w in CASES])
def test_every_contrast_vs_oracle_and_fixture(case, wide, alt, null):
    """Every contrast of the set (the fixture's own, every unit vector, a pairwise difference, four dense ones) from ONE
    Gram matrix and ONE factorisation per gene, against orc.wald_test at the tolerances of the Wald KAT test (SE 1e-10,
    statistic 1e-9 + 1e-13, p 1e-8 + 1e-300); the fixture's own contrast also against the unmodified reference's
    outputs.  From the caller's mu and from mu = sf exp(X beta)."""
    k, disp, mu, ridge, cons = kat(case)
    ref = oracle_ref(case, alt)
    tag = alt or "none"
    fix = tuple(k[f"wald_{q}_{tag}"][None, :] for q in ("p", "stat", "se"))
    for kw in (dict(mu=mu), dict(sf=k["sf"])):
        got = hw.wald_multi(k["X"], disp, k["lfc_beta"], ridge, cons, np.log(2) * null, alt, wide=wide, **kw)
        check(got, ref, f"{case} {tag} {list(kw)} vs oracle")
        check(tuple(a[:1] for a in got), fix, f"{case} {tag} {list(kw)} vs fixture")


def test_one_contrast_and_contrast_order_do_not_matter():
    """K = 1 and a permuted set give the same bits per contrast as the full set (nothing carries over between
    contrasts); NaN dispersion (all-zero gene): NaN for every contrast."""
    k, disp, mu, ridge, cons = kat("p8m")
    full = hw.wald_multi(k["X"], disp, k["lfc_beta"], ridge, cons, mu=mu)
    perm = np.random.default_rng(0).permutation(len(cons))
    for wide in (False, True):
        base = hw.wald_multi(k["X"], disp, k["lfc_beta"], ridge, cons, mu=mu, wide=wide)
        shuf = hw.wald_multi(k["X"], disp, k["lfc_beta"], ridge, cons[perm], mu=mu, wide=wide)
        one = hw.wald_multi(k["X"], disp, k["lfc_beta"], ridge, cons[3:4], mu=mu, wide=wide)
        for a, b, c in zip(base, shuf, one):
            assert np.array_equal(a[perm], b) and np.array_equal(a[3:4], c)
    d = disp.copy()
    d[2] = np.nan
    got = hw.wald_multi(k["X"], d, k["lfc_beta"], ridge, cons, mu=mu)
    for a, b in zip(got, full):
        assert np.isnan(a[:, 2]).all() and np.array_equal(np.delete(a, 2, 1), np.delete(b, 2, 1))


def test_pairwise_contrasts_needs_only_obs():
    from types import SimpleNamespace

    from pydeseq2_amd import pairwise_contrasts

    dds = SimpleNamespace(obs=pd.DataFrame({"group": ["b", "a", "c", "a", "b", "c"], "dose": [10, 2, 2, 10, 2, 10]}))
    assert pairwise_contrasts(dds, "group") == [["group", "b", "a"], ["group", "c", "a"], ["group", "c", "b"]]
    assert pairwise_contrasts(dds, "dose") == [["dose", "2", "10"]]  # levels sort as strings, as DeseqStats resolves them
    with pytest.raises(ValueError, match=r"The contrast variable \('batch'\) should be one of the design factors"):
        pairwise_contrasts(dds, "batch")


def test_entry_point_is_declared_and_the_abi_version_stays():
    import os
    import re

    from pydeseq2_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "deseq_hip.h")).read()
    assert re.search(r"int dsq_dev_wald_multi\(", hdr) and "dsq_dev_wald_multi" in _lib.EXPORTS
    assert re.search(r"#define DSQ_ABI_VERSION 5\b", hdr)
    from pydeseq2_amd import DeseqStats
    from pydeseq2_amd.pipeline import DeseqPipeline

    assert callable(DeseqStats.batch) and callable(DeseqPipeline.wald_multi)
