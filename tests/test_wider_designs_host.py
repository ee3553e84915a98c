"""Designs of 49 ... 128 columns without a GPU: the raised limit (DSQ_MAX_P = 128) as the header, the binding and the
design packer state it, the paired `~subject + condition` design of the façade, and the host instantiation of the
run-time-P templates over the workspace of the wider kernel family (tests/hostwide) against the reference KATs."""
import os
import re

import numpy as np
import pandas as pd
import pytest
from scipy.stats import f as f_dist

from oracle import nbglm_oracle as orc
from tests import hostwide as hw
from tests.helpers import assert_close, load_kat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_define(name):
    with open(os.path.join(ROOT, "include", "deseq_hip.h")) as fh:
        return int(re.search(rf"#define {name} (\d+)", fh.read()).group(1))


def test_width_limits_agree_and_shrinkage_stays_at_48():
    from pydeseq2_amd import _lib
    from pydeseq2_amd._design import MAX_DESIGN_COLUMNS

    assert _header_define("DSQ_MAX_P") == _lib.DSQ_MAX_P == MAX_DESIGN_COLUMNS == 128
    assert _header_define("DSQ_SHRINK_MAX_P") == _lib.DSQ_SHRINK_MAX_P == 48
    assert _header_define("DSQ_BFGS_MAX_P") == 12
    assert _header_define("DSQ_ABI_VERSION") == 5
    assert hw.lib().hw_max_p() == 128


@pytest.mark.parametrize("P", [65, 72, 128])
def test_design_pack_takes_up_to_128_columns(P):
    from pydeseq2_amd._design import DesignPack

    rng = np.random.default_rng(P)
    X = np.column_stack([np.ones(300)] + [rng.normal(size=300) for _ in range(P - 1)])
    D = DesignPack(X)
    assert D.P == P and D.full_rank
    assert np.array_equal(D.Xt[:, :300], X.T)


def test_design_pack_refuses_129_columns():
    from pydeseq2_amd._design import DesignPack

    rng = np.random.default_rng(1)
    X = np.column_stack([np.ones(300)] + [rng.normal(size=300) for _ in range(128)])
    with pytest.raises(ValueError, match="at most 128"):
        DesignPack(X)


def test_paired_design_of_64_subjects_builds_65_columns_without_the_gpu():
    from pydeseq2_amd.api import DeseqDataSet

    n_sub = 64
    idx = [f"s{i}" for i in range(2 * n_sub)]
    meta = pd.DataFrame({"subject": [f"p{i // 2:02d}" for i in range(2 * n_sub)],
                         "condition": ["A", "B"] * n_sub}, index=idx)
    counts = pd.DataFrame(np.arange(2 * n_sub * 5).reshape(2 * n_sub, 5) % 17, index=idx,
                          columns=[f"g{j}" for j in range(5)])
    dds = DeseqDataSet(counts=counts, metadata=meta, design="~subject + condition")
    assert dds._pipe_obj is None
    X = np.asarray(dds.obsm["design_matrix"], dtype=float)
    assert X.shape == (2 * n_sub, 65)
    assert np.linalg.matrix_rank(X) == 65
    assert list(dds.obsm["design_matrix"].columns)[-1] == "condition[T.B]"


@pytest.mark.parametrize("case", ["p65", "p72", "p128"])
def test_wider_templates_vs_reference_kats(case):
    """dsq_wide.h over WiderWork (matrices bound apart from the LDS part, as SlotGeom of dsq_k_wide.hip binds them)
    against the reference, at the tolerances of the 13 ... 48-column KATs
    (test_hostsim.py::test_wide_path_vs_reference_kats)."""
    k = load_kat(case)
    counts, X, sf = k["counts"], k["X"], k["sf"]
    N, P = X.shape
    maxd = float(max(10, N))
    tol = 2e-6
    m = hw.mom(counts, sf, X, 1e-8, maxd)
    assert_close(m["rough"], k["rough"], 1e-9, 1e-13, "rough")
    assert_close(m["moments"], k["moments"], 1e-10, 1e-14, "moments")
    assert_close(m["lin_mu"], k["lin_mu"], 1e-10, 0, "lin_mu")
    a, c = hw.alpha_mle(counts, X, k["mu_hat"], k["mom"], 1e-8, maxd)
    assert (c == k["gw_conv"]).all()
    assert_close(a, k["gw_alpha"], tol, 0, "genewise alpha")
    a, c = hw.alpha_mle(counts, X, k["mu_hat"], k["fitted"], 1e-8, maxd, prior_var=float(k["prior_var"]),
                        prior_reg=True)
    assert (c == k["map_conv"]).all()
    assert_close(a, k["map_alpha"], tol, 0, "MAP alpha")
    r = hw.lfc_fit(counts, sf, X, k["mom"])
    assert (r["conv"] == k["irls_conv"]).all()
    assert_close(r["beta"], k["irls_beta"], 1e-8, 1e-10, "irls beta")
    assert_close(r["mu"], k["irls_mu"], 1e-8, 1e-10, "irls mu")
    assert_close(r["H"], k["irls_H"], 1e-8, 1e-12, "irls H")
    disp = np.clip(k["map_alpha"], 1e-8, maxd)
    cutoff = f_dist.ppf(0.99, P, N - P)
    rd = orc.robust_mom_disp(k["normed"], X)
    r = hw.lfc_fit(counts, sf, X, disp, robust_disp=rd, cutoff=cutoff, contrast=k["contrast"])
    assert (r["conv"] == k["lfc_conv"]).all()
    assert_close(r["beta"], k["lfc_beta"], 1e-8, 1e-10, "lfc beta")
    assert_close(r["H"], k["lfc_H"], 1e-8, 1e-12, "lfc H")
    assert_close(r["se"], k["wald_se_none"], 1e-8, 0, "wald se")
    assert_close(r["stat"], k["wald_stat_none"], 1e-7, 1e-11, "wald stat")
    assert_close(r["p"], k["wald_p_none"], 1e-6, 1e-300, "wald p")
    ref_ck = orc.cooks_distance(counts, k["normed"], X, k["lfc_mu"], k["lfc_H"])
    assert_close(r["cooks"], ref_ck, 1e-7, 1e-300, "cooks")


def test_wider_rescue_vs_oracle():
    """maxiter = 2 sends every gene through the L-BFGS-B rescue over LbfgsbWork<128> (utils.py:374-413): the paired
    design against the oracle's restatement, which is checked to have taken the rescue for every gene."""
    X = np.column_stack([np.ones(128)] + [(np.arange(128) // 2 == s) for s in range(1, 64)] +
                        [np.arange(128) % 2 == 1]).astype(float)
    k = load_kat("p65")
    counts = k["counts"][:, :12]
    sf, disp = k["sf"], np.full(12, 0.1)
    assert np.array_equal(X, k["X"])
    calls = [0]
    fallback = orc._irls_fallback

    def spy(*a, **kw):
        calls[0] += 1
        return fallback(*a, **kw)

    orc._irls_fallback = spy
    try:
        start = np.linalg.qr(X)
        ref = [orc.irls_gene(counts[:, g], sf, X, disp[g], start, maxiter=2) for g in range(12)]
    finally:
        orc._irls_fallback = fallback
    assert calls[0] == 12
    r = hw.lfc_fit(counts, sf, X, disp, maxiter=2)
    assert (r["conv"] == np.array([x[3] for x in ref])).all()
    assert_close(r["beta"], np.array([x[0] for x in ref]), 1e-7, 1e-9, "rescue beta")
    assert_close(r["mu"], np.array([x[1] for x in ref]).T, 1e-7, 1e-10, "rescue mu")
    assert_close(r["H"], np.array([x[2] for x in ref]).T, 1e-7, 1e-12, "rescue H")
