"""The few-cell LFC fit (irls_gene<Wv, P, 3> / <Wv, P, 2> of csrc/dsq_irls.h) in its host build against the oracle, on the
seeded cases of tests/irls_two_cell_cases.py: every gene, diverging ones included, at the tolerances
tests/test_gpu_parity.py holds for the same quantities of this kernel."""
import numpy as np
import pytest

from tests import irls_two_cell_cases as tc


@pytest.mark.parametrize("name", tc.case_names())
def test_host_build_vs_oracle(name):
    c = tc.by_name(name)
    ref, got = c.oracle, c.host
    assert (ref["conv"] == got["conv"]).all(), np.nonzero(ref["conv"] != got["conv"])[0]
    cell = tc.orc.design_cells(c.X)[0]
    assert any((c.counts[cell == k].sum(0) == 0).any() for k in np.unique(cell)), "no gene is all zero in a group"
    assert np.bincount(cell).min() < 3, "no cell below three replicates"
    assert c.counts.max() >= 256 and (c.counts >= 64).any()
    assert np.log10(c.sf.max() / c.sf.min()) >= 2.0 - 1e-12
    tc.compare(got, ref, name + " host vs oracle", ("beta", "mu", "H", "se", "stat", "p", "cooks"))
