"""The few-cell LFC fit on the GPU (dsq_dev_lfc_fit2 -> k_irls<P, 3> / k_irls<P, 2>, staged with LDS-typed operands and
unstaged) on the seeded cases of tests/irls_two_cell_cases.py: against the oracle and against the host build of the same
templates at the tolerances of tests/test_gpu_parity.py, every gene's flags equal to the host build's, two consecutive
runs bit-identical.  Iteration counts are printed, not asserted."""
import numpy as np
import pytest

from tests import irls_two_cell_cases as tc

pytestmark = pytest.mark.gpu

VALUES = ("beta", "mu", "H", "cooks", "se", "stat", "p")


@pytest.fixture(scope="module")
def ctx():
    from pydeseq2_amd._lib import Context

    return Context(0)


@pytest.mark.parametrize("name", tc.case_names())
def test_device_vs_oracle_and_host_build(ctx, name):
    c = tc.by_name(name)
    got = tc.device_fit(ctx, c)
    again = tc.device_fit(ctx, c)
    assert got.keys() == again.keys()
    for k in got:
        assert np.array_equal(got[k], again[k], equal_nan=got[k].dtype.kind == "f"), f"{name}: {k} differs between two runs"
    ref, host = c.oracle, c.host
    print(f"[irls two-cell] {name}: device sweeps min / mean / max {got['iters'].min()} / {got['iters'].mean():.2f} / "
          f"{got['iters'].max()}, oracle {ref['iters'].min()} / {ref['iters'].mean():.2f} / {ref['iters'].max()}")
    assert set(np.unique(got["conv"])) <= {0, 1}, "a gene's convergence flag was not written"
    assert (got["conv"].astype(bool) == ref["conv"]).all(), np.nonzero(got["conv"].astype(bool) != ref["conv"])[0]
    assert (got["conv"].astype(bool) == host["conv"]).all()
    if "flags" in got:  # any_gt_all, any_gt_use, any_gt_use_nr, few_above of every gene
        assert set(np.unique(got["flags"])) <= {0, 1}, "a Cook's flag was not written"
        assert np.array_equal(got["flags"].astype(bool), np.stack(host["flags"]))
    names = [k for k in VALUES if k in got]
    tc.compare(got, ref, name + " device vs oracle", names)
    tc.compare(got, host, name + " device vs host build", names)
