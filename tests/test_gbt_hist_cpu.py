"""gbt_hist_cases on the CPU: the float32 tensor-op path of ops.gbt_hist
passes the checker on every case, the checker rejects one dropped and one
doubled residual at the largest cell, and the cases are what they claim."""

import pytest
import torch

from harmony_amd import ops
from tests import gbt_hist_cases as gc


@pytest.mark.parametrize("idx,variant", gc.params())
def test_tensor_op_path_passes(idx, variant):
    case = gc.make_case(idx, variant)
    cnt, s = ops.gbt_hist(case["bins"], case["resid"], case["node"],
                          case["n_nodes"], case["nb"])
    gc.check(cnt, s, case, label=(idx, variant))


def test_cases_are_what_they_claim():
    # three shapes have one node and so no empty-node variant
    assert len(gc.params()) == 4 * len(gc.SHAPES) - 3
    for idx, (B, F, nb, n_nodes) in enumerate(gc.SHAPES):
        assert n_nodes * nb <= ops.GBT_HIST_MAX_CELLS
        one = gc.make_case(idx, "one_cell")
        assert int((one["cnt"] > 0).sum()) == F
        assert float(one["cnt"].max()) == B <= 1000
        if n_nodes > 1:
            assert float(gc.make_case(idx, "empty_node")["cnt"][1].sum()) == 0
        r = gc.make_case(idx, "wide")["resid"].abs()
        if B >= 255:
            assert float(r.max() / r.min()) > 1e6
            assert bool((gc.make_case(idx, "wide")["resid"] < 0).any())
    assert max(s[3] * s[2] for s in gc.SHAPES) == ops.GBT_HIST_MAX_CELLS
    B, F, nb, n_nodes = gc.SHAPES[3]
    fc = min(F, ops.GBT_HIST_MAX_CELLS // (n_nodes * nb))
    assert fc == 4 and F % fc == 3


def test_checker_rejects_a_dropped_and_a_doubled_term():
    # the fullest cell of all cases: 1000 residuals
    idx = max(range(len(gc.SHAPES)), key=lambda i: gc.SHAPES[i][0])
    case = gc.make_case(idx, "one_cell")
    B, F, nb, n_nodes = gc.SHAPES[idx]
    s32 = ops.gbt_hist(case["bins"], case["resid"], case["node"], n_nodes,
                       nb)
    gc.check(*s32, case)
    r = case["resid"].double()
    # the residual nearest the average size
    term = r[(r.abs() - r.abs().mean()).abs().argmin()]
    for change in (-term, term):
        ref = case["sum"].clone()
        ref[n_nodes - 1, 2, nb - 1] += change
        with pytest.raises(AssertionError):
            gc.check(*s32, case, ref_sum=ref)
    # and one count off
    cnt = s32[0].clone()
    cnt[n_nodes - 1, 0, nb - 1] += 1
    with pytest.raises(AssertionError):
        gc.check(cnt, s32[1], case)
