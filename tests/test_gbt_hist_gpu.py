"""K10 (ops/csrc/gbt.hip) on the GPU against the float64 histogram of
gbt_hist_cases: every shape and variant, and bins given as int64 and uint8."""

import pytest
import torch

from tests import gbt_hist_cases as gc

pytestmark = pytest.mark.gpu


def _run(case, bins):
    from harmony_amd import ops

    kept = [t.clone() for t in (bins, case["resid"], case["node"])]
    args = (bins.cuda(), case["resid"].cuda(), case["node"].cuda())
    cnt, s = ops.gbt_hist(*args, case["n_nodes"], case["nb"])
    assert cnt.is_cuda and s.is_cuda
    for a, b in zip(args, kept):                  # inputs are not mutated
        assert torch.equal(a.cpu(), b)
    return cnt.cpu(), s.cpu()


@pytest.mark.parametrize("idx,variant", gc.params())
def test_kernel_vs_fp64(idx, variant):
    case = gc.make_case(idx, variant)
    cnt, s = _run(case, case["bins"])
    err, ratio = gc.check(cnt, s, case, label=(idx, variant))
    B, F, _nb, _n = gc.SHAPES[idx]
    assert float(cnt.sum()) == B * F
    print(f"gbt_hist {gc.SHAPES[idx]} {variant}: sum error {err:.3g}, "
          f"error / bound {ratio:.3f}, counts exact")


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8, torch.int32])
def test_bins_dtypes_through_the_wrapper(dtype):
    for idx in (1, 5):                            # nb 7 and 16 fit a uint8
        case = gc.make_case(idx, "random")
        cnt, s = _run(case, case["bins"].to(dtype))
        gc.check(cnt, s, case, label=(idx, dtype))
