"""K11 (ops/csrc/lasso.hip) on the GPU: one sweep through ops.lasso_cd on
every case of lasso_dense_cases.k11_cases against the float64 sweep. Rule and
tolerance: the docstring of lasso_dense_cases."""

import pytest
import torch

from tests import lasso_dense_cases as lc

pytestmark = pytest.mark.gpu

_CASES = {c[0]: c for c in lc.k11_cases()}


def _bits(t):
    return t.view(torch.int32)


def _run(label):
    from harmony_amd import ops

    _label, case, lam_n, exact = _CASES[label]
    X, w0, r0, col_sq = (case[k].cuda() for k in ("X", "w", "r", "col_sq"))
    kept = [t.clone() for t in (X, r0, w0, col_sq)]
    Xt = X.t().contiguous()
    w1, r1 = w0.clone(), r0.clone()
    ops._load_hip().lasso_cd(Xt, r1, w1, col_sq, lam_n)
    w2, r2 = ops.lasso_cd(X, r0, w0, col_sq, lam_n)
    for a, b in zip((X, r0, w0, col_sq), kept):   # inputs are not mutated
        assert torch.equal(a, b), label
    assert torch.equal(_bits(w1), _bits(w2)), label   # the same bits again
    assert torch.equal(_bits(r1), _bits(r2)), label
    lc.check(case, lam_n, w1.cpu(), r1.cpu(), label, exact)
    return case, w1.cpu(), r1.cpu()


@pytest.mark.parametrize("label", [c for c in _CASES if c.startswith("B ")])
def test_kernel_vs_fp64(label):
    case, w, _r = _run(label)
    if label.endswith("0.05") and case["X"].shape[0] > 1:
        assert float(w[2]) == 0.0 and float(case["w"][2]) != 0.0
        assert float(w[4]) == 0.0


@pytest.mark.parametrize("lam", lc.LAMS)
def test_zero_column(lam):
    case, w, r = _run(f"zero column lam {lam:g}")
    assert float(w[3]) == 0.0


@pytest.mark.parametrize("lam", lc.LAMS)
def test_one_feature(lam):
    _run(f"F 1 lam {lam:g}")


def test_lam_above_every_c():
    case, w, r = _run("lam above every c")
    assert float(w.abs().max()) == 0.0
    r0 = case["r"].double() + case["X"].double() @ case["w"].double()
    assert float((r.double() - r0).abs().max()) <= lc.R_TOL
