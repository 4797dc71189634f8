"""mlr_dense_cases on the CPU: the float32 tensor-op path passes every checker
on every case, one dropped and one doubled product at the largest sum are
rejected, every row's top-two gap clears 100 * dz, and the split arguments
the K4-MFMA binding refuses are refused before anything is launched."""

import pytest
import torch

from harmony_amd import ops
from tests import mlr_dense_cases as mc


@pytest.mark.parametrize("variant", mc.SOFTMAX_VARIANTS)
@pytest.mark.parametrize("idx", range(len(mc.SOFTMAX_SHAPES)))
def test_softmax_cases(idx, variant):
    z, y = mc.softmax_case(idx, variant)
    zero = torch.zeros(z.shape, dtype=torch.float64)
    assert bool((mc.gap_margin(z.double(), zero) > 0).all())
    g, loss, correct = ops.softmax_grad_ce(z, y)
    mc.check_softmax(g, loss, correct, z.double(), zero, y, mc.ATOL_SOFTMAX)
    if variant == "scale30" and z.shape[1] > 1:
        assert float(torch.exp(z[0, y[0]] - z[0].max())) == 0.0
        assert float(g[0, y[0]]) == -1.0


@pytest.mark.parametrize("shape", mc.FWD_SHAPES)
def test_fwd_cases(shape):
    X, W, y = mc.fwd_case(*shape)
    z, dz = mc.logits_ref(X, W)
    assert bool((mc.gap_margin(z, dz) > 0).all())       # no row left out
    g, loss, correct = ops.softmax_grad_ce(X @ W.t(), y)
    mc.check_softmax(g, loss, correct, z, dz, y, mc.ATOL_FUSED, shape)
    # a dropped last feature (a lost tail) is far outside the bound
    zt = X[:, :-1].double() @ W[:, :-1].double().t()
    if shape[1] > 1 and shape[2] > 1:
        with pytest.raises(AssertionError):
            mc.check_softmax(g, loss, correct, zt, dz, y, mc.ATOL_FUSED)


@pytest.mark.parametrize("idx", range(len(mc.GRAD_SHAPES)))
def test_grad_cases(idx):
    P, X, ref, bound = mc.grad_case(idx)
    mc.check_sum(P.t() @ X, ref, bound, idx)


def test_checker_rejects_a_dropped_and_a_doubled_product():
    # the longest gradient sum: 600 rows
    idx = max(range(len(mc.GRAD_SHAPES)), key=lambda i: mc.GRAD_SHAPES[i][0])
    P, X, ref, bound = mc.grad_case(idx)
    got = P.t() @ X
    terms = P[:, 0].double() * X[:, 500].double()
    b = int((terms.abs() - terms.abs().median()).abs().argmin())
    for change in (-terms[b], terms[b]):
        bad = ref.clone()
        bad[0, 500] += change
        with pytest.raises(AssertionError):
            mc.check_sum(got, bad, bound)
    # the longest logit sum: 2049 features; judged on the logits themselves
    X, W, y = mc.fwd_case(*mc.FWD_SHAPES[-1])
    z, dz = mc.logits_ref(X, W)
    z32 = X @ W.t()
    mc.check_sum(z32, z, dz)
    terms = X[3].double() * W[1].double()
    f = int((terms.abs() - terms.abs().mean()).abs().argmin())
    for change in (-terms[f], terms[f]):
        bad = z.clone()
        bad[3, 1] += change
        with pytest.raises(AssertionError):
            mc.check_sum(z32, bad, dz)


@pytest.mark.parametrize("B,F,C", sorted({c[:3] for c in mc.STEP_CASES}
                                         | {(256, 192, 10), (192, 192, 3)}))
def test_step_cases(B, F, C):
    case = mc.step_case(B, F, C)
    assert ops.mlr_step_ok(case["X"], C)
    assert bool((mc.gap_margin(case["z"], case["dz"]) > 0).all())
    out = ops.mlr_step_mfma(case["X"], case["W"], case["y"])   # CPU oracle
    mc.check_step(out, case, (B, F, C))
    if C == 1:            # softmax - onehot is 0: the gradient is all zeros
        assert float(case["grad"].abs().max()) < 1e-12
        return
    # one dropped 64-row tile of the gradient is rejected
    Xd = case["X"].clone()
    Xd[-64:] = 0
    p = ops.mlr_forward(case["X"], case["W"], case["y"])[0]
    with pytest.raises(AssertionError):
        mc.check_step((p.t() @ Xd, out[1], out[2]), case)


@pytest.mark.skipif(not ops.hip_available(), reason="HIP extension not built")
def test_binding_refuses_splits_that_do_not_divide_a_block():
    z = torch.zeros
    hip = ops._load_hip()
    X, Wt, y = z(192, 192), z(192, 16), z(192, dtype=torch.int64)
    for rb, sf, sb in ((128, 3, 2),      # the last 64-row block in two
                       (0, 2, 1),        # 192 features in two halves of 96
                       (96, 1, 1)):      # row_block no multiple of 64
        with pytest.raises(RuntimeError, match="64"):
            hip.mlr_step_mfma(X, Wt, y, rb, 10, sf, sb)
    with pytest.raises(RuntimeError, match="on device"):
        hip.mlr_step_mfma(X, Wt, y, 128, 10, 3, 1)
