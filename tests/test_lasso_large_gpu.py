"""K11L (ops/csrc/lasso_large.hip) on the GPU: one sweep through the lasso_cd
binding at the row counts where the kernel changes path, against a float64
sweep of the same inputs.

Tolerance. The float32 tensor-op loop of ops.lasso_cd, run on the CPU on
exactly these cases (scripts/lasso_large_ab.py --loop-error), is off the
float64 sweep by at most W_LOOP_ERR in a weight and R_LOOP_ERR in a residual
(largest over all cases below). The kernel sums a different tree over up to
65536 terms and the sweep compounds over six coordinates, so it is allowed
four times that. (K11L measured on an MI355X: 1.77e-7 and 8.30e-7 at most,
profiles/lasso_large_ab.md.)
"""

import pytest
import torch

# the cases (features 2 and 4 sit clear of 0 and of lam_n) and the float64
# sweep are shared with K11's tests
from tests.lasso_dense_cases import F, make_case, sweep64  # noqa: F401

pytestmark = pytest.mark.gpu

ROWS = [16368,    # first row count K11 refuses
        16384,    # the habitual batch size; last all-in-16-registers count
        32768,    # all-register boundary
        32769,    # first LDS row
        40001,    # ragged in the registers' last chunk and in LDS
        65535, 65536]
LAMS = [0.0, 0.05]            # lam_n = lam * B
W_LOOP_ERR, R_LOOP_ERR = 2.32e-7, 1.51e-6   # measured, see the docstring
W_TOL, R_TOL = 4 * W_LOOP_ERR, 4 * R_LOOP_ERR


def check(case, lam_n, w, r, label):
    w64, r64, margin = sweep64(case, lam_n)
    # float32 rounding moves c by about 1e-7 * B; no coordinate sits within
    # 1e-2 * B of the threshold, so the support cannot hinge on it
    assert margin > 1e-2 * case["X"].shape[0], (label, margin)
    w_err = float((w.double() - w64).abs().max())
    r_err = float((r.double() - r64).abs().max())
    print(f"{label}: w error {w_err:.3g} (loop {W_LOOP_ERR:g}), "
          f"r error {r_err:.3g} (loop {R_LOOP_ERR:g})")
    assert torch.equal(w != 0, w64 != 0), label
    assert w_err <= W_TOL and r_err <= R_TOL, (label, w_err, r_err)
    return w_err, r_err


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("B", ROWS)
def test_kernel_vs_fp64(B, lam):
    from harmony_amd import ops

    case, lam_n = make_case(B), lam * B
    X, w0, r0, col_sq = (case[k].cuda() for k in ("X", "w", "r", "col_sq"))
    Xt = X.t().contiguous()
    runs = []
    for _ in range(2):
        w, r = w0.clone(), r0.clone()
        ops._load_hip().lasso_cd(Xt, r, w, col_sq, lam_n)
        runs.append((w, r))
    kept = [t.clone() for t in (X, r0, w0, col_sq)]
    runs.append(ops.lasso_cd(X, r0, w0, col_sq, lam_n))
    for a, b in zip((X, r0, w0, col_sq), kept):   # inputs are not mutated
        assert torch.equal(a, b)
    for w, r in runs[1:]:                         # the same bits every time
        assert torch.equal(_bits(w), _bits(runs[0][0]))
        assert torch.equal(_bits(r), _bits(runs[0][1]))
    if lam:
        assert float(runs[0][0][2]) == 0.0 and float(w0[2]) != 0.0
    check(case, lam_n, runs[0][0].cpu(), runs[0][1].cpu(),
          f"B {B} lam_n {lam_n:g}")


def test_over_the_cap_takes_the_tensor_op_loop():
    from harmony_amd import ops

    B = ops.LASSO_CD_MAX_ROWS + 1
    case = make_case(B, 2)
    w, r = ops.lasso_cd(*(case[k].cuda() for k in ("X", "r", "w", "col_sq")),
                        0.05 * B)
    assert w.is_cuda and r.is_cuda
    check(case, 0.05 * B, w.cpu(), r.cpu(), f"B {B} fallback")
