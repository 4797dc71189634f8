"""lasso_dense_cases on the CPU: every margin of every K11 case, the float32
tensor-op loop's error against the float64 sweep (the measurement behind
W_LOOP_ERR and R_LOOP_ERR, printed per case), and the properties the cases
are built for."""

import torch

from harmony_amd import ops
from tests import lasso_dense_cases as lc


def test_margins_and_loop_error_on_every_case():
    w_max = r_max = 0.0
    for label, case, lam_n, exact in lc.k11_cases():
        B = case["X"].shape[0]
        assert B <= 16367 < ops.LASSO_CD_MAX_ROWS
        w, r = lc.loop32(case, lam_n)
        w_err, r_err, margin, same = lc.errors(case, lam_n, w, r, exact)
        print(f"{label}: loop w error {w_err:.3g}, r error {r_err:.3g}, "
              f"margin / B {margin / B:.3g}")
        assert margin > 1e-2 * B, (label, margin)
        assert same, label
        # the loop passes the kernel's check on whatever machine this is
        lc.check(case, lam_n, w, r, label, exact)
        w_max, r_max = max(w_max, w_err), max(r_max, r_err)
    print(f"largest: w {w_max:.3g} (W_LOOP_ERR {lc.W_LOOP_ERR:g}), "
          f"r {r_max:.3g} (R_LOOP_ERR {lc.R_LOOP_ERR:g})")
    # the constants are a measurement of this loop, not a wish: it is never
    # far below them
    assert w_max >= lc.W_LOOP_ERR / 2 and r_max >= lc.R_LOOP_ERR / 2
    assert (lc.W_TOL, lc.R_TOL) == (4 * lc.W_LOOP_ERR, 4 * lc.R_LOOP_ERR)


def test_cases_are_what_they_claim():
    labels = [c[0] for c in lc.k11_cases()]
    assert len(labels) == len(set(labels)) == 2 * len(lc.ROWS) + 5
    for B in lc.ROWS[1:]:
        case = lc.small_case(B)
        w, _r, _m = lc.sweep64(case, 0.05 * B)
        # feature 2 thresholds to 0, feature 4 stays there (d == 0)
        assert float(case["w"][2]) != 0 and float(case["w"][4]) == 0
        assert (w != 0).tolist() == [True, True, False, True, False, True]
        assert bool((lc.sweep64(case, 0.0)[0] != 0).all())
    one = lc.small_case(1)
    assert 1 <= int((lc.sweep64(one, 0.05)[0] != 0).sum()) < lc.F
    zc = lc.zero_column_case()
    assert float(zc["X"][:, 3].abs().max()) == 0 and float(zc["w"][3]) == 0
    assert zc["col_sq"][3] == torch.tensor(1e-9)
    for lam_n in (0.0, 0.05 * 1024):
        w, r, _m = lc.sweep64(zc, lam_n, (3,))
        assert float(w[3]) == 0
    case = lc.small_case(1024)
    w, r, margin = lc.sweep64(case, lc.HIGH_LAM * 1024)
    assert float(w.abs().max()) == 0 and margin > 1024
    r0 = case["r"].double() + case["X"].double() @ case["w"].double()
    assert float((r - r0).abs().max()) < 1e-12


def test_shared_helpers_keep_the_large_cases():
    # what test_lasso_large_gpu.py imports gives the case it always built
    B = 16368
    g = torch.Generator().manual_seed(B)
    X = torch.randn(B, 6, generator=g)
    y = X @ torch.tensor(lc.W_TRUE) + 0.1 * torch.randn(B, generator=g)
    case = lc.make_case(B)
    assert torch.equal(case["X"], X)
    assert torch.equal(case["r"], y - X @ torch.tensor(lc.W_IN))
    assert torch.equal(case["col_sq"], (X * X).sum(dim=0))
    assert lc.W_TRUE == [1.5, -2.0, 0.02, 0.8, 0.02, -1.2]
    assert lc.W_IN == [0.5, -1.0, 0.3, 0.75, 0.0, -1.15]
