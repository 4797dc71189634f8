"""Inputs, float64 sweep and checker for the dense Lasso sweep kernels behind
ops.lasso_cd: K11 (ops/csrc/lasso.hip, up to 16367 rows, tested in
test_lasso_dense_gpu.py) and K11L (lasso_large.hip, test_lasso_large_gpu.py).

make_case and sweep64 serve both. The K11 cases and their tolerance follow
the rule of test_lasso_large_gpu.py: the float32 tensor-op loop of
ops.lasso_cd, run on the CPU on exactly the K11 cases below, is off the
float64 sweep by at most W_LOOP_ERR in a weight and R_LOOP_ERR in a residual
(largest over all of them, measured by test_lasso_dense_cpu.py, which also
holds the constants to that measurement); the kernel sums another tree, so
it is allowed four times that. The support must be equal, which no rounding
can decide: every | |c| - lam_n | of the float64 sweep exceeds 1e-2 * B,
against a float32 rounding of c near 1e-7 * B.
"""

import functools

import torch

F = 6
# Features 2 and 4 have c near 0.02 B: clear of 0, and clear of lam_n, under
# which feature 2 thresholds from 0.3 to exactly 0 and feature 4 stays at 0.
# The later weights start near the truth so that the residual's noise in
# those two c stays a tenth of that.
W_TRUE = [1.5, -2.0, 0.02, 0.8, 0.02, -1.2]
W_IN = [0.5, -1.0, 0.3, 0.75, 0.0, -1.15]

LAMS = [0.0, 0.05]            # lam_n = lam * B
# K11 row counts: one row, around a wave (64) and a workgroup (1024), and
# the last count that fits 64 KiB of LDS
ROWS = [1, 63, 64, 65, 1023, 1024, 1025, 16367]
# Per K11 row count, the generator seed (and for one row the start) at which
# every margin of both lam holds with room to spare; found by trying seeds
# 0, 1, 2, ... and asserted by test_lasso_dense_cpu.py. The truth and start
# above serve every count from 63 rows: under lam, feature 2 thresholds to
# exactly 0 and feature 4 stays at 0 (the kernel's d == 0 skip). With one
# row, coordinate 0 alone fits the row, r becomes 0 and c = w x^2 for every
# later feature, so feature 4 needs a start other than 0 to clear lam_n = 0.
W_IN_ONE_ROW = (0.5, -1.0, 0.3, 0.75, 0.4, -1.15)
SMALL = {1: (18, W_IN_ONE_ROW), 63: (12, None), 64: (3, None), 65: (8, None),
         1023: (0, None), 1024: (0, None), 1025: (1, None),
         16367: (0, None)}
# Measured over k11_cases() with torch's dot product on four threads (the
# weight error is that of the one-row case, the residual error that of 1023
# rows). On one thread the dot product sums in sequence and the loop is off
# by 6.94e-7 and 3.89e-6, which the bound below still admits; the smaller
# pair is kept because it asks more of the kernel.
W_LOOP_ERR, R_LOOP_ERR = 3.13e-7, 1.24e-6
W_TOL, R_TOL = 4 * W_LOOP_ERR, 4 * R_LOOP_ERR


@functools.lru_cache(maxsize=None)
def make_case(B, nf=F, seed=None, w_in=None):
    g = torch.Generator().manual_seed(B if seed is None else seed)
    X = torch.randn(B, nf, generator=g)
    y = X @ torch.tensor(W_TRUE[:nf]) + 0.1 * torch.randn(B, generator=g)
    w = torch.tensor((W_IN if w_in is None else w_in)[:nf])
    return dict(X=X, w=w, r=y - X @ w, col_sq=(X * X).sum(dim=0))


def small_case(B):
    """The K11 case of B rows."""
    return make_case(B, F, *SMALL[B])


@functools.lru_cache(maxsize=None)
def zero_column_case(B=1024, col=3):
    """Column `col` all zero with a zero weight, col_sq clamped as the app
    clamps it (mlapps.lasso.ZERO_THRESHOLD)."""
    from harmony_amd.mlapps.lasso import ZERO_THRESHOLD

    base = small_case(B)
    X = base["X"].clone()
    X[:, col] = 0.0
    w = base["w"].clone()
    w[col] = 0.0
    y = base["r"] + base["X"] @ base["w"] - base["X"][:, col] * W_TRUE[col]
    return dict(X=X, w=w, r=y - X @ w,
                col_sq=(X * X).sum(dim=0).clamp_min(ZERO_THRESHOLD))


HIGH_LAM = 10.0     # lam_n = 10 B lies above every |c| (at most about 2 B)


def k11_cases():
    """Every K11 case: (label, case, lam_n, coordinates with c exactly 0)."""
    out = []
    for B in ROWS:
        for lam in LAMS:
            out.append((f"B {B} lam {lam:g}", small_case(B), lam * B, ()))
    for lam in LAMS:
        out.append((f"zero column lam {lam:g}", zero_column_case(),
                    lam * 1024, (3,)))
        out.append((f"F 1 lam {lam:g}", make_case(1025, 1), lam * 1025, ()))
    out.append(("lam above every c", small_case(1024), HIGH_LAM * 1024, ()))
    return out


def sweep64(case, lam_n, exact=()):
    """The float64 sweep: (w, r, smallest ||c| - lam_n| over coordinates).
    Coordinates in `exact` have c == 0 in any arithmetic (a zero column with
    a zero weight) and stay out of the margin."""
    X, col_sq = case["X"].double(), case["col_sq"].double()
    w, r = case["w"].double().clone(), case["r"].double().clone()
    margin = float("inf")
    for f in range(X.shape[1]):
        c = X[:, f] @ r + w[f] * col_sq[f]
        if f not in exact:
            margin = min(margin, abs(float(c.abs()) - lam_n))
        wn = torch.sign(c) * torch.clamp(c.abs() - lam_n, min=0.0) / col_sq[f]
        r += X[:, f] * (w[f] - wn)
        w[f] = wn
    return w, r, margin


def loop32(case, lam_n):
    """The float32 tensor-op loop of ops.lasso_cd on the CPU."""
    from harmony_amd import ops

    return ops.lasso_cd(case["X"], case["r"], case["w"], case["col_sq"],
                        lam_n)


def errors(case, lam_n, w, r, exact=()):
    """(w error, r error, margin, support equal) against the float64 sweep."""
    w64, r64, margin = sweep64(case, lam_n, exact)
    return (float((w.double() - w64).abs().max()),
            float((r.double() - r64).abs().max()), margin,
            bool(torch.equal(w != 0, w64 != 0)))


def check(case, lam_n, w, r, label, exact=()):
    w_err, r_err, margin, same = errors(case, lam_n, w, r, exact)
    assert margin > 1e-2 * case["X"].shape[0], (label, margin)
    print(f"{label}: w error {w_err:.3g} (loop {W_LOOP_ERR:g}, bound "
          f"{W_TOL:.3g}), r error {r_err:.3g} (loop {R_LOOP_ERR:g}, bound "
          f"{R_TOL:.3g})")
    assert same, label
    assert w_err <= W_TOL and r_err <= R_TOL, (label, w_err, r_err)
    return w_err, r_err
