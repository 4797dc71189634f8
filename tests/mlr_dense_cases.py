"""Inputs, float64 references and checkers for the dense float32 MLR kernels:
K4 (ops/csrc/mlr.hip: mlr_softmax_grad behind ops.softmax_grad_ce, mlr_fwd,
mlr_grad) and K4-MFMA (mlr_mfma.hip behind ops.mlr_step_mfma and
ops.mlr_step_mfma_pipelined).

Bounds, all evaluated in float64 per output element, U = 2^-24:
* a float32 sum of n products, in any order, fma or not, atomics included,
  is within (n + 1) * U * sum |term_i| of the exact sum (Higham, Accuracy
  and Stability of Numerical Algorithms, eq. 3.7). This is dz for a logit
  (n = F) and the bound of a gradient element (n = B);
* g = softmax - onehot keeps the atol of tests/test_ops_gpu.py (2e-5 for
  softmax_grad_ce, 2e-4 for mlr_fwd and the K4-MFMA step), on top of 2 * the
  row's largest dz, a softmax being 2-Lipschitz in the sup norm of its
  logits. The fast exp is off by (|z - m| + 4) * 2^-23 relative and
  |z - m| exp(z - m) <= 1 / e, so saturated rows need no more;
* a gradient computed from such a g adds sum_b dg_b |X_bf|;
* a row's loss m + log(s) - z_label: 2 dz for the logits, (C + 8) * 2^-23
  for s (C roundings and the exp error above, s >= 1), 2^-21 + 3 * 2^-23 *
  |log s| for the fast log, 2^-23 * (|m| + |log s| + |z_label|) for the two
  adds; the sum of B rows adds (B + 1) * U * sum |loss_i|;
* correct is exact: every case is built so that each row's top two float64
  logits are more than 100 * dz apart (test_mlr_dense_cpu.py asserts it for
  every row).
Features (forward) and rows (gradient) at the ends and at the kernels' tile
edges carry products 32 times the usual size, so a tail or a tile that is
dropped or read twice is far outside these bounds.
"""

import functools

import torch

U = 2.0 ** -24
ATOL_SOFTMAX, ATOL_FUSED = 2e-5, 2e-4

SOFTMAX_SHAPES = [(1, 1), (255, 2), (257, 16), (64, 17), (33, 1024)]
SOFTMAX_VARIANTS = ["scale1", "scale30", "offset1e4"]
FWD_SHAPES = [(1, 1, 1), (5, 3, 16), (4, 1024, 10), (7, 1028, 16),
              (9, 2049, 3)]
GRAD_SHAPES = [(1, 1, 1), (511, 3, 10), (512, 1024, 16), (513, 1025, 10),
               (600, 1027, 1)]
# ops.mlr_step_mfma: (B, F, C, row_block, splitf, splitb); None = default
STEP_CASES = [
    (64, 64, 1, 0, None, None),       # one tile, one class
    (64, 64, 16, 0, 1, 1),            # no padding column
    (64, 192, 10, 0, 3, 1),           # splitf = F / 64
    (192, 64, 10, 0, 1, 3),           # splitb = B / 64
    (192, 512, 16, 64, 8, 1),         # 64-row blocks, splitf at its largest
    (192, 192, 1, 64, 3, 1),
    (320, 192, 10, 128, 1, 1),        # last block of 64 rows
    (320, 192, 10, 128, 3, 1),
    (320, 512, 1, 128, None, None),   # default splits over a short block
    (320, 64, 16, 0, None, None),
    (320, 512, 10, 0, 8, 5),          # both splits at their largest
    (128, 512, 10, 128, 8, 2),        # splitb = row_block / 64
    (64, 512, 10, 128, None, None),   # row_block above B
]
EDGES = (0, 63, 64, 511, 512, 1023, 1024)


def _boost(t, dim, by):
    n = t.shape[dim]
    idx = torch.tensor(sorted({e for e in EDGES if e < n} | {n - 1}))
    t.index_copy_(dim, idx, t.index_select(dim, idx) * by)


def logits_ref(X, W):
    """(z64 [B, C], dz [B, C]) of z = X @ W^T."""
    z = X.double() @ W.double().t()
    a = X.double().abs() @ W.double().abs().t()
    return z, (X.shape[1] + 1) * U * a


def gap_margin(z, dz):
    """Per row: top-two gap of z minus 100 * the row's largest dz; inf for
    one class."""
    if z.shape[1] == 1:
        return torch.full((z.shape[0],), float("inf"), dtype=torch.float64)
    top = z.topk(2, dim=1).values
    return top[:, 0] - top[:, 1] - 100 * dz.max(dim=1).values


def _separate(X, W):
    """Move rows of X along their top class's weights until every row's
    top-two gap clears 150 * dz (gap_margin then holds with room)."""
    if W.shape[0] == 1:
        return X
    for _ in range(50):
        z, dz = logits_ref(X, W)
        top = z.topk(2, dim=1)
        short = 150 * dz.max(dim=1).values + 1e-3 - (top.values[:, 0]
                                                     - top.values[:, 1])
        bad = short > 0
        if not bool(bad.any()):
            return X
        wt = W.double()[top.indices[:, 0]]
        step = (short.clamp_min(0) * 2 + 1e-3) / (wt * wt).sum(dim=1)
        X = (X.double() + (bad * step).unsqueeze(1) * wt).float()
    raise AssertionError("rows could not be separated")


def softmax_ref(z, y):
    """float64 (g [B, C], loss per row [B], correct)."""
    m = z.max(dim=1, keepdim=True).values
    e = torch.exp(z - m)
    s = e.sum(dim=1, keepdim=True)
    g = e / s
    g.scatter_add_(1, y.view(-1, 1), torch.full((z.shape[0], 1), -1.0,
                                                dtype=torch.float64))
    ce = (m + torch.log(s)).squeeze(1) - z.gather(1, y.view(-1, 1)).squeeze(1)
    return g, ce, int((z.argmax(dim=1) == y).sum())


def loss_bound(z, y, dzr):
    m = z.max(dim=1).values
    logs = torch.log(torch.exp(z - m.unsqueeze(1)).sum(dim=1))
    zl = z.gather(1, y.view(-1, 1)).squeeze(1)
    C = z.shape[1]
    row = (2 * dzr + (C + 8) * 2 * U + 8 * U + 6 * U * logs.abs()
           + 2 * U * (m.abs() + logs.abs() + zl.abs()))
    ce = m + logs - zl
    return float(row.sum() + (z.shape[0] + 1) * U * ce.abs().sum())


def check_softmax(g, loss, correct, z, dz, y, atol, label=""):
    """g, loss and correct of a softmax kernel against float64 logits z
    known to dz; returns {name: (error, bound)}."""
    g64, ce, cor = softmax_ref(z, y)
    dzr = dz.max(dim=1).values
    gb = atol + 2 * dzr.unsqueeze(1)
    gerr = (g.double() - g64).abs()
    assert g.shape == g64.shape and bool((gerr <= gb).all()), (
        label, "g", float((gerr - gb).max()))
    lb = loss_bound(z, y, dzr)
    lerr = abs(float(loss) - float(ce.sum()))
    assert lerr <= lb, (label, "loss", lerr, lb)
    assert int(correct) == cor, (label, "correct", int(correct), cor)
    return {"g": (float(gerr.max()), float(gb.max())), "loss": (lerr, lb)}


def check_sum(got, ref, bound, label=""):
    err = (got.double() - ref).abs()
    assert got.shape == ref.shape and bool((err <= bound).all()), (
        label, float((err - bound).max()))
    live = bound > 0
    ratio = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.
    return float(err.max()), ratio


# ------------------------------------------------------------------ cases

@functools.lru_cache(maxsize=None)
def softmax_case(idx, variant):
    """(logits f32 [B, C], labels); row 0's label sits on a class whose
    exp underflows to 0 under scale30."""
    B, C = SOFTMAX_SHAPES[idx]
    g = torch.Generator().manual_seed(10 * idx + SOFTMAX_VARIANTS.index(variant))
    z = torch.randn(B, C, generator=g) * (30.0 if variant == "scale30" else 1.0)
    y = torch.randint(0, C, (B,), generator=g)
    if variant == "offset1e4":
        z = z + 1e4
    if C > 1:
        top = z.argmax(dim=1, keepdim=True)
        # the row's largest logit leads by at least 0.01 (ten float32 steps
        # at 1e4), so correct cannot hinge on a tie
        z.scatter_(1, top, z.gather(1, top) + 0.01)
        if variant == "scale30":
            y[0] = (int(top[0]) + 1) % C
            z[0, y[0]] = z[0].max() - 200.0
    return z, y


@functools.lru_cache(maxsize=None)
def fwd_case(B, F, C, seed=0, wscale=0.1):
    """(X [B, F], W [C, F], labels) with separated rows."""
    g = torch.Generator().manual_seed(seed + B + 7 * F + 13 * C)
    X = torch.randn(B, F, generator=g)
    W = torch.randn(C, F, generator=g) * wscale
    y = torch.randint(0, C, (B,), generator=g)
    _boost(X, 1, 8.0)
    _boost(W, 1, 4.0)
    return _separate(X, W), W, y


@functools.lru_cache(maxsize=None)
def grad_case(idx):
    """(P [B, C], X [B, F], g64 [C, F], bound [C, F])."""
    B, F, C = GRAD_SHAPES[idx]
    g = torch.Generator().manual_seed(idx)
    P = torch.randn(B, C, generator=g)
    X = torch.randn(B, F, generator=g)
    _boost(P, 0, 8.0)
    _boost(X, 0, 4.0)
    return (P, X) + grad_ref(P, X)


def grad_ref(P, X):
    ref = P.double().t() @ X.double()
    return ref, (X.shape[0] + 1) * U * (P.double().abs().t() @ X.double().abs())


@functools.lru_cache(maxsize=None)
def step_case(B, F, C):
    """One MLR step: X, W, y and the float64 (z, dz, grad, grad bound)."""
    X, W, y = fwd_case(B, F, C, seed=1, wscale=0.05)
    _boost(X, 0, 2.0)               # rows at the ends and at tile edges
    X = _separate(X, W)
    z, dz = logits_ref(X, W)
    g64, _ce, _cor = softmax_ref(z, y)
    dg = ATOL_FUSED + 2 * dz.max(dim=1).values
    ref = g64.t() @ X.double()
    bound = ((B + 1) * U * (g64.abs().t() @ X.double().abs())
             + (dg.unsqueeze(1) * X.double().abs()).sum(dim=0, keepdim=True))
    return dict(X=X, W=W, y=y, z=z, dz=dz, grad=ref, bound=bound)


def check_step(out, case, label="", slack=1.0):
    """(grad [C, F], loss, correct) of one step; returns the error figures."""
    grad, loss, correct = out
    err, ratio = check_sum(grad.cpu(), case["grad"], slack * case["bound"],
                           (label, "grad"))
    z, dz, y = case["z"], case["dz"], case["y"]
    _g, ce, cor = softmax_ref(z, y)
    lb = loss_bound(z, y, dz.max(dim=1).values)
    lerr = abs(float(loss) - float(ce.sum()))
    assert lerr <= lb, (label, "loss", lerr, lb)
    assert int(correct) == cor, (label, "correct", int(correct), cor)
    return {"grad": (err, ratio), "loss": (lerr, lb)}
