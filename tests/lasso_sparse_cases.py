"""Shared inputs, fp64 evaluation and error bounds for the sparse-Lasso tests
(test_lasso_sparse_cpu.py, test_lasso_sparse_gpu.py).

Coordinate descent is sequential, so a whole sweep is never compared with
another whole sweep: small differences compound. Each coordinate is checked
against fp64 GIVEN the outputs that preceded it (teacher forcing), so no
error compounds. With u = 2^-24 and X the fp64 densification restricted to
the present columns (compacted: no B x F array is built):

  residual    R = y - X w_out;  |r_out[i] - R[i]| <= E[i]
              E[i] = 2 (2 k_i + 1) u M_i, k_i the row's entry count,
              M_i = |y_i| + sum_f |x_if| (|w_in_f| + |w_in_f - w_out_f|)
              (a row takes at most k_i updates while r is built and k_i in
              the sweep, each one rounding at the magnitude M_i bounds)
  coordinate  for present feature k (column f, n_f entries), with
              w^(k) = (w_out before k, w_in from k on), r^(k) = y - X w^(k),
              c = x_f . r^(k) + w_in_f cs,  wn = soft(c, lam_n) / cs:
              |w_out_f - wn| <= dc / cs + 4 u |wn|
              dc = 2 (n_f + 2) u (sum_i |x_if r^(k)_i| + |w_in_f cs|)
                   + sum_i |x_if| E[i]
              cs is the fp32 col_sq value handed to the op
  untouched   features absent from the batch, zero-length segments and
              columns with col_sq <= 1e-9 come back bit-identical to w_in

lam_n reaches the op as fp32, so the fp64 evaluation uses that fp32 value.
Nothing here is tuned to an implementation.
"""

from pathlib import Path

import torch

U = 2.0 ** -24
ZERO_THRESHOLD = 1e-9
GOLDEN = Path(__file__).parent / "golden" / "lasso" / "sample_lasso_64"

# (B, F, column lengths, present ids or None for a random ascending subset).
# Rows within a column are a sorted random subset, so consecutive columns
# overlap in rows but map entries to different lanes: the shape that shows a
# missing barrier between one column's scatter and the next one's gather.
SHAPES = [
    (1, 4, [1], None),
    (5, 4, [5, 1, 0, 3], None),
    (67, 130, [67, 0, 1, 64, 65, 33, 2, 7, 12, 40], None),
    (200, 2 ** 20 + 3, [200, 1, 63, 64, 65, 128, 129, 0, 17], None),
    (1030, 40, [1030, 1025, 1024, 1023, 5, 0, 700] + [50] * 20, None),
    # first present id 0, last F-1; column 1 carries no mass (col_sq clamps
    # to 1e-9) and a non-zero weight
    (40, 1000, [9, 4, 0, 30, 40], [0, 17, 500, 998, 999]),
]
TINY_COLUMN = {5: 1}          # shape index -> column whose values are 1e-7


def lams(B):
    return (0.0, 0.3, 0.05 * B)


def col_sq_of(feat_ptr, feat_val):
    """What the app hands to the op: fp32 per-column sum of squares, clamped."""
    nf = feat_ptr.shape[0] - 1
    seg = torch.repeat_interleave(torch.arange(nf),
                                  feat_ptr[1:] - feat_ptr[:-1])
    cs = torch.zeros(nf, dtype=torch.float32)
    cs.index_add_(0, seg, feat_val * feat_val)
    return cs.clamp_min(ZERO_THRESHOLD)


def make_case(idx):
    B, F, lens, ids = SHAPES[idx]
    g = torch.Generator().manual_seed(100 + idx)
    nf = len(lens)
    if ids is None:
        ids = torch.randperm(F, generator=g)[:nf].sort().values
    else:
        ids = torch.tensor(ids)
    feat_ptr = torch.zeros(nf + 1, dtype=torch.int64)
    feat_ptr[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int64), 0)
    rows = [torch.randperm(B, generator=g)[:n].sort().values for n in lens]
    feat_row = torch.cat(rows).to(torch.int32)
    feat_val = torch.randn(int(feat_ptr[-1]), generator=g)
    if idx in TINY_COLUMN:
        k = TINY_COLUMN[idx]
        feat_val[int(feat_ptr[k]):int(feat_ptr[k + 1])] *= 1e-7
    y = torch.randn(B, generator=g)
    # non-zero on every second present feature and on one absent feature
    w_in = torch.zeros(F)
    w_in[ids[1::2] if nf > 1 else ids] = torch.randn(
        ids[1::2].shape[0] if nf > 1 else nf, generator=g)
    present = torch.zeros(F, dtype=torch.bool)
    present[ids] = True
    absent = (~present).nonzero().flatten()
    if absent.numel():
        w_in[absent[absent.numel() // 2]] = 0.625
    return dict(B=B, F=F, feat_ids=ids.to(torch.int32), feat_ptr=feat_ptr,
                feat_row=feat_row, feat_val=feat_val, y=y, w_in=w_in,
                col_sq=col_sq_of(feat_ptr, feat_val))


def case_from_batch(batch, y, seed):
    """A case over a SparseBatch (the golden sample)."""
    g = torch.Generator().manual_seed(seed)
    F = batch.shape[1]
    w_in = torch.zeros(F)
    ids = batch.feat_ids.long()
    w_in[ids[1::2]] = torch.randn(ids[1::2].shape[0], generator=g)
    return dict(B=batch.shape[0], F=F, feat_ids=batch.feat_ids,
                feat_ptr=batch.feat_ptr, feat_row=batch.feat_row,
                feat_val=batch.feat_val, y=y, w_in=w_in,
                col_sq=col_sq_of(batch.feat_ptr, batch.feat_val))


def op_args(case, device="cpu"):
    return tuple(case[k].to(device) for k in
                 ("feat_ids", "feat_ptr", "feat_row", "feat_val", "y",
                  "w_in", "col_sq"))


def check(case, lam_n, w_out, r_out, label=""):
    """Residual, coordinate and untouched-weight checks of one sweep's
    outputs (CPU tensors). Returns (worst coordinate error / bound, worst
    residual error / bound) after asserting both are <= 1."""
    B, F = case["B"], case["F"]
    ids = case["feat_ids"].long()
    ptr = case["feat_ptr"]
    nf = ids.shape[0]
    lens = ptr[1:] - ptr[:-1]
    seg = torch.repeat_interleave(torch.arange(nf), lens)
    X = torch.zeros((B, nf), dtype=torch.float64)
    X[case["feat_row"].long(), seg] = case["feat_val"].double()
    y = case["y"].double()
    w_in, cs = case["w_in"], case["col_sq"]
    assert w_out.dtype == torch.float32 and w_out.shape == (F,)
    assert r_out.dtype == torch.float32 and r_out.shape == (B,)
    lam = float(torch.tensor(lam_n, dtype=torch.float32))

    # untouched weights: bit-identical
    swept = torch.zeros(F, dtype=torch.bool)
    live = (lens > 0) & (cs > ZERO_THRESHOLD)
    swept[ids[live]] = True
    assert torch.equal(w_out.view(torch.int32)[~swept],
                       w_in.view(torch.int32)[~swept]), \
        f"{label}: a weight outside the swept columns changed"

    wi, wo = w_in[ids].double(), w_out[ids].double()
    # residual
    R = y - X @ wo
    k_i = torch.bincount(case["feat_row"].long(), minlength=B).double()
    M = y.abs() + X.abs() @ (wi.abs() + (wi - wo).abs())
    E = 2.0 * (2.0 * k_i + 1.0) * U * M
    r_err = (r_out.double() - R).abs()
    r_ratio = float((r_err / E.clamp_min(1e-300)).max())
    assert bool((r_err <= E).all()), \
        f"{label}: residual error/bound {r_ratio:.3f}"

    # coordinates, teacher-forced
    r = y - X @ wi
    c_ratio = 0.0
    for k in range(nf):
        if not bool(live[k]):
            continue
        x = X[:, k]
        csk = float(cs[k])
        c = float(x @ r) + float(wi[k]) * csk
        wn = (1.0 if c > 0 else -1.0 if c < 0 else 0.0) \
            * max(abs(c) - lam, 0.0) / csk
        dc = 2.0 * (float(lens[k]) + 2.0) * U * (
            float((x * r).abs().sum()) + abs(float(wi[k]) * csk)) \
            + float(x.abs() @ E)
        bound = dc / csk + 4.0 * U * abs(wn)
        err = abs(float(wo[k]) - wn)
        c_ratio = max(c_ratio, err / max(bound, 1e-300))
        assert err <= bound, \
            f"{label}: coordinate {k} (feature {int(ids[k])}) off by " \
            f"{err:.3e}, bound {bound:.3e}"
        r = r + x * (wi[k] - wo[k])
    return c_ratio, r_ratio
