"""SparseBins — one GBT mini-batch as binned sparse entries.

The reference builds every GBT sample with createSparse (GBTETDataParser), so
its trainer works on sparse vectors. Here a block is quantised ONCE at load
time, on the CPU, straight from its CSR form: an absent entry is the value
0.0, and every feature present in the block gets exactly the bin edges
gbt.quantize computes on the densified block, without building it. Memory
follows nnz and the number of present features, never B * F.

Bin edges. torch.quantile (linear interpolation) over the B values of a
column reads the sorted column at floor and ceil of ranks = q * (B - 1) and
lerps. The B values of a sparse column are its entries merged with B - len
implied zeros: with the column segment sorted and `neg` of its entries
negative, virtual position p is entry p for p < neg, 0.0 for the next
B - len positions, and entry p - (B - len) after them.

Two views of the same entries are kept:
  * CSR side: keys int64 [nnz] = row * F + col, sorted, with key_bin int32
    [nnz] — bin_of() finds a (row, feature) by searchsorted;
  * column side over the present features (the input of K10s,
    ops.gbt_hist_sparse): feat_ids int32 [nf] ascending, feat_ptr int64
    [nf+1], feat_row / feat_bin / feat_idx int32 [nnz] (rows ascending
    within a feature; feat_idx is the compact feature index of the entry),
    zero_bin int32 [nf] — the bin of an absent entry: the bin of 0.0 under
    the feature's edges, 0 for a categorical feature. A feature absent from
    the block has all edges 0, so its zero bin is 0 and it is not stored.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from harmony_amd.mlapps.sparse_batch import (SparseBatch, column_index,
                                             group_by_column)

_FIELDS = ("keys", "key_bin", "feat_ids", "feat_ptr", "feat_row", "feat_bin",
           "feat_idx", "zero_bin")
_CMP_CHUNK = 1 << 18    # entries per edge comparison (x (nb - 1) booleans)


def _column_edges(sval: torch.Tensor, ptr: torch.Tensor, B: int,
                  num_bins: int) -> torch.Tensor:
    """Quantile edges float32 [nf, nb-1] of columns given as value-sorted
    segments sval[ptr[k]:ptr[k+1]] plus implied zeros, following
    torch.quantile step by step (float32 ranks, floor / ceil, lerp)."""
    nf = ptr.shape[0] - 1
    q = torch.linspace(0, 1, num_bins + 1)[1:-1]
    ranks = q * (B - 1)
    below = ranks.to(torch.int64)
    weights = ranks - below
    above = ranks.ceil().to(torch.int64)
    length = ptr[1:] - ptr[:-1]
    nzero = (B - length).unsqueeze(1)                       # [nf, 1]
    csum = torch.zeros(sval.shape[0] + 1, dtype=torch.int64)
    csum[1:] = torch.cumsum((sval < 0).long(), 0)
    neg = (csum[ptr[1:]] - csum[ptr[:-1]]).unsqueeze(1)     # [nf, 1]
    base = ptr[:-1].unsqueeze(1)
    last = max(sval.shape[0] - 1, 0)

    def read(p: torch.Tensor) -> torch.Tensor:
        p = p.unsqueeze(0).expand(nf, -1)
        in_neg = p < neg
        in_zero = ~in_neg & (p < neg + nzero)
        e = base + torch.where(in_neg, p, p - nzero)
        v = sval[e.clamp(0, last)]
        return torch.where(in_zero, torch.zeros_like(v), v)

    return torch.lerp(read(below), read(above),
                      weights.unsqueeze(0).expand(nf, -1))


class SparseBins:
    """The binned sparse batch (see the module docstring for the fields).
    Built on the CPU from a SparseBatch or a raw CSR tuple (row_ptr, col,
    val, num_features); feature_types as in gbt.quantize, with the same
    validation of categorical columns."""

    def __init__(self, batch, num_bins: int,
                 feature_types: Optional[torch.Tensor] = None):
        # column-major order twice: rows ascending (kept; a SparseBatch
        # brings it), values ascending (for the quantiles); both group the
        # entries by feature
        if isinstance(batch, SparseBatch):
            batch = batch.to("cpu")
            row_ptr, col, val, F = (batch.row_ptr, batch.col.long(),
                                    batch.val, batch.num_features)
            feat_ids, ptr, crow, cval = (batch.feat_ids.long(),
                                         batch.feat_ptr, batch.feat_row,
                                         batch.feat_val)
        else:
            row_ptr, col, val, F = batch
            row_ptr = row_ptr.to(device="cpu", dtype=torch.int64)
            col = col.to(device="cpu", dtype=torch.int64)
            val = val.to(device="cpu", dtype=torch.float32)
            by_row, feat_ids, ptr, crow = column_index(row_ptr, col)
            cval = val[by_row]
        self.num_features = int(F)
        self.num_bins = int(num_bins)
        B = row_ptr.shape[0] - 1
        self.num_rows = B
        nb = self.num_bins
        nf = feat_ids.shape[0]
        idx = torch.repeat_interleave(torch.arange(nf), ptr[1:] - ptr[:-1])
        ccol, crow = feat_ids[idx], crow.long()
        by_val = torch.argsort(val, stable=True)
        by_val = by_val[torch.argsort(col[by_val], stable=True)]
        edges = _column_edges(val[by_val], ptr, B, nb)       # [nf, nb-1]
        cbin = torch.empty(ccol.shape[0], dtype=torch.int64)
        for lo in range(0, ccol.shape[0], _CMP_CHUNK):
            hi = lo + _CMP_CHUNK
            # searchsorted (left) = number of edges strictly below the value
            cbin[lo:hi] = (edges[idx[lo:hi]]
                           < cval[lo:hi].unsqueeze(1)).sum(dim=1)
        cbin.clamp_(0, nb - 1)
        zero_bin = (edges < 0).sum(dim=1).clamp_(0, nb - 1)
        if feature_types is not None:
            from harmony_amd.mlapps.gbt import MAX_CATEGORIES

            limit = min(nb, MAX_CATEGORIES)
            is_cat = feature_types.to("cpu")[feat_ids] != 0   # [nf]
            ecat = is_cat[idx]
            bad = ecat & ((cval < 0) | (cval != cval.floor())
                          | (cval >= limit) | ~torch.isfinite(cval))
            if bool(bad.any()):
                # rows ascending within ascending features: the first bad
                # entry is the one quantize reports
                e = int(bad.nonzero()[0])
                raise ValueError(
                    f"categorical feature {int(ccol[e])}: value "
                    f"{float(cval[e])!r} is not an integer in "
                    f"0..{limit - 1} (cardinality is limited by num_bins = "
                    f"{nb} and {MAX_CATEGORIES})")
            cbin = torch.where(ecat, cval.long(), cbin)
            zero_bin = torch.where(is_cat, torch.zeros_like(zero_bin),
                                   zero_bin)
        self.feat_ids = feat_ids.to(torch.int32)
        self.feat_ptr = ptr
        self.feat_row = crow.to(torch.int32)
        self.feat_bin = cbin.to(torch.int32)
        self.feat_idx = idx.to(torch.int32)
        self.zero_bin = zero_bin.to(torch.int32)
        # the parsers keep file order inside a row, so sort the keys
        keys = crow * self.num_features + ccol
        order = torch.argsort(keys)
        self.keys = keys[order].contiguous()
        self.key_bin = self.feat_bin[order].contiguous()

    @property
    def shape(self) -> Tuple[int, int]:
        return (self.num_rows, self.num_features)

    @property
    def nnz(self) -> int:
        return self.keys.shape[0]

    @property
    def device(self) -> torch.device:
        return self.keys.device

    def _like(self) -> "SparseBins":
        out = object.__new__(SparseBins)
        out.num_features = self.num_features
        out.num_bins = self.num_bins
        out.num_rows = self.num_rows
        return out

    def to(self, device) -> "SparseBins":
        out = self._like()
        for name in _FIELDS:
            setattr(out, name, getattr(self, name).to(device))
        return out

    def prefix(self, n: int) -> "SparseBins":
        """The first n rows (n == 0: the empty batch a stopped worker
        serves). Bins, present features and zero bins are kept — the dense
        reslice slices the bins without re-quantising — and the column side
        is rebuilt; a feature the prefix has no entry of keeps an empty
        segment."""
        n = max(0, min(int(n), self.num_rows))
        out = self._like()
        out.num_rows = n
        F = self.num_features
        m = int(torch.searchsorted(
            self.keys, torch.tensor([n * F], dtype=torch.int64,
                                    device=self.device)))
        out.keys = self.keys[:m]
        out.key_bin = self.key_bin[:m]
        out.feat_ids = self.feat_ids
        out.zero_bin = self.zero_bin
        # keys ascend row-major
        order, _, out.feat_ptr, out.feat_row = group_by_column(
            out.keys // F, out.keys % F, self.feat_ids)
        out.feat_bin = out.key_bin[order].contiguous()
        out.feat_idx = torch.repeat_interleave(
            torch.arange(self.feat_ids.shape[0], dtype=torch.int32,
                         device=self.device),
            out.feat_ptr[1:] - out.feat_ptr[:-1])
        return out

    def bin_of(self, feat: torch.Tensor) -> torch.Tensor:
        """int64 [B]: the bin of feature feat[i] in row i — the stored bin
        of the entry (i, feat[i]) if the row has one, else the feature's
        zero bin (0 for a feature absent from the block)."""
        B, F = self.shape
        feat = feat.long()
        out = torch.zeros(B, dtype=torch.int64, device=self.device)
        nf = self.feat_ids.shape[0]
        if B == 0 or nf == 0:
            return out
        ids = self.feat_ids.long()
        k = torch.searchsorted(ids, feat).clamp_(max=nf - 1)
        out = torch.where(ids[k] == feat, self.zero_bin[k].long(), out)
        if self.nnz == 0:
            return out
        want = torch.arange(B, device=self.device) * F + feat
        pos = torch.searchsorted(self.keys, want).clamp_(max=self.nnz - 1)
        return torch.where(self.keys[pos] == want, self.key_bin[pos].long(),
                           out)

    def to_dense_bins(self) -> torch.Tensor:
        """int64 [B, F] dense bins (tests only: B*F elements)."""
        B, F = self.shape
        zb = torch.zeros(F, dtype=torch.int64, device=self.device)
        zb[self.feat_ids.long()] = self.zero_bin.long()
        bins = zb.unsqueeze(0).repeat(B, 1)
        bins.view(-1)[self.keys] = self.key_bin.long()
        return bins
