"""SparseBatch — one MLR mini-batch as CSR plus a static column index.

The reference keeps MLR samples as SparseVectors (MLRETDataParser
createSparse) and its per-sample update touches only a sample's non-zeros
(MLRTrainer.java:374-398). A batch here holds the rows as CSR for the
forward, and — built once at load time — the same entries grouped by
column (CSC over the features that occur in the batch) for the gradient:
with the index static, G = P^T @ X is a per-feature gather-reduce with one
writer per element and no atomics, and the summation order is a function
of the data alone.
"""

from __future__ import annotations

from typing import Tuple

import torch


class SparseBatch:
    """row_ptr int64 [B+1], col int32 [nnz], val float32 [nnz] (CSR; each
    (row, col) at most once), and the column index over present features:
    feat_ids int32 [nf] distinct columns ascending, feat_ptr int64 [nf+1],
    feat_row int32 [nnz], feat_val float32 [nnz], rows ascending within a
    feature."""

    def __init__(self, row_ptr: torch.Tensor, col: torch.Tensor,
                 val: torch.Tensor, num_features: int):
        self.row_ptr = row_ptr.to(torch.int64).contiguous()
        self.col = col.to(torch.int32).contiguous()
        self.val = val.to(torch.float32).contiguous()
        self.num_features = int(num_features)
        dev = self.row_ptr.device
        B = self.row_ptr.shape[0] - 1
        row_of = torch.repeat_interleave(
            torch.arange(B, dtype=torch.int32, device=dev),
            self.row_ptr[1:] - self.row_ptr[:-1])
        # CSR is row-major, so a stable sort by column leaves the rows of
        # each feature ascending
        order = torch.argsort(self.col, stable=True)
        self.feat_row = row_of[order].contiguous()
        self.feat_val = self.val[order].contiguous()
        self.feat_ids, counts = torch.unique_consecutive(
            self.col[order], return_counts=True)
        self.feat_ptr = torch.zeros(self.feat_ids.shape[0] + 1,
                                    dtype=torch.int64, device=dev)
        self.feat_ptr[1:] = torch.cumsum(counts, 0)

    @property
    def shape(self) -> Tuple[int, int]:
        return (self.row_ptr.shape[0] - 1, self.num_features)

    @property
    def nnz(self) -> int:
        return self.col.shape[0]

    @property
    def device(self) -> torch.device:
        return self.row_ptr.device

    def to(self, device) -> "SparseBatch":
        out = object.__new__(SparseBatch)
        out.num_features = self.num_features
        for name in ("row_ptr", "col", "val", "feat_ids", "feat_ptr",
                     "feat_row", "feat_val"):
            setattr(out, name, getattr(self, name).to(device))
        return out

    def to_dense(self) -> torch.Tensor:
        """[B, F] dense copy (tests only: B*F elements)."""
        B, F = self.shape
        X = torch.zeros((B, F), dtype=torch.float32, device=self.device)
        row_of = torch.repeat_interleave(
            torch.arange(B, device=self.device),
            self.row_ptr[1:] - self.row_ptr[:-1])
        X[row_of, self.col.long()] = self.val
        return X

    def prefix(self, n: int) -> "SparseBatch":
        """The first n rows as a new batch with a rebuilt column index
        (n == 0: the empty batch a stopped worker serves)."""
        n = max(0, min(int(n), self.shape[0]))
        row_ptr = self.row_ptr[:n + 1]
        nnz = int(row_ptr[-1])
        return SparseBatch(row_ptr, self.col[:nnz], self.val[:nnz],
                           self.num_features)
