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


def is_sparse(a: dict) -> bool:
    """The app argument sparse=true."""
    return str(a.get("sparse", "")).lower() in ("true", "1")


def group_by_column(row_of: torch.Tensor, col: torch.Tensor, feat_ids=None):
    """Entries (row_of[e], col[e]) in row-major order, each (row, col) at
    most once, grouped by column: the permutation `order` (rows ascending
    inside a column), feat_ids (the distinct columns ascending, in col's
    dtype), feat_ptr int64 [nf+1] and feat_row int32 = row_of[order]. With
    feat_ids given the segments are those features', empty ones included."""
    # the input is row-major, so a stable sort by column leaves the rows of
    # each feature ascending
    order = torch.argsort(col, stable=True)
    scol = col[order]
    if feat_ids is None:
        feat_ids, counts = torch.unique_consecutive(scol, return_counts=True)
    else:
        counts = torch.bincount(
            torch.searchsorted(feat_ids.long(), scol.long()),
            minlength=feat_ids.shape[0])
    feat_ptr = torch.zeros(feat_ids.shape[0] + 1, dtype=torch.int64,
                           device=col.device)
    feat_ptr[1:] = torch.cumsum(counts, 0)
    return order, feat_ids, feat_ptr, row_of[order].to(torch.int32)


def column_index(row_ptr: torch.Tensor, col: torch.Tensor):
    """group_by_column of CSR (row_ptr int64 [B+1], col [nnz])."""
    B = row_ptr.shape[0] - 1
    row_of = torch.repeat_interleave(
        torch.arange(B, dtype=torch.int32, device=row_ptr.device),
        row_ptr[1:] - row_ptr[:-1])
    return group_by_column(row_of, col)


def csr_row_blocks(row_ptr, col, val, n: int, n_blocks: int):
    """A parsed CSR file of n rows cut into torch.chunk's row ranges, so
    block i holds the rows the dense loaders give it: yields (lo, hi,
    row_ptr, col, val) per block, row_ptr rebased to the block; one empty
    block for n == 0."""
    size = -(-n // n_blocks) if n else 0
    for lo in range(0, max(1, n), max(1, size)):
        hi = min(n, lo + size)
        e0, e1 = int(row_ptr[lo]), int(row_ptr[hi])
        yield lo, hi, row_ptr[lo:hi + 1] - e0, col[e0:e1], val[e0:e1]


def drop_repeats(cols: torch.Tensor):
    """For the synthetic generators' per-row random feature subset (k draws,
    sorted, repeats dropped): from row-sorted cols [B, k], the mask `keep`
    of each row's distinct draws and the CSR row_ptr of cols[keep]."""
    keep = torch.ones(cols.shape, dtype=torch.bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    row_ptr = torch.zeros(cols.shape[0] + 1, dtype=torch.int64)
    row_ptr[1:] = torch.cumsum(keep.sum(dim=1), 0)
    return keep, row_ptr


def reslice(b, frac):
    """TrainingDataProvider reslice of an (x, y) block, x dense or one of the
    sparse batch types. frac <= 0 -> EMPTY batch: a stopped worker
    (StopWorkerOp) does zero work and its sparse pulls/pushes carry zero
    keys."""
    n = 0 if frac <= 0 else max(1, int(b[0].shape[0] * frac))
    x = b[0].prefix(n) if hasattr(b[0], "prefix") else b[0][:n]
    return (x, b[1][:n])


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
        order, self.feat_ids, self.feat_ptr, self.feat_row = column_index(
            self.row_ptr, self.col)
        self.feat_val = self.val[order].contiguous()

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
