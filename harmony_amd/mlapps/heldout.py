"""Held-out test data for the supervised apps (MLR, Lasso, GBT).

Reference: dolphin/core/worker/TestDataProvider.java hands every worker the
file of -test_data_path as ONE split, and Trainer.evaluateModel(trainingData,
testData) reports the test metrics of the final model and of every
checkpoint under offline model evaluation.

Here the app arg test_data_path (with or without file://, as `input`) is read
in the app's build(), before any training, so a missing or unreadable file
fails the job at once. Every rank reads the WHOLE file with the app's own
parser for its mode (dense rows, or CSR with sparse=true: no tensor of n * F
elements is built there). The test metrics are then the same on every rank
and independent of the world size, and evaluation adds no collective beyond
the model pull. A job without the arg is unchanged.
"""

from __future__ import annotations

from typing import List, Optional

import torch

from harmony_amd.mlapps.sparse_batch import SparseBatch, is_sparse

SUPPORTED_APPS = ("mlr", "lasso", "gbt")


def test_path(app_args: dict) -> Optional[str]:
    p = app_args.get("test_data_path")
    return str(p) if p else None


def load_rows(path: str, num_features: int, sparse: bool):
    """The whole file: (X [n, F], y) dense, or (row_ptr, col, val, y)."""
    from harmony_amd import dataloader as dl

    if sparse:
        return dl.parse_libsvm_csr_split(path, 0, 1, num_features)
    return dl.parse_libsvm_split(path, 0, 1, num_features)


def row_blocks(a: dict, device: torch.device, label_dtype=None) -> List:
    """The test rows of app args `a` (an app's defaults(): num_features,
    batch_size, sparse) in blocks of at most batch_size rows, (X, y) or
    (SparseBatch, y) on the device; [] without test_data_path."""
    path = test_path(a)
    if path is None:
        return []
    F = int(a["num_features"])
    size = max(1, int(a["batch_size"]))
    blocks = []
    if is_sparse(a):
        row_ptr, col, val, y = load_rows(path, F, True)
        if label_dtype is not None:
            y = y.to(label_dtype)
        for lo in range(0, y.shape[0], size):
            hi = min(y.shape[0], lo + size)
            e0, e1 = int(row_ptr[lo]), int(row_ptr[hi])
            x = SparseBatch(row_ptr[lo:hi + 1] - e0, col[e0:e1], val[e0:e1],
                            F)
            blocks.append((x.to(device), y[lo:hi].to(device)))
        return blocks
    X, y = load_rows(path, F, False)
    if label_dtype is not None:
        y = y.to(label_dtype)
    for lo in range(0, y.shape[0], size):
        blocks.append((X[lo:lo + size].to(device),
                       y[lo:lo + size].to(device)))
    return blocks
