"""Held-out test data for MLR, Lasso, GBT and LDA.

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

LDA has no labels to predict, so its test metric is document completion
(lda_test_set below): the file has the -input format, one document per line
of word ids; the tokens at even positions of a document are observed, those
at odd positions are scored, and LDATrainer.evaluate_test() folds the
observed half in against the frozen table (ops.lda_foldin, kernel K7e) and
reports the per-word perplexity of the scored half. There is no RNG in it.
"""

from __future__ import annotations

from typing import List, Optional

import torch

from harmony_amd.mlapps.sparse_batch import SparseBatch, is_sparse

SUPPORTED_APPS = ("mlr", "lasso", "gbt", "lda")


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


class LDATestSet:
    """Held-out documents as (word, count) pairs sorted by word id within a
    document: CSR over the observed halves (obs_ptr int64 [D + 1], obs_word
    int64, obs_cnt int32) and over the scored halves (sc_*), on the device."""

    def __init__(self, obs, sc, num_docs: int, num_scored_tokens: int):
        self.obs_ptr, self.obs_word, self.obs_cnt = obs
        self.sc_ptr, self.sc_word, self.sc_cnt = sc
        self.num_docs = num_docs
        self.num_scored_tokens = num_scored_tokens


def _pairs(doc: torch.Tensor, word: torch.Tensor, num_docs: int,
           num_vocabs: int):
    """(ptr, word, count) of the distinct (doc, word) among the tokens, in
    (doc, word) order."""
    key, cnt = torch.unique(doc * num_vocabs + word, return_counts=True)
    ptr = torch.zeros(num_docs + 1, dtype=torch.int64)
    ptr[1:] = torch.bincount(key // num_vocabs, minlength=num_docs).cumsum(0)
    return ptr, key % num_vocabs, cnt.to(torch.int32)


def lda_test_set(a: dict, device: torch.device) -> Optional[LDATestSet]:
    """The held-out documents of app args `a` (lda.defaults(): num_vocabs),
    split for document completion; None without test_data_path.

    Every rank reads the whole file. A word id >= num_vocabs raises
    ValueError; a document of fewer than 2 tokens has no scored half and is
    left out; a file without any other document raises ValueError. Tokens at
    even positions (0, 2, ...) of a document, in file order, are observed,
    those at odd positions are scored."""
    path = test_path(a)
    if path is None:
        return None
    from harmony_amd import dataloader as dl

    V = int(a["num_vocabs"])
    offsets, words = dl.parse_lda_split(path, 0, 1)
    offsets, words = offsets.long().cpu(), words.long().cpu()
    if words.numel() and (int(words.max()) >= V or int(words.min()) < 0):
        raise ValueError(
            f"test_data_path {path}: word id {int(words.max())} outside "
            f"0..{V - 1} (num_vocabs {V})")
    lengths = offsets[1:] - offsets[:-1]
    keep = lengths >= 2
    D = int(keep.sum())
    if D == 0:
        raise ValueError(
            f"test_data_path {path}: no document with at least 2 tokens")
    # per token: its document's index among the kept ones, its position
    line = torch.repeat_interleave(torch.arange(lengths.shape[0]), lengths)
    pos = torch.arange(words.shape[0]) - offsets[:-1][line]
    doc = (keep.long().cumsum(0) - 1)[line]
    kept = keep[line]
    observed = kept & (pos % 2 == 0)
    scored = kept & (pos % 2 == 1)
    obs = _pairs(doc[observed], words[observed], D, V)
    sc = _pairs(doc[scored], words[scored], D, V)
    return LDATestSet(tuple(t.to(device) for t in obs),
                      tuple(t.to(device) for t in sc), D, int(scored.sum()))
