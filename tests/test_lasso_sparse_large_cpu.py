"""ops.lasso_sparse_windows, the clean-window table of K11sL, on a
hand-written column index against flags written out by hand."""

import pytest
import torch

from harmony_amd import ops

SOLO = 5
# 38 columns; column k holds row 100 + k alone unless listed here
SPECIAL = {
    1: [7, 101], 2: [7],              # share row 7 inside a window (4 and 16)
    7: [9], 8: [9, 108],              # share row 9 across a boundary of 4
    15: [11], 16: [11],               # share row 11 across a boundary of both
    20: [300, 301, 302, 303, 304],    # SOLO entries: still clean
    21: [],                           # no entries: does not dirty its window
    33: [200, 201, 202, 203, 204, 205],   # SOLO + 1 entries
}
# width 4: windows 0 (columns 1, 2) and 8 (column 33) are dirty; the last
# window is columns 36, 37. Width 16: 0 (1, 2; 7, 8) and 2 (33) are dirty.
FLAGS = {4: [0, 1, 1, 1, 1, 1, 1, 1, 0, 1], 16: [0, 1, 0]}


def _index(device="cpu"):
    cols = [SPECIAL.get(k, [100 + k]) for k in range(38)]
    ptr = torch.tensor([0] + [len(c) for c in cols]).cumsum(0)
    row = torch.tensor([r for c in cols for r in c], dtype=torch.int32)
    return ptr.to(device), row.to(device)


@pytest.mark.parametrize("width", [4, 16])
def test_flags(width):
    got = ops.lasso_sparse_windows(*_index(), width, SOLO)
    assert got.dtype == torch.uint8
    assert got.tolist() == FLAGS[width]
    # tensor ops alone, no host read: the same call traces on the meta device
    meta = ops.lasso_sparse_windows(*_index("meta"), width, SOLO)
    assert meta.device.type == "meta" and meta.dtype == torch.uint8
    assert meta.shape == got.shape


def test_no_entries_at_all():
    ptr = torch.zeros(6, dtype=torch.int64)
    row = torch.zeros(0, dtype=torch.int32)
    assert ops.lasso_sparse_windows(ptr, row, 4, SOLO).tolist() == [1, 1]
