"""Shared inputs, fp64 evaluations and error bounds for the sparse-MLR tests
(test_mlr_sparse_cpu.py, test_mlr_sparse_gpu.py).

Bounds: with u = 2^-24, an fp32 sum of n products in any order differs from
the exact sum by at most n*u*sum|terms| to first order; the factor 2 covers
the fp32 rounding of the inputs. Nothing here is tuned to an implementation.
"""

from pathlib import Path

import torch

U = 2.0 ** -24
GOLDEN = Path(__file__).parent / "golden" / "mlr" / "sample_mlr_32"

# comments, blank lines, a row without features, an out-of-range index
# (9 >= F = 6), a repeated index (2, last value wins) and unsorted indices
HAND_TEXT = """# header comment
1 0:0.5 3:0.25

2
0 5:1.5 2:-1.0 9:7.0 1:0.125
   # indented comment
1 2:1.0 4:2.0 2:3.0 0:-0.75 2:0.375
3 3:1e-3 1:2.5e2
"""
HAND_F = 6


def job_file_lines():
    """The 256-line, 4-feature data of test_dataloader.test_mlr_job_from_file."""
    return [f"{i % 3} {i % 3}:1.0 3:{0.1 * (i % 7)}" for i in range(256)]


def segments(lengths, n_index, every, seed, absent=None):
    """Random segmented entries: ptr int64 [S+1], idx int32 [nnz] in
    [0, n_index) never equal to `absent`, val float32 [nnz]. Segment s has
    lengths[s] entries (indices may repeat inside a segment: the ops sum
    them). If `every` is not None, each non-empty segment's first entry
    points at index `every` — the feature present in every row that has
    entries at all (a row of length 0 can hold no feature)."""
    g = torch.Generator().manual_seed(seed)
    ptr = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.tensor(lengths, dtype=torch.int64), 0)
    nnz = int(ptr[-1])
    idx = torch.randint(0, n_index, (nnz,), generator=g)
    if absent is not None:
        idx[idx == absent] = (absent + 1) % n_index
    if every is not None:
        idx[ptr[:-1][torch.tensor(lengths) > 0]] = every
    val = torch.randn(nnz, generator=g)
    return ptr, idx.to(torch.int32), val


def seg_of(ptr):
    return torch.repeat_interleave(torch.arange(ptr.shape[0] - 1),
                                   ptr[1:] - ptr[:-1])


def gather_reduce64(ptr, idx, val, table):
    """fp64 out[s, :] = sum_e val[e] * table[idx[e], :], the sum of the
    terms' magnitudes, and each segment's length n."""
    S = ptr.shape[0] - 1
    seg = seg_of(ptr)
    terms = val.double().unsqueeze(1) * table[idx.long()].double()
    out = torch.zeros((S, table.shape[1]), dtype=torch.float64)
    mag = torch.zeros_like(out)
    out.index_add_(0, seg, terms)
    mag.index_add_(0, seg, terms.abs())
    return out, mag, (ptr[1:] - ptr[:-1]).double()


def bound(n, mag):
    """2 * n * u * sum|terms| per element (n per segment, broadcast)."""
    return 2.0 * n.unsqueeze(1) * U * mag
