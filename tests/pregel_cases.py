"""Shared cases for the Pregel graph-input / pull-kernel tests
(test_pregel_graph.py on CPU, test_pregel_gpu.py on the GPU): fixture
paths, the float64 PageRank reference with its derived error bound, and the
hand-made pull index with its brute-force evaluation."""

from __future__ import annotations

import functools
from pathlib import Path

import torch

GOLDEN = Path(__file__).parent / "golden" / "pregel"
SHORTEST_PATH = str(GOLDEN / "shortest_path")
ADJ_LIST = str(GOLDEN / "adj_list")

# Dijkstra from vertex 0 on shortest_path, worked by hand from the file
SSSP_FROM_0 = [0.0, 2.0, 3.0, 4.0, 7.0, 10.0, 6.0, 9.0, 10.0, 15.0]

U32 = 2.0 ** -24          # float32 unit roundoff


def pagerank_f64(src: torch.Tensor, dst: torch.Tensor, n: int, iters: int):
    """float64 power iteration with the engine's semantics (a vertex
    without out-edges sends nothing) -> (ranks [n], bound [n]).

    bound is the tolerance for a float32 run. One float32 iteration at a
    vertex with in-degree d computes 0.15/n + 0.85 * sum_{d terms}
    (v_u / outdeg_u): one rounding for the division of each term, d - 1 for
    the sum in any order, one for the multiply and one for the add — at
    most d + 2 roundings on any operand's path, so (standard recursive-
    summation analysis, all terms non-negative) its local error is at most
    (d + 2) * 2^-24 * S_k with S_k the sum of the term magnitudes,
    0.15/n + 0.85 * sum |v_u / outdeg_u|, in iteration k. Errors already in
    the inputs pass through a non-negative operator of column sum <= 0.85,
    so they do not grow; adding the local errors over the iterations gives
        iters * (d + 2) * 2^-24 * max_k S_k       per vertex."""
    src, dst = src.long(), dst.long()
    outdeg = torch.bincount(src, minlength=n).clamp_min(1).double()
    indeg = torch.bincount(dst, minlength=n).double()
    v = torch.full((n,), 1.0 / n, dtype=torch.float64)
    smax = torch.zeros(n, dtype=torch.float64)
    for _ in range(iters):
        s = torch.zeros(n, dtype=torch.float64)
        s.index_add_(0, dst, (v / outdeg)[src])
        v = 0.15 / n + 0.85 * s
        smax = torch.maximum(smax, v)      # every term is >= 0: S_k == v
    return v, iters * (indeg + 2.0) * U32 * smax


@functools.lru_cache(maxsize=None)
def adj_list_reference(iters: int = 10):
    """(src, dst, n, ranks_f64, bound) for the adj_list fixture; computed
    once and shared — callers must not modify the tensors."""
    from harmony_amd.dataloader import parse_graph

    with open(ADJ_LIST) as f:
        src, dst, _w, max_id = parse_graph(f, weighted=False)
    n = max_id + 1
    ref, bound = pagerank_f64(src, dst, n, iters)
    return src, dst, n, ref, bound


# ------------------------------------------------- hand-made pull index

SPECIAL_DEGREES = [0, 1, 2, 63, 64, 65, 200, 1000]
NUM_ROWS = 257
NUM_SOURCES = 300


@functools.lru_cache(maxsize=None)
def handmade_index():
    """R = 257 rows over 300 sources: the first rows have in-degrees
    {0, 1, 2, 63, 64, 65, 200, 1000} (below / at / above one wave, and rows
    that loop many times for every group width), the rest 0..5.
    -> dict(in_ptr, in_src, in_w, vert_msg, vert_msg_inf, mask). Shared:
    callers must not modify the tensors."""
    g = torch.Generator().manual_seed(1234)
    deg = torch.randint(0, 6, (NUM_ROWS,), generator=g)
    deg[:len(SPECIAL_DEGREES)] = torch.tensor(SPECIAL_DEGREES)
    in_ptr = torch.zeros(NUM_ROWS + 1, dtype=torch.int64)
    in_ptr[1:] = torch.cumsum(deg, 0)
    e = int(in_ptr[-1])
    in_src = torch.randint(0, NUM_SOURCES, (e,), generator=g).to(torch.int32)
    in_w = torch.randint(1, 10, (e,), generator=g).to(torch.float32)
    vert_msg = torch.rand(NUM_SOURCES, generator=g) * 8.0
    vert_msg_inf = vert_msg.clone()
    vert_msg_inf[torch.rand(NUM_SOURCES, generator=g) < 0.3] = float("inf")
    mask = torch.rand(NUM_SOURCES, generator=g) < 0.5
    return dict(in_ptr=in_ptr, in_src=in_src, in_w=in_w, vert_msg=vert_msg,
                vert_msg_inf=vert_msg_inf, mask=mask)


def brute_force_pull(in_ptr, in_src, in_w, w_const, vert_msg, mask,
                     combiner, add_weight):
    """Plain Python loop over rows and edges. -> (out float64 [R],
    flag uint8 [R], abs_sum float64 [R], degree [R]): out is exact for min
    (the float32 per-edge values are formed first, as the op does) and a
    float64 sum of those float32 values for add; abs_sum is the sum of
    their magnitudes (for the add bound)."""
    R = in_ptr.shape[0] - 1
    src = in_src.long()
    v = vert_msg[src]
    if add_weight:
        v = v + (in_w if in_w is not None else w_const)   # float32, 1 round
    v = v.tolist()
    ptr = in_ptr.tolist()
    src = src.tolist()
    m = None if mask is None else mask.tolist()
    out, flag, asum = [], [], []
    for r in range(R):
        acc = float("inf") if combiner == "min" else 0.0
        a, any_sent = 0.0, 0
        for e in range(ptr[r], ptr[r + 1]):
            if m is not None and not m[src[e]]:
                continue
            any_sent = 1
            acc = min(acc, v[e]) if combiner == "min" else acc + v[e]
            a += abs(v[e]) if v[e] != float("inf") else 0.0
        out.append(acc)
        flag.append(any_sent)
        asum.append(a)
    deg = (in_ptr[1:] - in_ptr[:-1]).double()
    return (torch.tensor(out, dtype=torch.float64),
            torch.tensor(flag, dtype=torch.uint8),
            torch.tensor(asum, dtype=torch.float64), deg)


def pull_configs():
    """(combiner, use_mask, use_weights, add_weight) over both combiners,
    with / without mask, with / without per-edge weights."""
    out = []
    for combiner in ("add", "min"):
        for use_mask in (False, True):
            for use_w in (False, True):
                out.append((combiner, use_mask, use_w, True))
            out.append((combiner, use_mask, False, False))
    return out


def add_bound(deg: torch.Tensor, abs_sum: torch.Tensor) -> torch.Tensor:
    """pagerank_f64's bound for ONE iteration of a plain sum: d terms, each
    possibly rounded once when the weight was added, d - 1 additions —
    within the same (d + 2) * 2^-24 * sum|terms|."""
    return (deg + 2.0) * U32 * abs_sum
