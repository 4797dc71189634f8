"""Isolated A/B: K10w (levels wider than 8192 cells) against the scatter_add_
pair that HARMONY_FORCE_TORCH_OPS=1 forces on the same device, and a whole
build_tree at depth 10. Three arms per shape, timed in alternating rounds:
K10w, K10w with every pass kept in LDS (HARMONY_GBT_HIST_DIRECT=0), torch.
Reports the median over the rounds and the spread (max - min) / median of
each arm; outputs are compared with the float64 bound of the tests first.

  python scripts/gbt_hist_wide_ab.py [--rounds 7] [--iters 200]
"""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from harmony_amd import ops  # noqa: E402
from harmony_amd.mlapps.gbt import build_tree  # noqa: E402

ARMS = {"k10w": {}, "k10w_lds_only": {"HARMONY_GBT_HIST_DIRECT": "0"},
        "torch": {"HARMONY_FORCE_TORCH_OPS": "1"}}


def timed(fn, env, iters):
    os.environ.update(env)
    try:
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3
    finally:
        for k in env:
            del os.environ[k]


def ab(label, fn, rounds, iters):
    for env in ARMS.values():                   # warm every arm
        timed(fn, env, 3)
    ms = {arm: [] for arm in ARMS}
    for _ in range(rounds):
        for arm, env in ARMS.items():
            ms[arm].append(timed(fn, env, iters))
    med = {a: statistics.median(v) for a, v in ms.items()}
    cells = "  ".join(
        f"{a} {med[a]:8.3f} ms (spread {(max(v) - min(v)) / med[a]:4.0%})"
        for a, v in ms.items())
    print(f"{label}: {cells}  torch / k10w {med['torch'] / med['k10w']:5.2f}x",
          flush=True)


def within_bound(bins, resid, node, n_nodes, nb):
    """Largest error / bound of K10w against float64, counts exact."""
    cnt, s = ops.gbt_hist(bins, resid, node, n_nodes, nb)
    B, F = bins.shape
    idx = ((node.long().unsqueeze(1) * F + torch.arange(F, device="cuda"))
           * nb + bins.long()).reshape(-1)
    r = resid.double().unsqueeze(1).expand(B, F).reshape(-1)
    ref = [torch.zeros(n_nodes * F * nb, dtype=torch.float64, device="cuda")
           .index_add_(0, idx, v) for v in (torch.ones_like(r), r, r.abs())]
    assert torch.equal(cnt.double().reshape(-1), ref[0]), "counts"
    bound = (ref[0] + 1) * 2.0 ** -24 * ref[2]
    err = (s.double().reshape(-1) - ref[1]).abs()
    assert bool((err <= bound).all()), "sums"
    return float((err[bound > 0] / bound[bound > 0]).max())


def case(B, F, nb, n_nodes, skew, rounds, iters):
    g = torch.Generator().manual_seed(1)
    bins = torch.randint(0, nb, (B, F), generator=g).int().cuda()
    resid = torch.randn(B, generator=g).cuda()
    node = torch.randint(0, n_nodes, (B,), generator=g)
    if skew:
        node[torch.rand(B, generator=g) < 0.9] = 0
    node = node.int().cuda()
    ratio = within_bound(bins, resid, node, n_nodes, nb)
    ab(f"B={B:6d} F={F} nb={nb:3d} nodes={n_nodes:4d} "
       f"{'skew  ' if skew else 'random'} err/bound {ratio:.3f}",
       lambda: ops.gbt_hist(bins, resid, node, n_nodes, nb), rounds, iters)


def tree(rounds, iters):
    g = torch.Generator().manual_seed(2)
    bins = torch.randint(0, 64, (65536, 32), generator=g).cuda()
    resid = torch.randn(65536, generator=g).cuda()
    ab("build_tree B=65536 F=32 nb=64 depth=10",
       lambda: build_tree(bins, resid, 64, 10, 1.0), rounds, iters)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    for skew in (False, True):
        case(65536, 32, 64, 256, skew, a.rounds, a.iters)
        case(65536, 32, 64, 1024, skew, a.rounds, a.iters)
    case(65536, 32, 256, 64, False, a.rounds, a.iters)
    case(4096, 32, 64, 1024, False, a.rounds, a.iters)
    tree(a.rounds, max(1, a.iters // 8))
