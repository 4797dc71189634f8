"""Isolated A/B of the GBT split search on MI355X: K10b (ops.gbt_best_split,
two launches) against the torch path of the same op on the same GPU, at
n_nodes in {1, 8, 64}, F in {32, 784}, nb = 64, all-continuous and
half-categorical types; and a whole tree build through K10b (build_tree with
all-zero feature types) against the untyped build_tree (the tensor-op search;
both make one host copy per level) on the same batch. Runs are interleaved
round by round; each figure is the median over rounds of a per-round median,
with the min..max over rounds.

  python scripts/gbt_split_ab.py [--out profiles/gbt_split_ab.md]
"""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from harmony_amd import ops  # noqa: E402
from harmony_amd.mlapps import gbt  # noqa: E402

hip = ops._load_hip()
assert hip is not None and torch.cuda.is_available(), "needs the GPU build"

ROUNDS = 5
OUT = []


def emit(line=""):
    print(line, flush=True)
    OUT.append(line)


def bench_dev(fn, iters, warmup):
    """Median device time (ms) of fn's launches, by device events."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), \
            torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def bench_host(fn, iters, warmup):
    """Median host time (ms) of fn, which ends in a device -> host copy."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def interleaved(cases, bench, iters=20, warmup=3, rounds=ROUNDS):
    """{name: fn} -> {name: (median, min, max)} in microseconds."""
    res = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            res[k].append(bench(fn, iters, warmup) * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}


def fmt(t):
    return f"{t[0]:9.1f} us ({t[1]:.1f}..{t[2]:.1f})"


def torch_path(cnt, s, ftype, lam):
    os.environ["HARMONY_FORCE_TORCH_OPS"] = "1"
    try:
        return ops.gbt_best_split(cnt, s, ftype, lam)
    finally:
        del os.environ["HARMONY_FORCE_TORCH_OPS"]


def level_histograms(n_nodes, F, nb, seed):
    """One level's K10 output on a seeded batch of 16384 rows."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    B = 16384
    bins = torch.randint(0, nb, (B, F), generator=g, device="cuda")
    resid = torch.randn(B, generator=g, device="cuda")
    node = torch.randint(0, n_nodes, (B,), generator=g, device="cuda")
    return ops.gbt_hist(bins, resid, node, n_nodes, nb)


def op_ab():
    emit("## K10b against the torch path of ops.gbt_best_split, nb = 64")
    emit()
    emit("| n_nodes | F | types | K10b (2 launches) | torch path | "
         "torch / K10b | same answer |")
    emit("|---|---|---|---|---|---|---|")
    for F in (32, 784):
        for n_nodes in (1, 8, 64):
            cnt, s = level_histograms(n_nodes, F, 64, seed=n_nodes + F)
            for label, ftype in (
                    ("continuous", torch.zeros(F, dtype=torch.int32)),
                    ("half categorical",
                     (torch.arange(F) % 2 * 64).to(torch.int32))):
                ftype = ftype.cuda()
                a = ops.gbt_best_split(cnt, s, ftype, 1.0)
                b = torch_path(cnt, s, ftype, 1.0)
                same = all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
                res = interleaved({
                    "hip": lambda: ops.gbt_best_split(cnt, s, ftype, 1.0),
                    "torch": lambda: torch_path(cnt, s, ftype, 1.0),
                }, bench_dev)
                emit(f"| {n_nodes} | {F} | {label} | {fmt(res['hip'])} | "
                     f"{fmt(res['torch'])} | "
                     f"{res['torch'][0] / res['hip'][0]:.2f}x | "
                     f"{'yes' if same else 'NO'} |")
    emit()


def leaf_ids(tree, bins):
    """The leaf each row reaches: the tree's routing with the leaf's index
    as its value (exact in fp32)."""
    probe = gbt.GBTree(tree.depth, tree.feature, tree.threshold,
                       [float(i) for i in range(1 << tree.depth)],
                       tree.cat_mask)
    return probe.predict_bins(bins)


def build_ab():
    emit("## build_tree through K10b (all-zero types) against the untyped "
         "build_tree")
    emit()
    emit("Host time of one call, device synchronised before and after (the "
         "call ends in the leaf values' device -> host copy). B = 16384, "
         "nb = 64, lam = 1.")
    emit()
    emit("| F | max_depth | typed (K10 + K10b, one copy per level) | "
         "untyped (tensor ops, one copy per level) | untyped / typed | "
         "typed against untyped tree |")
    emit("|---|---|---|---|---|---|")
    for F in (32, 784):
        g = torch.Generator(device="cuda").manual_seed(F)
        bins = torch.randint(0, 64, (16384, F), generator=g, device="cuda")
        resid = torch.randn(16384, generator=g, device="cuda")
        zero = torch.zeros(F, dtype=torch.int32, device="cuda")
        for depth in (1, 4, 6):
            a = gbt.build_tree(bins, resid, 64, depth, 1.0, zero)
            b = gbt.build_tree(bins, resid, 64, depth, 1.0)
            # the splits are compared exactly; the leaf values come from
            # float atomics (K10's and scatter_add_'s summation order varies
            # from call to call), so the predictions are compared by size
            nodes = sum(1 for i in range(len(a.feature))
                        if (a.feature[i], a.threshold[i])
                        != (b.feature[i], b.threshold[i]))
            rows = int((leaf_ids(a, bins) != leaf_ids(b, bins)).sum())
            dp = float((a.predict_bins(bins) - b.predict_bins(bins))
                       .abs().max())
            same = (f"{nodes} of {len(a.feature)} nodes differ, {rows} rows "
                    f"reach another leaf, largest prediction difference "
                    f"{dp:.1e}")
            res = interleaved({
                "typed": lambda: gbt.build_tree(bins, resid, 64, depth, 1.0,
                                                zero),
                "untyped": lambda: gbt.build_tree(bins, resid, 64, depth,
                                                  1.0),
            }, bench_host, iters=10, warmup=2)
            emit(f"| {F} | {depth} | {fmt(res['typed'])} | "
                 f"{fmt(res['untyped'])} | "
                 f"{res['untyped'][0] / res['typed'][0]:.2f}x | {same} |")
    emit()
    emit("Nodes that differ while every row reaches the same leaf hold "
         "equivalent splits: thresholds on either side of an empty bin give "
         "the same partition and exactly the same gain. K10b takes the "
         "lowest such candidate; the untyped search takes whichever "
         "torch's device argmax returns. The leaf values come from float "
         "atomics in both builds, so predictions agree to rounding only.")
    emit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    emit("# GBT split search: K10b A/B")
    emit()
    emit(f"Device: {torch.cuda.get_device_name(0)}; {ROUNDS} interleaved "
         f"rounds; op times are device-event times of one call (20 timed "
         f"after 3 warm-up per round), build times host times of one call "
         f"(10 timed after 2 warm-up per round). Measured by "
         f"scripts/gbt_split_ab.py.")
    emit()
    op_ab()
    build_ab()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
