"""Isolated A/B of GBT forest prediction on MI355X: K10p
(ops.gbt_forest_predict, one launch for the whole packed forest) against the
per-tree GBTree.predict_bins loop from an empty cache, which is what
GBTTrainer._forest_pred does on a block it has not seen. Same device, same
process; B = 4096, depth 4, T in {1, 4, 16, 256, 1024}; dense F = 32 and
sparse F = 2^20 with 32 draws per row. Times are wall-clock around a
synchronised call (both paths do host work: the loop builds three host
tensors per tree, K10p packs the forest), the median of the repeats after a
warm-up. The pack time (gbt.pack_forest, host only) is also given alone.

  python scripts/gbt_predict_ab.py [--out profiles/gbt_predict_ab.md]
"""

import argparse
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from harmony_amd import ops  # noqa: E402
from harmony_amd.mlapps import gbt  # noqa: E402
from harmony_amd.mlapps.sparse_bins import SparseBins  # noqa: E402

hip = ops._load_hip()
assert hip is not None and torch.cuda.is_available(), "needs the GPU build"

B, K, NB, DEPTH, STEP = 4096, 32, 64, 4, 0.1
TREES = (1, 4, 16, 256, 1024)
OUT = []


def emit(line=""):
    print(line, flush=True)
    OUT.append(line)


def wall_ms(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return f"{t[0]:8.3f} ms ({t[1]:.3f}..{t[2]:.3f})"


def random_forest(T, F, g, typed):
    ni = (1 << DEPTH) - 1
    out = []
    for _ in range(T):
        thr = torch.randint(0, NB, (ni,), generator=g)
        if typed:
            thr[torch.rand(ni, generator=g) < 0.2] = -2
        out.append(gbt.GBTree(
            depth=DEPTH, feature=torch.randint(0, F, (ni,),
                                               generator=g).tolist(),
            threshold=thr.tolist(),
            leaf_value=torch.randn(1 << DEPTH, generator=g).tolist(),
            cat_mask=torch.randint(0, 2 ** 62, (ni,), generator=g).tolist()
            if typed else None))
    return out


def sparse_batch(F, g):
    cols = torch.randint(0, F, (B, K), generator=g).sort(dim=1).values
    keep = torch.ones((B, K), dtype=torch.bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    row_ptr = torch.zeros(B + 1, dtype=torch.int64)
    row_ptr[1:] = torch.cumsum(keep.sum(dim=1), 0)
    vals = torch.randn(B, K, generator=g)
    return SparseBins((row_ptr, cols[keep], vals[keep], F), NB)


def loop(forest, bins):
    pred = torch.zeros(bins.shape[0], device="cuda")
    for t in forest:
        pred = pred + STEP * t.predict_bins(bins)
    return pred


def shape_ab(name, bins, F, g, sparse):
    emit(f"### {name}")
    emit()
    emit("| T | predict_bins loop | K10p (pack + check + copy + launch) | "
         "pack alone (host) | K10p from a packed device forest | "
         "loop / K10p |")
    emit("|---|---|---|---|---|---|")
    for T in TREES:
        if sparse:
            # half of the node features present in the block, half not
            ids = bins.feat_ids.long().cpu()
            forest = random_forest(T, F, g, typed=True)
            for t in forest:
                for n in range(0, len(t.feature), 2):
                    t.feature[n] = int(ids[torch.randint(
                        0, ids.shape[0], (1,), generator=g)])
        else:
            forest = random_forest(T, F, g, typed=True)
        want = loop(forest, bins)
        got = gbt.forest_predict(forest, bins, STEP)
        assert torch.equal(got, want), "K10p differs from the loop"
        packed = gbt.pack_forest(forest, DEPTH)
        dev_packed = packed.cuda()
        reps = 5 if T >= 256 else 15
        t_loop = wall_ms(lambda: loop(forest, bins), reps, 2)
        t_k = wall_ms(lambda: ops.gbt_forest_predict(
            bins, gbt.pack_forest(forest, DEPTH), DEPTH, STEP), reps, 2)
        t_pack = wall_ms(lambda: gbt.pack_forest(forest, DEPTH), reps, 1)
        t_dev = wall_ms(lambda: ops.gbt_forest_predict(
            bins, dev_packed, DEPTH, STEP), reps, 2)
        emit(f"| {T} | {fmt(t_loop)} | {fmt(t_k)} | {fmt(t_pack)} | "
             f"{fmt(t_dev)} | {t_loop[0] / t_k[0]:.1f} |")
    emit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    emit(f"Device: {torch.cuda.get_device_name(0)}; B = {B}, depth {DEPTH}, "
         f"nb = {NB}, typed forests (rows of 77 words). Wall-clock "
         f"milliseconds around a synchronised call: median (min..max) of 15 "
         f"repeats (5 from T = 256 on) after 2 warm-up calls. Every K10p "
         f"result was torch.equal to the loop's.")
    emit()
    g = torch.Generator().manual_seed(11)
    dense = torch.randint(0, NB, (B, 32), generator=g).cuda()
    shape_ab("Dense, F = 32", dense, 32, g, sparse=False)
    F = 2 ** 20
    sb = sparse_batch(F, g).to("cuda")
    shape_ab(f"Sparse, F = 2^20, {K} draws per row (nnz {sb.nnz})", sb, F,
             g, sparse=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
