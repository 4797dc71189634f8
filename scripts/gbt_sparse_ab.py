"""Isolated A/B of the GBT level histogram on MI355X: K10s
(ops.gbt_hist_sparse, over a SparseBins) against dense K10 (ops.gbt_hist) on
the same batch densified, at B = 4096, 32 non-zeros per row, nb = 64, for
n_nodes 1 and 8 and F from 64 to 2^20 (at 2^20 only K10s runs: the dense
bins would take 16 GiB as int32). Runs are interleaved round by round; each
figure is the median over rounds of a per-round median device time, with the
min..max over rounds. Also records the peak memory of one wide sparse job.

  python scripts/gbt_sparse_ab.py [--out profiles/gbt_sparse_ab.md]
"""

import argparse
import statistics
import sys

import torch

sys.path.insert(0, ".")
from harmony_amd import ops  # noqa: E402
from harmony_amd.mlapps.sparse_bins import SparseBins  # noqa: E402

hip = ops._load_hip()
assert hip is not None and torch.cuda.is_available(), "needs the GPU build"

ROUNDS = 5
B, K, NB = 4096, 32, 64
DENSE_MAX_F = 2 ** 16
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


def interleaved(cases, iters=10, warmup=2, rounds=ROUNDS):
    """{name: fn} -> {name: (median, min, max)} in microseconds."""
    res = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            res[k].append(bench_dev(fn, iters, warmup) * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}


def fmt(t):
    return f"{t[0]:9.1f} us ({t[1]:.1f}..{t[2]:.1f})"


def make_batch(F, seed):
    """B rows of K random columns each (repeats dropped), normal values."""
    g = torch.Generator().manual_seed(seed)
    cols = torch.randint(0, F, (B, K), generator=g).sort(dim=1).values
    keep = torch.ones((B, K), dtype=torch.bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    vals = torch.randn(B, K, generator=g)
    row_ptr = torch.zeros(B + 1, dtype=torch.int64)
    row_ptr[1:] = torch.cumsum(keep.sum(dim=1), 0)
    return SparseBins((row_ptr, cols[keep], vals[keep], F), NB).to("cuda")


def shape_ab(F):
    sb = make_batch(F, seed=F)
    nf, nnz = sb.feat_ids.shape[0], sb.nnz
    g = torch.Generator(device="cuda").manual_seed(F)
    resid = torch.randn(B, generator=g, device="cuda")
    emit(f"### F = {F}")
    emit()
    emit(f"nnz {nnz} ({nnz / B:.1f} per row, density {nnz / (B * F):.2e}), "
         f"present features {nf}, mean column length {nnz / nf:.1f}. Dense "
         f"int32 bins: {B * F * 4 / 2 ** 20:.0f} MiB; the sparse batch: "
         f"{(nnz * 24 + nf * 16) / 2 ** 20:.2f} MiB.")
    emit()
    dense = None
    if F <= DENSE_MAX_F:
        dense = sb.to_dense_bins().int()
    emit("| n_nodes | K10s (totals + kernel) | K10s kernel alone | "
         "dense K10 (zero fill + kernel) | K10 / K10s | histogram, sparse | "
         "histogram, dense |")
    emit("|---|---|---|---|---|---|---|")
    for n_nodes in (1, 8):
        node = torch.randint(0, n_nodes, (B,), generator=g, device="cuda")
        node32 = node.int()
        side = (sb.feat_ptr, sb.feat_row, sb.feat_bin, sb.feat_idx,
                sb.zero_bin)
        ncnt = torch.zeros(n_nodes, device="cuda").scatter_add_(
            0, node, torch.ones_like(resid))
        nsum = torch.zeros(n_nodes, device="cuda").scatter_add_(
            0, node, resid)
        cases = {
            "s": lambda: ops.gbt_hist_sparse(*side, resid, node32, n_nodes,
                                             NB),
            "k": lambda: hip.gbt_hist_sparse(*side, resid, node32, ncnt,
                                             nsum, NB),
        }
        if dense is not None:
            cases["d"] = lambda: ops.gbt_hist(dense, resid, node32, n_nodes,
                                              NB)
            # same histograms on the present features
            cs, ss = cases["s"]()
            cd, sd = cases["d"]()
            ids = sb.feat_ids.long()
            assert torch.equal(cs, cd[:, ids]), "counts differ"
            scale = float(resid.abs().sum())
            assert float((ss - sd[:, ids]).abs().max()) < 1e-5 * scale
            del cs, ss, cd, sd
        res = interleaved(cases)
        hs = n_nodes * nf * NB * 8 / 2 ** 20
        hd = n_nodes * F * NB * 8 / 2 ** 20
        if dense is not None:
            emit(f"| {n_nodes} | {fmt(res['s'])} | {fmt(res['k'])} | "
                 f"{fmt(res['d'])} | {res['d'][0] / res['s'][0]:.2f} | "
                 f"{hs:.1f} MiB | {hd:.1f} MiB |")
        else:
            emit(f"| {n_nodes} | {fmt(res['s'])} | {fmt(res['k'])} | "
                 f"not run | | {hs:.1f} MiB | {hd:.1f} MiB |")
    emit()
    del dense
    torch.cuda.empty_cache()


def wide_job_peak():
    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.dolphin.master import run_job
    from harmony_amd.runtime.bootstrap import init_executor

    F = 2 ** 20
    job = JobConfig(job_id="ab_gbt_wide", app="gbt", max_num_epochs=1,
                    num_mini_batches=2,
                    app_args={"num_features": F, "batch_size": B,
                              "nnz_per_row": K, "num_bins": NB,
                              "max_depth": 4, "sparse": "true"})
    ctx = init_executor(RuntimeConfig(device="cuda"))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    s = run_job(job, ctx).summary()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    emit(f"### Wide job: F = 2^20, B = {B}, {K} non-zeros per row, nb = {NB}, "
         f"depth 4, 2 batches")
    emit()
    emit(f"Peak device memory allocated {peak / 2 ** 20:.0f} MiB; one dense "
         f"int64 batch of bins would be {B * F * 8 / 2 ** 30:.0f} GiB. "
         f"{s['num_batches']} batches, {int(s['num_trees'])} trees, compute "
         f"{s['comp_time_sec'] * 1e3:.1f} ms in all, mse {s['mse']:.4f}.")
    emit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    emit(f"Device: {torch.cuda.get_device_name(0)}; B = {B}, {K} draws per "
         f"row, nb = {NB}; device-event times of one op call, {ROUNDS} "
         f"interleaved rounds of 10 timed calls after 2 warm-up calls.")
    emit()
    for F in (64, 1024, 4096, 2 ** 16, 2 ** 20):
        shape_ab(F)
    wide_job_peak()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
