"""Isolated A/B of the Lasso sweep on MI355X: K11s (ops.lasso_cd_sparse) at
each forced thread count and at the host rule's choice, against dense K11
(residual GEMV + ops.lasso_cd) on the same data densified, at mean column
lengths of about 1, 16, 256 and B. Runs are interleaved round by round; each
figure is the median over rounds of a per-round median device time, with the
min..max over rounds. Also records the peak memory of the wide sparse job.

  python scripts/lasso_sparse_ab.py [--out profiles/lasso_sparse_ab.md]
"""

import argparse
import statistics
import sys

import torch

sys.path.insert(0, ".")
from harmony_amd import ops  # noqa: E402
from harmony_amd.mlapps import lasso  # noqa: E402
from harmony_amd.mlapps.sparse_batch import SparseBatch  # noqa: E402

hip = ops._load_hip()
assert hip is not None and torch.cuda.is_available(), "needs the GPU build"

ROUNDS = 5
THREADS = (64, 256, 1024)
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
    return f"{t[0]:10.1f} us ({t[1]:.1f}..{t[2]:.1f})"


def make_batch(B, F, k, seed, density=0.25, noise=0.1):
    """The app's synthetic sparse batch, built on the GPU; k >= F gives the
    fully dense batch."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    w_true = torch.randn(F, generator=g, device="cuda") * (
        torch.rand(F, generator=g, device="cuda") < density)
    if k >= F:
        cols = torch.arange(F, device="cuda").expand(B, F).contiguous()
        keep = torch.ones((B, F), dtype=torch.bool, device="cuda")
    else:
        cols = torch.randint(0, F, (B, k), generator=g, device="cuda") \
            .sort(dim=1).values
        keep = torch.ones((B, k), dtype=torch.bool, device="cuda")
        keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    vals = torch.randn(cols.shape, generator=g, device="cuda") * keep
    y = (vals * w_true[cols]).sum(dim=1) \
        + noise * torch.randn(B, generator=g, device="cuda")
    row_ptr = torch.zeros(B + 1, dtype=torch.int64, device="cuda")
    row_ptr[1:] = torch.cumsum(keep.sum(dim=1), 0)
    return SparseBatch(row_ptr, cols[keep].to(torch.int32), vals[keep], F), y


def shape_ab(B, F, k, dense_iters=10, dense_rounds=ROUNDS):
    x, y = make_batch(B, F, k, seed=B + F + k)
    nnz, nf = x.nnz, x.feat_ids.shape[0]
    # the threshold shrinks a weight by lam_n / col_sq: 0.1 at the mean
    # column, so that weights move whatever the column length (the app's
    # default lam = 0.05 zeroes every weight of a 1-entry column)
    lam_n = 0.1 * nnz / nf
    col_sq = lasso._sparse_col_sq(x)
    idx = (x.feat_ids, x.feat_ptr, x.feat_row, x.feat_val)
    # a model in mid-training: one sweep from zero
    w0 = torch.zeros(F, device="cuda")
    w1, _ = ops.lasso_cd_sparse(*idx, y, w0, col_sq, lam_n)
    w2, r2 = ops.lasso_cd_sparse(*idx, y, w1, col_sq, lam_n)
    pick = ops.lasso_sparse_threads(nf, nnz)
    emit(f"### B = {B}, F = {F}: mean column length {nnz / nf:.1f}")
    emit()
    emit(f"nnz {nnz}, present features {nf}, {nnz / B:.1f} non-zeros per "
         f"row, lam_n {lam_n:.3g}; the timed sweep starts from a model with "
         f"{int((w1 != 0).sum())} non-zero weights and moves "
         f"{int((w2 != w1).sum())}. Host rule: {pick} threads. A dense batch "
         f"would take {B * F * 4 / 2 ** 30:.3f} GiB.")
    emit()
    cases = {}
    for t in THREADS:
        cases[f"K11s, {t} threads"] = (
            lambda t=t: ops.lasso_cd_sparse(*idx, y, w1, col_sq, lam_n,
                                            _force_threads=t))
    cases["K11s, host rule"] = (
        lambda: ops.lasso_cd_sparse(*idx, y, w1, col_sq, lam_n))
    res = interleaved(cases)
    dense = None
    if dense_iters:
        X = x.to_dense()
        dcs = torch.linalg.vector_norm(X, dim=0).square().clamp_min(1e-9)

        def dense_sweep():
            ops.lasso_cd(X, y - X @ w1, w1, dcs, lam_n)

        dense_sweep()                       # builds the transposed copy
        wd, rd = ops.lasso_cd(X, y - X @ w1, w1, dcs, lam_n)
        present = torch.zeros(F, dtype=torch.bool, device="cuda")
        present[x.feat_ids.long()] = True
        emit(f"Dense K11 against K11s on the present features: largest "
             f"weight difference {float((wd - w2)[present].abs().max()):.2e}"
             f", largest residual difference "
             f"{float((rd - r2).abs().max()):.2e} (K11 also drives "
             f"{int(((w1 != 0) & ~present).sum())} absent features' weights "
             f"to zero).")
        emit()
        dense = interleaved({"dense": dense_sweep}, iters=dense_iters,
                            warmup=1, rounds=dense_rounds)["dense"]
        del X
    emit("| sweep | device time, median (min..max over rounds) |")
    emit("|---|---|")
    for name, t in res.items():
        emit(f"| {name} | {fmt(t)} |")
    if dense is not None:
        emit(f"| dense K11 (residual GEMV + sweep, 1024 threads; "
             f"{dense_rounds} rounds of {dense_iters}) | {fmt(dense)} |")
    best = min(THREADS, key=lambda t: res[f"K11s, {t} threads"][0])
    tb = res[f"K11s, {best} threads"][0]
    tp = res[f"K11s, {pick} threads"][0]
    emit()
    line = (f"Fastest forced count: {best} threads. The host rule's {pick} "
            f"threads take {tp / tb:.2f}x the fastest.")
    if dense is not None:
        line += (f" Dense K11 takes {dense[0] / res['K11s, host rule'][0]:.2f}"
                 f"x the time of K11s at the host rule's choice.")
    emit(line)
    emit()
    torch.cuda.empty_cache()


def wide_job_peak():
    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.dolphin.master import run_job
    from harmony_amd.runtime.bootstrap import init_executor

    F, B = 2 ** 20, 1024
    job = JobConfig(job_id="ab_lasso_wide", app="lasso", max_num_epochs=1,
                    num_mini_batches=2,
                    app_args={"num_features": F, "num_parts": 16,
                              "batch_size": B, "nnz_per_row": 32,
                              "sparse": "true"})
    ctx = init_executor(RuntimeConfig(device="cuda"))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    s = run_job(job, ctx).summary()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    emit("### Wide job: F = 2^20, B = 1024, 32 non-zeros per row, 2 batches")
    emit()
    emit(f"Peak device memory allocated {peak / 2 ** 20:.0f} MiB; one dense "
         f"batch would be {B * F * 4 / 2 ** 20:.0f} MiB. "
         f"{s['num_batches']} batches, compute {s['comp_time_sec'] * 1e3:.1f}"
         f" ms in all, mse {s['mse']:.4f}.")
    emit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--no-wide-dense", action="store_true",
                    help="skip dense K11 on the 8 GiB densified wide batch")
    args = ap.parse_args()
    emit(f"Device: {torch.cuda.get_device_name(0)}; device-event times of "
         f"one op call (clone of w + one launch), {ROUNDS} interleaved "
         f"rounds of 10 timed calls after 2 warm-up calls.")
    emit()
    B = 2048
    shape_ab(B, 2 ** 20, 32, dense_iters=0 if args.no_wide_dense else 2,
             dense_rounds=2)
    shape_ab(B, 4096, 32)
    shape_ab(B, 1024, 32)
    shape_ab(B, 256, 32)
    shape_ab(B, 64, 32)
    shape_ab(B, 64, 64)
    wide_job_peak()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
