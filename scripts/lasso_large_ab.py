"""K11L (ops/csrc/lasso_large.hip) measurements for profiles/lasso_large_ab.md.

  python scripts/lasso_large_ab.py --loop-error   # CPU: float32 loop vs fp64
  python scripts/lasso_large_ab.py                # GPU: isolated A/B
  python scripts/lasso_large_ab.py --job          # GPU: one Lasso job

The A/B alternates the two paths `--rounds` times on the same inputs and
prints each path's median and its min..max over the rounds.
"""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from harmony_amd import ops  # noqa: E402


def loop_error():
    from tests import test_lasso_large_gpu as t

    os.environ["HARMONY_FORCE_TORCH_OPS"] = "1"
    worst_w = worst_r = 0.0
    cases = [(B, t.F) for B in t.ROWS] + [(ops.LASSO_CD_MAX_ROWS + 1, 2)]
    for B, nf in cases:
        for lam in t.LAMS:
            case = t.make_case(B, nf)
            w, r = ops.lasso_cd(case["X"], case["r"], case["w"],
                                case["col_sq"], lam * B)
            w64, r64, margin = t.sweep64(case, lam * B)
            w_err = float((w.double() - w64).abs().max())
            r_err = float((r.double() - r64).abs().max())
            print(f"B {B} F {nf} lam_n {lam * B:g}: loop w error {w_err:.3g} "
                  f"r error {r_err:.3g} margin/B {margin / B:.3g}")
            worst_w, worst_r = max(worst_w, w_err), max(worst_r, r_err)
    print(f"largest loop error: w {worst_w:.3g} r {worst_r:.3g}")


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def inputs(B, F):
    g = torch.Generator().manual_seed(1)
    X = torch.randn(B, F, generator=g).cuda()
    y = torch.randn(B, generator=g).cuda()
    return X, y, torch.zeros(F, device="cuda"), \
        (X * X).sum(dim=0).clamp_min(1e-9)


def sweep_ms(X, r, w, col_sq, torch_ops, iters):
    if torch_ops:
        os.environ["HARMONY_FORCE_TORCH_OPS"] = "1"
    try:
        return timed(lambda: ops.lasso_cd(X, r, w, col_sq,
                                          0.05 * X.shape[0]), iters)
    finally:
        os.environ.pop("HARMONY_FORCE_TORCH_OPS", None)


def report(name, ms):
    print(f"  {name:28s} median {statistics.median(ms):8.3f} ms  "
          f"(min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} rounds)")
    return statistics.median(ms)


def ab(rounds):
    F = 256
    for B in (16384, 32768, 65536):
        args = inputs(B, F)
        hip, loop = [], []
        for _ in range(rounds):
            hip.append(sweep_ms(*args, torch_ops=False, iters=50))
            loop.append(sweep_ms(*args, torch_ops=True, iters=5))
        print(f"B {B} F {F}: one sweep")
        a = report("K11L", hip)
        b = report("tensor-op loop", loop)
        print(f"  K11L is {b / a:.1f}x the loop's speed")
    below, above = inputs(16367, F), inputs(16368, F)
    k11, k11l = [], []
    for _ in range(rounds):
        k11.append(sweep_ms(*below, torch_ops=False, iters=50))
        k11l.append(sweep_ms(*above, torch_ops=False, iters=50))
    print(f"dispatch boundary, F {F}: one sweep")
    a = report("K11  at B 16367", k11)
    b = report("K11L at B 16368", k11l)
    print(f"  K11L / K11 time {b / a:.2f}")


def job(rounds):
    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.dolphin.master import run_job
    from harmony_amd.runtime.bootstrap import init_executor

    ctx = init_executor(RuntimeConfig(device="cuda"))
    ms = []
    for i in range(rounds + 1):
        cfg = JobConfig(job_id=f"lasso_large_{i}", app="lasso",
                        max_num_epochs=10, num_mini_batches=4,
                        app_args={"num_features": 256, "batch_size": 16384})
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = run_job(cfg, ctx).summary()
        torch.cuda.synchronize()
        if i:                                   # the first job warms up
            ms.append((time.perf_counter() - t0) / s["num_batches"] * 1e3)
    print("Lasso job, batch_size 16384, num_features 256, 40 steps a job")
    report("time per step", ms)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop-error", action="store_true")
    ap.add_argument("--job", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.loop_error:
        loop_error()
    else:
        assert torch.cuda.is_available(), "the timings need a GPU"
        job(a.rounds) if a.job else ab(a.rounds)
