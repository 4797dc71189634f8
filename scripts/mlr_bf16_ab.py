#!/usr/bin/env python3
"""A/B: MLR compute phase, float32 default vs data_dtype=bfloat16.

  f32_pair   ops.mlr_forward + ops.mlr_grad_gemm on float32 X: the rocBLAS
             pair and the fused softmax kernel, the trainer's default body
  bf16_step  ops.mlr_step_mfma on the same X rounded to bf16: K4-BF16
             (ops/csrc/mlr_bf16.hip)
  *_fwd      ops.mlr_forward alone on either X

Both paths run in one process on the same data, alternating round by round
after a warm-up of every variant; a round times `iters` calls between two
device synchronisations. Reported: the median round, the spread (min..max
over the rounds), and the bytes of X each path has to stream (two passes
for a step, one for a forward) over the median call time, against the HBM
peak. That rate is a call-level figure (it includes the small prologue,
epilogue and reduce launches), not a single kernel's.

Run on a GPU box:  python scripts/mlr_bf16_ab.py [--out profiles/x.md]
"""
import argparse
import statistics
import time

import torch

from harmony_amd import ops

HBM_PEAK = 8.0e12          # MI355X, bytes/s


def round_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def measure(B, F, C, iters, rounds):
    g = torch.Generator().manual_seed(0)
    X32 = torch.randn(B, F, generator=g).bfloat16().float().cuda()
    X16 = X32.bfloat16()
    W = (torch.randn(C, F, generator=g) * 0.01).cuda()
    y = torch.randint(0, C, (B,), generator=g).cuda()
    wt = torch.zeros((F, 16), device="cuda")

    def f32_pair():
        p, loss, corr = ops.mlr_forward(X32, W, y)
        return ops.mlr_grad_gemm(p, X32), loss, corr

    variants = {
        "f32_pair": (f32_pair, 2 * X32.numel() * 4),
        "bf16_step": (lambda: ops.mlr_step_mfma(X16, W, y, Wt_buf=wt),
                      2 * X16.numel() * 2),
        "f32_fwd": (lambda: ops.mlr_forward(X32, W, y), X32.numel() * 4),
        "bf16_fwd": (lambda: ops.mlr_forward(X16, W, y), X16.numel() * 2),
    }
    # same data (X32 is exact in bf16): the two steps differ by fp32
    # summation order alone
    g0, l0, c0 = f32_pair()
    g1, l1, c1 = variants["bf16_step"][0]()
    rel = float((g1 - g0).abs().max() / g0.abs().max())
    dl = abs(float(l1) - float(l0)) / abs(float(l0))
    assert rel < 1e-3 and dl < 1e-4 and int(c1) == int(c0), (rel, dl)
    for fn, _ in variants.values():
        for _ in range(5):
            fn()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, _) in variants.items():
            times[k].append(round_ms(fn, iters))
    rows = []
    for k, (_, nbytes) in variants.items():
        med = statistics.median(times[k])
        rows.append(f"| {B} x {F} | {k} | {med:.4f} | {min(times[k]):.4f} .. "
                    f"{max(times[k]):.4f} | {nbytes / 2**20:.0f} | "
                    f"{nbytes / (med * 1e-3) / 1e12:.2f} | "
                    f"{nbytes / (med * 1e-3) / HBM_PEAK * 100:.0f}% |")
    sf, sb = ops.mlr_bf16_splits(B, F)
    note = (f"{B} x {F}, C = {C}: splitf = {sf}, splitb = {sb}; bf16 step vs "
            f"f32 pair on the same data: grad max-abs/max-abs {rel:.2e}, "
            f"loss rel {dl:.2e}, correct equal")
    return rows, note


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.hip_available(), \
        "this measurement needs the GPU and the HIP extension"
    lines = [f"device: {torch.cuda.get_device_name(0)}; {args.rounds} "
             f"alternating rounds of {args.iters} calls; HBM peak taken as "
             f"{HBM_PEAK / 1e12:.1f} TB/s", "",
             "| shape | variant | median ms/call | min .. max | X MiB "
             "streamed | TB/s | of HBM peak |", "|---|---|---|---|---|---|---|"]
    notes = []
    for B, F in ((16384, 16384), (4096, 4096)):
        rows, note = measure(B, F, 10, args.iters, args.rounds)
        lines += rows
        notes.append(note)
    text = "\n".join(lines + [""] + notes) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
