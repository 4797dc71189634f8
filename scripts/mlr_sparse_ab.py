"""Isolated A/B of the MLR compute phase on MI355X: the dense path
(ops.mlr_forward + ops.mlr_grad_gemm on the densified batch) against the
sparse one (ops.mlr_sparse_forward + ops.mlr_sparse_grad, K4s) on identical
data. Runs are interleaved round by round; each figure is the median over
rounds of a per-round median device time, with the min..max over rounds.

  python scripts/mlr_sparse_ab.py [--out profiles/mlr_sparse_ab.md] [--quick]
"""

import argparse
import statistics
import sys

import torch

sys.path.insert(0, ".")
from harmony_amd import ops  # noqa: E402
from harmony_amd.mlapps.sparse_batch import SparseBatch  # noqa: E402

hip = ops._load_hip()
assert hip is not None and torch.cuda.is_available(), "needs the GPU build"

C = 10
ROUNDS = 5
OUT = []


def emit(line=""):
    print(line, flush=True)
    OUT.append(line)


def bench_dev(fn, iters=20, warmup=3):
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


def interleaved(cases):
    """{name: fn} -> {name: (median, min, max)} in microseconds."""
    res = {k: [] for k in cases}
    for _ in range(ROUNDS):
        for k, fn in cases.items():
            res[k].append(bench_dev(fn) * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}


def make_batch(B, F, k, seed):
    """B rows with (up to) k distinct random features each, on the GPU."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    cols = torch.randint(0, F, (B, k), generator=g, device="cuda") \
        .sort(dim=1).values
    keep = torch.ones((B, k), dtype=torch.bool, device="cuda")
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    vals = torch.randn((B, k), generator=g, device="cuda")
    row_ptr = torch.zeros(B + 1, dtype=torch.int64, device="cuda")
    row_ptr[1:] = torch.cumsum(keep.sum(dim=1), 0)
    x = SparseBatch(row_ptr, cols[keep].to(torch.int32), vals[keep], F)
    y = torch.randint(0, C, (B,), generator=g, device="cuda")
    return x, y


def fmt(t):
    return f"{t[0]:9.1f} us ({t[1]:.1f}..{t[2]:.1f})"


def shape_ab(B, F, k, dense=True, sweep=False):
    x, y = make_batch(B, F, k, seed=B + F + k)
    nnz, nf = x.nnz, x.feat_ids.shape[0]
    W = torch.randn(C, F, device="cuda") * 0.01
    Wt = ops.mlr_sparse_wt(W)
    Cp = Wt.shape[1]
    gf = ops.mlr_sparse_group(B, nnz)
    gg = ops.mlr_sparse_group(nf, nnz)
    emit(f"### B = {B}, F = {F}, {nnz / B:.1f} non-zeros per row "
         f"({100.0 * nnz / (B * F):.3g} % dense)")
    emit()
    emit(f"nnz {nnz}, present features {nf}; groups chosen: forward {gf} "
         f"lanes per row, gradient {gg} lanes per feature. A dense batch "
         f"would take {B * F * 4 / 2 ** 30:.2f} GiB; the CSR and the column "
         f"index together take {(nnz * 16 + (B + nf) * 8 + nf * 4) / 2 ** 20:.1f} MiB.")
    emit()
    P = ops.mlr_sparse_forward(x.row_ptr, x.col, x.val, W, y, Wt_buf=Wt)[0]
    Ppad = torch.zeros(B, Cp, device="cuda")

    def sparse_phase():
        p, _l, _c = ops.mlr_sparse_forward(x.row_ptr, x.col, x.val, W, y,
                                           Wt_buf=Wt)
        ops.mlr_sparse_grad(x.feat_ids, x.feat_ptr, x.feat_row, x.feat_val,
                            p, F)

    def grad_padded():
        Ppad[:, :C] = P
        hip.mlr_sparse_grad(x.feat_ids, x.feat_ptr, x.feat_row, x.feat_val,
                            Ppad[:, :C], F, gg)

    Ppad[:, :C] = P

    cases = {
        "sparse phase (Wt fill + fwd + softmax + grad)": sparse_phase,
        "  Wt fill alone": lambda: ops.mlr_sparse_wt(W, Wt),
        "  mlr_sparse_fwd kernel alone": lambda: hip.mlr_sparse_fwd(
            x.row_ptr, x.col, x.val, Wt, C, gf),
        "  mlr_sparse_grad alone (zeroes G; P already padded)": lambda:
            hip.mlr_sparse_grad(x.feat_ids, x.feat_ptr, x.feat_row,
                                x.feat_val, Ppad[:, :C], F, gg),
        "  mlr_sparse_grad with the P pad copy": grad_padded,
    }
    if dense:
        X = x.to_dense()

        def dense_phase():
            p, _l, _c = ops.mlr_forward(X, W, y)
            ops.mlr_grad_gemm(p, X)

        cases = {"dense phase (parent: mlr_forward + mlr_grad_gemm)":
                 dense_phase, **cases}
        # faster and different is not faster: same gradient either way
        pd = ops.mlr_forward(X, W, y)[0]
        gd = ops.mlr_grad_gemm(pd, X)
        gs = ops.mlr_sparse_grad(x.feat_ids, x.feat_ptr, x.feat_row,
                                 x.feat_val, P, F)
        emit(f"max |G_sparse - G_dense| = {float((gs - gd).abs().max()):.3e} "
             f"(max |G| = {float(gd.abs().max()):.3e})")
        emit()
    res = interleaved(cases)
    emit("| variant | median of 5 rounds (min..max) |")
    emit("|---|---|")
    for kk, t in res.items():
        emit(f"| {kk.strip()} | {fmt(t)} |")
    emit()
    if dense:
        d = res["dense phase (parent: mlr_forward + mlr_grad_gemm)"]
        s = res["sparse phase (Wt fill + fwd + softmax + grad)"]
        emit(f"dense / sparse = {d[0] / s[0]:.2f}x; the dense path's own "
             f"run-to-run range is {100 * (d[2] - d[1]) / d[0]:.1f} % of its "
             f"median.")
        emit()
    if sweep:
        sw = {}
        for g in (1, 4, 8, 16, 32, 64):
            sw[f"fwd G={g}"] = (lambda g=g: hip.mlr_sparse_fwd(
                x.row_ptr, x.col, x.val, Wt, C, g))
            sw[f"grad G={g}"] = (lambda g=g: hip.mlr_sparse_grad(
                x.feat_ids, x.feat_ptr, x.feat_row, x.feat_val, Ppad[:, :C],
                F, g))
        r = interleaved(sw)
        emit("Group sweep (kernel alone):")
        emit()
        emit("| lanes | forward | gradient |")
        emit("|---|---|---|")
        for g in (1, 4, 8, 16, 32, 64):
            emit(f"| {g} | {fmt(r[f'fwd G={g}'])} | {fmt(r[f'grad G={g}'])} |")
        emit()
    return res


def crossover(B, F):
    """Density at which the dense phase starts to win at this shape."""
    emit(f"### Crossover at B = {B}, F = {F}")
    emit()
    emit("| non-zeros per row | % dense | dense phase | sparse phase |")
    emit("|---|---|---|---|")
    first = None
    for k in (128, 512, 768, 1024, 1536, 2048, 4096):
        x, y = make_batch(B, F, k, seed=k)
        W = torch.randn(C, F, device="cuda") * 0.01
        Wt = ops.mlr_sparse_wt(W)
        X = x.to_dense()

        def dense_phase():
            p, _l, _c = ops.mlr_forward(X, W, y)
            ops.mlr_grad_gemm(p, X)

        def sparse_phase():
            p, _l, _c = ops.mlr_sparse_forward(x.row_ptr, x.col, x.val, W, y,
                                               Wt_buf=Wt)
            ops.mlr_sparse_grad(x.feat_ids, x.feat_ptr, x.feat_row,
                                x.feat_val, p, F)

        r = interleaved({"d": dense_phase, "s": sparse_phase})
        dens = 100.0 * x.nnz / (B * F)
        emit(f"| {x.nnz / B:.1f} | {dens:.3g} | {fmt(r['d'])} | "
             f"{fmt(r['s'])} |")
        if first is None and r["d"][0] < r["s"][0]:
            first = dens
        del X
    emit()
    emit("dense first wins at "
         + (f"{first:.3g} % dense" if first is not None
            else "no density measured here"))
    emit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--quick", action="store_true",
                    help="small shapes only (a rehearsal of the script)")
    args = ap.parse_args()
    torch.manual_seed(0)
    emit(f"Device: {torch.cuda.get_device_name(0)}; C = {C}; times are "
         f"device-event medians of 20 launches per round.")
    emit()
    if args.quick:
        shape_ab(256, 784, 150, sweep=True)
        crossover(256, 1024)
    else:
        shape_ab(4096, 784, 166, sweep=True)   # the sample's shape, ~19 %
        shape_ab(16384, 16384, 32, sweep=True)
        shape_ab(16384, 16384, 256, sweep=True)
        shape_ab(16384, 2 ** 20, 32, dense=False, sweep=True)
        crossover(16384, 16384)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
