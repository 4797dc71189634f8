"""Isolated A/B of NMF gradient variants + LDA sampler timing on MI355X."""

import sys
import time

import torch

sys.path.insert(0, ".")
from harmony_amd import ops  # noqa: E402

hip = ops._load_hip()
assert hip is not None


def bench(fn, iters=20, warmup=4):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e3


def bench_dev(fn, iters=20, warmup=4):
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
    ts.sort()
    return ts[len(ts) // 2]


def nmf_step_ab(L, R, uniq, m, row_ptr, col_g, col, vals, perm, seg_ptr,
                row_sorted):
    """Whole compute phase (gradient + L update), legacy composition against
    ops.nmf_step, R gathered ([n_uniq, k], local ids) or
    indexed (the whole table, global ids). Row bytes: each pass gathers
    nnz rows of 4*k bytes; TB/s is both passes' row bytes over the time."""
    n, k = L.shape
    nnz = col.shape[0]
    row_bytes = 2 * nnz * 4 * k
    step_t = torch.tensor(0.01, device="cuda")
    table = torch.rand(m, k, device="cuda")
    table[uniq] = R
    i32 = torch.int32
    cs32 = (perm.to(i32), seg_ptr.to(i32), row_sorted.to(i32))
    row_ptr32, col32, col_g32, uniq32 = (row_ptr.to(i32), col.to(i32),
                                         col_g.to(i32), uniq.to(i32))
    Lw = L.clone()

    def legacy():
        lg, rg, sq = hip.nmf_grad_twopass(L, R, row_ptr, col, vals, perm,
                                          seg_ptr, row_sorted, 0.0)
        Lw[:] = (L - step_t * lg).clamp_(0.0, 1e6)

    def legacy_with_gathers():
        Rg = table[uniq]
        Lb = L[l_rows]
        lg, rg, sq = hip.nmf_grad_twopass(Lb, Rg, row_ptr, col, vals, perm,
                                          seg_ptr, row_sorted, 0.0)
        Lw[l_rows] = (Lb - step_t * lg).clamp_(0.0, 1e6)

    l_rows = torch.arange(n, device="cuda")
    cases = {"legacy twopass + torch L chain": legacy,
             "legacy incl. R and L gathers": legacy_with_gathers}
    if hasattr(hip, "nmf_step"):
        def gathered():
            Ln, rg, sq = hip.nmf_step(L, 0, n, R, row_ptr32, col32, vals,
                                      *cs32, None, step_t, 0.0, 1e6,
                                      False)
            Lw.copy_(Ln)

        def gathered_with_gather():
            Ln, rg, sq = hip.nmf_step(L, 0, n, table[uniq], row_ptr32,
                                      col32, vals, *cs32, None, step_t,
                                      0.0, 1e6, False)
            Lw.copy_(Ln)

        def indexed():
            Ln, rg, sq = hip.nmf_step(L, 0, n, table, row_ptr32, col_g32,
                                      vals, *cs32, uniq32, step_t, 0.0,
                                      1e6, False)
            Lw.copy_(Ln)

        cases["nmf_step gathered R"] = gathered
        cases["nmf_step gathered R incl. gather"] = \
            gathered_with_gather
        cases["nmf_step indexed R"] = indexed
    res = {kk: [] for kk in cases}
    for _ in range(3):
        for kk, fn in cases.items():
            res[kk].append(bench_dev(fn))
    print(f"row bytes per compute phase: {row_bytes / 1e6:.0f} MB")
    for kk, tt in res.items():
        t = min(tt)
        print(f"{kk:42s} {t * 1e3:8.1f} us  {row_bytes / t / 1e9:6.2f} TB/s "
              f"(runs: {[f'{x * 1e3:.0f}' for x in tt]})")


def scatter_apply_ab():
    """Owner-side nmf_sgd apply at the bench shape: 65536 rows x 100."""
    n, vd = 65536, 100
    shard = torch.rand(n, vd, device="cuda")
    rows = torch.randperm(n, device="cuda")
    deltas = torch.randn(n, vd, device="cuda")
    moved = 3 * n * vd * 4 + n * 8       # read shard+delta, write shard, rows
    tt = [bench_dev(lambda: hip.scatter_apply(shard, rows, deltas, 2, 0.01,
                                              1e6)) for _ in range(3)]
    t = min(tt)
    print(f"scatter_apply 65536x100 (this build)       {t * 1e3:8.1f} us  "
          f"{moved / 1e6:.0f} MB  {moved / t / 1e9:6.2f} TB/s")


def main():
    torch.manual_seed(0)
    # bench default shapes: 16384 rows x 128 nnz, rank 100, 65536 cols
    n, k, nnz_per_row, m = 16384, 100, 128, 65536
    nnz = n * nnz_per_row
    L = torch.rand(n, k, device="cuda")
    row_ptr = torch.arange(0, nnz + 1, nnz_per_row, device="cuda")
    col_g = torch.randint(0, m, (nnz,), device="cuda")
    uniq, col = torch.unique(col_g, return_inverse=True)
    R = torch.rand(uniq.shape[0], k, device="cuda")
    vals = torch.rand(nnz, device="cuda")
    perm = torch.argsort(col, stable=True)
    counts = torch.bincount(col, minlength=uniq.shape[0])
    seg_ptr = torch.zeros(uniq.shape[0] + 1, dtype=torch.int64, device="cuda")
    seg_ptr[1:] = counts.cumsum(0)
    row_of = torch.repeat_interleave(torch.arange(n, device="cuda"),
                                     row_ptr[1:] - row_ptr[:-1])
    row_sorted = row_of[perm]

    print("nnz:", nnz, "uniq cols:", uniq.shape[0])
    variants = {
        "nmf_onepass_atomic": lambda: hip.nmf_grad(L, R, row_ptr, col, vals, 0.0),
        "nmf_twopass": lambda: hip.nmf_grad_twopass(
            L, R, row_ptr, col, vals, perm, seg_ptr, row_sorted, 0.0),
    }
    nmf_step_ab(L, R, uniq, m, row_ptr, col_g, col, vals, perm, seg_ptr,
                row_sorted)
    scatter_apply_ab()
    if "--step-only" in sys.argv:
        return
    # LDA: bench default 8192 docs x 128 tokens, K=256, V=100k, Zipf sorted
    D, T, K, V = 8192, 128, 256, 100000
    g = torch.Generator().manual_seed(1)
    u = torch.rand(D * T, generator=g)
    w = (u * u * V).long().clamp_(0, V - 1).view(D, T).sort(dim=1).values.reshape(-1)
    uw, wl = torch.unique(w, return_inverse=True)
    wl = wl.cuda()
    z = torch.randint(0, K, (D * T,), dtype=torch.int32).cuda()
    offs = torch.arange(0, (D + 1) * T, T, device="cuda")
    dt = torch.zeros(D, K, dtype=torch.int32, device="cuda")
    dt.view(-1).scatter_add_(0, (torch.arange(D, device="cuda")
                                 .repeat_interleave(T) * K + z.long()),
                             torch.ones(D * T, dtype=torch.int32, device="cuda"))
    wt = torch.zeros(uw.shape[0], K, dtype=torch.int32, device="cuda")
    wt.view(-1).scatter_add_(0, wl * K + z.long(),
                             torch.ones(D * T, dtype=torch.int32, device="cuda"))
    ts_sum = wt.sum(0).to(torch.int32)
    variants["lda_gibbs_sorted"] = lambda: hip.lda_gibbs(
        dt, wt, ts_sum, offs, wl, z, 0.1, 0.01, V, 42)
    # unsorted tokens for comparison (cache-locality delta)
    w2 = (u * u * V).long().clamp_(0, V - 1)
    uw2, wl2 = torch.unique(w2, return_inverse=True)
    wl2 = wl2.cuda()
    z2 = z.clone()
    wt2 = torch.zeros(uw2.shape[0], K, dtype=torch.int32, device="cuda")
    wt2.view(-1).scatter_add_(0, wl2 * K + z2.long(),
                              torch.ones(D * T, dtype=torch.int32, device="cuda"))
    variants["lda_gibbs_unsorted"] = lambda: hip.lda_gibbs(
        dt, wt2, ts_sum, offs, wl2, z2, 0.1, 0.01, V, 42)

    rounds = {kk: [] for kk in variants}
    for r in range(3):
        for kk, fn in variants.items():
            rounds[kk].append(bench(fn))
    for kk, tt in rounds.items():
        print(f"{kk:22s} {min(tt):8.3f} ms (runs: {[f'{t:.3f}' for t in tt]})")


if __name__ == "__main__":
    main()
