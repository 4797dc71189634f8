"""Isolated A/B of the sparse Lasso sweep above K11s's row limit, on MI355X,
at B = 16384, 32768 and the limit of K11sL, for F = 2^20 with 8 and 32
non-zeros per row (short columns) and F = 4096 with 32 (columns of a few
hundred entries). Three designs on the same seeded inputs:

  (a) the tensor-op loop, which is what ops.lasso_cd_sparse ran at these row
      counts before K11sL. Measured from a checkout of that commit:
        cd <checkout> && python <here>/scripts/lasso_sparse_large_ab.py \
            --loop-out loop.json
      (only the public wrapper is used, so the script runs there as it is);
  (b) K11sL with every window dirty: the sequential design at this row count;
  (c) K11sL with the table of ops.lasso_sparse_windows.

  python scripts/lasso_sparse_large_ab.py --loop loop.json \
      [--out profiles/lasso_sparse_large_ab.md]

(b) and (c) are interleaved round by round; each figure is the median over
rounds of a per-round median device time, with the min..max over rounds.
"""

import argparse
import json
import statistics
import time

import torch

from lasso_sparse_ab import OUT, emit, fmt, interleaved, make_batch

from harmony_amd import ops  # noqa: E402
from harmony_amd.mlapps import lasso  # noqa: E402

LIMIT = 40928
SHAPES = [(B, F, k) for F, k in ((2 ** 20, 8), (2 ** 20, 32), (4096, 32))
          for B in (16384, 32768, LIMIT)]
# between the two regimes, for the thread rule; (a) is not measured here
SHAPES += [(32768, 2 ** 16, 32), (32768, 2 ** 14, 32)]
SOLO_LENS = (64, 256, 1024)


def inputs(B, F, k):
    x, y = make_batch(B, F, k, seed=B + F + k)
    nnz, nf = x.nnz, x.feat_ids.shape[0]
    # the threshold shrinks a weight by lam_n / col_sq: 0.1 at the mean column
    lam_n = 0.1 * nnz / nf
    # a model in mid-training: a quarter of the weights set
    g = torch.Generator(device="cuda").manual_seed(B + F + k + 1)
    w = torch.randn(F, generator=g, device="cuda") * (
        torch.rand(F, generator=g, device="cuda") < 0.25)
    return x, y, w, lam_n, lasso._sparse_col_sq(x)


def loop_times(path):
    """(a): wall time of whole calls, each ended by a synchronise; as many
    calls as fit in 10 s, three at the most."""
    res = {}
    for B, F, k in SHAPES[:9]:
        x, y, w, lam_n, col_sq = inputs(B, F, k)
        ts = []
        while len(ts) < 3 and sum(ts) < 10:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.lasso_cd_sparse(x.feat_ids, x.feat_ptr, x.feat_row,
                                x.feat_val, y, w, col_sq, lam_n)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        res[f"{B},{F},{k}"] = (statistics.median(ts) * 1e6, len(ts))
        print(B, F, k, res[f"{B},{F},{k}"], flush=True)
    with open(path, "w") as f:
        json.dump(res, f)


def shape_ab(B, F, k, loop):
    hip = ops._load_hip()
    x, y, w, lam_n, col_sq = inputs(B, F, k)
    nnz, nf = x.nnz, x.feat_ids.shape[0]
    idx = (x.feat_ids, x.feat_ptr, x.feat_row, x.feat_val)
    r = torch.empty_like(y)

    def sweep(threads, table):
        wn = w.clone()
        hip.lasso_cd_sparse(*idx, y, wn, col_sq, lam_n, r, threads, table)
        return wn

    # no column of the wide shapes comes near any of the limits
    solos = SOLO_LENS if nnz / nf > 8 else (ops.LASSO_SPARSE_SOLO_LEN,)
    tables = {(t, s): ops.lasso_sparse_windows(x.feat_ptr, x.feat_row,
                                               t // 64, s)
              for t in (256, 1024) for s in solos}
    pick = ops.lasso_sparse_large_threads(nf, nnz)
    emit(f"### B = {B}, F = {F}, {k} per row: mean column length "
         f"{nnz / nf:.1f}")
    emit()
    w_seq = sweep(64, None)
    diff = max(float((sweep(t, tab) - w_seq).abs().max())
               for (t, _s), tab in tables.items())
    emit(f"nnz {nnz}, present features {nf}, longest column "
         f"{int((x.feat_ptr[1:] - x.feat_ptr[:-1]).max())}, lam_n "
         f"{lam_n:.3g}; the sweep starts from {int((w != 0).sum())} non-zero "
         f"weights and moves {int((w_seq != w).sum())}. Largest weight "
         f"difference between any (c) and the 64-thread sequential sweep: "
         f"{diff:.2e}. Thread rule: {pick}.")
    emit()
    cases = {"(b) all dirty, 64 threads": lambda: sweep(64, None)}
    for t in (256, 1024):
        cases[f"(b) all dirty, {t} threads"] = lambda t=t: sweep(t, None)
    for (t, s), tab in tables.items():
        share = float(tab.float().mean())
        cases[f"(c) table, {t} threads, solo_len {s}: "
              f"{100 * share:.1f} % of windows clean"] = (
            lambda t=t, tab=tab: sweep(t, tab))
    res = interleaved(cases, iters=3, warmup=1, rounds=3)
    emit("| sweep | time, median (min..max over rounds) |")
    emit("|---|---|")
    a, n = loop.get(f"{B},{F},{k}", (None, 0))
    if a:
        emit(f"| (a) tensor-op loop at the parent commit (wall time of "
             f"{n} call{'s' if n > 1 else ''}, median) | {a:10.1f} us |")
    for name, t in res.items():
        emit(f"| {name} | {fmt(t)} |")
    c = res[next(n for n in res if n.startswith(
        f"(c) table, {pick} threads, solo_len {ops.LASSO_SPARSE_SOLO_LEN}:"))]
    b = min(v[0] for n, v in res.items() if n.startswith("(b)"))
    emit()
    emit(f"(c) at the rule's {pick} threads and solo_len "
         f"{ops.LASSO_SPARSE_SOLO_LEN}: "
         + (f"{a / c[0]:.0f}x faster than (a), " if a else "")
         + f"{b / c[0]:.2f}x the speed of the fastest (b).")
    emit()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop-out", help="measure (a) only and write it here")
    ap.add_argument("--loop", help="the file --loop-out wrote")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.loop_out:
        return loop_times(args.loop_out)
    assert ops.LASSO_SPARSE_MAX_ROWS == LIMIT
    with open(args.loop) as f:
        loop = json.load(f)
    emit(f"Device: {torch.cuda.get_device_name(0)}; (b), (c): device-event "
         f"times of one binding call (clone of w + one launch), 3 interleaved "
         f"rounds of 3 timed calls after 1 warm-up call.")
    emit()
    for shape in SHAPES:
        shape_ab(*shape, loop)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
