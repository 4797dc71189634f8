"""A/B of gbt.build_tree on MI355X: this tree's mlapps/gbt.py and
sparse_bins.py against another commit's copies of the two files, loaded from
a directory into the same process and run interleaved, plus that commit
against a second load of itself for the run-to-run spread.

  mkdir /tmp/parent
  git show REV:harmony_amd/mlapps/gbt.py > /tmp/parent/gbt.py
  git show REV:harmony_amd/mlapps/sparse_bins.py > /tmp/parent/sparse_bins.py
  python scripts/gbt_builder_ab.py --parent /tmp/parent \
      [--out profiles/gbt_one_builder.md]
"""

import argparse
import importlib.util
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from harmony_amd import ops  # noqa: E402
from harmony_amd.mlapps import gbt as new_gbt  # noqa: E402
from harmony_amd.mlapps import sparse_bins as new_sb  # noqa: E402

ROUNDS, ITERS, WARMUP = 5, 10, 2
OUT = []


def emit(line=""):
    print(line, flush=True)
    OUT.append(line)


def load_parent(directory, tag):
    mods = {}
    for name in ("sparse_bins", "gbt"):
        spec = importlib.util.spec_from_file_location(
            f"parent_{tag}_{name}", Path(directory) / f"{name}.py")
        m = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = m
        spec.loader.exec_module(m)
        mods[name] = m
    mods["gbt"].SparseBins = mods["sparse_bins"].SparseBins
    return mods["gbt"], mods["sparse_bins"]


def bench_host(fn):
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(ITERS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True,
                    help="directory with the other commit's gbt.py and "
                         "sparse_bins.py")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert ops._load_hip() is not None and torch.cuda.is_available()
    variants = {"parent": load_parent(args.parent, "a"),
                "new": (new_gbt, new_sb),
                "parent2": load_parent(args.parent, "b")}
    emit("# build_tree with one level loop against the parent commit's "
         "three builders")
    emit()
    emit(f"Device: {torch.cuda.get_device_name(0)}. Host time of one "
         f"build_tree call in microseconds, device synchronised before and "
         f"after; {ITERS} timed calls after {WARMUP} warm-ups per round, "
         f"{ROUNDS} rounds, the three variants interleaved inside every "
         f"round (parent, new, parent again from a second load of the same "
         f"files). Each figure is the median over rounds of the per-round "
         f"median, with min..max over rounds. B = 16384, nb = 64, lam = 1. "
         f"spread = largest |parent2 - parent| of one round. The sparse "
         f"input has about 8 (F = 32) and 31 (F = 784) entries per row and "
         f"no feature types. Measured by scripts/gbt_builder_ab.py.")
    emit()
    emit("| input | F | depth | parent | new | parent again | new - parent "
         "| spread | new / parent |")
    emit("|---|---|---|---|---|---|---|---|---|")
    worst = None
    B, nb = 16384, 64
    for F in (32, 784):
        g = torch.Generator().manual_seed(F)
        bins = torch.randint(0, nb, (B, F), generator=g)
        resid = torch.randn(B, generator=g).cuda()
        zero = torch.zeros(F, dtype=torch.int32, device="cuda")
        # about 8 (F = 32) and 32 (F = 784) entries per row
        X = torch.randn(B, F, generator=g)
        mask = torch.rand(B, F, generator=g) < (0.25 if F == 32 else 0.04)
        row_ptr = torch.zeros(B + 1, dtype=torch.int64)
        row_ptr[1:] = torch.cumsum(mask.sum(dim=1), 0)
        rows, cols = mask.nonzero(as_tuple=True)
        csr = (row_ptr, cols.to(torch.int32), X[rows, cols], F)
        inputs = {}
        for v, (_gbt, sb) in variants.items():
            inputs[v] = {"dense untyped": (bins.cuda(), None),
                         "dense typed": (bins.cuda(), zero),
                         "sparse": (sb.SparseBins(csr, nb).to("cuda"), None)}
        for kind in ("dense untyped", "dense typed", "sparse"):
            for depth in (1, 4, 6):
                res = {v: [] for v in variants}
                for _ in range(ROUNDS):
                    for v, (gmod, _sb) in variants.items():
                        x, ft = inputs[v][kind]
                        res[v].append(bench_host(
                            lambda: gmod.build_tree(x, resid, nb, depth, 1.0,
                                                    ft)))
                med = {v: statistics.median(t) for v, t in res.items()}
                spread = max(abs(a - b) for a, b in zip(res["parent"],
                                                        res["parent2"]))
                delta = med["new"] - med["parent"]

                def fmt(v):
                    return (f"{med[v]:.0f} ({min(res[v]):.0f}.."
                            f"{max(res[v]):.0f})")
                emit(f"| {kind} | {F} | {depth} | {fmt('parent')} | "
                     f"{fmt('new')} | {fmt('parent2')} | {delta:+.0f} | "
                     f"{spread:.0f} | {med['new'] / med['parent']:.3f} |")
                row = (delta - spread, kind, F, depth, delta, spread,
                       med["new"] / med["parent"])
                if worst is None or row[0] > worst[0]:
                    worst = row
    emit()
    _, kind, F, depth, delta, spread, ratio = worst
    emit(f"Worst row (largest new - parent beyond the spread): {kind}, "
         f"F = {F}, depth {depth}: {delta:+.0f} us against a spread of "
         f"{spread:.0f} us, new / parent = {ratio:.3f}.")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
