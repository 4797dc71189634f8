#!/usr/bin/env python3
"""K7e (ops.lda_foldin) at the bench's LDA shape: kernel time with one and
with two pairs in flight, the tensor-op path on the same device, and the
achieved bytes/s against the byte model. Feeds profiles/lda_foldin_ab.md.

  python scripts/lda_foldin_ab.py [--docs 16384] [--tokens 128]
        [--vocabs 100000] [--iters 20] [--reps 15] [--out FILE.json]

Held-out documents are drawn like the synthetic training batches of
mlapps/lda.py (a squared uniform over the vocabulary), the table is a
random count table of the density a trained one has. Times are device
events around one call, median of --reps after 3 warm calls; the variants
alternate inside one repetition. Needs a GPU: it does not fall back."""

import argparse
import json
import os
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

from harmony_amd import ops  # noqa: E402


def make_inputs(D, T, V, K, device):
    g = torch.Generator().manual_seed(1234 + K)
    u = torch.rand(D, T, generator=g)
    words = (u * u * V).long().clamp_(0, V - 1)
    docs = torch.arange(D).unsqueeze(1).expand(D, T)
    pos = torch.arange(T).unsqueeze(0).expand(D, T)
    pairs = []
    for first in (0, 1):
        sel = pos % 2 == first
        key, cnt = torch.unique(docs[sel] * V + words[sel],
                                return_counts=True)
        ptr = torch.zeros(D + 1, dtype=torch.int64)
        ptr[1:] = torch.bincount(key // V, minlength=D).cumsum(0)
        pairs += [ptr.to(device), (key % V).to(device),
                  cnt.to(torch.int32).to(device)]
    table = torch.randint(0, 40, (V + 1, K), generator=g, dtype=torch.int32)
    table *= (torch.rand(V + 1, K, generator=g) < 0.1).to(torch.int32)
    table[V] = table[:V].sum(dim=0)
    return table.to(device), pairs


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=16384)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--vocabs", type=int, default=100000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--topics", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.hip_available(), "needs a GPU"
    dev = torch.device("cuda")
    V, I = args.vocabs, args.iters
    results = []
    for K in args.topics:
        table, pairs = make_inputs(args.docs, args.tokens, V, K, dev)
        wt, nk = table[:V], table[V].contiguous()
        n_obs, n_sc = pairs[1].shape[0], pairs[4].shape[0]
        row_bytes = (I * n_obs + n_sc) * K * 4
        token_bytes = (I + 1) * args.docs * args.tokens * K * 4

        def kernel():
            return ops._hip.lda_foldin(wt, nk, *pairs, 0.1, 0.01, V, I)

        def torch_path():
            os.environ["HARMONY_FORCE_TORCH_OPS"] = "1"
            try:
                return ops.lda_foldin(wt, nk, *pairs, 0.1, 0.01, V, I)
            finally:
                del os.environ["HARMONY_FORCE_TORCH_OPS"]

        times = {"pf1": [], "pf2": []}
        outs = {}
        for pf in ("1", "2"):                 # warm both, keep the outputs
            os.environ["HARMONY_LDA_FOLDIN_PF"] = pf
            outs[pf] = kernel()
            timed(kernel, 0)
        for _ in range(args.reps):            # alternate the variants
            for pf in ("1", "2"):
                os.environ["HARMONY_LDA_FOLDIN_PF"] = pf
                times["pf" + pf] += timed(kernel, 1, warm=0)
        del os.environ["HARMONY_LDA_FOLDIN_PF"]
        same = all(torch.equal(a, b) for a, b in zip(outs["1"], outs["2"]))
        t_torch = timed(torch_path, 3, warm=1)
        ref = torch_path()
        rel = float(((outs["1"][1] - ref[1]).abs() / ref[1].abs()).max())
        row = {"K": K, "docs": args.docs, "tokens": args.tokens, "V": V,
               "iters": I, "obs_pairs": n_obs, "scored_pairs": n_sc,
               "row_bytes": row_bytes, "token_model_bytes": token_bytes,
               "pf1_equals_pf2": same, "ll_max_rel_vs_torch": rel,
               "torch_ms": statistics.median(t_torch)}
        for name, ts in times.items():
            med = statistics.median(ts)
            row[name + "_ms"] = med
            row[name + "_ms_min_max"] = [min(ts), max(ts)]
            row[name + "_TBps"] = row_bytes / (med * 1e-3) / 1e12
        results.append(row)
        print(json.dumps(row), flush=True)
        del table, wt, nk, pairs, outs, ref
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
