"""Isolated A/B of the LDA MH sweep kernel (bench-shaped data)."""

import os
import sys
import time

import torch

sys.path.insert(0, ".")
from harmony_amd import ops  # noqa: E402

hip = ops._load_hip()


def main():
    D, T, K, V = 16384, 128, 256, 100000
    g = torch.Generator().manual_seed(1)
    u = torch.rand(D * T, generator=g)
    w = (u * u * V).long().clamp_(0, V - 1).view(D, T).sort(1).values.reshape(-1)
    uw, wl = torch.unique(w, return_inverse=True)
    R = uw.shape[0]
    wt = torch.zeros(R, K, dtype=torch.int32)
    z = torch.randint(0, K, (D * T,), generator=g, dtype=torch.int32)
    wt.view(-1).scatter_add_(0, wl * K + z.long(),
                             torch.ones(D * T, dtype=torch.int32))
    nk = torch.bincount(z.long(), minlength=K).int()
    dt = torch.zeros(D, K, dtype=torch.int32)
    tok_doc = torch.arange(D).repeat_interleave(T)
    dt.view(-1).scatter_add_(0, tok_doc * K + z.long(),
                             torch.ones(D * T, dtype=torch.int32))
    dev = "cuda"
    wt, nk, dt = wt.to(dev), nk.to(dev), dt.to(dev)
    wl64 = wl.to(dev)
    offs = torch.arange(0, (D + 1) * T, T, dtype=torch.int64, device=dev)
    z = z.to(dev)
    import os as _os

    for bw in ("1", "2", "4", "8"):
        _os.environ["HARMONY_LDA_BUILD_WAVES"] = bw
        for _ in range(2):
            hip.lda_alias_build(wt, nk, 0.01, V)
        torch.cuda.synchronize()
        ts = []
        for _ in range(10):
            t0 = time.perf_counter()
            hip.lda_alias_build(wt, nk, 0.01, V)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        print(f"alias_build waves={bw}: {ts[len(ts)//2]*1e3:.3f} ms")
    _os.environ.pop("HARMONY_LDA_BUILD_WAVES", None)
    tabs = hip.lda_alias_build(wt, nk, 0.01, V)
    prob, alias, tp, ta, qv, qsum, invden = tabs
    torch.cuda.synchronize()
    print(f"uniq words {R}")
    for thr, pf in (("128", "0"), ("128", "1"), ("64", "0"), ("64", "1"),
                    ("256", "1")):
        os.environ["HARMONY_LDA_MH_THREADS"] = thr
        os.environ["HARMONY_LDA_MH_PREFETCH"] = pf
        zz = z.clone()
        dtt = dt.clone()
        for _ in range(3):
            hip.lda_mh(dtt, wt, invden, prob, alias, tp, ta, qv, offs,
                       wl64, zz, 0.1, 0.01, 42)
        torch.cuda.synchronize()
        ts = []
        for i in range(15):
            t0 = time.perf_counter()
            hip.lda_mh(dtt, wt, invden, prob, alias, tp, ta, qv, offs,
                       wl64, zz, 0.1, 0.01, 43 + i)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        print(f"threads={thr} prefetch={pf}: {ts[len(ts)//2]*1e3:.3f} ms")


def _event_median_us(fn, iters=30, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def packed_ab():
    """Wave sampler at the bench shape: legacy arrays vs packed records
    (K7d), fused apply vs the separate lda_apply_all. One LDA step's device
    work per variant, `shard` standing in for the single-owner table. (The
    variant with the counts inside the records, refreshed every step, was
    measured with an earlier form of this function and removed from the
    source: profiles/r04_lda_step.md.)"""
    D, T, K, V = 16384, 128, 256, 100000
    g = torch.Generator().manual_seed(1)
    u = torch.rand(D * T, generator=g)
    w = (u * u * V).long().clamp_(0, V - 1).view(D, T).sort(1).values.reshape(-1)
    uw, wl = torch.unique(w, return_inverse=True)
    R = uw.shape[0]
    z0 = torch.randint(0, K, (D * T,), generator=g, dtype=torch.int32)
    ones = torch.ones(D * T, dtype=torch.int32)
    shard0 = torch.zeros(V + 1, K, dtype=torch.int32)
    shard0.view(-1).scatter_add_(0, w * K + z0.long(), ones)
    shard0[V] = torch.bincount(z0.long(), minlength=K).int()
    dt0 = torch.zeros(D, K, dtype=torch.int32)
    dt0.view(-1).scatter_add_(
        0, torch.arange(D).repeat_interleave(T) * K + z0.long(), ones)
    dev = "cuda"
    offs = torch.arange(0, (D + 1) * T, T, dtype=torch.int64, device=dev)
    wl64, wl32 = wl.to(dev), wl.to(dev).to(torch.int32)
    rows64 = uw.to(dev)                       # word id == shard row here
    rows32 = rows64.to(torch.int32)
    word_rows = w.to(dev)
    print(f"packed A/B: {D} docs x {T} tokens, K={K}, {R} unique words")

    st = {}

    def reset():
        st["shard"] = shard0.to(dev)
        st["z"] = z0.to(dev)
        st["dt"] = dt0.to(dev)
        st["seed"] = 100

    def seed():
        st["seed"] += 1
        return st["seed"]

    res = {}
    reset()
    wt = st["shard"][rows64]
    res["build legacy (dense input)"] = _event_median_us(
        lambda: hip.lda_alias_build(wt, st["shard"][V], 0.01, V), 10)
    rec, top = ops.lda_packed_alloc(R, K, dev)
    res["build packed (shard in place)"] = _event_median_us(
        lambda: ops.lda_alias_build_packed(st["shard"], rows32,
                                           st["shard"][V], 0.01, V, rec, top),
        10)
    prob, alias, tp, ta, qv, _, invden = hip.lda_alias_build(
        wt, st["shard"][V], 0.01, V)
    res["piece: torch gather shard[rows]"] = _event_median_us(
        lambda: st["shard"][rows64])
    res["piece: z.clone()"] = _event_median_us(lambda: st["z"].clone())

    def legacy():
        pulled = st["shard"][rows64]
        old = st["z"].clone()
        hip.lda_mh_wave(st["dt"], pulled, invden, prob, alias, tp, ta, qv,
                        offs, wl64, st["z"], 0.1, 0.01, seed())
        hip.lda_apply_all(st["shard"], word_rows, old, st["z"], V)

    def legacy_sampler_only():
        hip.lda_mh_wave(st["dt"], wt, invden, prob, alias, tp, ta, qv,
                        offs, wl64, st["z"], 0.1, 0.01, seed())

    def packed(fused):
        def step():
            pulled = st["shard"][rows64]
            if fused:
                ops.lda_mh_wave_packed(
                    st["dt"], pulled, rec, top, invden, offs, wl32, st["z"],
                    0.1, 0.01, seed(), shard=st["shard"],
                    row_of_local=rows32, summary_row=V)
            else:
                old = st["z"].clone()
                ops.lda_mh_wave_packed(
                    st["dt"], pulled, rec, top, invden, offs, wl32, st["z"],
                    0.1, 0.01, seed())
                hip.lda_apply_all(st["shard"], word_rows, old, st["z"], V)
        return step

    def packed_sampler_only(fused):
        def step():
            kw = (dict(shard=st["shard"], row_of_local=rows32, summary_row=V)
                  if fused else {})
            ops.lda_mh_wave_packed(st["dt"], wt, rec, top, invden, offs,
                                   wl32, st["z"], 0.1, 0.01, seed(), **kw)
        return step

    cases = [("step legacy: gather+clone+mh_wave+apply_all", legacy),
             ("sampler only: legacy mh_wave", legacy_sampler_only)]
    for fused in (False, True):
        tag = "fused apply" if fused else "separate apply"
        cases.append((f"step packed: {tag}", packed(fused)))
        cases.append((f"sampler only packed: {tag}",
                      packed_sampler_only(fused)))
    for rnd in range(2):                      # two interleaved rounds
        for name, fn in cases:
            reset()
            res[f"{name} [round {rnd}]"] = _event_median_us(fn)
    for k, v in res.items():
        print(f"{k}: {v:.1f} us")


if __name__ == "__main__":
    if "--packed" in sys.argv:
        packed_ab()
    else:
        main()
