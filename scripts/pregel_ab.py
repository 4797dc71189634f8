"""A/B on one GPU: Pregel supersteps with the fused pull path (K13,
ops.pregel_pull over the static pull index) against the unfused path
(per-edge messages + merge_key_deltas + scatter apply), which is the
engine's default and unchanged.

Synthetic ring+random graph, 2^20 vertices, out-degree 8; PageRank at 20
iterations and SSSP from vertex 0. Each variant is warmed up once, then the
two are timed alternately `--repeats` times; a run is timed with a host
clock around engine.run() ending in a device synchronise, and divided by the
supersteps it ran. Reports median and min..max, checks that both paths
compute the same thing, and writes profiles/pregel_pull_ab.md.

  python scripts/pregel_ab.py [--log2n 20] [--degree 8] [--repeats 7]
"""

import argparse
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from harmony_amd.config import JobConfig, RuntimeConfig  # noqa: E402
from harmony_amd.pregel.engine import PregelEngine  # noqa: E402
from harmony_amd.pregel.graphapps import (  # noqa: E402
    PageRankComputation, ShortestPathComputation,
    make_ring_plus_random_graph)
from harmony_amd.runtime.bootstrap import init_executor  # noqa: E402
from harmony_amd.runtime.control import ControlPlane  # noqa: E402


def make_engine(ctx, app, n, deg, fused, tag):
    comp = (PageRankComputation(num_iters=20) if app == "pagerank"
            else ShortestPathComputation(source=0))
    job = JobConfig(job_id=f"ab_{app}_{tag}", app=app, app_args={})
    engine = PregelEngine(job, comp, n, ctx, ControlPlane(ctx.store, 0, 1),
                          max_supersteps=500, fused=fused)
    graph = make_ring_plus_random_graph(n, deg, 0, n, ctx.device, 4242)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    engine.set_graph(graph)
    torch.cuda.synchronize()
    return engine, time.perf_counter() - t0


def timed_run(engine):
    # run() restarts from superstep 0 semantics: values are re-initialised
    # by the computation at superstep 0 and both message buffers cleared
    engine.cur = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vals = engine.run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt / engine.supersteps_run, engine.supersteps_run, vals


def ab(ctx, app, n, deg, repeats):
    engines = {}
    build = {}
    for name, fused in (("unfused", False), ("fused", True)):
        engines[name], build[name] = make_engine(ctx, app, n, deg, fused,
                                                 name)
    times = {k: [] for k in engines}
    steps = {}
    vals = {}
    for name, e in engines.items():          # warm-up, untimed
        _, steps[name], vals[name] = timed_run(e)
    for _ in range(repeats):                 # alternate the two variants
        for name, e in engines.items():
            t, s, _v = timed_run(e)
            assert s == steps[name]
            times[name].append(t)
    a, b = vals["unfused"].squeeze(1), vals["fused"].squeeze(1)
    if app == "shortestpath":
        same = "bitwise equal" if torch.equal(a, b) else "DIFFERENT"
    else:
        same = f"max |diff| {float((a - b).abs().max()):.3e} " \
               f"(max value {float(a.max()):.3e})"
    rows = []
    for name in ("unfused", "fused"):
        ts = times[name]
        rows.append((name, steps[name], statistics.median(ts) * 1e3,
                     min(ts) * 1e3, max(ts) * 1e3, build[name] * 1e3))
    ratio = rows[0][2] / rows[1][2]
    return rows, ratio, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--degree", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="profiles/pregel_pull_ab.md")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    ctx = init_executor(RuntimeConfig(device="cuda"))
    n = 1 << args.log2n
    lines = [
        "# Pregel pull kernel (K13): fused vs unfused supersteps",
        "",
        f"Device: {torch.cuda.get_device_name(0)}, one GPU. Synthetic "
        f"ring+random graph, {n} vertices, out-degree {args.degree} "
        f"({n * args.degree} edges). Host clock around `engine.run()` "
        "ending in a device synchronise, divided by the supersteps run; "
        f"1 warm-up run, then {args.repeats} runs per variant, alternating. "
        "`set_graph` is the one-time cost of loading the graph into the "
        "engine (for fused: building the pull index) and is not part of "
        "the per-superstep time.",
        "",
        "| app | path | supersteps | ms/superstep median | min | max | "
        "set_graph ms |",
        "|---|---|---|---|---|---|---|",
    ]
    notes = []
    for app in ("pagerank", "shortestpath"):
        rows, ratio, same = ab(ctx, app, n, args.degree, args.repeats)
        for name, s, med, lo, hi, bld in rows:
            lines.append(f"| {app} | {name} | {s} | {med:.3f} | {lo:.3f} | "
                         f"{hi:.3f} | {bld:.1f} |")
        notes.append(f"- {app}: unfused / fused = {ratio:.2f}x "
                     f"(medians); results: {same}.")
    lines += [""] + notes + [
        "",
        "Reproduce: `python scripts/pregel_ab.py`.",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
