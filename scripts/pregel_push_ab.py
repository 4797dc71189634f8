"""A/B on one GPU: Pregel push (K13p, ops.pregel_push along the out-edges of
the sending vertices) against pull (K13, ops.pregel_pull over every in-edge),
at the op level and through whole SSSP / connected-components jobs, and the
two numbers the engine takes from it: the default push_threshold and the
runner's default -direction.

  python scripts/pregel_push_ab.py            # everything, writes the profile

The driver runs every GPU step as a child process under its own `timeout`
and stops at the first one that fails; a step writes its figures as JSON and
the driver assembles profiles/pregel_push_ab.md from them.

Steps (also runnable alone with --step NAME --json FILE):
  op8, op64    pregel_pull against pregel_push on the ring+random graph at
               2^20 x 8 and 2^20 x 64, frontier shares 2^-14 .. 1 of the
               edges (a random vertex subset), plus one row where the same
               share is a single hub
  job_*        SSSP and CC, pull against auto, on 2^20 x 8, 2^20 x 64 and a
               1024 x 1024 four-neighbour grid
  sync         SSSP on 4096 x 8, auto against pull: what the host read of
               the direction choice costs

Timing: one warm-up, then `--repeats` (7) alternated runs per variant. Op
level: host clock around 10 back-to-back calls ending in a device
synchronise, divided by 10 (so launch overhead counts as it does in the
engine). Job level: host clock around engine.run() ending in a device
synchronise.
"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

sys.path.insert(0, ".")
from harmony_amd import ops  # noqa: E402
from harmony_amd.config import JobConfig, RuntimeConfig  # noqa: E402
from harmony_amd.ops.rng import rng_u32  # noqa: E402
from harmony_amd.pregel.engine import LocalGraph, PregelEngine  # noqa: E402
from harmony_amd.pregel.graphapps import (  # noqa: E402
    ConnectedComponentsComputation, ShortestPathComputation)
from harmony_amd.runtime.bootstrap import init_executor  # noqa: E402
from harmony_amd.runtime.control import ControlPlane  # noqa: E402

SEED = 4242
LOG2N = 20
SHARES_LOG2 = list(range(-14, 1))
HUB_SHARE_LOG2 = -6
CALLS = 10


# ------------------------------------------------------------------ graphs

def ring_random_edges(n, deg, device):
    """graphapps.make_ring_plus_random_graph's edge list (same formula, same
    graph), generated on the device: (src, dst) int64, sources ascending."""
    vs = torch.arange(n, dtype=torch.int64, device=device)
    ring = (vs + 1) % n
    ctr = (vs.unsqueeze(1) * (deg - 1)
           + torch.arange(deg - 1, dtype=torch.int64, device=device))
    extra = rng_u32(SEED & 0xFFFFFFFF, ctr.reshape(-1)) % n
    dst = torch.cat([ring.unsqueeze(1), extra.view(n, deg - 1)],
                    dim=1).reshape(-1)
    return vs.repeat_interleave(deg), dst


def grid_edges(side, device):
    """side x side four-neighbour grid, both directions of every link."""
    idx = torch.arange(side * side, dtype=torch.int64,
                       device=device).view(side, side)
    a = torch.cat([idx[:, :-1].reshape(-1), idx[:-1, :].reshape(-1)])
    b = torch.cat([idx[:, 1:].reshape(-1), idx[1:, :].reshape(-1)])
    return torch.cat([a, b]), torch.cat([b, a])


def graph_from_edges(src, dst, n):
    """LocalGraph of the whole graph on one rank; edges grouped by source,
    each source's edges in list order."""
    order = torch.argsort(src, stable=True)
    row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=src.device)
    row_ptr[1:] = torch.cumsum(torch.bincount(src, minlength=n), 0)
    return LocalGraph(vertex_lo=0, row_ptr=row_ptr,
                      edge_dst=dst[order].contiguous(),
                      out_degree=(row_ptr[1:] - row_ptr[:-1]).float(),
                      num_vertices_global=n)


def make_edges(name, device):
    if name == "grid":
        src, dst = grid_edges(1024, device)
        return src, dst, 1024 * 1024
    deg = {"r8": 8, "r64": 64}[name]
    src, dst = ring_random_edges(1 << LOG2N, deg, device)
    return src, dst, 1 << LOG2N


def make_engine(ctx, app, name, direction, threshold, tag,
                max_supersteps=5000):
    src, dst, n = make_edges(name, ctx.device)
    if app == "cc":
        comp = ConnectedComponentsComputation(n)
        if name != "grid":                  # the grid is symmetric already
            src, dst = torch.cat([src, dst]), torch.cat([dst, src])
    else:
        comp = ShortestPathComputation(source=0)
    job = JobConfig(job_id=f"pab_{app}_{name}_{tag}", app=app, app_args={})
    engine = PregelEngine(job, comp, n, ctx, ControlPlane(ctx.store, 0, 1),
                          max_supersteps=max_supersteps, fused=True,
                          direction=direction, push_threshold=threshold)
    engine.set_graph(graph_from_edges(src, dst, n))
    return engine


# ---------------------------------------------------------------- op level

def time_calls(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / CALLS


def alternate(fns, repeats):
    """{name: fn} -> {name: [seconds per call] * repeats}, one warm-up each."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(time_calls(fn))
    return times


def step_op(name, repeats):
    ctx = init_executor(RuntimeConfig(device="cuda"))
    dev = ctx.device
    engine = make_engine(ctx, "sssp", name, "auto", 0.0, "op")
    pull, push = engine.pull, engine.push
    n, n_edges = pull.n_local, int(push.out_row.shape[0])
    g = torch.Generator().manual_seed(7)
    vm = (torch.rand(n, generator=g) * 16.0).to(dev)
    perm = torch.randperm(n, generator=g)
    everyone = torch.arange(n, dtype=torch.int32, device=dev)
    rows = []
    for lg in SHARES_LOG2:
        nf = max(1, int(n * 2.0 ** lg))
        frontier = torch.sort(perm[:nf]).values.to(dev, torch.int32)
        mask = torch.zeros(n, dtype=torch.bool, device=dev)
        mask[frontier.long()] = True
        edges = nf * (n_edges // n)

        def do_pull():
            return ops.pregel_pull(pull.in_ptr, pull.in_src, pull.in_w, 1.0,
                                   vm, mask, "min", True)

        def do_push():
            return ops.pregel_push(push.out_ptr, push.out_row, push.out_w,
                                   1.0, vm, frontier, pull.num_rows, "min",
                                   True, _edges_hint=edges)

        def do_push_mask():      # the engine's form: no compaction
            return ops.pregel_push(push.out_ptr, push.out_row, push.out_w,
                                   1.0, vm, everyone, pull.num_rows, "min",
                                   True, send_mask=mask, _edges_hint=edges)

        a, b, c = do_pull(), do_push(), do_push_mask()
        same = all(torch.equal(a[i], x[i]) for x in (b, c) for i in (0, 1))
        t = alternate({"pull": do_pull, "push": do_push,
                       "pushm": do_push_mask}, repeats)
        rows.append(dict(share_log2=lg, nf=nf, edges=edges, equal=same,
                         pull_ms=statistics.median(t["pull"]) * 1e3,
                         push_ms=statistics.median(t["push"]) * 1e3,
                         pushm_ms=statistics.median(t["pushm"]) * 1e3))
        print(rows[-1], flush=True)
    # the same share as one hub: vertex 0 owns the first h edges of the
    # list, every other vertex none (the rows stay those of the graph)
    h = int(n_edges * 2.0 ** HUB_SHARE_LOG2)
    hub_ptr = torch.full((n + 1,), h, dtype=torch.int64, device=dev)
    hub_ptr[0] = 0
    hub_front = torch.zeros(1, dtype=torch.int32, device=dev)

    def do_hub():
        return ops.pregel_push(hub_ptr, push.out_row, push.out_w, 1.0, vm,
                               hub_front, pull.num_rows, "min", True,
                               _edges_hint=h)

    t = alternate({"hub": do_hub}, repeats)
    hub = dict(share_log2=HUB_SHARE_LOG2, edges=h,
               push_ms=statistics.median(t["hub"]) * 1e3)
    print(hub, flush=True)
    return dict(graph=name, n=n, edges=n_edges, rows=rows, hub=hub,
                device=torch.cuda.get_device_name(0))


# --------------------------------------------------------------- job level

def timed_run(engine):
    engine.cur = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vals = engine.run()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, vals


def ab_jobs(ctx, app, name, threshold, repeats):
    engines = {d: make_engine(ctx, app, name, d, threshold, d)
               for d in ("pull", "auto")}
    vals, times = {}, {d: [] for d in engines}
    for d, e in engines.items():
        _t, vals[d] = timed_run(e)
    for _ in range(repeats):
        for d, e in engines.items():
            times[d].append(timed_run(e)[0])
    out = dict(app=app, graph=name, equal=torch.equal(vals["pull"],
                                                      vals["auto"]))
    for d, e in engines.items():
        ts = times[d]
        out[d] = dict(supersteps=e.supersteps_run, push=e.push_supersteps,
                      pull=e.pull_supersteps,
                      total_ms=statistics.median(ts) * 1e3,
                      min_ms=min(ts) * 1e3, max_ms=max(ts) * 1e3)
    print(out, flush=True)
    return out


def step_job(name, threshold, repeats):
    ctx = init_executor(RuntimeConfig(device="cuda"))
    return dict(rows=[ab_jobs(ctx, app, name, threshold, repeats)
                      for app in ("sssp", "cc")])


def step_sync(threshold, repeats):
    global LOG2N
    LOG2N = 12
    ctx = init_executor(RuntimeConfig(device="cuda"))
    res = ab_jobs(ctx, "sssp", "r8", threshold, repeats)
    res["graph"] = "4096 x 8"
    return res


# ------------------------------------------------------------------ driver

def crossover(op):
    """Largest power-of-two share up to which push, in the form the engine
    calls it (all vertices + mask), is no slower than pull at every measured
    share (None: not even at the smallest)."""
    best = None
    for r in sorted(op["rows"], key=lambda r: r["share_log2"]):
        if r["pushm_ms"] > r["pull_ms"]:
            break
        best = r["share_log2"]
    return best


def run_step(step, path, limit, extra=()):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, __file__,
           "--step", step, "--json", path, *extra]
    print("+", " ".join(cmd), flush=True)
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        raise SystemExit(f"step {step} ended with status {rc}; stopping")
    with open(path) as f:
        return json.load(f)


def fmt_share(lg):
    return "1" if lg == 0 else f"2^{lg}"


def write_profile(out, ops_res, thr_log2, jobs, sync, repeats):
    L = [
        "# Pregel push kernel (K13p) against pull (K13)",
        "",
        f"Device: {ops_res[0]['device']}, one GPU. Synthetic ring+random "
        f"graphs with 2^{LOG2N} vertices (seed {SEED}) and a 1024 x 1024 "
        f"four-neighbour grid. 1 warm-up, then {repeats} alternated runs per "
        "variant; medians. Reproduce: `python scripts/pregel_push_ab.py`.",
        "",
        "## Op level: `pregel_pull` (with the matching mask) against "
        "`pregel_push`",
        "",
        f"Host clock around {CALLS} back-to-back calls ending in a device "
        f"synchronise, divided by {CALLS}. The frontier is a random vertex "
        "subset whose out-edges are the given share of all edges. push "
        "includes its pre-pass (fill, frontier degrees, prefix sum). "
        "`push` gets the compacted frontier; `push, mask` is the form the "
        "engine calls (frontier = all vertices, narrowed by the send mask "
        "inside the pre-pass, so no compaction and no host read), and the "
        "one the crossover and the threshold are taken from.",
        "",
    ]
    for op in ops_res:
        L += [f"### {op['graph']}: {op['n']} vertices, {op['edges']} edges",
              "",
              "| share of edges | frontier vertices | pull ms | push ms | "
              "push, mask ms | pull / push, mask | results |",
              "|---|---|---|---|---|---|---|"]
        for r in op["rows"]:
            L.append(f"| {fmt_share(r['share_log2'])} | {r['nf']} | "
                     f"{r['pull_ms']:.4f} | {r['push_ms']:.4f} | "
                     f"{r['pushm_ms']:.4f} | "
                     f"{r['pull_ms'] / r['pushm_ms']:.2f} | "
                     f"{'equal' if r['equal'] else 'DIFFERENT'} |")
        h = op["hub"]
        L += [f"| {fmt_share(h['share_log2'])}, one hub | 1 | | "
              f"{h['push_ms']:.4f} | | | |", ""]
        c = crossover(op)
        L += [f"Crossover: push is no slower than pull up to a share of "
              f"{fmt_share(c) if c is not None else 'none'}.", ""]
    L += ["## Default `push_threshold`", ""]
    if thr_log2 is None:
        L += ["push was never at least as fast as pull on both graphs: no "
              "threshold is derived and `auto` is not recommended.", ""]
    else:
        L += [f"The largest power-of-two share at which push is no slower "
              f"than pull on both graphs is {fmt_share(thr_log2 + 1)}; halved "
              f"once as a margin (the crossover moves with degree and skew, "
              f"and the table has two graphs): **push_threshold = "
              f"{fmt_share(thr_log2)} = {2.0 ** thr_log2:g}**.", ""]
    L += ["## Job level: `direction=\"pull\"` against `\"auto\"`", "",
          "Host clock around `engine.run()` ending in a device synchronise. "
          "`auto` runs with the threshold above.", "",
          "| app | graph | direction | supersteps | push | pull | total ms | "
          "ms/superstep | min..max total ms | results |",
          "|---|---|---|---|---|---|---|---|---|---|"]
    for j in jobs + [sync]:
        for d in ("pull", "auto"):
            r = j[d]
            L.append(f"| {j['app']} | {j['graph']} | {d} | "
                     f"{r['supersteps']} | "
                     f"{r['push']} | {r['pull']} | {r['total_ms']:.2f} | "
                     f"{r['total_ms'] / r['supersteps']:.4f} | "
                     f"{r['min_ms']:.2f}..{r['max_ms']:.2f} | "
                     f"{'equal' if j['equal'] else 'DIFFERENT'} |")
    L += [""]
    for j in jobs:
        L.append(f"- {j['app']} on {j['graph']}: pull / auto = "
                 f"{j['pull']['total_ms'] / j['auto']['total_ms']:.2f}x")
    spread = sync["pull"]["max_ms"] - sync["pull"]["min_ms"]
    delta = sync["auto"]["total_ms"] - sync["pull"]["total_ms"]
    within = delta <= spread
    no_slower = all(j["auto"]["total_ms"] <= j["pull"]["total_ms"]
                    for j in jobs)
    L += ["", "## What the host read of the direction choice costs", "",
          f"SSSP on 4096 x 8: auto - pull = {delta:+.3f} ms per run "
          f"(medians, {sync['auto']['supersteps']} supersteps); the spread "
          f"(max - min of the {repeats} runs) of pull itself is "
          f"{spread:.3f} ms.", "",
          "## Default `-direction`", "",
          f"auto within pull's spread on 4096 x 8: {'yes' if within else 'no'}"
          f"; auto no slower than pull on all three job-level graphs (both "
          f"apps): {'yes' if no_slower else 'no'}. The runner's default "
          f"`-direction` is therefore "
          f"**{'auto' if within and no_slower else 'pull'}**.", "",
          "Reading the job table: a fused superstep at 2^20 vertices and a "
          "low degree is bound by the host's launches of its per-vertex "
          "tensor ops, which are O(n_local) and the same in both directions, "
          "not by the send + combine kernel. There push saves little device "
          "time, and `auto` adds a host read of the frontier's edge count "
          "and three launches (pre-pass, prefix sum, push) where pull has "
          "one. `direction=\"push\"` needs no host read.", ""]
    text = "\n".join(L)
    print(text)
    with open(out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--json")
    ap.add_argument("--threshold", type=float, default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="profiles/pregel_push_ab.md")
    ap.add_argument("--workdir", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    if args.step:
        s = args.step
        if s in ("op8", "op64"):
            res = step_op("r" + s[2:], args.repeats)
        elif s.startswith("job_"):
            res = step_job(s[4:], args.threshold, args.repeats)
        elif s == "sync":
            res = step_sync(args.threshold, args.repeats)
        else:
            raise SystemExit(f"unknown step {s}")
        with open(args.json, "w") as f:
            json.dump(res, f)
        return
    work = args.workdir or tempfile.mkdtemp(prefix="pregel_push_ab_")
    os.makedirs(work, exist_ok=True)
    rep = ["--repeats", str(args.repeats)]
    ops_res = [run_step(s, os.path.join(work, s + ".json"), 240, rep)
               for s in ("op8", "op64")]
    cross = [crossover(o) for o in ops_res]
    thr_log2 = None if None in cross else min(cross) - 1
    thr = 0.0 if thr_log2 is None else 2.0 ** thr_log2
    extra = rep + ["--threshold", repr(thr)]
    jobs = []
    for g in ("r8", "r64", "grid"):
        jobs += run_step("job_" + g, os.path.join(work, g + ".json"), 300,
                         extra)["rows"]
    sync = run_step("sync", os.path.join(work, "sync.json"), 120, extra)
    write_profile(args.out, ops_res, thr_log2, jobs, sync, args.repeats)


if __name__ == "__main__":
    main()
