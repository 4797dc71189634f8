"""Pregel job runner — jobserver glue (reference pregel/jobserver/
PregelJobEntity + PregelMaster.start)."""

from __future__ import annotations

import os
import time
from typing import Optional

from harmony_amd import dataloader as dl
from harmony_amd.config import JobConfig
from harmony_amd.pregel.engine import PregelEngine
from harmony_amd.pregel.graphapps import (ConnectedComponentsComputation,
                                          PageRankComputation,
                                          ShortestPathComputation,
                                          make_graph_from_edges,
                                          make_ring_plus_random_graph,
                                          ring_plus_random_edges,
                                          symmetrise)
from harmony_amd.runtime.control import ControlPlane, TaskUnitScheduler
from harmony_amd.utils import stable_seed

PREGEL_APPS = {"pagerank", "shortestpath", "connectedcomponents"}


def local_vertex_range(num_vertices: int, rank: int, world: int):
    lo = (num_vertices * rank) // world
    hi = (num_vertices * (rank + 1)) // world
    return lo, hi


def _use_fused(setting, device) -> bool:
    """-fused_messages auto|true|false; auto = on when the device is a GPU
    and the HIP extension is loaded."""
    from harmony_amd import ops

    s = str(setting).lower()
    if s in ("true", "1", "yes"):
        return True
    if s in ("false", "0", "no"):
        return False
    if s != "auto":
        raise ValueError(f"-fused_messages must be auto|true|false, "
                         f"got {setting!r}")
    return device.type == "cuda" and ops.hip_available()


def _flag(setting, name: str) -> bool:
    s = str(setting).lower()
    if s in ("true", "1", "yes"):
        return True
    if s in ("false", "0", "no"):
        return False
    raise ValueError(f"-{name} must be true|false, got {setting!r}")


def _write_part(out_dir: str, rank: int, lo: int, values) -> None:
    """<dir>/part-<rank>: one "vertexId value" line per local vertex."""
    out_dir = dl._strip_scheme(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    vals = values.reshape(-1).tolist()
    with open(os.path.join(out_dir, f"part-{rank}"), "w") as f:
        for i, v in enumerate(vals):
            f.write(f"{lo + i} {v!r}\n")


def run_pregel_job(job: JobConfig, ctx, cp: Optional[ControlPlane] = None,
                   tus: Optional[TaskUnitScheduler] = None) -> dict:
    """App args: -input <adjacency list> (file:// accepted; without it the
    synthetic ring+random graph of -num_vertices/-out_degree is used),
    -output <dir> (each rank writes part-<rank>), -fused_messages
    auto|true|false, -direction pull|push|auto and -push_threshold <share
    of the local edges> (fused path only, see PregelEngine), plus -num_iters
    (pagerank), -source/-edge_weight (shortestpath) and -undirected
    true|false (connectedcomponents, default true: every edge is also
    followed backwards, which gives weakly connected components; false
    gives label(v) = the smallest id with a path to v).

    -direction defaults to pull: see profiles/pregel_push_ab.md."""
    a = dict(num_vertices=1024, out_degree=4, num_iters=20, source=0,
             edge_weight=1.0, fused_messages="auto", direction="pull",
             undirected="true")
    a.update(job.app_args)
    cp = cp or ControlPlane(ctx.store, ctx.rank, ctx.world_size)
    n = int(a["num_vertices"])
    weighted = job.app == "shortestpath"
    parsed = None
    if a.get("input"):
        # first scan: the id range sizes the tables, so it comes before them
        parsed = dl.parse_graph_file(a["input"], weighted, ctx.world_size)
        n_file = parsed[3] + 1
        if "num_vertices" not in job.app_args:
            n = n_file
        elif n < n_file:
            raise ValueError(
                f"-num_vertices {n} is smaller than the input's largest "
                f"vertex id + 1 ({n_file})")
    # align the vertex partition with the table partition: the engine's
    # tables use contiguous even blocks, so the local range is rank-even too
    if job.app == "pagerank":
        comp = PageRankComputation(num_iters=int(a["num_iters"]))
    elif job.app == "shortestpath":
        comp = ShortestPathComputation(source=int(a["source"]),
                                       edge_weight=float(a["edge_weight"]))
    elif job.app == "connectedcomponents":
        # refuses more vertices than float32 labels can tell apart, before
        # any table is built
        comp = ConnectedComponentsComputation(n)
        if _flag(a["undirected"], "undirected"):
            # every rank holds the whole edge list anyway (each one parses
            # the whole file), so appending the reversed edges before the
            # list is partitioned by source needs no communication
            if parsed is None:
                src, dst = ring_plus_random_edges(
                    n, int(a["out_degree"]), stable_seed(job.job_id, "graph"))
                parsed = (src, dst, None, n - 1)
            src, dst = symmetrise(parsed[0], parsed[1])
            parsed = (src, dst, None, parsed[3])
    else:
        raise KeyError(job.app)
    t0 = time.perf_counter()
    # the engine derives its shard layout from Table ownership; build tables
    # first, then the graph over the local key range
    engine = PregelEngine(job, comp, n, ctx=ctx, cp=cp, tus=tus,
                          max_supersteps=int(a.get("max_supersteps", 200)),
                          fused=_use_fused(a["fused_messages"], ctx.device),
                          direction=str(a["direction"]).lower(),
                          push_threshold=(float(a["push_threshold"])
                                          if "push_threshold" in a else None))
    lo, hi = engine.local_vertex_range()
    if parsed is not None:
        row_ptr, edge_dst, edge_w, _n, num_edges = dl.load_graph_partition(
            a.get("input", ""), lo, hi, weighted, ctx.world_size,
            parsed=parsed)
        graph = make_graph_from_edges(row_ptr, edge_dst, edge_w, lo, n,
                                      ctx.device)
    else:
        graph = make_ring_plus_random_graph(
            n, int(a["out_degree"]), lo, hi, ctx.device,
            stable_seed(job.job_id, "graph"))   # rank-independent graph
        num_edges = n * int(a["out_degree"])
    engine.set_graph(graph)
    values = engine.run()
    if a.get("output"):
        _write_part(str(a["output"]), ctx.rank, lo, values)
    dt = time.perf_counter() - t0
    return {
        "job_id": job.job_id,
        "rank": ctx.rank,
        "num_batches": engine.supersteps_run,     # supersteps as "batches"
        "supersteps": engine.supersteps_run,
        "num_vertices": n,
        "num_edges": num_edges,
        "fused_messages": engine.fused,
        "direction": engine.direction,
        "push_supersteps": engine.push_supersteps,
        "pull_supersteps": engine.pull_supersteps,
        "num_local_vertices": int(values.shape[0]),
        "total_examples": int(values.shape[0]) * engine.supersteps_run,
        "elapsed_sec": dt,
        "data_processing_rate": (int(values.shape[0]) * engine.supersteps_run
                                 / dt if dt else 0.0),
    }
