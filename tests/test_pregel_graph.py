"""Pregel on real graphs (CPU): adjacency-list parsers, per-edge weights,
the pull index + ops.pregel_pull torch reference, the fused engine path and
run_pregel_job's -input / -output."""

import pytest
import torch

from tests import pregel_cases as pc
from tests.dist_helper import run_dist


# ------------------------------------------------------------- 1. parsers

def _lines(path):
    with open(path) as f:
        return f.read().splitlines()


def test_parse_shortest_path_fixture():
    from harmony_amd.dataloader import parse_graph

    src, dst, w, max_id = parse_graph(_lines(pc.SHORTEST_PATH), weighted=True)
    assert src.dtype == dst.dtype == torch.int64 and w.dtype == torch.float32
    assert src.shape[0] == 30 and max_id == 9
    # first and last data lines of the file: "0 1 2 2 3" and "9 7 6 8 5"
    assert src[:2].tolist() == [0, 0] and dst[:2].tolist() == [1, 2]
    assert w[:2].tolist() == [2.0, 3.0]
    assert src[-2:].tolist() == [9, 9] and dst[-2:].tolist() == [7, 8]
    assert w[-2:].tolist() == [6.0, 5.0]
    # "3 1 4 2 1 4 7 5 6 6 8"
    sel = src == 3
    assert dst[sel].tolist() == [1, 2, 4, 5, 6]
    assert w[sel].tolist() == [4.0, 1.0, 7.0, 6.0, 8.0]


def test_parse_adj_list_fixture():
    from harmony_amd.dataloader import parse_graph

    lines = _lines(pc.ADJ_LIST)
    src, dst, w, max_id = parse_graph(lines, weighted=False)
    assert w is None
    assert src.shape[0] == 9644 and max_id == 2292
    assert "4 " in lines                     # a vertex with no out-edges
    assert int((src == 4).sum()) == 0
    assert int(torch.bincount(dst, minlength=2293).max()) == 184


def test_parse_comments_blank_and_odd_token():
    from harmony_amd.dataloader import parse_graph

    text = ["# header", "", "0 1 5 2 7 3", "   ", "#2 9 9", "7", "2 0 4"]
    src, dst, w, max_id = parse_graph(text, weighted=True)
    # the trailing unpaired "3" of line "0 ..." is ignored
    assert src.tolist() == [0, 0, 2] and dst.tolist() == [1, 2, 0]
    assert w.tolist() == [5.0, 7.0, 4.0]
    assert max_id == 7                      # "7" alone is still a vertex
    src, dst, w, max_id = parse_graph(text, weighted=False)
    assert src.tolist() == [0] * 5 + [2, 2]
    assert dst.tolist() == [1, 5, 2, 7, 3, 0, 4] and w is None


@pytest.mark.parametrize("path,weighted", [(pc.SHORTEST_PATH, True),
                                           (pc.ADJ_LIST, False)])
def test_native_parser_matches_python(path, weighted):
    from harmony_amd import ops
    from harmony_amd.dataloader import parse_graph

    nat = ops._load_hip()
    if nat is None:
        pytest.skip("extension not built: the Python parser is the only one")
    with open(path, "rb") as f:
        buf = f.read()
    ns, nd, nw, nmax = nat.parse_graph_bytes(buf, weighted)
    ps, pd, pw, pmax = parse_graph(buf.decode().splitlines(), weighted)
    assert torch.equal(ns, ps) and torch.equal(nd, pd)
    assert int(nmax[0]) == pmax
    if weighted:
        assert torch.equal(nw, pw)
    else:
        assert nw.numel() == 0
    # a buffer with comments, CRLF, a lone vertex and an odd trailing token
    odd = b"# c\n\n0 1 5 2 7 3\r\n7\n2 0 4"
    ns, nd, nw, nmax = nat.parse_graph_bytes(odd, True)
    ps, pd, pw, pmax = parse_graph(odd.decode().splitlines(), True)
    assert torch.equal(ns, ps) and torch.equal(nd, pd)
    assert torch.equal(nw, pw) and int(nmax[0]) == pmax == 7


def test_load_graph_partition_splits_by_source(tmp_path):
    from harmony_amd.dataloader import load_graph_partition

    parts = [load_graph_partition("file://" + pc.SHORTEST_PATH, lo, hi, True)
             for lo, hi in ((0, 5), (5, 10))]
    assert [p[3] for p in parts] == [10, 10]          # same on every rank
    assert [p[4] for p in parts] == [30, 30]
    assert sum(int(p[1].shape[0]) for p in parts) == 30
    row_ptr, dst, w, _n, _e = parts[1]
    assert row_ptr.tolist() == [0, 3, 6, 9, 12, 14]
    assert dst[:3].tolist() == [3, 7, 8] and w[:3].tolist() == [6.0, 1.0, 3.0]


# ---------------------------------------------------------- engine helpers

def _engine_run(app, path, fused, job_id, **kw):
    """Single-process engine run on a fixture -> final values [n]."""
    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.dataloader import (load_graph_partition,
                                        parse_graph_file)
    from harmony_amd.pregel.engine import PregelEngine
    from harmony_amd.pregel.graphapps import (PageRankComputation,
                                              ShortestPathComputation,
                                              make_graph_from_edges)
    from harmony_amd.runtime.bootstrap import init_executor
    from harmony_amd.runtime.control import ControlPlane

    ctx = init_executor(RuntimeConfig(device=kw.pop("device", "cpu")))
    weighted = app == "shortestpath"
    comp = (ShortestPathComputation(source=kw.get("source", 0)) if weighted
            else PageRankComputation(num_iters=kw.get("num_iters", 10)))
    parsed = parse_graph_file(path, weighted)
    n = parsed[3] + 1
    row_ptr, dst, w, _n, _e = load_graph_partition(path, 0, n, weighted,
                                                   parsed=parsed)
    job = JobConfig(job_id=job_id, app=app, app_args={})
    engine = PregelEngine(job, comp, n, ctx, ControlPlane(ctx.store, 0, 1),
                          fused=fused)
    engine.set_graph(make_graph_from_edges(row_ptr, dst, w, 0, n,
                                           ctx.device))
    return engine.run().squeeze(1).cpu()


def _job_worker(rank, world, app, path, out_dir, extra):
    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.pregel.runner import run_pregel_job
    from harmony_amd.runtime.bootstrap import init_executor

    ctx = init_executor(RuntimeConfig(device="cpu"))
    args = {"input": "file://" + path, "output": out_dir}
    args.update(extra)
    job = JobConfig(job_id=f"pg_{app}_{world}", app=app, app_args=args)
    s = run_pregel_job(job, ctx)
    return {k: s[k] for k in ("num_vertices", "num_edges", "fused_messages",
                              "num_local_vertices")}


def _read_parts(out_dir, world):
    vals = {}
    for r in range(world):
        with open(f"{out_dir}/part-{r}") as f:
            for ln in f:
                k, v = ln.split()
                assert int(k) not in vals
                vals[int(k)] = float(v)
    assert sorted(vals) == list(range(len(vals)))
    return torch.tensor([vals[k] for k in range(len(vals))],
                        dtype=torch.float64)


# ---------------------------------------------------------- 2. SSSP golden

@pytest.mark.parametrize("fused", [False, True])
def test_sssp_golden_single(fused):
    d = _engine_run("shortestpath", pc.SHORTEST_PATH, fused, f"sg{fused}")
    assert d.tolist() == pc.SSSP_FROM_0


@pytest.mark.parametrize("fused", [False, True])
def test_sssp_from_other_source(fused):
    # the fixture's edges are symmetric: dist(9 -> 0) == dist(0 -> 9)
    d = _engine_run("shortestpath", pc.SHORTEST_PATH, fused, f"s9{fused}",
                    source=9)
    assert d[0] == 15.0 and d[9] == 0.0


@pytest.mark.parametrize("fused", ["false", "true"])
def test_sssp_golden_two_ranks_through_job(tmp_path, fused):
    out = str(tmp_path / "out")
    res = run_dist(_job_worker, world=2, timeout=120,
                   args=("shortestpath", pc.SHORTEST_PATH, out,
                         {"source": 0, "fused_messages": fused}))
    assert all(r["num_vertices"] == 10 and r["num_edges"] == 30
               for r in res)
    assert all(r["fused_messages"] == (fused == "true") for r in res)
    assert sum(r["num_local_vertices"] for r in res) == 10
    assert _read_parts(out, 2).tolist() == pc.SSSP_FROM_0


@pytest.mark.parametrize("fused", [False, True])
def test_sssp_per_edge_weights_replace_the_constant(fused):
    """graph.edge_weight, when present, is what an edge adds; without it
    the computation's constant is used, as before."""
    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.pregel.engine import LocalGraph, PregelEngine
    from harmony_amd.pregel.graphapps import ShortestPathComputation
    from harmony_amd.runtime.bootstrap import init_executor
    from harmony_amd.runtime.control import ControlPlane

    ctx = init_executor(RuntimeConfig(device="cpu"))
    got = {}
    for name, w in (("own", torch.tensor([5.0, 1.0, 1.0])), ("const", None)):
        # 0 -> 1 (5), 0 -> 2 (1), 2 -> 1 (1)
        g = LocalGraph(vertex_lo=0, row_ptr=torch.tensor([0, 2, 2, 3]),
                       edge_dst=torch.tensor([1, 2, 1]),
                       out_degree=torch.tensor([2.0, 0.0, 1.0]),
                       num_vertices_global=3, edge_weight=w)
        job = JobConfig(job_id=f"ew_{name}_{fused}", app="shortestpath",
                        app_args={})
        engine = PregelEngine(job, ShortestPathComputation(edge_weight=3.0),
                              3, ctx, ControlPlane(ctx.store, 0, 1),
                              fused=fused)
        engine.set_graph(g)
        got[name] = engine.run().squeeze(1).tolist()
    assert got["own"] == [0.0, 2.0, 1.0]
    assert got["const"] == [0.0, 3.0, 3.0]


# ------------------------------------------------- 3. PageRank on adj_list

@pytest.mark.parametrize("fused", [False, True])
def test_pagerank_adj_list_against_float64(fused):
    _s, _d, n, ref, bound = pc.adj_list_reference(10)
    v = _engine_run("pagerank", pc.ADJ_LIST, fused, f"pa{fused}",
                    num_iters=10).double()
    assert v.shape[0] == n == 2293
    err = (v - ref).abs()
    print("max err / bound:", float((err / bound).max()))
    assert bool((err <= bound).all()), float((err / bound).max())


def test_pagerank_adj_list_fused_two_ranks(tmp_path):
    _s, _d, n, ref, bound = pc.adj_list_reference(10)
    out = str(tmp_path / "out")
    res = run_dist(_job_worker, world=2, timeout=120,
                   args=("pagerank", pc.ADJ_LIST, out,
                         {"num_iters": 10, "fused_messages": "true"}))
    assert all(r["num_vertices"] == n and r["num_edges"] == 9644
               and r["fused_messages"] for r in res)
    v = _read_parts(out, 2)
    err = (v - ref).abs()
    print("max err / bound:", float((err / bound).max()))
    assert bool((err <= bound).all()), float((err / bound).max())


# ------------------------------- 4. ops.pregel_pull reference, brute force

def _check_against_brute(out, flag, brute, combiner):
    b_out, b_flag, b_abs, deg = brute
    assert out.dtype == torch.float32 and flag.dtype == torch.uint8
    assert torch.equal(flag, b_flag)
    if combiner == "min":
        assert torch.equal(out.double(), b_out)
    else:
        err = (out.double() - b_out).abs()
        assert bool((err <= pc.add_bound(deg, b_abs)).all())


@pytest.mark.parametrize("combiner,use_mask,use_w,add_weight",
                         pc.pull_configs())
def test_pull_reference_against_brute_force(combiner, use_mask, use_w,
                                            add_weight):
    from harmony_amd import ops

    ix = pc.handmade_index()
    deg = ix["in_ptr"][1:] - ix["in_ptr"][:-1]
    assert deg[:8].tolist() == pc.SPECIAL_DEGREES and deg.shape[0] == 257
    in_w = ix["in_w"] if use_w else None
    mask = ix["mask"] if use_mask else None
    vm = ix["vert_msg_inf"] if combiner == "min" else ix["vert_msg"]
    out, flag = ops.pregel_pull(ix["in_ptr"], ix["in_src"], in_w, 1.5, vm,
                                mask, combiner, add_weight)
    brute = pc.brute_force_pull(ix["in_ptr"], ix["in_src"], in_w, 1.5, vm,
                                mask, combiner, add_weight)
    _check_against_brute(out, flag, brute, combiner)
    if combiner == "min":
        assert bool(torch.isinf(out).any())     # inf inputs / empty rows


@pytest.mark.parametrize("combiner,ident", [("add", 0.0),
                                            ("min", float("inf"))])
def test_pull_reference_all_false_mask_gives_identity(combiner, ident):
    from harmony_amd import ops

    ix = pc.handmade_index()
    mask = torch.zeros(pc.NUM_SOURCES, dtype=torch.bool)
    out, flag = ops.pregel_pull(ix["in_ptr"], ix["in_src"], ix["in_w"], 0.0,
                                ix["vert_msg"], mask, combiner, True)
    assert int(flag.sum()) == 0
    assert torch.equal(out, torch.full((pc.NUM_ROWS,), ident))


def test_host_group_rule():
    from harmony_amd.ops import pregel_pull_group

    assert pregel_pull_group(100, 0) == 1
    assert pregel_pull_group(100, 100) == 1
    assert pregel_pull_group(100, 101) == 2
    assert pregel_pull_group(257, 2000) == 8
    assert pregel_pull_group(1, 64) == 64
    assert pregel_pull_group(1, 10 ** 6) == 64
    assert pregel_pull_group(0, 0) == 1


def test_pull_index_layout_two_owners():
    """Local rows first (empty ranges kept), then the distinct remote
    destinations in ascending key order; sources in original edge order."""
    from harmony_amd.config import TableConfig
    from harmony_amd.et.table import Table
    from harmony_amd.pregel.engine import LocalGraph, build_pull_index

    # 8 vertices, 2 ranks: rank 0 owns 0..3. Local vertices 0..3 with edges
    # 0->{5,1}, 1->{7,5}, 2->{}, 3->{1,2,5}
    t = Table(TableConfig(table_id="pi/msg", num_keys=8, value_dim=1,
                          num_blocks=8, update_fn="add", init_fn="zeros"),
              0, 2, torch.device("cpu"))
    g = LocalGraph(vertex_lo=0,
                   row_ptr=torch.tensor([0, 2, 4, 4, 7]),
                   edge_dst=torch.tensor([5, 1, 7, 5, 1, 2, 5]),
                   out_degree=torch.tensor([2., 2., 0., 3.]),
                   num_vertices_global=8,
                   edge_weight=torch.arange(7, dtype=torch.float32))
    p = build_pull_index(g, t)
    assert p.n_local == 4 and p.remote_keys.tolist() == [5, 7]
    assert p.in_src.dtype == torch.int32 and p.in_ptr.dtype == torch.int64
    #            rows:  0   1       2    3   | 5          7
    assert p.in_ptr.tolist() == [0, 0, 2, 3, 3, 6, 7]
    assert p.in_src.tolist() == [0, 3, 3, 0, 1, 3, 1]
    assert p.in_w.tolist() == [1., 4., 5., 0., 3., 6., 2.]


def test_fused_needs_the_hook():
    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.pregel.engine import Computation, PregelEngine
    from harmony_amd.runtime.bootstrap import init_executor
    from harmony_amd.runtime.control import ControlPlane

    ctx = init_executor(RuntimeConfig(device="cpu"))
    job = JobConfig(job_id="nohook", app="pagerank", app_args={})
    with pytest.raises(ValueError, match="vertex_messages"):
        PregelEngine(job, Computation(), 8, ctx,
                     ControlPlane(ctx.store, 0, 1), fused=True)


# --------------------------------------------- 5. -num_vertices too small

def test_num_vertices_smaller_than_input_is_rejected(monkeypatch):
    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.pregel import runner
    from harmony_amd.runtime.bootstrap import init_executor

    def no_tables(*a, **k):
        raise AssertionError("tables were built before the check")

    monkeypatch.setattr(runner, "PregelEngine", no_tables)
    ctx = init_executor(RuntimeConfig(device="cpu"))
    job = JobConfig(job_id="small", app="shortestpath",
                    app_args={"input": pc.SHORTEST_PATH, "num_vertices": 9})
    with pytest.raises(ValueError, match="num_vertices"):
        runner.run_pregel_job(job, ctx)


# ------------------------------------------------- public interface (CLI)

def test_run_shortest_path_script_with_input(tmp_path):
    """bin/run_shortest_path.sh -input ... -output ...: the standalone
    launcher end to end, file:// accepted."""
    import json
    import subprocess
    from pathlib import Path

    import os
    import sys

    root = Path(__file__).resolve().parent.parent
    out_dir = tmp_path / "sp"
    # the script calls `python`: make that this interpreter
    shim = tmp_path / "shim"
    shim.mkdir()
    (shim / "python").write_text(f'#!/bin/sh\nexec "{sys.executable}" "$@"\n')
    (shim / "python").chmod(0o755)
    env = dict(os.environ, PATH=f"{shim}{os.pathsep}{os.environ['PATH']}")
    out = subprocess.run(
        ["bash", str(root / "bin" / "run_shortest_path.sh"), "-device", "cpu",
         "-input", "file://" + pc.SHORTEST_PATH, "-source", "0",
         "-output", str(out_dir), "-fused_messages", "true"],
        capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-1500:]
    s = json.loads(out.stdout.strip().splitlines()[-1])
    assert s["num_vertices"] == 10 and s["num_edges"] == 30
    assert s["fused_messages"] is True
    assert _read_parts(str(out_dir), 1).tolist() == pc.SSSP_FROM_0


def test_jobserver_submit_with_input(tmp_path):
    """-input / -output through the job server's submit path."""
    import threading

    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.jobserver import client
    from harmony_amd.jobserver.server import JobServerDriver
    from harmony_amd.runtime.bootstrap import init_executor
    from tests.dist_helper import free_port

    port = free_port()
    ctx = init_executor(RuntimeConfig(device="cpu"))
    driver = JobServerDriver(ctx, scheduler="default", port=port)
    t = threading.Thread(target=driver.run, daemon=True)
    t.start()
    out_dir = tmp_path / "js"
    job = JobConfig(job_id="sp_in", app="shortestpath", max_num_epochs=1,
                    num_mini_batches=1,
                    app_args={"input": pc.SHORTEST_PATH, "source": 0,
                              "output": str(out_dir)})
    r = client.submit(job, port=port, wait=True, timeout=60)
    client.shutdown(port=port)
    t.join(timeout=30)
    assert r["status"] == "done", r
    assert r["per_rank"][0]["num_edges"] == 30
    assert _read_parts(str(out_dir), 1).tolist() == pc.SSSP_FROM_0
