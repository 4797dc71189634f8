"""Pregel push (CPU): the ops.pregel_push torch fallback on the cases the
GPU file runs through K13p, the engine's direction choice, the
connected-components app, and the two-rank and job cases."""

import pytest
import torch

from tests import pregel_cases as pc
from tests import pregel_push_cases as ppc
from tests.dist_helper import run_dist


@pytest.mark.parametrize("use_w,add_weight,inf_msgs", ppc.PUSH_CONFIGS)
@pytest.mark.parametrize("frontier", ppc.FRONTIERS)
def test_fallback_against_pull_and_brute_force(frontier, use_w, add_weight,
                                               inf_msgs):
    ppc.check_kernel_case("cpu", frontier, use_w, add_weight, inf_msgs)


def test_handmade_out_csr_shape():
    c = ppc.handmade_out_csr()
    deg = c["out_ptr"][1:] - c["out_ptr"][:-1]
    assert deg[:9].tolist() == ppc.SPECIAL_DEGREES and deg.shape[0] == 300
    hub = c["out_row"][int(c["out_ptr"][8]):int(c["out_ptr"][9])]
    assert hub.shape[0] == 20000 and bool((hub == ppc.HUB_ROW).all())
    assert bool((c["vert_msg"] < 0).any()) and bool((c["vert_msg"] > 0).any())
    assert bool(torch.isinf(c["vert_msg_inf"]).any())
    fr = c["frontiers"]
    assert fr["half_repeats"].shape[0] == fr["half"].shape[0] + 40
    assert all(f.dtype == torch.int32 for f in fr.values())


def test_fallback_skips_malformed_ids_and_rows():
    ppc.check_malformed("cpu")


def test_fallback_add_raises_and_empty_shapes():
    ppc.check_add_raises_and_empty_shapes("cpu")


# --------------------------------------------------------------- engine

def test_engine_push_sssp_fixture():
    ppc.check_engine_sssp_fixture("cpu", "cpu")


def test_engine_directions_agree_on_synthetic():
    ppc.check_engine_synthetic("cpu", "cpu")


def test_engine_push_star():
    ppc.check_engine_star("cpu", "cpu")


def test_engine_refusals():
    ppc.check_engine_refusals("cpu", "cpu")


def test_push_index_layout_two_owners():
    """out_row names the pull index's rows: local rows as they are, remote
    destinations by their position in remote_keys; edge order kept, the
    weights the graph's own tensor."""
    from harmony_amd.config import TableConfig
    from harmony_amd.et.table import Table
    from harmony_amd.pregel.engine import (LocalGraph, build_pull_index,
                                           build_push_index)

    # the graph of test_pull_index_layout_two_owners
    t = Table(TableConfig(table_id="ppi/msg", num_keys=8, value_dim=1,
                          num_blocks=8, update_fn="min", init_fn="zeros"),
              0, 2, torch.device("cpu"))
    g = LocalGraph(vertex_lo=0,
                   row_ptr=torch.tensor([0, 2, 4, 4, 7]),
                   edge_dst=torch.tensor([5, 1, 7, 5, 1, 2, 5]),
                   out_degree=torch.tensor([2., 2., 0., 3.]),
                   num_vertices_global=8,
                   edge_weight=torch.arange(7, dtype=torch.float32))
    pull = build_pull_index(g, t, keep_rows=True)
    push = build_push_index(g, pull, t)
    assert pull.remote_keys.tolist() == [5, 7] and pull.num_rows == 6
    assert push.out_ptr.tolist() == [0, 2, 4, 4, 7]
    assert push.out_row.dtype == torch.int32
    assert push.out_row.tolist() == [4, 1, 5, 4, 1, 2, 4]
    assert push.out_w is g.edge_weight
    assert pull.row_of_edge is None            # handed over, not kept twice
    with pytest.raises(ValueError, match="keep_rows"):
        build_push_index(g, build_pull_index(g, t), t)


# ------------------------------------------------- connected components

def test_components_fixture_shape():
    """What the fixture promises: components of 4, 2, 1, 3 and 6; a vertex
    that is only a destination; the largest id early in the file."""
    src, dst, n = ppc.components_edges()
    assert n == 16 and len(src) == 12
    want = ppc.union_find_labels()
    sizes = sorted(want.count(x) for x in set(want))
    assert sizes == [1, 2, 3, 4, 6]
    assert 13 in dst and 13 not in src
    with open(ppc.COMPONENTS) as f:
        data = [ln for ln in f if not ln.startswith("#")]
    assert "15" in data[0].split()
    # every component with more than one vertex straddles the two-rank
    # boundary (ids 0..7 | 8..15)
    for root in set(want):
        members = [v for v in range(n) if want[v] == root]
        if len(members) > 1:
            assert min(members) < 8 <= max(members), members


def test_connected_components_fixture(tmp_path):
    ppc.check_cc_fixture("cpu", tmp_path, "cpu")


def test_connected_components_synthetic_is_one_component(tmp_path):
    """Without -input: the ring makes the symmetrised synthetic graph one
    component, so every label is 0."""
    from harmony_amd.config import JobConfig
    from harmony_amd.pregel.runner import run_pregel_job

    job = JobConfig(job_id="cc_syn", app="connectedcomponents",
                    app_args={"num_vertices": 200, "out_degree": 3,
                              "output": str(tmp_path), "direction": "auto",
                              "fused_messages": "true"})
    s = run_pregel_job(job, ppc.make_ctx("cpu"))
    assert s["num_edges"] == 2 * 200 * 3
    assert ppc.read_parts(str(tmp_path), 1) == [0.0] * 200


def test_too_many_vertices_are_refused_before_tables(monkeypatch):
    from harmony_amd.config import JobConfig
    from harmony_amd.pregel import runner

    def no_tables(*a, **k):
        raise AssertionError("tables were built before the check")

    monkeypatch.setattr(runner, "PregelEngine", no_tables)
    job = JobConfig(job_id="cc_big", app="connectedcomponents",
                    app_args={"num_vertices": 2 ** 24 + 1})
    with pytest.raises(ValueError, match=r"2\^24"):
        runner.run_pregel_job(job, ppc.make_ctx("cpu"))


def _job_worker(rank, world, app, path, out_dir, extra):
    from harmony_amd.config import JobConfig
    from harmony_amd.pregel.runner import run_pregel_job

    args = {"input": "file://" + path, "output": out_dir,
            "fused_messages": "true", "direction": "push"}
    args.update(extra)
    job = JobConfig(job_id=f"ppj_{app}_{world}", app=app, app_args=args)
    s = run_pregel_job(job, ppc.make_ctx("cpu"))
    return {k: s[k] for k in ("direction", "push_supersteps",
                              "pull_supersteps", "supersteps",
                              "num_local_vertices")}


@pytest.mark.parametrize("app,path,extra", [
    ("connectedcomponents", ppc.COMPONENTS, {}),
    ("shortestpath", pc.SHORTEST_PATH, {"source": 0}),
])
def test_push_two_ranks_equal_one_rank(tmp_path, app, path, extra):
    """The part files of world 2 equal those of world 1 with -direction
    push: the remote-row numbering of the push index against the pull
    index's remote_keys."""
    outs = {}
    for world in (1, 2):
        out = str(tmp_path / f"w{world}")
        res = run_dist(_job_worker, world=world, timeout=120,
                       args=(app, path, out, extra))
        assert all(r["direction"] == "push" and r["pull_supersteps"] == 0
                   and r["push_supersteps"] == r["supersteps"] for r in res)
        outs[world] = ppc.read_parts(out, world)
    assert outs[2] == outs[1]
    want = (ppc.union_find_labels() if app == "connectedcomponents"
            else pc.SSSP_FROM_0)
    assert outs[1] == want


def test_run_connected_components_script(tmp_path):
    """bin/run_connected_components.sh -input ... -output ...: the
    standalone launcher end to end."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    out_dir = tmp_path / "cc"
    # the script calls `python`: make that this interpreter
    shim = tmp_path / "shim"
    shim.mkdir()
    (shim / "python").write_text(f'#!/bin/sh\nexec "{sys.executable}" "$@"\n')
    (shim / "python").chmod(0o755)
    env = dict(os.environ, PATH=f"{shim}{os.pathsep}{os.environ['PATH']}")
    out = subprocess.run(
        ["bash", str(root / "bin" / "run_connected_components.sh"),
         "-device", "cpu", "-input", "file://" + ppc.COMPONENTS,
         "-output", str(out_dir), "-fused_messages", "true",
         "-direction", "auto"],
        capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-1500:]
    s = json.loads(out.stdout.strip().splitlines()[-1])
    assert s["num_vertices"] == 16 and s["num_edges"] == 24
    assert s["direction"] == "auto"
    assert s["push_supersteps"] + s["pull_supersteps"] == s["supersteps"]
    assert ppc.read_parts(str(out_dir), 1) == ppc.union_find_labels()
