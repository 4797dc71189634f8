"""Shared cases for the Pregel push tests (test_pregel_push_cpu.py through
the torch fallback, test_pregel_push_gpu.py through K13p): the hand-made
out-CSR with its frontiers and its inverted (pull) index, the checks both
files run with the device as a parameter, and the connected-components
references."""

from __future__ import annotations

import functools

import pytest
import torch

from tests import pregel_cases as pc

COMPONENTS = str(pc.GOLDEN / "components")

SPECIAL_DEGREES = [0, 1, 2, 63, 64, 65, 200, 1000, 20000]
HUB = 8                       # the source with 20000 out-edges
HUB_ROW = 100                 # the one row all of them end in
NUM_SOURCES = 300
NUM_ROWS = 257
W_CONST = 1.5


# ------------------------------------------------- hand-made out-CSR

@functools.lru_cache(maxsize=None)
def handmade_out_csr():
    """300 sources over R = 257 rows: out-degrees {0, 1, 2, 63, 64, 65, 200,
    1000, 20000} on the first nine sources, 0..5 on the rest; all 20000
    edges of the hub end in one row, the other destinations are random.
    Messages in [-8, 8) so both branches of the ordered-integer min run.
    Shared: callers must not modify the tensors."""
    g = torch.Generator().manual_seed(4321)
    deg = torch.randint(0, 6, (NUM_SOURCES,), generator=g)
    deg[:len(SPECIAL_DEGREES)] = torch.tensor(SPECIAL_DEGREES)
    out_ptr = torch.zeros(NUM_SOURCES + 1, dtype=torch.int64)
    out_ptr[1:] = torch.cumsum(deg, 0)
    e = int(out_ptr[-1])
    out_row = torch.randint(0, NUM_ROWS, (e,), generator=g).to(torch.int32)
    out_row[int(out_ptr[HUB]):int(out_ptr[HUB + 1])] = HUB_ROW
    out_w = torch.randint(1, 10, (e,), generator=g).to(torch.float32)
    vert_msg = torch.rand(NUM_SOURCES, generator=g) * 16.0 - 8.0
    vert_msg_inf = vert_msg.clone()
    vert_msg_inf[torch.rand(NUM_SOURCES, generator=g) < 0.3] = float("inf")
    half = (torch.rand(NUM_SOURCES, generator=g) < 0.5).nonzero().squeeze(1)
    reps = half[torch.randint(0, half.shape[0], (40,), generator=g)]
    frontiers = {
        "empty": torch.zeros(0, dtype=torch.int64),
        "hub": torch.tensor([HUB]),
        "zero_degree": torch.tensor([0]),
        "last": torch.tensor([NUM_SOURCES - 1]),
        "half": half,
        "everyone": torch.arange(NUM_SOURCES),
        "half_repeats": torch.sort(torch.cat([half, reps])).values,
    }
    frontiers = {k: v.to(torch.int32) for k, v in frontiers.items()}
    return dict(out_ptr=out_ptr, out_row=out_row, out_w=out_w,
                vert_msg=vert_msg, vert_msg_inf=vert_msg_inf,
                frontiers=frontiers)


FRONTIERS = ["empty", "hub", "zero_degree", "last", "half", "everyone",
             "half_repeats"]

# (use_w, add_weight, inf_msgs)
PUSH_CONFIGS = [(True, True, False), (False, True, False),
                (False, False, False), (True, True, True),
                (False, True, True), (False, False, True)]


def invert(out_ptr, out_row, out_w, num_rows):
    """The pull index of the same edge list, by a stable sort on row (the
    rows must lie in [0, num_rows)). -> (in_ptr, in_src, in_w)."""
    n = out_ptr.shape[0] - 1
    src = torch.repeat_interleave(torch.arange(n), out_ptr[1:] - out_ptr[:-1])
    row = out_row.long()
    order = torch.argsort(row, stable=True)
    in_ptr = torch.zeros(num_rows + 1, dtype=torch.int64)
    in_ptr[1:] = torch.cumsum(torch.bincount(row, minlength=num_rows), 0)
    return (in_ptr, src[order].to(torch.int32).contiguous(),
            None if out_w is None else out_w[order].contiguous())


@functools.lru_cache(maxsize=None)
def handmade_pull_index():
    c = handmade_out_csr()
    return invert(c["out_ptr"], c["out_row"], c["out_w"], NUM_ROWS)


def mask_of(frontier, n):
    m = torch.zeros(n, dtype=torch.bool)
    f = frontier.long()
    m[f[(f >= 0) & (f < n)]] = True
    return m


@functools.lru_cache(maxsize=None)
def brute(frontier_name, use_w, add_weight, inf_msgs):
    """brute_force_pull on the inverted index, computed once per case and
    shared -> (out float32 [R], flag uint8 [R])."""
    c = handmade_out_csr()
    in_ptr, in_src, in_w = handmade_pull_index()
    vm = c["vert_msg_inf"] if inf_msgs else c["vert_msg"]
    mask = mask_of(c["frontiers"][frontier_name], NUM_SOURCES)
    out, flag, _a, _d = pc.brute_force_pull(
        in_ptr, in_src, in_w if use_w else None, W_CONST, vm, mask, "min",
        add_weight)
    return out.to(torch.float32), flag


def _to(t, device):
    return None if t is None else t.to(device)


def check_kernel_case(device, frontier_name, use_w, add_weight, inf_msgs):
    """push == pull with the matching mask == brute force, bit for bit, and
    a second push run repeats the first."""
    from harmony_amd import ops

    c = handmade_out_csr()
    in_ptr, in_src, in_w = handmade_pull_index()
    vm = c["vert_msg_inf"] if inf_msgs else c["vert_msg"]
    fr = c["frontiers"][frontier_name]
    w = c["out_w"] if use_w else None
    args = (_to(c["out_ptr"], device), _to(c["out_row"], device),
            _to(w, device), W_CONST, _to(vm, device), _to(fr, device),
            NUM_ROWS, "min", add_weight)
    runs = [ops.pregel_push(*args) for _ in range(2)]
    p_out, p_flag = ops.pregel_pull(
        _to(in_ptr, device), _to(in_src, device),
        _to(in_w if use_w else None, device), W_CONST, _to(vm, device),
        _to(mask_of(fr, NUM_SOURCES), device), "min", add_weight)
    b_out, b_flag = brute(frontier_name, use_w, add_weight, inf_msgs)
    out, flag = runs[0]
    assert out.dtype == torch.float32 and flag.dtype == torch.uint8
    assert out.shape == (NUM_ROWS,) and flag.shape == (NUM_ROWS,)
    assert out.device.type == torch.device(device).type
    assert torch.equal(flag.cpu(), b_flag)
    assert torch.equal(out.cpu(), b_out)
    assert torch.equal(flag, p_flag)
    assert torch.equal(out.view(torch.int32), p_out.view(torch.int32))
    assert torch.equal(out.view(torch.int32), runs[1][0].view(torch.int32))
    assert torch.equal(flag, runs[1][1])
    # the engine's form: the frontier of all vertices narrowed by the mask
    m_out, m_flag = ops.pregel_push(
        *args[:5], _to(c["frontiers"]["everyone"], device), NUM_ROWS, "min",
        add_weight, send_mask=_to(mask_of(fr, NUM_SOURCES), device))
    assert torch.equal(out.view(torch.int32), m_out.view(torch.int32))
    assert torch.equal(flag, m_flag)
    if frontier_name in ("everyone", "half"):
        # both signs reach the combine
        assert bool((out < 0).any()) and bool((out > 0).any())
    if frontier_name == "hub":
        assert int(flag.sum()) == 1 and int(flag[HUB_ROW]) == 1


def check_malformed(device):
    """A frontier id of n_local and one of -1, and a row of R: the result
    of the index without them."""
    from harmony_amd import ops

    c = handmade_out_csr()
    fr = c["frontiers"]["half"]
    bad_fr = torch.cat([torch.tensor([-1], dtype=torch.int32), fr,
                        torch.tensor([NUM_SOURCES], dtype=torch.int32)])
    # the first out-edge of a sending vertex with edges gets the row R
    v = next(int(x) for x in fr.tolist()
             if c["out_ptr"][x + 1] > c["out_ptr"][x] and x != HUB)
    e_bad = int(c["out_ptr"][v])
    bad_row = c["out_row"].clone()
    bad_row[e_bad] = NUM_ROWS
    # the same index without that edge
    keep = torch.ones(bad_row.shape[0], dtype=torch.bool)
    keep[e_bad] = False
    good_ptr = c["out_ptr"].clone()
    good_ptr[v + 1:] -= 1
    in_ptr, in_src, in_w = invert(good_ptr, c["out_row"][keep],
                                  c["out_w"][keep], NUM_ROWS)
    b_out, b_flag, _a, _d = pc.brute_force_pull(
        in_ptr, in_src, in_w, W_CONST, c["vert_msg"],
        mask_of(fr, NUM_SOURCES), "min", True)
    out, flag = ops.pregel_push(
        c["out_ptr"].to(device), bad_row.to(device), c["out_w"].to(device),
        W_CONST, c["vert_msg"].to(device), bad_fr.to(device), NUM_ROWS,
        "min", True)
    assert torch.equal(out.cpu(), b_out.to(torch.float32))
    assert torch.equal(flag.cpu(), b_flag)


def check_add_raises_and_empty_shapes(device):
    from harmony_amd import ops

    c = handmade_out_csr()
    args = (c["out_ptr"].to(device), c["out_row"].to(device), None, W_CONST,
            c["vert_msg"].to(device))
    with pytest.raises(ValueError, match="min"):
        ops.pregel_push(*args, c["frontiers"]["half"].to(device), NUM_ROWS,
                        "add", False)
    # nf = 0: filled tensors of the full shape
    out, flag = ops.pregel_push(
        *args, torch.zeros(0, dtype=torch.int32, device=device), NUM_ROWS,
        "min", False)
    assert out.shape == (NUM_ROWS,) and flag.shape == (NUM_ROWS,)
    assert out.dtype == torch.float32 and flag.dtype == torch.uint8
    assert bool(torch.isposinf(out).all()) and int(flag.sum()) == 0
    # R = 0: empty results (every row is then out of range)
    out, flag = ops.pregel_push(*args, c["frontiers"]["half"].to(device), 0,
                                "min", False)
    assert out.shape == (0,) and flag.shape == (0,)
    assert out.dtype == torch.float32 and flag.dtype == torch.uint8


# --------------------------------------------------------------- engine

def make_ctx(device):
    from harmony_amd.config import RuntimeConfig
    from harmony_amd.runtime.bootstrap import init_executor

    return init_executor(RuntimeConfig(device=device))


def run_engine(device, comp, graph_fn, n, job_id, fused=True,
               direction="pull", push_threshold=None, max_supersteps=200):
    """-> (final values [n] on the CPU, the engine)."""
    from harmony_amd.config import JobConfig
    from harmony_amd.pregel.engine import PregelEngine
    from harmony_amd.runtime.control import ControlPlane

    ctx = make_ctx(device)
    job = JobConfig(job_id=job_id, app="pregel", app_args={})
    engine = PregelEngine(job, comp, n, ctx, ControlPlane(ctx.store, 0, 1),
                          max_supersteps=max_supersteps, fused=fused,
                          direction=direction, push_threshold=push_threshold)
    engine.set_graph(graph_fn(ctx.device))
    return engine.run().squeeze(1).cpu(), engine


def sssp():
    from harmony_amd.pregel.graphapps import ShortestPathComputation

    return ShortestPathComputation(source=0)


def fixture_graph(path, weighted):
    from harmony_amd.dataloader import (load_graph_partition,
                                        parse_graph_file)
    from harmony_amd.pregel.graphapps import make_graph_from_edges

    parsed = parse_graph_file(path, weighted)
    n = parsed[3] + 1
    row_ptr, dst, w, _n, _e = load_graph_partition(path, 0, n, weighted,
                                                   parsed=parsed)
    return n, lambda dev: make_graph_from_edges(row_ptr, dst, w, 0, n, dev)


def synthetic(n=4096, deg=8):
    from harmony_amd.pregel.graphapps import make_ring_plus_random_graph

    return lambda dev: make_ring_plus_random_graph(n, deg, 0, n, dev, 4242)


def star(n=4096):
    """Vertex 0 points to 1..n-1 and nothing else: one hub, a frontier of
    one whose edges are the whole graph."""
    from harmony_amd.pregel.graphapps import make_graph_from_edges

    row_ptr = torch.full((n + 1,), n - 1, dtype=torch.int64)
    row_ptr[0] = 0
    dst = torch.arange(1, n, dtype=torch.int64)
    return lambda dev: make_graph_from_edges(row_ptr, dst, None, 0, n, dev)


def check_engine_sssp_fixture(device, tag):
    n, gf = fixture_graph(pc.SHORTEST_PATH, True)
    d, e = run_engine(device, sssp(), gf, n, f"pp_fix_{tag}",
                      direction="push")
    assert d.tolist() == pc.SSSP_FROM_0
    assert e.push_supersteps == e.supersteps_run and e.pull_supersteps == 0


def check_engine_synthetic(device, tag):
    """push, auto (threshold 1/16, passed explicitly), pull and the unfused
    engine agree bit for bit on 4096 x 8; auto uses both directions."""
    n = 4096
    got, eng = {}, {}
    for name, fused, direction, thr in (
            ("unfused", False, "pull", None), ("pull", True, "pull", None),
            ("push", True, "push", None), ("auto", True, "auto", 1.0 / 16)):
        got[name], eng[name] = run_engine(
            device, sssp(), synthetic(n, 8), n, f"pp_syn_{name}_{tag}",
            fused=fused, direction=direction, push_threshold=thr)
    assert bool(torch.isfinite(got["unfused"]).all())
    for name in ("pull", "push", "auto"):
        assert torch.equal(got[name], got["unfused"]), name
    a = eng["auto"]
    # the CPU simulation of this graph predicts 5 push + 3 pull over 8
    print(f"auto, threshold 1/16: {a.push_supersteps} push + "
          f"{a.pull_supersteps} pull over {a.supersteps_run} supersteps")
    assert a.push_supersteps >= 1 and a.pull_supersteps >= 1
    # SSSP sends (possibly to nobody) in every superstep
    for e in (eng["pull"], eng["push"], a):
        assert e.push_supersteps + e.pull_supersteps == e.supersteps_run
    assert eng["pull"].push_supersteps == 0
    assert eng["push"].pull_supersteps == 0


def check_engine_star(device, tag):
    n = 4096
    pull, _e = run_engine(device, sssp(), star(n), n, f"pp_star_pl_{tag}",
                          direction="pull")
    push, e = run_engine(device, sssp(), star(n), n, f"pp_star_ps_{tag}",
                         direction="push")
    assert torch.equal(push, pull)
    assert push.tolist() == [0.0] + [1.0] * (n - 1)
    assert e.push_supersteps == e.supersteps_run


def check_engine_refusals(device, tag):
    from harmony_amd.pregel.graphapps import PageRankComputation

    with pytest.raises(ValueError, match="min"):
        run_engine(device, PageRankComputation(num_iters=2), synthetic(64, 2),
                   64, f"pp_ref_pr_{tag}", direction="push")
    for direction in ("push", "auto"):
        with pytest.raises(ValueError, match="fused"):
            run_engine(device, sssp(), synthetic(64, 2), 64,
                       f"pp_ref_uf_{direction}_{tag}", fused=False,
                       direction=direction)
    # auto with the add combiner is allowed and always pulls
    _v, e = run_engine(device, PageRankComputation(num_iters=2),
                       synthetic(64, 2), 64, f"pp_ref_auto_{tag}",
                       direction="auto")
    assert e.push_supersteps == 0 and e.pull_supersteps == 2
    assert e.supersteps_run == 3       # the last superstep sends nothing


# ------------------------------------------------- connected components

@functools.lru_cache(maxsize=None)
def components_edges():
    """(src list, dst list, n) of the components fixture."""
    from harmony_amd.dataloader import parse_graph

    with open(COMPONENTS) as f:
        src, dst, _w, max_id = parse_graph(f, weighted=False)
    return src.tolist(), dst.tolist(), max_id + 1


def union_find_labels():
    """Smallest id of every vertex's weak component, by union-find."""
    src, dst, n = components_edges()
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for s, d in zip(src, dst):
        a, b = find(s), find(d)
        if a != b:
            parent[max(a, b)] = min(a, b)     # the root is the smallest id
    return [float(find(v)) for v in range(n)]


def reachability_labels():
    """label(v) = the smallest id with a directed path to v (v included),
    by relaxing every edge until nothing changes."""
    src, dst, n = components_edges()
    label = list(range(n))
    changed = True
    while changed:
        changed = False
        for s, d in zip(src, dst):
            if label[s] < label[d]:
                label[d] = label[s]
                changed = True
    return [float(x) for x in label]


def read_parts(out_dir, world):
    vals = {}
    for r in range(world):
        with open(f"{out_dir}/part-{r}") as f:
            for ln in f:
                k, v = ln.split()
                assert int(k) not in vals
                vals[int(k)] = float(v)
    assert sorted(vals) == list(range(len(vals)))
    return [vals[k] for k in range(len(vals))]


def run_cc_job(device, out_dir, job_id, **extra):
    """run_pregel_job on the components fixture -> (labels, summary)."""
    from harmony_amd.config import JobConfig
    from harmony_amd.pregel.runner import run_pregel_job

    args = {"input": "file://" + COMPONENTS, "output": str(out_dir)}
    args.update(extra)
    job = JobConfig(job_id=job_id, app="connectedcomponents", app_args=args)
    s = run_pregel_job(job, make_ctx(device))
    return read_parts(str(out_dir), 1), s


# (fused_messages, direction)
CC_VARIANTS = [("false", "pull"), ("true", "pull"), ("true", "push"),
               ("true", "auto")]


def check_cc_fixture(device, tmp_path, tag):
    want = union_find_labels()
    assert len(want) == 16 and len(set(want)) == 5
    for fused, direction in CC_VARIANTS:
        got, s = run_cc_job(device, tmp_path / f"{fused}_{direction}",
                            f"cc_{fused}_{direction}_{tag}",
                            fused_messages=fused, direction=direction)
        assert got == want, (fused, direction)
        assert s["num_vertices"] == 16 and s["num_edges"] == 24
        assert s["direction"] == direction
        if direction == "push":
            assert s["push_supersteps"] == s["supersteps"]
            assert s["pull_supersteps"] == 0
    directed = reachability_labels()
    assert directed != want                  # -undirected matters here
    for fused, direction in CC_VARIANTS:
        got, s = run_cc_job(device, tmp_path / f"d_{fused}_{direction}",
                            f"ccd_{fused}_{direction}_{tag}",
                            fused_messages=fused, direction=direction,
                            undirected="false")
        assert got == directed, (fused, direction)
        assert s["num_edges"] == 12
