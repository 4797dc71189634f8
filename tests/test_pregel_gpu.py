"""Pregel pull kernel (K13) and the fused engine path on the GPU."""

import pytest
import torch

from tests import pregel_cases as pc

pytestmark = pytest.mark.gpu

GROUPS = [0, 1, 2, 4, 8, 16, 32, 64]      # 0 = the host rule's own choice


def _dev(t):
    return None if t is None else t.cuda()


def _pull_both(ix_args, combiner, add_weight, group):
    """(cpu reference result, gpu result, gpu result of a second run)."""
    from harmony_amd import ops

    in_ptr, in_src, in_w, w_const, vm, mask = ix_args
    ref = ops.pregel_pull(in_ptr, in_src, in_w, w_const, vm, mask, combiner,
                          add_weight)
    dargs = (_dev(in_ptr), _dev(in_src), _dev(in_w), w_const, _dev(vm),
             _dev(mask))
    runs = [ops.pregel_pull(*dargs, combiner, add_weight, _force_group=group)
            for _ in range(2)]
    return ref, [(o.cpu(), f.cpu()) for o, f in runs]


def _check(ref, runs, combiner, deg, abs_sum):
    (r_out, r_flag), (out, flag), (out2, flag2) = ref, runs[0], runs[1]
    assert out.dtype == torch.float32 and flag.dtype == torch.uint8
    assert torch.equal(flag, r_flag)
    if combiner == "min":
        assert torch.equal(out, r_out)
    else:
        err = (out.double() - r_out.double()).abs()
        assert bool((err <= pc.add_bound(deg, abs_sum)).all())
    # no atomics, fixed order: two runs agree bit for bit
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    assert torch.equal(flag, flag2)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("combiner,use_mask,use_w,add_weight",
                         pc.pull_configs())
def test_kernel_against_reference(combiner, use_mask, use_w, add_weight,
                                  group):
    ix = pc.handmade_index()
    in_w = ix["in_w"] if use_w else None
    mask = ix["mask"] if use_mask else None
    vm = ix["vert_msg_inf"] if combiner == "min" else ix["vert_msg"]
    args = (ix["in_ptr"], ix["in_src"], in_w, 1.5, vm, mask)
    ref, runs = _pull_both(args, combiner, add_weight, group)
    _o, _f, abs_sum, deg = pc.brute_force_pull(*args, combiner, add_weight)
    _check(ref, runs, combiner, deg, abs_sum)


@pytest.mark.parametrize("group", [1, 8, 64])
@pytest.mark.parametrize("combiner,ident", [("add", 0.0),
                                            ("min", float("inf"))])
def test_kernel_all_false_mask(combiner, ident, group):
    ix = pc.handmade_index()
    mask = torch.zeros(pc.NUM_SOURCES, dtype=torch.bool)
    args = (ix["in_ptr"], ix["in_src"], ix["in_w"], 0.0, ix["vert_msg"], mask)
    _ref, runs = _pull_both(args, combiner, True, group)
    out, flag = runs[0]
    assert int(flag.sum()) == 0
    assert torch.equal(out, torch.full((pc.NUM_ROWS,), ident))


@pytest.mark.parametrize("group", [1, 8, 64])
@pytest.mark.parametrize("combiner", ["add", "min"])
def test_kernel_one_row_and_no_rows(combiner, group):
    ix = pc.handmade_index()
    # R = 1: the 1000-edge row alone
    lo, hi = int(ix["in_ptr"][7]), int(ix["in_ptr"][8])
    in_ptr = torch.tensor([0, hi - lo])
    args = (in_ptr, ix["in_src"][lo:hi].contiguous(),
            ix["in_w"][lo:hi].contiguous(), 0.0, ix["vert_msg"], None)
    ref, runs = _pull_both(args, combiner, True, group)
    _o, _f, abs_sum, deg = pc.brute_force_pull(*args, combiner, True)
    assert runs[0][0].shape == (1,)
    _check(ref, runs, combiner, deg, abs_sum)
    # R = 0: nothing to launch, empty results
    args = (torch.zeros(1, dtype=torch.int64),
            torch.zeros(0, dtype=torch.int32), None, 0.0, ix["vert_msg"],
            None)
    ref, runs = _pull_both(args, combiner, False, group)
    assert runs[0][0].shape == (0,) and runs[0][1].shape == (0,)
    assert ref[0].shape == (0,)


# ------------------------------------------------ 7. engine on the fixtures

def _engine(app, graph_fn, n, fused, job_id, **kw):
    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.pregel.engine import PregelEngine
    from harmony_amd.pregel.graphapps import (PageRankComputation,
                                              ShortestPathComputation)
    from harmony_amd.runtime.bootstrap import init_executor
    from harmony_amd.runtime.control import ControlPlane

    ctx = init_executor(RuntimeConfig(device="cuda"))
    comp = (ShortestPathComputation(source=kw.get("source", 0))
            if app == "shortestpath"
            else PageRankComputation(num_iters=kw.get("num_iters", 10)))
    job = JobConfig(job_id=job_id, app=app, app_args={})
    engine = PregelEngine(job, comp, n, ctx, ControlPlane(ctx.store, 0, 1),
                          max_supersteps=200, fused=fused)
    g = graph_fn(ctx.device)
    engine.set_graph(g)
    return engine.run().squeeze(1).cpu(), g


def _fixture_graph(path, weighted):
    from harmony_amd.dataloader import (load_graph_partition,
                                        parse_graph_file)
    from harmony_amd.pregel.graphapps import make_graph_from_edges

    parsed = parse_graph_file(path, weighted)
    n = parsed[3] + 1
    row_ptr, dst, w, _n, _e = load_graph_partition(path, 0, n, weighted,
                                                   parsed=parsed)
    return n, lambda dev: make_graph_from_edges(row_ptr, dst, w, 0, n, dev)


def test_engine_fused_sssp_fixture():
    n, gf = _fixture_graph(pc.SHORTEST_PATH, True)
    d, _g = _engine("shortestpath", gf, n, True, "gpu_sp_fix")
    assert d.tolist() == pc.SSSP_FROM_0


def test_engine_fused_pagerank_fixture():
    _s, _d, n, ref, bound = pc.adj_list_reference(10)
    n2, gf = _fixture_graph(pc.ADJ_LIST, False)
    assert n2 == n
    v, _g = _engine("pagerank", gf, n, True, "gpu_pr_fix", num_iters=10)
    err = (v.double() - ref).abs()
    print("max err / bound:", float((err / bound).max()))
    assert bool((err <= bound).all()), float((err / bound).max())


# --------------------------------------- 8. synthetic, fused against unfused

def _synthetic(n=4096, deg=8):
    from harmony_amd.pregel.graphapps import make_ring_plus_random_graph

    return lambda dev: make_ring_plus_random_graph(n, deg, 0, n, dev, 4242)


def test_synthetic_pagerank_fused_matches_unfused():
    n, deg, iters = 4096, 8, 10
    fused, g = _engine("pagerank", _synthetic(n, deg), n, True, "gpu_pr_f",
                       num_iters=iters)
    plain, _g = _engine("pagerank", _synthetic(n, deg), n, False, "gpu_pr_u",
                        num_iters=iters)
    src = torch.arange(n).repeat_interleave(deg)
    ref, bound = pc.pagerank_f64(src, g.edge_dst.cpu(), n, iters)
    err = (fused.double() - plain.double()).abs()
    print("max |fused - unfused| / bound:", float((err / bound).max()),
          " max |fused - f64| / bound:",
          float(((fused.double() - ref).abs() / bound).max()))
    assert bool((err <= bound).all())
    assert bool(((fused.double() - ref).abs() <= bound).all())


def test_synthetic_sssp_fused_equals_unfused():
    n, deg = 4096, 8
    fused, _g = _engine("shortestpath", _synthetic(n, deg), n, True,
                        "gpu_sp_f")
    plain, _g = _engine("shortestpath", _synthetic(n, deg), n, False,
                        "gpu_sp_u")
    assert bool(torch.isfinite(plain).all())      # the ring reaches everyone
    assert torch.equal(fused, plain)


def test_job_auto_picks_fused_on_gpu(tmp_path):
    """run_pregel_job: -fused_messages auto is on with a GPU and the
    extension; -input/-output work on cuda."""
    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.pregel.runner import run_pregel_job
    from harmony_amd.runtime.bootstrap import init_executor

    ctx = init_executor(RuntimeConfig(device="cuda"))
    out = tmp_path / "out"
    job = JobConfig(job_id="gpu_job_sp", app="shortestpath",
                    app_args={"input": pc.SHORTEST_PATH, "output": str(out)})
    s = run_pregel_job(job, ctx)
    assert s["fused_messages"] is True and s["num_edges"] == 30
    got = [float(ln.split()[1]) for ln in open(out / "part-0")]
    assert got == pc.SSSP_FROM_0
