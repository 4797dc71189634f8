"""Sparse GBT on the GPU: K10s (ops/csrc/gbt_hist_sparse.hip) against fp64,
the binding called directly, tree equality through K10s, K10b and bin_of
routing, and one job over a feature space no dense batch fits."""

import json
import math
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from harmony_amd import ops
from harmony_amd.mlapps import gbt
from tests import gbt_sparse_cases as gc

pytestmark = pytest.mark.gpu

DEV = "cuda"
REPO = str(Path(__file__).resolve().parents[1])
TORCH_PATH_CASE = 3          # n_nodes * nb = 8192 + nb


def _node_totals(resid, node, n_nodes):
    cnt = torch.zeros(n_nodes, device=resid.device).scatter_add_(
        0, node.long(), torch.ones_like(resid))
    s = torch.zeros(n_nodes, device=resid.device).scatter_add_(
        0, node.long(), resid)
    return cnt, s


@pytest.mark.parametrize("idx", range(len(gc.SHAPES)))
def test_kernel_vs_fp64(idx):
    case = gc.make_case(idx)
    args = gc.hist_args(case, DEV)
    cnt, s = ops.gbt_hist_sparse(*args)
    assert cnt.device.type == "cuda"
    ratio = gc.check_hist(case, cnt, s, f"case {idx}")
    print(f"case {idx}: nf {cnt.shape[1]}, sum error / bound {ratio:.4f}")
    cnt2, s2 = ops.gbt_hist_sparse(*args)
    assert torch.equal(cnt.view(torch.int32), cnt2.view(torch.int32))
    gc.check_hist(case, cnt2, s2, f"case {idx}, second run")


@pytest.mark.parametrize("idx", [0, 1, 2, 4, 7])
def test_binding_is_the_kernel(idx):
    case = gc.make_case(idx)
    hip = ops._load_hip()
    assert hip is not None and hasattr(hip, "gbt_hist_sparse")
    ptr, row, fbin, fidx, zb, resid, node, n_nodes, nb = gc.hist_args(
        case, DEV)
    nc, ns = _node_totals(resid, node, n_nodes)
    cnt, s = hip.gbt_hist_sparse(ptr, row, fbin, fidx, zb, resid,
                                 node.int(), nc, ns, nb)
    gc.check_hist(case, cnt, s, f"binding, case {idx}")
    # the wrapper's result is this call's
    wcnt, _ = ops.gbt_hist_sparse(ptr, row, fbin, fidx, zb, resid, node,
                                  n_nodes, nb)
    assert torch.equal(cnt, wcnt)


def test_over_wide_level():
    # the binding refuses n_nodes * nb > 8192; the wrapper takes the torch
    # path there, as its docstring says
    case = gc.make_case(TORCH_PATH_CASE)
    hip = ops._load_hip()
    assert case["n_nodes"] * case["nb"] > hip.gbt_hist_sparse_max_cells()
    assert hip.gbt_hist_sparse_max_cells() == ops.GBT_HIST_MAX_CELLS
    ptr, row, fbin, fidx, zb, resid, node, n_nodes, nb = gc.hist_args(
        case, DEV)
    nc, ns = _node_totals(resid, node, n_nodes)
    with pytest.raises(RuntimeError, match="too wide"):
        hip.gbt_hist_sparse(ptr, row, fbin, fidx, zb, resid, node.int(),
                            nc, ns, nb)
    cnt, s = ops.gbt_hist_sparse(ptr, row, fbin, fidx, zb, resid, node,
                                 n_nodes, nb)
    gc.check_hist(case, cnt, s, "torch path on the device")


def test_no_present_feature_launches_nothing():
    hip = ops._load_hip()
    z32 = torch.zeros(0, dtype=torch.int32, device=DEV)
    cnt, s = hip.gbt_hist_sparse(
        torch.zeros(1, dtype=torch.int64, device=DEV), z32, z32, z32, z32,
        torch.ones(4, device=DEV), torch.zeros(4, dtype=torch.int32,
                                               device=DEV),
        torch.full((1,), 4.0, device=DEV), torch.full((1,), 4.0, device=DEV),
        8)
    assert cnt.shape == s.shape == (1, 0, 8)


@pytest.mark.parametrize("idx", range(len(gc.TREE_SHAPES)))
def test_sparse_tree_equals_dense_tree(idx):
    case = gc.make_tree_case(idx)
    resid = case["resid"].to(DEV)
    types = case["types"].to(DEV)
    dense_bins = case["dense_bins"].to(DEV)
    sb = case["sb"].to(DEV)
    dense = gbt.build_tree(dense_bins, resid, gc.TREE_NB, gc.TREE_DEPTH,
                           gc.TREE_LAM, types)
    assert gc.n_splits(dense) >= 4
    sparse = gbt.build_tree(sb, resid, gc.TREE_NB, gc.TREE_DEPTH,
                            gc.TREE_LAM, types)
    gc.assert_same_tree(sparse, dense, f"tree case {idx}")
    # and the tree the CPU builds from the same data
    cpu = gbt.build_tree(case["sb"], case["resid"], gc.TREE_NB,
                         gc.TREE_DEPTH, gc.TREE_LAM, case["types"])
    gc.assert_same_tree(sparse, cpu, f"tree case {idx}, CPU")
    assert torch.equal(sparse.predict_bins(sb),
                       dense.predict_bins(dense_bins))


# The wide job of test_wide_job_stays_small, run in a process of its own: the
# limit is on torch.cuda.max_memory_allocated() of the process that runs the
# job, and in the suite's process tensors other tests left behind count too.
_WIDE_JOB = """
import json, sys
import torch
sys.path.insert(0, ".")
from harmony_amd import ops
from harmony_amd.config import JobConfig, RuntimeConfig
from harmony_amd.dolphin.master import run_job
from harmony_amd.mlapps import gbt
from harmony_amd.mlapps.sparse_bins import SparseBins
from harmony_amd.runtime.bootstrap import init_executor

calls = []
hip = ops._load_hip()
class Spy:
    def __getattr__(self, name):
        return getattr(hip, name)
    def gbt_hist_sparse(self, *a):
        calls.append(1)
        return hip.gbt_hist_sparse(*a)
ops._hip = Spy()
job = JobConfig(job_id="t_gbt_sparse_wide", app="gbt", max_num_epochs=1,
                num_mini_batches=2,
                app_args={"num_features": 2 ** 20, "batch_size": 256,
                          "nnz_per_row": 8, "max_depth": 3, "num_bins": 32,
                          "sparse": "true"})
ctx = init_executor(RuntimeConfig(device="cuda"))
blocks = gbt.make_batches(job, 0, torch.device("cuda"))
ok = all(isinstance(x, SparseBins) and x.shape == (256, 2 ** 20)
         and x.feat_ids.shape[0] <= 2048 for x, _y in blocks)
s = run_job(job, ctx).summary()
torch.cuda.synchronize()
print("RESULT " + json.dumps({
    "blocks_ok": ok, "kernel_calls": len(calls),
    "num_batches": s["num_batches"], "num_trees": s["num_trees"],
    "mse": s["mse"], "peak": torch.cuda.max_memory_allocated()}))
"""


def test_wide_job_stays_small():
    out = subprocess.run([sys.executable, "-c", _WIDE_JOB],
                         capture_output=True, text=True, timeout=120,
                         cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    r = json.loads(line[-1][len("RESULT "):])
    print(f"wide job: peak allocated {r['peak'] / 2 ** 20:.2f} MiB")
    assert r["blocks_ok"]
    assert r["kernel_calls"] == 2 * 3        # K10s once per tree level
    assert r["num_batches"] == 2 and r["num_trees"] == 2
    assert math.isfinite(r["mse"])
    assert r["peak"] < 64 * 2 ** 20
