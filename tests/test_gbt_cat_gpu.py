"""K10b (ops/csrc/gbt_split.hip) on the GPU: every case of gbt_cat_cases
through the kernel against the fp64 checker (run on the CPU from the kernel's
outputs), bit-identical reruns, the nb > 64 torch path, K10 -> K10b ->
routing through build_tree, and whole typed jobs."""

import pytest
import torch

from tests import gbt_cat_cases as gc

pytestmark = pytest.mark.gpu

_CASES = gc.all_cases()


def _split(case, device="cuda"):
    from harmony_amd import ops

    return ops.gbt_best_split(case["cnt"].to(device), case["s"].to(device),
                              case["ftype"].to(device), case["lam"])


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("idx", range(len(_CASES)))
def test_kernel_vs_fp64(idx):
    case = _CASES[idx]
    outs = _split(case)
    assert all(t.is_cuda for t in outs)
    worst = gc.check(case, outs, "K10b")
    print(f"{case['name']}: worst shortfall / bound {worst:.3f}")
    again = _split(case)
    for a, b in zip(outs, again):           # checker item 3: bit-identical
        assert torch.equal(_bits(a), _bits(b)), case["name"]


def test_kernel_is_what_runs():
    # the binding itself, not the wrapper's torch path
    from harmony_amd import ops

    case = _CASES[-2]
    hip = ops._load_hip()
    outs = hip.gbt_best_split(case["cnt"].cuda(), case["s"].cuda(),
                              case["ftype"].cuda(), case["lam"])
    gc.check(case, outs, "binding")
    with pytest.raises(RuntimeError, match="nb must be"):
        hip.gbt_best_split(torch.zeros(1, 1, 65).cuda(),
                           torch.zeros(1, 1, 65).cuda(),
                           case["ftype"][:1].cuda(), 1.0)


@pytest.mark.parametrize("kind", ["cont", "mixed"])
def test_nb65_takes_the_torch_path(kind):
    case = gc.random_case(8, 5, 65, kind, 1.0, seed=65)
    outs = _split(case)
    assert all(t.is_cuda for t in outs)
    gc.check(case, outs, "nb65")


def test_build_tree_isolates_category_subset_gpu():
    from harmony_amd.mlapps.gbt import build_tree

    bins, y, types = gc.subset_fixture("cuda")
    t = build_tree(bins, y, 16, 1, 1.0, feature_types=types)
    assert t.feature == [2] and t.threshold == [-2]
    assert t.cat_mask == [0x52]
    pred = t.predict_bins(bins)
    assert pred.is_cuda and bool((torch.sign(pred) == y).all())
    u = build_tree(bins, y, 16, 1, 1.0)
    assert u.cat_mask is None
    assert int((torch.sign(u.predict_bins(bins)) != y).sum()) >= 1


def test_zero_types_match_untyped_build_gpu():
    # deeper than one level: K10 -> K10b -> device routing, level by level
    from harmony_amd.mlapps.gbt import build_tree

    g = torch.Generator().manual_seed(3)
    bins = torch.randint(0, 32, (700, 6), generator=g).cuda()
    resid = torch.randint(-4, 5, (700,), generator=g).float().cuda()
    a = build_tree(bins, resid, 32, 4, 1.0)
    b = build_tree(bins, resid, 32, 4, 1.0,
                   feature_types=torch.zeros(6, dtype=torch.int32))
    assert torch.equal(a.predict_bins(bins), b.predict_bins(bins))


def _run(job):
    from harmony_amd.config import RuntimeConfig
    from harmony_amd.dolphin.master import run_job
    from harmony_amd.runtime.bootstrap import init_executor

    return run_job(job, init_executor(RuntimeConfig(device="cuda"))).summary()


def _job(job_id, **kw):
    from harmony_amd.config import JobConfig

    args = {"num_features": 8, "batch_size": 512, "num_bins": 32,
            "max_depth": 3, "step_size": 0.3, "num_categorical": 2,
            "num_categories": 8}
    args.update(kw)
    return JobConfig(job_id=job_id, app="gbt", max_num_epochs=2,
                     num_mini_batches=2, app_args=args)


def test_typed_regression_job_gpu():
    s = _run(_job("g_gbt_cat"))
    assert s["num_batches"] == 4 and s["num_trees"] == 4
    assert s["mse"] == s["mse"]                        # finite, not NaN


def test_typed_multiclass_job_gpu():
    s = _run(_job("g_gbt_cat_mc", objective="multiclass", num_classes=3))
    assert s["num_batches"] == 4 and s["num_trees"] == 3 * 4
    assert 0.0 <= s["error_rate"] <= 1.0
