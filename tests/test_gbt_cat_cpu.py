"""GBT feature types on the CPU: the torch path of ops.gbt_best_split (K10b's
oracle) against the fp64 checker and an exhaustive subset search, typed
build_tree / predict, quantize, the tree codec, the metadata file and whole
jobs."""

import copy
import pickle

import numpy as np
import pytest
import torch

from tests import gbt_cat_cases as gc

_CASES = gc.all_cases()


@pytest.mark.parametrize("idx", range(len(_CASES)))
def test_torch_path_vs_fp64(idx):
    from harmony_amd import ops

    case = _CASES[idx]
    outs = ops.gbt_best_split(case["cnt"], case["s"], case["ftype"],
                              case["lam"])
    worst = gc.check(case, outs, "torch")
    print(f"{case['name']}: worst shortfall / bound {worst:.3f}")


def test_cases_cover_the_listed_contents():
    # the builder's own promises: every shape, and every planted situation
    shapes = {tuple(c["cnt"].shape) for c in _CASES}
    for n, F, nb in gc.SHAPES:
        assert (n, F, nb) in shapes
    kinds = set()
    for c in gc.shape_cases():
        t = c["ftype"]
        kinds.add("cont" if not t.any() else "cat" if t.all() else "mixed")
    assert kinds == {"cont", "cat", "mixed"}
    p = gc.planted_case(64)
    live = (p["cnt"] > 0).sum(dim=2)
    assert int(live[7, 1]) == 64 and int(live[0, 1]) == 1
    assert int(live[5, 1]) == 2 and not p["cnt"][2].any()
    assert {v[1] for v in p["planted"].values()} >= {-2, -1, 10}


def _exhaustive_run(lam, seed):
    """The op against the exhaustive optimum on 200 histograms of at most
    10 live categories: (worst relative shortfall, worst shortfall / bound,
    worst excess / bound), the bound that of checker item 2."""
    from harmony_amd import ops

    cnt, s = gc.random_categorical(200, 16, 10, seed)
    ftype = torch.tensor([5], dtype=torch.int32)
    _, thr, mask, _ = ops.gbt_best_split(cnt, s, ftype, lam)
    rel, short, excess = 0.0, -np.inf, -np.inf
    for i in range(cnt.shape[0]):
        c, v = cnt[i, 0].tolist(), s[i, 0].tolist()
        best, terms = gc.exhaustive_best(c, v, lam)
        got = gc.returned_gain64(c, v, lam, int(thr[i]), int(mask[i]))
        bound = gc.ULPS * terms
        if got is None:                     # pass-through: nothing to gain
            assert best <= gc.MIN_GAIN + bound, (i, best)
            continue
        if best > 0:
            rel = max(rel, (best - got) / best)
        short = max(short, (best - got) / bound)
        excess = max(excess, (got - best) / bound)
    return rel, short, excess


def test_lam0_scan_equals_exhaustive_subsets():
    # Fisher: for lam = 0 the optimum over all subsets is a cut of the mean
    # order
    rel, short, excess = _exhaustive_run(0.0, seed=11)
    print(f"lam 0: worst relative shortfall of the mean-ordered scan "
          f"against all subsets {rel:.3e}")
    assert short <= 1.0 and excess <= 1.0, (short, excess)


@pytest.mark.parametrize("lam", [1.0, 10.0])
def test_lam_positive_never_beats_exhaustive(lam):
    rel, short, excess = _exhaustive_run(lam, seed=12)
    print(f"lam {lam:g}: worst relative shortfall of the mean-ordered scan "
          f"against all subsets {rel:.3e}")
    assert excess <= 1.0, excess


# ------------------------------------------------------------- build_tree

def test_build_tree_isolates_category_subset():
    from harmony_amd.mlapps.gbt import build_tree

    bins, y, types = gc.subset_fixture()
    t = build_tree(bins, y, 16, 1, 1.0, feature_types=types)
    assert t.feature == [2] and t.threshold == [-2]
    assert t.cat_mask == [0x52]
    pred = t.predict_bins(bins)
    assert bool((torch.sign(pred) == y).all())
    # the same data without types: no single threshold isolates {1, 4, 6}
    u = build_tree(bins, y, 16, 1, 1.0)
    assert u.cat_mask is None
    assert int((torch.sign(u.predict_bins(bins)) != y).sum()) >= 1


def test_unseen_category_goes_left():
    from harmony_amd.mlapps.gbt import GBTree

    t = GBTree(1, [0], [-2], [-1.0, 1.0], [0x52])
    out = t.predict_bins(torch.tensor([[1], [4], [6], [0], [9], [63]]))
    assert out.tolist() == [1.0, 1.0, 1.0, -1.0, -1.0, -1.0]
    t63 = GBTree(1, [0], [-2], [-1.0, 1.0], [gc.signed64(1 << 63)])
    assert t63.predict_bins(torch.tensor([[63], [62]])).tolist() == [1., -1.]


def test_zero_types_match_untyped_build():
    from harmony_amd.mlapps.gbt import build_tree

    g = torch.Generator().manual_seed(3)
    bins = torch.randint(0, 32, (700, 6), generator=g)
    resid = torch.randint(-4, 5, (700,), generator=g).float()
    a = build_tree(bins, resid, 32, 4, 1.0)
    b = build_tree(bins, resid, 32, 4, 1.0,
                   feature_types=torch.zeros(6, dtype=torch.int32))
    assert a.cat_mask is None and b.cat_mask == [0] * 15
    assert torch.equal(a.predict_bins(bins), b.predict_bins(bins))


# --------------------------------------------------------------- quantize

def test_quantize_with_types():
    from harmony_amd.mlapps.gbt import quantize

    g = torch.Generator().manual_seed(5)
    X = torch.randn(300, 4, generator=g)
    X[:, 2] = torch.randint(0, 8, (300,), generator=g).float()
    types = torch.tensor([0, 0, 8, 0], dtype=torch.int32)
    plain = quantize(X, 16)
    typed = quantize(X, 16, types)
    assert typed.dtype == plain.dtype
    assert torch.equal(typed[:, 2], X[:, 2].long())
    for f in (0, 1, 3):
        assert torch.equal(typed[:, f], plain[:, f])
    assert torch.equal(quantize(X, 16, None), plain)
    for bad in (-1.0, 2.5, 16.0):
        Y = X.clone()
        Y[17, 2] = bad
        with pytest.raises(ValueError, match=r"feature 2.*" + str(bad)):
            quantize(Y, 16, types)


# ------------------------------------------------------------------ codec

def _tree(depth, seed, masks):
    from harmony_amd.mlapps.gbt import GBTree

    g = torch.Generator().manual_seed(seed)
    ni = (1 << depth) - 1
    return GBTree(
        depth=depth,
        feature=torch.randint(0, 50, (ni,), generator=g).tolist(),
        threshold=torch.randint(-2, 30, (ni,), generator=g).tolist(),
        leaf_value=torch.randn(1 << depth, generator=g).tolist(),
        cat_mask=masks)


def test_codec_masks_roundtrip_and_layouts():
    from harmony_amd.mlapps.gbt import decode_trees, encode_trees

    depth, ni = 2, 3
    base = 1 + 2 * ni + (1 << depth)
    masks = [gc.signed64(1 << 63), 1 << 31, gc.signed64((1 << 63) | (1 << 31)
                                                        | 5)]
    old = _tree(depth, 1, None)
    new = _tree(depth, 2, masks)
    e_old = encode_trees([(0, old)], depth)
    e_new = encode_trees([(3, new)], depth)
    assert e_old.shape == (1, base) and e_old.dtype == torch.int32
    assert e_new.shape == (1, base + 2 * ni) and e_new.dtype == torch.int32
    (k, t), = decode_trees(e_new, depth)
    assert k == 3 and t.cat_mask == masks
    assert t.feature == new.feature and t.threshold == new.threshold
    (k, t), = decode_trees(e_old, depth)
    assert k == 0 and t.cat_mask is None
    # a batch with any masked tree is extended as a whole (equal row length
    # for the all-gather); a tree without masks sends zeros
    both = encode_trees([(0, old), (3, new)], depth)
    assert both.shape == (2, base + 2 * ni)
    d = decode_trees(both, depth)
    assert d[0][1].cat_mask == [0] * ni and d[1][1].cat_mask == masks
    # rows of the two layouts, mixed: told apart by their length
    d = decode_trees([e_old[0], e_new[0], e_old[0]], depth)
    assert [t.cat_mask for _, t in d] == [None, masks, None]
    assert d[2][1].threshold == old.threshold


def test_tree_pickled_without_the_field_predicts_as_before():
    from harmony_amd.mlapps.gbt import GBTree

    t = GBTree(depth=2, feature=[0, 1, 1], threshold=[2, 1, -1],
               leaf_value=[10.0, 20.0, 30.0, 40.0])
    legacy = copy.copy(t)
    del legacy.__dict__["cat_mask"]            # as pickled before the field
    assert "cat_mask" not in legacy.__dict__
    back = pickle.loads(pickle.dumps(legacy))
    assert "cat_mask" not in back.__dict__ and back.cat_mask is None
    bins = torch.tensor([[0, 0], [0, 5], [5, 0], [5, 9]])
    assert back.predict_bins(bins).tolist() == [10.0, 20.0, 30.0, 30.0]


# ------------------------------------------------------- metadata and jobs

def _run(job):
    from harmony_amd.config import RuntimeConfig
    from harmony_amd.dolphin.master import run_job
    from harmony_amd.runtime.bootstrap import init_executor

    return run_job(job, init_executor(RuntimeConfig(device="cpu"))).summary()


def _golden_job(**kw):
    from harmony_amd.config import JobConfig

    args = {"input": str(gc.GOLDEN), "num_features": 4, "num_bins": 8,
            "max_depth": 2, "step_size": 0.5}
    args.update(kw)
    return JobConfig(job_id="t_gbt_cat_file", app="gbt", max_num_epochs=2,
                     num_mini_batches=2, app_args=args)


def test_metadata_types_and_unbinned_column(tmp_path):
    from harmony_amd import dataloader as dl
    from harmony_amd.mlapps import gbt

    job = _golden_job()
    types = gbt.feature_types(gbt.defaults(job))
    assert types.dtype == torch.int32 and types.tolist() == [0, 0, 0, 4]
    X, y = dl.parse_libsvm_split(str(gc.GOLDEN), 0, 1, 4)
    assert X.shape == (32, 4)
    blocks = gbt.make_batches(job, 0, torch.device("cpu"))
    assert len(blocks) == 2
    got = torch.cat([b[0] for b in blocks])
    assert torch.equal(got[:, 3], X[:, 3].long())
    assert set(got[:, 3].tolist()) == {0, 1, 2, 3}
    # the explicit `metadata` argument, and files that give no types
    empty = tmp_path / "none.meta"
    empty.write_text("0:0 1:0 4:7\n")          # only the y-entry is non-zero
    for meta in (str(empty), str(tmp_path / "missing.meta")):
        j = _golden_job(metadata=meta)
        assert gbt.feature_types(gbt.defaults(j)) is None
        plain = torch.cat([b[0] for b in
                           gbt.make_batches(j, 0, torch.device("cpu"))])
        assert torch.equal(plain[:, :3], got[:, :3])
    part = tmp_path / "part.meta"
    part.write_text("3:4\n")                   # unnamed features: continuous
    j = _golden_job(metadata=str(part))
    assert gbt.feature_types(gbt.defaults(j)).tolist() == [0, 0, 0, 4]


def test_job_over_the_fixture():
    s = _run(_golden_job())
    assert s["num_batches"] == 4
    assert s["num_trees"] == 4


def _synthetic_job(job_id, **kw):
    from harmony_amd.config import JobConfig

    args = {"num_features": 8, "batch_size": 1024, "num_bins": 32,
            "max_depth": 2, "step_size": 0.3, "noise": 0.05,
            "num_categorical": 2, "num_categories": 8}
    args.update(kw)
    return JobConfig(job_id=job_id, app="gbt", max_num_epochs=4,
                     num_mini_batches=2, app_args=args)


def test_synthetic_job_types_beat_ordinal_binning(monkeypatch):
    from harmony_amd.mlapps import gbt

    job = _synthetic_job("t_gbt_cat_syn")
    typed = _run(job)
    # the same data with the types suppressed: the category ids are binned
    # like any other column and split by thresholds
    monkeypatch.setattr(gbt, "feature_types", lambda app_args: None)
    plain = _run(job)
    print(f"final mse with types {typed['mse']:.4f}, "
          f"without {plain['mse']:.4f}")
    assert typed["num_trees"] == plain["num_trees"] == 8
    assert typed["mse"] < plain["mse"]


def _todays_generator(job, rank, device):
    """The synthetic branch of make_batches as it was before feature types
    (regression and multiclass), inlined."""
    from harmony_amd.mlapps import gbt
    from harmony_amd.utils import stable_seed

    a = gbt.defaults(job)
    F = a["num_features"]
    g = torch.Generator().manual_seed(stable_seed(job.job_id, "data", rank))
    w = torch.randn(F, generator=g)
    mc = a["objective"] == "multiclass"
    if mc:
        W = torch.randn(a["num_classes"], F, generator=g)
    blocks = []
    n_blocks = job.num_worker_blocks or job.num_mini_batches
    for _ in range(n_blocks):
        X = torch.randn(a["batch_size"], F, generator=g)
        if mc:
            y = (X @ W.t() + a["noise"]
                 * torch.randn(a["batch_size"], a["num_classes"],
                               generator=g)).argmax(dim=1).float()
        else:
            y = (X @ w + torch.sin(3 * X[:, 0]) * 2
                 + a["noise"] * torch.randn(a["batch_size"], generator=g))
        qs = torch.quantile(X, torch.linspace(0, 1, a["num_bins"] + 1)[1:-1],
                            dim=0)
        bins = torch.searchsorted(qs.t().contiguous(), X.t().contiguous()
                                  ).t().contiguous().clamp_(
                                      0, a["num_bins"] - 1)
        blocks.append((bins.to(device), y.to(device)))
    return blocks


@pytest.mark.parametrize("objective", ["regression", "multiclass"])
def test_no_categorical_batches_are_bit_identical(objective):
    from harmony_amd.mlapps import gbt

    job = _synthetic_job("t_gbt_cat_same", num_categorical=0,
                         batch_size=257, objective=objective)
    assert gbt.feature_types(gbt.defaults(job)) is None
    now = gbt.make_batches(job, 0, torch.device("cpu"))
    then = _todays_generator(job, 0, torch.device("cpu"))
    assert len(now) == len(then) == 2
    for (b0, y0), (b1, y1) in zip(now, then):
        assert b0.dtype == b1.dtype and torch.equal(b0, b1)
        assert torch.equal(y0.view(torch.int32), y1.view(torch.int32))


def test_synthetic_categorical_columns():
    from harmony_amd.mlapps import gbt

    job = _synthetic_job("t_gbt_cat_cols", batch_size=300)
    types = gbt.feature_types(gbt.defaults(job))
    assert types.tolist() == [0] * 6 + [8, 8]
    for bins, y in gbt.make_batches(job, 0, torch.device("cpu")):
        assert set(bins[:, 6].tolist()) == set(range(8))
        assert int(bins[:, 6:].max()) == 7 and int(bins[:, 6:].min()) == 0
