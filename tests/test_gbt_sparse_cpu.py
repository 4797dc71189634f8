"""Sparse GBT on the CPU: SparseBins against quantize on the densified block,
the torch path of ops.gbt_hist_sparse against fp64, tree equality with the
dense builder, the sparse fixture and whole jobs."""

import math

import pytest
import torch

from harmony_amd import ops
from harmony_amd.mlapps import gbt
from harmony_amd.mlapps.sparse_batch import SparseBatch
from harmony_amd.mlapps.sparse_bins import SparseBins
from tests import gbt_sparse_cases as gc

ALL = range(len(gc.SHAPES))


# -------------------------------------------------------------- SparseBins

@pytest.mark.parametrize("idx", ALL)
def test_bins_equal_quantize_of_the_dense_block(idx):
    case = gc.make_case(idx)
    sb = case["sb"]
    assert sb.shape == (case["B"], case["F"])
    assert sb.nnz == int(case["mask"].sum())
    assert torch.equal(sb.to_dense_bins(), case["dense_bins"])
    # the stored order: keys sorted, features ascending, rows ascending
    # within a feature
    assert bool((sb.keys[1:] > sb.keys[:-1]).all())
    assert bool((sb.feat_ids[1:] > sb.feat_ids[:-1]).all())
    seg = sb.feat_idx.long() * case["B"] + sb.feat_row.long()
    assert bool((seg[1:] > seg[:-1]).all())
    assert int(sb.feat_ptr[-1]) == sb.nnz
    assert sb.feat_ids.shape[0] == int(case["mask"].any(dim=0).sum())


def test_from_a_sparse_batch():
    case = gc.make_case(0)
    row_ptr, col, val = case["csr"]
    sb = SparseBins(SparseBatch(row_ptr, col, val, case["F"]), case["nb"],
                    case["types"])
    assert torch.equal(sb.to_dense_bins(), case["dense_bins"])
    assert sb.to("cpu").device.type == "cpu"


@pytest.mark.parametrize("value", [-1.0, 2.5, 64.0, float("inf")])
def test_bad_category_raises_as_quantize(value):
    case = gc.make_case(0)
    F, nb = case["F"], case["nb"]
    X = case["X"].clone()
    mask = case["mask"].clone()
    r = int(mask[:, F - 1].nonzero()[3])
    X[r, F - 1] = value
    with pytest.raises(ValueError) as dense:
        gbt.quantize(X, nb, case["types"])
    with pytest.raises(ValueError) as sparse:
        SparseBins((*gc._csr_from_dense_mask(X, mask), F), nb, case["types"])
    assert str(sparse.value) == str(dense.value)


@pytest.mark.parametrize("idx", ALL)
def test_bin_of_equals_the_dense_gather(idx):
    case = gc.make_case(idx)
    B, F = case["B"], case["F"]
    g = torch.Generator().manual_seed(idx)
    ids = case["sb"].feat_ids.long()
    for feat in (torch.randint(0, F, (B,), generator=g),
                 ids[torch.randint(0, ids.shape[0], (B,), generator=g)],
                 torch.zeros(B, dtype=torch.int64),
                 torch.full((B,), F - 1, dtype=torch.int64)):
        want = case["dense_bins"].gather(1, feat.unsqueeze(1)).squeeze(1)
        got = case["sb"].bin_of(feat)
        assert got.dtype == torch.int64 and torch.equal(got, want)


@pytest.mark.parametrize("idx", ALL)
def test_prefix_equals_the_slice_of_the_dense_bins(idx):
    case = gc.make_case(idx)
    B = case["B"]
    for n in (0, 1, B):
        p = case["sb"].prefix(n)
        assert p.shape == (n, case["F"])
        assert torch.equal(p.to_dense_bins(), case["dense_bins"][:n])
        assert int(p.feat_ptr[-1]) == p.nnz == int(case["mask"][:n].sum())
        feat = torch.arange(n) % case["F"]
        assert torch.equal(
            p.bin_of(feat),
            case["dense_bins"][:n].gather(1, feat.unsqueeze(1)).squeeze(1))


def test_no_tensor_of_batch_times_features():
    B, F, k = 256, 2 ** 20, 8
    g = torch.Generator().manual_seed(5)
    cols = torch.randint(0, F, (B, k), generator=g).sort(dim=1).values
    keep = torch.ones((B, k), dtype=torch.bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    row_ptr = torch.zeros(B + 1, dtype=torch.int64)
    row_ptr[1:] = torch.cumsum(keep.sum(dim=1), 0)
    sb = SparseBins((row_ptr, cols[keep], torch.randn(int(keep.sum()),
                                                      generator=g), F), 32)
    largest = max(getattr(sb, name).numel() for name in (
        "keys", "key_bin", "feat_ids", "feat_ptr", "feat_row", "feat_bin",
        "feat_idx", "zero_bin"))
    assert largest <= B * k + 1


# ---------------------------------------------------------------- torch op

@pytest.mark.parametrize("idx", ALL)
def test_torch_path_vs_fp64(idx):
    case = gc.make_case(idx)
    cnt, s = ops.gbt_hist_sparse(*gc.hist_args(case))
    ratio = gc.check_hist(case, cnt, s, f"case {idx}")
    print(f"case {idx}: nf {cnt.shape[1]}, sum error / bound {ratio:.4f}")


def test_check_sees_a_moved_entry():
    case = gc.make_case(0)
    cnt, s = ops.gbt_hist_sparse(*gc.hist_args(case))
    bad = cnt.clone()
    bad[0, 0, 0] += 1
    with pytest.raises(AssertionError):
        gc.check_hist(case, bad, s)
    bad = s.clone()
    bad[0, 0] += 1e-2
    with pytest.raises(AssertionError):
        gc.check_hist(case, cnt, bad)


def test_no_present_feature_gives_empty_histograms():
    B = 4
    sb = SparseBins((torch.zeros(B + 1, dtype=torch.int64),
                     torch.zeros(0, dtype=torch.int32), torch.zeros(0), 9), 8)
    assert sb.feat_ids.shape[0] == 0 and sb.nnz == 0
    cnt, s = ops.gbt_hist_sparse(
        sb.feat_ptr, sb.feat_row, sb.feat_bin, sb.feat_idx, sb.zero_bin,
        torch.ones(B), torch.zeros(B, dtype=torch.int64), 1, 8)
    assert cnt.shape == s.shape == (1, 0, 8)
    tree = gbt.build_tree(sb, torch.ones(B), 8, 2, 1.0)
    assert tree.threshold == [-1] * 3 and tree.feature == [0] * 3
    assert tree.leaf_value[0] == pytest.approx(4 / 5)


# ---------------------------------------------------------- tree equality

@pytest.mark.parametrize("idx", range(len(gc.TREE_SHAPES)))
def test_sparse_tree_equals_dense_tree(idx):
    case = gc.make_tree_case(idx)
    dense = gbt.build_tree(case["dense_bins"], case["resid"], gc.TREE_NB,
                           gc.TREE_DEPTH, gc.TREE_LAM, case["types"])
    assert gc.n_splits(dense) >= 4
    assert -2 in dense.threshold         # the categorical column is used
    sparse = gbt.build_tree(case["sb"], case["resid"], gc.TREE_NB,
                            gc.TREE_DEPTH, gc.TREE_LAM, case["types"])
    gc.assert_same_tree(sparse, dense, f"tree case {idx}")
    assert torch.equal(sparse.predict_bins(case["sb"]),
                       dense.predict_bins(case["dense_bins"]))


def test_untyped_sparse_tree():
    # without feature types: zeros for the split search, cat_mask None
    case = gc.make_tree_case(1)
    X = case["X"]
    dense_bins = gbt.quantize(X, gc.TREE_NB)
    mask = X != 0
    sb = SparseBins((*gc._csr_from_dense_mask(X, mask), case["F"]),
                    gc.TREE_NB)
    zeros = torch.zeros(case["F"], dtype=torch.int32)
    dense = gbt.build_tree(dense_bins, case["resid"], gc.TREE_NB,
                           gc.TREE_DEPTH, gc.TREE_LAM, zeros)
    sparse = gbt.build_tree(sb, case["resid"], gc.TREE_NB, gc.TREE_DEPTH,
                            gc.TREE_LAM)
    assert gc.n_splits(dense) >= 4
    assert sparse.cat_mask is None
    assert (sparse.feature, sparse.threshold, sparse.leaf_value) == \
        (dense.feature, dense.threshold, dense.leaf_value)
    assert torch.equal(sparse.predict_bins(sb),
                       dense.predict_bins(dense_bins))


# ------------------------------------------------------- fixture and jobs

def _run(job, device="cpu"):
    from harmony_amd.config import RuntimeConfig
    from harmony_amd.dolphin.master import run_job
    from harmony_amd.runtime.bootstrap import init_executor

    return run_job(job, init_executor(RuntimeConfig(device=device))).summary()


def _golden_job(sparse):
    from harmony_amd.config import JobConfig

    return JobConfig(job_id="t_gbt_sparse_file", app="gbt", max_num_epochs=2,
                     num_mini_batches=1,
                     app_args={"input": str(gc.GOLDEN),
                               "num_features": gc.GOLDEN_F, "num_bins": 8,
                               "max_depth": 3, "step_size": 0.5,
                               "sparse": sparse})


def test_fixture_first_tree_sparse_equals_dense(monkeypatch):
    from harmony_amd import dataloader as dl

    row_ptr, col, _val, y = dl.parse_libsvm_csr_split(str(gc.GOLDEN), 0, 1,
                                                      gc.GOLDEN_F)
    assert y.shape[0] == 48 and torch.equal(y, y.round())
    assert 2000 < int(col.max()) < gc.GOLDEN_F
    assert gbt.feature_types(gbt.defaults(_golden_job("true"))
                             ).nonzero().flatten().tolist() == [5]
    built = []
    real = gbt.build_tree

    def recording(bins, *args, **kw):
        tree = real(bins, *args, **kw)
        built.append((type(bins), tree))
        return tree

    monkeypatch.setattr(gbt, "build_tree", recording)
    s_sparse = _run(_golden_job("true"))
    n = len(built)
    s_dense = _run(_golden_job("false"))
    assert s_sparse["num_trees"] == s_dense["num_trees"] == 2
    assert n == 2 and len(built) == 4
    assert built[0][0] is SparseBins and built[n][0] is torch.Tensor
    assert gc.n_splits(built[n][1]) >= 2
    gc.assert_same_tree(built[0][1], built[n][1], "first tree")


def test_fixture_blocks_are_the_dense_blocks_binned():
    # the row ranges of torch.chunk, 48 rows in 5 blocks: 10, 10, 10, 10, 8
    import dataclasses

    cpu = torch.device("cpu")
    sparse = gbt.make_batches(dataclasses.replace(
        _golden_job("true"), num_mini_batches=5), 0, cpu)
    dense = gbt.make_batches(dataclasses.replace(
        _golden_job("false"), num_mini_batches=5), 0, cpu)
    assert [x.shape[0] for x, _y in sparse] == [10, 10, 10, 10, 8]
    assert len(dense) == 5
    for (xs, ys), (xd, yd) in zip(sparse, dense):
        assert isinstance(xs, SparseBins) and xs.shape == xd.shape
        assert torch.equal(xs.to_dense_bins(), xd)
        assert torch.equal(ys, yd)


def _synthetic_job(job_id, max_num_epochs=3, **kw):
    from harmony_amd.config import JobConfig

    args = {"num_features": 4096, "batch_size": 256, "num_bins": 16,
            "max_depth": 3, "step_size": 0.3, "nnz_per_row": 8,
            "sparse": "true"}
    args.update(kw)
    return JobConfig(job_id=job_id, app="gbt", max_num_epochs=max_num_epochs,
                     num_mini_batches=2, app_args=args)


def test_sparse_flag_from_cli():
    from harmony_amd.config import JobConfig
    from harmony_amd.jobserver.client import _parse_flags

    def sparse(argv):
        _kw, app_args, _w = _parse_flags(argv)
        return gbt._is_sparse(gbt.defaults(
            JobConfig(job_id="j", app="gbt", app_args=app_args)))

    assert sparse(["-sparse", "true"]) and sparse(["-sparse", "1"])
    assert not sparse(["-sparse", "false"]) and not sparse([])


def test_synthetic_blocks_are_sparse_bins():
    job = _synthetic_job("t_gbt_sparse_syn", num_categorical=2,
                         num_categories=6)
    cpu = torch.device("cpu")
    blocks = gbt.make_batches(job, 0, cpu)
    again = gbt.make_batches(job, 0, cpu)
    assert len(blocks) == 2
    for (x, y), (x2, y2) in zip(blocks, again):
        assert isinstance(x, SparseBins) and x.shape == (256, 4096)
        assert y.shape == (256,) and y.dtype == torch.float32
        assert torch.equal(x.keys, x2.keys) and torch.equal(y, y2)
        assert torch.equal(x.key_bin, x2.key_bin)
        assert 256 <= x.nnz <= 256 * 8
        # the first categorical column is present in every row, unbinned
        assert int(x.feat_ids[-2]) == 4094 or int(x.feat_ids[-1]) == 4094
        b = x.bin_of(torch.full((256,), 4094))
        assert 0 <= int(b.min()) and int(b.max()) <= 5
    # dense jobs are untouched by the new arguments
    dense = gbt.make_batches(_synthetic_job("t_gbt_sparse_syn",
                                            sparse="false",
                                            num_features=16), 0, cpu)
    assert isinstance(dense[0][0], torch.Tensor)


def test_sparse_regression_job(monkeypatch):
    seen = []
    real = ops.gbt_hist_sparse
    monkeypatch.setattr(ops, "gbt_hist_sparse",
                        lambda *a, **k: seen.append(1) or real(*a, **k))
    first = _run(_synthetic_job("t_gbt_sparse_reg", max_num_epochs=1))
    calls = len(seen)
    last = _run(_synthetic_job("t_gbt_sparse_reg"))
    assert calls == 2 * 3                  # one K10s call per tree level
    assert first["num_batches"] == 2 and last["num_batches"] == 6
    assert last["num_trees"] == 6
    assert last["total_examples"] == 6 * 256
    assert math.isfinite(first["mse"]) and math.isfinite(last["mse"])
    print(f"mse: first epoch {first['mse']:.4f}, last {last['mse']:.4f}")
    assert last["mse"] < first["mse"]


def test_sparse_multiclass_job():
    s = _run(_synthetic_job("t_gbt_sparse_mc", objective="multiclass",
                            num_classes=3, num_categorical=1))
    assert s["num_batches"] == 6
    assert s["num_trees"] == 3 * 6
    assert math.isfinite(s["error_rate"]) and 0.0 <= s["error_rate"] <= 1.0


def test_reslice_uses_prefix():
    from harmony_amd.config import RuntimeConfig
    from harmony_amd.runtime.bootstrap import init_executor
    from harmony_amd.runtime.control import ControlPlane

    job = _synthetic_job("t_gbt_sparse_share", max_num_epochs=1)
    ctx = init_executor(RuntimeConfig(device="cpu"))
    cp = ControlPlane(ctx.store, ctx.rank, ctx.world_size)
    _tables, trainer, provider = gbt.build(job, ctx, cp)
    for share, rows in ((0.25, 64), (0.0, 0)):
        provider.set_share(share)
        for x, y in provider.epoch_iter(0):
            assert isinstance(x, SparseBins)
            assert x.shape == (rows, 4096) and y.shape[0] == rows
            trainer.set_batch_data((x, y))
            trainer.pull_model()
            trainer.local_compute()
            assert trainer.num_batch_examples() == rows
            if rows == 0:
                assert trainer.new_tree.threshold == [-1] * 7
