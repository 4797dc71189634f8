"""build_tree, the sparse loaders and the column index against
tests/golden/gbt/builder_parent.json, which tests/gbt_builder_cases.record()
wrote at the commit before the three tree builders, the three sparse loaders
and the three column-index builds were merged into one each: the trees
equal list for list, every field of every block equal bit for bit."""

import pytest
import torch

from tests import gbt_builder_cases as bc

GOLD = bc.load()
TREES = [(i, k) for i in range(bc.N_TREE_CASES) for k in bc.KINDS]


def test_fixture_is_complete():
    assert sorted(GOLD["trees"]) == sorted(bc.tree_name(i, k)
                                           for i, k in TREES)
    assert sorted(GOLD["sparse_blocks"]) == sorted(bc.block_sets())
    assert sorted(GOLD["dense_blocks"]) == ["gbt", "lasso", "mlr"]
    # the small deep case: nodes without samples, and nodes whose best
    # candidate gains nothing yet is recorded by the untyped search
    deep = GOLD["trees"][bc.tree_name(bc.N_TREE_CASES - 1, "dense_untyped")]
    passthrough = [f for f, t in zip(deep["feature"], deep["threshold"])
                   if t == -1]
    assert 0 in passthrough and any(f != 0 for f in passthrough)


@pytest.mark.parametrize("idx,kind", TREES)
def test_tree_equals_the_recorded_tree(idx, kind):
    want = GOLD["trees"][bc.tree_name(idx, kind)]
    tree, _ = bc.build(bc.tree_case(idx), kind)
    assert tree.depth == want["depth"]
    got = bc.tree_lists(tree)
    for name in ("feature", "threshold", "leaf_value", "cat_mask"):
        assert got[name] == want[name], (idx, kind, name)
    assert (tree.cat_mask is None) == kind.endswith("_untyped")


@pytest.mark.parametrize("idx", range(bc.N_TREE_CASES))
def test_untyped_and_zero_typed_differ_only_at_passthrough_nodes(idx):
    # what the recorded trees say about the two dense searches: the same
    # thresholds and leaves; `feature` may differ where nothing splits
    case = bc.tree_case(idx)
    untyped = GOLD["trees"][bc.tree_name(idx, "dense_untyped")]
    bins = case["inputs"]["dense_untyped"]
    from harmony_amd.mlapps import gbt

    zero = gbt.build_tree(bins, case["resid"], case["nb"], case["depth"],
                          case["lam"], torch.zeros_like(case["types"]))
    assert zero.threshold == untyped["threshold"]
    assert zero.leaf_value == untyped["leaf_value"]
    assert zero.cat_mask == [0] * len(zero.feature)
    assert all(a == b for a, b, t in zip(zero.feature, untyped["feature"],
                                         zero.threshold) if t != -1)


def test_sparse_blocks_equal_the_recorded_digests():
    got = bc.sparse_block_records()
    for name, want in GOLD["sparse_blocks"].items():
        assert len(got[name]["blocks"]) == len(want["blocks"]), name
        for i, (g, w) in enumerate(zip(got[name]["blocks"], want["blocks"])):
            assert g == w, (name, "block", i)
        assert got[name]["prefix"] == want["prefix"], (name, "prefix")


def test_dense_blocks_equal_the_recorded_digests():
    assert bc.dense_block_records() == GOLD["dense_blocks"]


def test_sparse_bins_take_the_index_of_a_sparse_batch():
    # from a SparseBatch or from its raw CSR: the same SparseBins
    from harmony_amd.mlapps.sparse_batch import SparseBatch
    from harmony_amd.mlapps.sparse_bins import SparseBins
    from tests import gbt_sparse_cases as gc

    for idx in range(len(gc.SHAPES)):
        case = gc.make_case(idx)
        raw = case["sb"]
        via = SparseBins(SparseBatch(*case["csr"], case["F"]), case["nb"],
                         case["types"])
        assert bc.describe(via) == bc.describe(raw), idx
