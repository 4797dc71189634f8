"""Forest prediction on the CPU: ops.gbt_forest_predict and gbt.forest_predict
against GBTTrainer._forest_pred from an empty cache (torch.equal), sparse
against dense, the packed-forest round trip and the checks that keep a bad
forest off the device."""

import pytest
import torch

from harmony_amd import ops
from harmony_amd.mlapps import gbt
from tests import gbt_predict_cases as pc

ALL = range(pc.N_CASES)


@pytest.mark.parametrize("idx", ALL)
def test_wrapper_equals_the_forest_loop(idx):
    case = pc.make_case(idx)
    got = ops.gbt_forest_predict(case["bins"], case["packed"], case["depth"],
                                 pc.STEP)
    assert got.dtype == torch.float32
    assert got.shape == (case["bins"].shape[0],)
    assert torch.equal(got, case["want"])
    assert torch.equal(gbt.forest_predict(case["forest"], case["bins"],
                                          pc.STEP), case["want"])


def test_cases_reach_every_node_kind():
    # the inputs do what their notes say, so a pass above means something
    case = pc.make_case(3)
    thr = torch.tensor([t.threshold for t in case["forest"]])
    assert bool((thr == -2).any()) and bool((thr == -1).any())
    assert int(case["bins"].max()) >= 64
    masks = torch.tensor([t.cat_mask for t in case["forest"]])
    assert bool((masks == -1).any()) and bool((masks < 0).any())
    assert pc.make_case(2)["forest"][0].cat_mask is None
    assert len(pc.make_case(5)["forest"]) == 0
    assert not bool(pc.make_case(5)["want"].any())
    big = pc.make_case(6)
    assert len(big["forest"]) == ops.gbt_predict_group_trees(
        big["packed"].shape[1]) + 1
    sp = pc.make_case(7)["bins"]
    lengths = torch.bincount(sp.keys // pc.WIDE_F, minlength=sp.shape[0])
    assert int(lengths.min()) == 0
    present = set(sp.feat_ids.tolist())
    feats = {f for t in pc.make_case(7)["forest"] for f in t.feature}
    assert feats - present and feats & present
    assert int((sp.keys % pc.WIDE_F == 7).sum()) == int((lengths > 0).sum())
    wide = pc.make_case(8)["bins"]
    assert int(wide.keys.max()) > 2 ** 32
    # summation order shows: the reversed forest gives other bits
    c1 = pc.make_case(1)
    assert not torch.equal(pc.oracle(c1["forest"][::-1], c1["bins"]),
                           c1["want"])


def test_sparse_equals_dense_on_the_densified_bins():
    case = pc.small_sparse_case()
    dense = case["bins"].to_dense_bins()
    got = ops.gbt_forest_predict(dense, case["packed"], case["depth"],
                                 pc.STEP)
    assert torch.equal(got, case["want"])
    assert torch.equal(ops.gbt_forest_predict(
        case["bins"], case["packed"], case["depth"], pc.STEP), got)


@pytest.mark.parametrize("idx", [1, 2, 4])
def test_pack_round_trip(idx):
    case = pc.make_case(idx)
    d = case["depth"]
    packed = case["packed"]
    assert packed.dtype == torch.int32 and packed.is_contiguous()
    # the one device format: what encode_trees gives for the same trees
    assert torch.equal(packed, gbt.encode_trees(
        [(0, t) for t in case["forest"]], d))
    assert packed.shape == (len(case["forest"]),
                            pc.row_len(d, case["forest"][0].cat_mask
                                       is not None))
    back = gbt.decode_trees(packed, d)
    assert [k for k, _t in back] == [0] * len(case["forest"])
    for (_k, got), want in zip(back, case["forest"]):
        assert got.feature == want.feature
        assert got.threshold == want.threshold
        assert got.cat_mask == want.cat_mask
        assert torch.equal(torch.tensor(got.leaf_value),
                           torch.tensor(want.leaf_value))
    assert torch.equal(gbt.pack_forest([t for _k, t in back], d), packed)


def _bad(case, value):
    packed = case["packed"].clone()
    packed[1, 2] = value           # a feature word of the second tree
    return packed


@pytest.mark.parametrize("value", ["F", -1])
def test_feature_out_of_range_raises(value):
    case = pc.make_case(1)
    F = case["bins"].shape[1]
    with pytest.raises(ValueError, match="feature index"):
        ops.gbt_forest_predict(case["bins"],
                               _bad(case, F if value == "F" else value),
                               case["depth"], pc.STEP)


def test_wrong_row_length_raises():
    case = pc.make_case(1)
    with pytest.raises(ValueError, match="row"):
        ops.gbt_forest_predict(case["bins"], case["packed"][:, :-1],
                               case["depth"], pc.STEP)
    with pytest.raises(ValueError, match="row"):
        ops.gbt_forest_predict(case["bins"], case["packed"],
                               case["depth"] + 1, pc.STEP)


def test_depth_9_takes_the_torch_path():
    g = torch.Generator().manual_seed(9)
    forest = pc.random_forest(2, 9, 6, 16, True, g)
    bins = torch.randint(0, 16, (70, 6), generator=g)
    assert ops.GBT_PREDICT_MAX_DEPTH == 8
    assert torch.equal(gbt.forest_predict(forest, bins, pc.STEP),
                       pc.oracle(forest, bins))
