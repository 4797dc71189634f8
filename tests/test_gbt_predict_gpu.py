"""K10p on the device: ops.gbt_forest_predict against the forest loop run on
the CPU, bit for bit, for every case of gbt_predict_cases; the binding, its
limits, and the host check that keeps a bad forest from being launched."""

import pytest
import torch

from harmony_amd import ops
from harmony_amd.mlapps import gbt
from harmony_amd.mlapps.sparse_bins import SparseBins
from tests import gbt_predict_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _hip():
    hip = ops._load_hip()
    assert hip is not None, "the HIP extension is not built"
    return hip


@pytest.mark.parametrize("idx", range(pc.N_CASES))
def test_kernel_equals_the_cpu_loop(idx):
    case = pc.make_case(idx)
    bins = case["bins"].to(DEV)
    got = ops.gbt_forest_predict(bins, case["packed"], case["depth"],
                                 pc.STEP)
    assert got.device.type == "cuda" and got.dtype == torch.float32
    assert torch.equal(got.cpu(), case["want"])
    again = ops.gbt_forest_predict(bins, case["packed"].to(DEV),
                                   case["depth"], pc.STEP)
    assert torch.equal(again, got)
    assert torch.equal(gbt.forest_predict(case["forest"], bins,
                                          pc.STEP).cpu(), case["want"])


def test_small_sparse_equals_dense_on_device():
    case = pc.small_sparse_case()
    sp = case["bins"].to(DEV)
    a = ops.gbt_forest_predict(sp, case["packed"], case["depth"], pc.STEP)
    b = ops.gbt_forest_predict(sp.to_dense_bins(), case["packed"],
                               case["depth"], pc.STEP)
    assert torch.equal(a.cpu(), case["want"])
    assert torch.equal(b.cpu(), case["want"])


def test_the_binding_is_the_kernel():
    hip = _hip()
    assert hasattr(hip, "gbt_forest_predict")
    assert hip.gbt_predict_max_depth() == ops.GBT_PREDICT_MAX_DEPTH
    assert hip.gbt_predict_lds_words() == ops.GBT_PREDICT_LDS_WORDS
    case = pc.make_case(3)
    bins = case["bins"].to(DEV)
    F = bins.shape[1]
    direct = hip.gbt_forest_predict(bins, case["packed"].to(DEV),
                                    case["depth"], pc.STEP, F, None, None,
                                    None)
    assert torch.equal(direct, ops.gbt_forest_predict(
        bins, case["packed"], case["depth"], pc.STEP))
    assert torch.equal(direct.cpu(), case["want"])


def test_the_wrapper_calls_the_binding(monkeypatch):
    hip = _hip()
    calls = []
    real = hip.gbt_forest_predict
    monkeypatch.setattr(hip, "gbt_forest_predict",
                        lambda *a: calls.append(1) or real(*a))
    for idx in (1, 7):
        case = pc.make_case(idx)
        ops.gbt_forest_predict(case["bins"].to(DEV), case["packed"],
                               case["depth"], pc.STEP)
    assert len(calls) == 2


def test_depth_9_is_refused_by_the_binding_and_answered_by_the_wrapper():
    hip = _hip()
    g = torch.Generator().manual_seed(9)
    forest = pc.random_forest(2, 9, 6, 16, True, g)
    bins = torch.randint(0, 16, (70, 6), generator=g)
    packed = gbt.pack_forest(forest, 9)
    with pytest.raises(RuntimeError, match="too deep"):
        hip.gbt_forest_predict(bins.to(DEV), packed.to(DEV), 9, pc.STEP, 6,
                               None, None, None)
    got = ops.gbt_forest_predict(bins.to(DEV), packed, 9, pc.STEP)
    assert torch.equal(got.cpu(), pc.oracle(forest, bins))


@pytest.mark.parametrize("idx", [1, 7])
def test_bad_feature_index_is_never_launched(idx, monkeypatch):
    hip = _hip()
    launched = []
    monkeypatch.setattr(hip, "gbt_forest_predict",
                        lambda *a: launched.append(1))
    case = pc.make_case(idx)
    bins = case["bins"].to(DEV)
    assert isinstance(case["bins"], SparseBins) == (idx == 7)
    for value in (bins.shape[1], -1):
        packed = case["packed"].clone()
        packed[1, 2] = value
        with pytest.raises(ValueError, match="feature index"):
            ops.gbt_forest_predict(bins, packed, case["depth"], pc.STEP)
    assert launched == []
