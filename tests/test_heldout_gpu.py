"""Held-out test data on the device: the GBT dense and sparse jobs and one
sparse MLR job of test_heldout_cpu.py, with the same assertions. The GBT
metrics must be exactly what the forest loop on the CPU gives."""

import pytest

from harmony_amd import ops
from tests import heldout_cases as hc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["dense", "sparse"])
def test_gbt_test_metric_is_the_cpu_forest_loop(mode, tmp_path, monkeypatch):
    calls = []
    real = ops.gbt_forest_predict
    monkeypatch.setattr(ops, "gbt_forest_predict",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    s, trainer, (X, y, mask) = hc.run_gbt(mode, tmp_path, device="cuda")
    assert trainer.test_blocks[0][1].device.type == "cuda"
    assert len(calls) == 1          # one launch for the whole forest
    hc.check_gbt(mode, s, trainer, X, y, mask)


def test_mlr_sparse_test_metrics():
    s, trainer = hc.run(hc.mlr_job("t_ho_mlr_gpu", "true"), device="cuda")
    assert trainer.test_blocks[0][1].device.type == "cuda"
    hc.check_mlr(s, trainer)
