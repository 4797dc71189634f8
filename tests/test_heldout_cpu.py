"""Held-out test data on the CPU: the test_data_path app arg through MLR,
Lasso and GBT jobs, Trainer.evaluate_test and the offline evaluator."""

import pytest
import torch

from harmony_amd.dolphin.trainer import Trainer
from harmony_amd.mlapps import gbt, lasso, mlr
from harmony_amd.mlapps.sparse_batch import SparseBatch
from tests import heldout_cases as hc


def test_flag_from_cli():
    from harmony_amd.jobserver.client import _parse_flags

    _kw, app_args, _w = _parse_flags(
        ["-app", "lasso", "-test_data_path", "file:///data/held_out",
         "-num_features", "10"])
    assert app_args["test_data_path"] == "file:///data/held_out"


def test_default_spi_returns_nothing():
    from harmony_amd.dolphin.trainer import TrainerContext

    t = Trainer(TrainerContext(job_id="j", rank=0, world_size=1,
                               device=torch.device("cpu")))
    assert t.evaluate_test() == {} and t.test_blocks == []


@pytest.mark.parametrize("app", ["mlr", "lasso", "gbt"])
def test_missing_file_fails_in_build(app, tmp_path, monkeypatch):
    from harmony_amd.dolphin.worker import WorkerTasklet

    ran = []
    monkeypatch.setattr(WorkerTasklet, "run",
                        lambda self: ran.append(1) or pytest.fail("ran"))
    missing = tmp_path / "no_such_file"
    job = {"mlr": hc.mlr_job("t_ho_missing_mlr", "false", test=missing),
           "lasso": hc.lasso_job("t_ho_missing_lasso", "true", test=missing),
           "gbt": hc.gbt_job("t_ho_missing_gbt", missing)}[app]
    with pytest.raises(FileNotFoundError):
        hc.run(job)
    assert ran == []


def test_file_scheme_is_accepted():
    _t, trainer, _p = hc.hand_built(hc.lasso_job(
        "t_ho_scheme", "false", test="file://" + str(hc.LASSO_TEST)))
    assert sum(y.shape[0] for _x, y in trainer.test_blocks) == 50


def test_other_apps_ignore_the_arg_and_say_so(capfd):
    from harmony_amd.config import JobConfig

    job = JobConfig(job_id="t_ho_nmf", app="nmf", max_num_epochs=1,
                    num_mini_batches=1,
                    app_args={"num_cols": 64, "rank": 4, "nnz_per_row": 4,
                              "rows_per_batch": 32,
                              "test_data_path": "/no/such/file"})
    s, _trainer = hc.run(job)
    assert not [k for k in s if k.startswith("test_")]
    assert "test_data_path is ignored" in capfd.readouterr().err


# ------------------------------------------------------------------ Lasso

def test_fixture_row_count():
    # the reference's held-out file: 68 lines, of which 17 are its header
    # comments and one is blank, and 50 data rows ("50 instances")
    text = hc.LASSO_TEST.read_text().splitlines()
    assert len(text) == 68
    y, X, k = hc.data_rows(hc.LASSO_TEST)
    assert y.shape[0] == 50 and X.shape == (50, 10) and int(k.min()) >= 9


@pytest.mark.parametrize("sparse", ["false", "true"])
def test_lasso_test_mse(sparse):
    s, trainer = hc.run(hc.lasso_job(f"t_ho_lasso_{sparse}", sparse))
    assert s["test_examples"] == 50
    x0 = trainer.test_blocks[0][0]
    assert isinstance(x0, SparseBatch) == (sparse == "true")
    w = trainer.accessor.pull_all()[:5].reshape(-1)
    assert float(w.abs().max()) > 0
    want, bound = hc.lasso_mse64(w)
    print(f"sparse={sparse}: test_mse {s['test_mse']!r}, fp64 {want!r}, "
          f"error {abs(s['test_mse'] - want):.3e}, bound {bound:.3e}, "
          f"train mse {s['mse']:.4f}")
    assert abs(s["test_mse"] - want) <= bound


def test_lasso_dense_and_sparse_agree_on_one_model():
    # the two jobs train slightly different weights (fp32 summation order),
    # so the two evaluation paths are compared on the SAME pushed weights
    g = torch.Generator().manual_seed(3)
    w0 = torch.randn(5, 2, generator=g)
    got = {}
    for sparse in ("false", "true"):
        _t, trainer, _p = hc.hand_built(
            hc.lasso_job(f"t_ho_lasso_same_{sparse}", sparse))
        trainer.accessor.push_dense(w0.clone())
        got[sparse] = trainer.evaluate_test()
        assert got[sparse] == trainer.evaluate_test()      # same bits
    want, bound = hc.lasso_mse64(w0.reshape(-1))
    for sparse, res in got.items():
        assert res["test_examples"] == 50
        assert abs(res["test_mse"] - want) <= bound, sparse
    assert abs(got["true"]["test_mse"] - got["false"]["test_mse"]) <= bound


def test_lasso_blocks_hold_at_most_batch_size_rows():
    job = hc.lasso_job("t_ho_lasso_blocks", "true")
    job.app_args["batch_size"] = 16
    _t, trainer, _p = hc.hand_built(job)
    assert [y.shape[0] for _x, y in trainer.test_blocks] == [16, 16, 16, 2]
    whole = hc.hand_built(hc.lasso_job("t_ho_lasso_whole", "true"))[1]
    w0 = torch.full((5, 2), 0.25)
    trainer.accessor.push_dense(w0.clone())
    whole.accessor.push_dense(w0.clone())
    want, bound = hc.lasso_mse64(w0.reshape(-1))
    assert abs(trainer.evaluate_test()["test_mse"] - want) <= bound
    assert abs(whole.evaluate_test()["test_mse"] - want) <= bound


def test_offline_evaluation_reports_test_mse_per_checkpoint(tmp_path):
    job = hc.lasso_job("t_ho_lasso_offline", "false", max_num_epochs=3,
                       model_chkp_per_epoch=True, offline_model_eval=True,
                       chkp_path=str(tmp_path))
    s, _trainer = hc.run(job)
    keys = [f"offline/epoch{e}/test_mse" for e in range(3)]
    assert all(k in s for k in keys), sorted(s)
    assert s["offline/epoch2/test_mse"] == s["test_mse"]
    assert s["offline/epoch0/test_mse"] != s["offline/epoch2/test_mse"]
    assert s["offline/epoch1/test_examples"] == 50


def test_no_flag_no_change():
    for job in (hc.lasso_job("t_ho_lasso_none", "true", test=None),
                hc.mlr_job("t_ho_mlr_none", "false", test=None),
                hc.gbt_job("t_ho_gbt_none", None)):
        s, trainer = hc.run(job)
        assert not [k for k in s if k.startswith("test_")], sorted(s)
        assert trainer.test_blocks == [] and trainer.evaluate_test() == {}


# -------------------------------------------------------------------- MLR

@pytest.mark.parametrize("sparse", ["false", "true"])
def test_mlr_test_metrics(sparse):
    s, trainer = hc.run(hc.mlr_job(f"t_ho_mlr_{sparse}", sparse))
    hc.check_mlr(s, trainer)


def test_evaluate_test_leaves_the_training_state():
    job = hc.mlr_job("t_ho_mlr_state", "true")
    results = []
    for probe in (False, True):
        _t, trainer, provider = hc.hand_built(job)
        for i, batch in enumerate(provider.epoch_iter(0)):
            trainer.set_batch_data(batch)
            trainer.pull_model()
            trainer.local_compute()
            trainer.push_update()
            if probe and i == 0:
                mid = trainer.evaluate_test()
                assert mid["test_examples"] == 16
        assert i == 1
        results.append(trainer.evaluate_model())
    assert results[0] == results[1] and results[0]["accuracy"] >= 0


def test_gbt_evaluate_test_leaves_the_training_state(tmp_path):
    X, y, _m = hc.gbt_test_data("t_ho_gbt_state", "dense")
    job = hc.gbt_job("t_ho_gbt_state",
                     hc.write_libsvm(tmp_path / "held_out", X, y))
    results = []
    for probe in (False, True):
        _t, trainer, provider = hc.hand_built(job)
        for epoch in range(2):
            for batch in provider.epoch_iter(epoch):
                trainer.set_batch_data(batch)
                trainer.pull_model()
                trainer.local_compute()
                trainer.push_update()
                if probe:
                    cache = dict(trainer._pred_cache)
                    mse = trainer._mse
                    assert trainer.evaluate_test()["test_examples"] == 200
                    assert trainer._pred_cache == cache
                    assert trainer._mse == mse
        results.append(trainer.evaluate_model())
    assert results[0] == results[1] and results[0]["num_trees"] == 4


# -------------------------------------------------------------------- GBT

@pytest.mark.parametrize("mode", list(hc.GBT_MODES))
def test_gbt_test_metric_is_the_forest_loop(mode, tmp_path):
    s, trainer, (X, y, mask) = hc.run_gbt(mode, tmp_path)
    hc.check_gbt(mode, s, trainer, X, y, mask)


def test_gbt_bad_category_in_the_test_file_raises(tmp_path):
    X, y, _m = hc.gbt_test_data("t_ho_gbt_badcat", "cat")
    X[3, hc.GBT_F - 1] = 2.5
    path = hc.write_libsvm(tmp_path / "held_out", X, y)
    for sparse in ("false", "true"):
        job = hc.gbt_job("t_ho_gbt_badcat", path, num_categorical=2,
                         num_categories=8, sparse=sparse)
        with pytest.raises(ValueError, match="categorical feature 7"):
            hc.hand_built(job)


def test_apps_list_the_arg():
    for mod in (mlr, lasso, gbt):
        assert "test_data_path" in mod.__doc__
