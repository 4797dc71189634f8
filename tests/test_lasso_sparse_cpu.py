"""Sparse Lasso on the CPU: the op's torch reference against fp64, the
SparseBatch-based make_batches, the trainer and whole jobs."""

import math

import pytest
import torch

from harmony_amd import ops
from tests import lasso_sparse_cases as lc
from tests.dist_helper import run_dist

_CASES = {}


def _case(idx):
    if idx not in _CASES:
        _CASES[idx] = lc.make_case(idx)
    return _CASES[idx]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(
        a.view(torch.int32) if a.dtype == torch.float32 else a,
        b.view(torch.int32) if b.dtype == torch.float32 else b)


# ---------------------------------------------------------------------- op

@pytest.mark.parametrize("idx", range(len(lc.SHAPES)))
def test_torch_path_vs_fp64(idx):
    case = _case(idx)
    args = lc.op_args(case)
    kept = [t.clone() for t in args]
    for lam_n in lc.lams(case["B"]):
        w_out, r_out = ops.lasso_cd_sparse(*args, lam_n)
        cr, rr = lc.check(case, lam_n, w_out, r_out,
                          f"case {idx} lam_n {lam_n}")
        print(f"case {idx} lam_n {lam_n:g}: coordinate error/bound {cr:.3f}, "
              f"residual error/bound {rr:.3f}")
    for a, b in zip(args, kept):                  # inputs are not mutated
        assert _same_bits(a, b)


def test_checks_see_a_small_perturbation():
    # the checks are tight enough to matter: one output weight moved by a
    # relative 1e-3 on a full-length column trips them
    case = _case(2)
    w_out, r_out = ops.lasso_cd_sparse(*lc.op_args(case), 0.3)
    lc.check(case, 0.3, w_out, r_out)
    f = int(case["feat_ids"][0])
    assert float(w_out[f]) != 0.0
    bad = w_out.clone()
    bad[f] *= 1.0 + 1e-3
    with pytest.raises(AssertionError):
        lc.check(case, 0.3, bad, r_out)


def test_empty_inputs_return_clones():
    case = _case(1)
    ids, ptr, row, val, y, w, cs = lc.op_args(case)
    w0, r0 = ops.lasso_cd_sparse(ids[:0], ptr[:1], row[:0], val[:0], y, w,
                                 cs[:0], 0.3)
    assert _same_bits(w0, w) and _same_bits(r0, y)
    assert w0.data_ptr() != w.data_ptr() and r0.data_ptr() != y.data_ptr()
    w0, r0 = ops.lasso_cd_sparse(ids, torch.zeros_like(ptr), row[:0],
                                 val[:0], y[:0], w, cs, 0.3)
    assert _same_bits(w0, w) and r0.shape == (0,)


def test_thread_rule_is_a_function_of_the_batch():
    for nf, nnz in ((1, 1), (60000, 65536), (4096, 65536), (16, 4096),
                    (10, 10 * 2048), (3, 3 * 16000)):
        t = ops.lasso_sparse_threads(nf, nnz)
        assert t in (64, 256, 1024)
        assert t == ops.lasso_sparse_threads(nf, nnz)
    assert ops.lasso_sparse_threads(60000, 65536) == 64
    assert ops.lasso_sparse_threads(3, 3 * 16000) == 1024
    assert ops.lasso_sparse_threads(0, 0) == 64


# ------------------------------------------------------------ make_batches

def _syn_job(job_id, F, B, k, lam=0.05, **kw):
    from harmony_amd.config import JobConfig

    return JobConfig(job_id=job_id, app="lasso",
                     app_args={"num_features": F, "num_parts": 8,
                               "batch_size": B, "nnz_per_row": k,
                               "lam": lam, "sparse": "true"}, **kw)


def test_synthetic_batches():
    from harmony_amd.mlapps import lasso
    from harmony_amd.mlapps.sparse_batch import SparseBatch

    F, B, k = 2 ** 20, 256, 32
    job = _syn_job("ls_syn", F, B, k, max_num_epochs=1, num_mini_batches=2)
    cpu = torch.device("cpu")
    blocks, w_true = lasso.make_batches(job, 0, cpu)
    again, w_again = lasso.make_batches(job, 0, cpu)
    other, _ = lasso.make_batches(job, 1, cpu)
    assert len(blocks) == 2 and w_true.shape == (F,)
    assert torch.equal(w_true, w_again)
    for (x, y), (x2, y2) in zip(blocks, again):
        assert isinstance(x, SparseBatch) and x.shape == (B, F)
        assert y.shape == (B,) and y.dtype == torch.float32
        for name in ("row_ptr", "col", "val", "feat_ids", "feat_ptr",
                     "feat_row", "feat_val"):
            assert _same_bits(getattr(x, name), getattr(x2, name)), name
        assert _same_bits(y, y2)                 # deterministic per rank
        lens = x.row_ptr[1:] - x.row_ptr[:-1]
        assert int(lens.max()) <= k and int(lens.min()) >= 1
        # each (row, col) at most once, in the CSR and in the column index
        row_of = torch.repeat_interleave(torch.arange(B), lens)
        key = row_of * F + x.col.long()
        assert key.unique().shape[0] == key.shape[0]
        seg = torch.repeat_interleave(torch.arange(x.feat_ids.shape[0]),
                                      x.feat_ptr[1:] - x.feat_ptr[:-1])
        key = seg * B + x.feat_row.long()
        assert key.unique().shape[0] == key.shape[0]
        assert bool((x.feat_ids[1:] > x.feat_ids[:-1]).all())
        # nothing of size B*F: the largest tensor follows the non-zeros
        largest = max(t.numel() for t in (
            x.row_ptr, x.col, x.val, x.feat_ids, x.feat_ptr, x.feat_row,
            x.feat_val, y))
        assert largest <= B * k + 1 and largest * 1000 < B * F
        # y = x . w_true + noise
        dot = torch.zeros(B, dtype=torch.float64)
        dot.index_add_(0, row_of, x.val.double() * w_true[x.col.long()].double())
        assert float((y.double() - dot).abs().max()) < 1.0   # noise 0.1
    assert not torch.equal(blocks[0][0].col, other[0][0].col)


def test_sparse_flag_from_cli():
    from harmony_amd.config import JobConfig
    from harmony_amd.jobserver.client import _parse_flags
    from harmony_amd.mlapps import lasso

    def sparse(argv):
        _kw, app_args, _w = _parse_flags(argv)
        return lasso._is_sparse(lasso.defaults(
            JobConfig(job_id="j", app="lasso", app_args=app_args)))

    assert sparse(["-sparse", "true"]) and sparse(["-sparse", "1"])
    assert not sparse(["-sparse", "false"]) and not sparse([])


# -------------------------------------------------------------------- jobs

def _run(job):
    from harmony_amd.config import RuntimeConfig
    from harmony_amd.dolphin.master import run_job
    from harmony_amd.runtime.bootstrap import init_executor

    return run_job(job, init_executor(RuntimeConfig(device="cpu"))).summary()


def _golden_job(sparse):
    from harmony_amd.config import JobConfig

    return JobConfig(job_id="ls_golden", app="lasso", max_num_epochs=2,
                     num_mini_batches=2,
                     app_args={"input": str(lc.GOLDEN), "num_features": 10,
                               "num_parts": 5, "lam": 0.5,
                               "sparse": sparse})


def test_golden_sample_is_full_columns():
    from harmony_amd import dataloader as dl

    row_ptr, col, _val, y = dl.parse_libsvm_csr_split(str(lc.GOLDEN), 0, 1,
                                                      10)
    assert y.shape[0] == 64
    assert torch.equal(row_ptr, torch.arange(65) * 10)
    assert torch.equal(col.view(64, 10),
                       torch.arange(10, dtype=torch.int32).expand(64, 10))


def test_golden_job_sparse_matches_dense():
    # every column is present in every batch, so the two paths differ only
    # in fp32 summation order
    s1 = _run(_golden_job("true"))
    s2 = _run(_golden_job("false"))
    assert s1["num_batches"] == s2["num_batches"] == 4
    assert s1["total_examples"] == s2["total_examples"] == 2 * 64
    assert math.isfinite(s1["mse"])
    assert s1["mse"] == pytest.approx(s2["mse"], rel=1e-3)


def test_synthetic_job_converges():
    # the reported mse is the last batch's; the same job id gives the same
    # data, so the 1-epoch job's figure is the first epoch's.
    # lam: the soft-threshold shrinks a weight by lam_n / col_sq = lam * F / k
    # (a column holds about B * k / F unit-variance entries), which leaves a
    # bias of about (lam * F / k)^2 per active entry in the mse whatever the
    # epoch. At the default lam = 0.05 that is 0.04 * 4 active entries per
    # row, far above the noise floor of 0.01, and the mse shows the bias,
    # not the convergence. lam = 0.005 puts it at 0.0016, below the noise.
    first = _run(_syn_job("ls_job", 64, 512, 16, lam=0.005,
                          max_num_epochs=1, num_mini_batches=2))
    last = _run(_syn_job("ls_job", 64, 512, 16, lam=0.005,
                         max_num_epochs=4, num_mini_batches=2))
    assert first["num_batches"] == 2 and last["num_batches"] == 8
    assert last["total_examples"] == 8 * 512
    assert math.isfinite(first["mse"]) and math.isfinite(last["mse"])
    print(f"mse: first epoch {first['mse']:.4f}, last {last['mse']:.4f}")
    assert last["mse"] < first["mse"]


def test_reslice_and_empty_batch():
    from harmony_amd.config import RuntimeConfig
    from harmony_amd.mlapps import lasso
    from harmony_amd.mlapps.sparse_batch import SparseBatch
    from harmony_amd.runtime.bootstrap import init_executor
    from harmony_amd.runtime.control import ControlPlane

    job = _syn_job("ls_share", 64, 128, 8, max_num_epochs=1,
                   num_mini_batches=2)
    ctx = init_executor(RuntimeConfig(device="cpu"))
    cp = ControlPlane(ctx.store, ctx.rank, ctx.world_size)
    _tables, trainer, provider = lasso.build(job, ctx, cp)
    for share, rows in ((0.25, 32), (0.0, 0)):
        provider.set_share(share)
        for x, y in provider.epoch_iter(0):
            assert isinstance(x, SparseBatch)
            assert x.shape == (rows, 64) and y.shape[0] == rows
            assert getattr(x, "_harmony_colsq", None) is None
            trainer.set_batch_data((x, y))
            trainer.pull_model()
            trainer.local_compute()
            assert trainer.num_batch_examples() == rows
            assert trainer.delta.shape == (64,)
            if rows == 0:
                assert not bool(trainer.delta.any())
            else:
                assert bool(trainer.delta.any())
                assert x._harmony_colsq.shape == x.feat_ids.shape


def _two_rank_worker(rank, world):
    s = _run(_syn_job("ls_two", 64, 128, 8, max_num_epochs=2,
                      num_mini_batches=2))
    return (s["num_batches"], s["mse"])


def test_two_ranks():
    res = run_dist(_two_rank_worker, world=2)
    assert res[0][0] == res[1][0] == 4
    assert all(math.isfinite(mse) for _nb, mse in res)
