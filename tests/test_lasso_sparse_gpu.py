"""K11s (ops/csrc/lasso_sparse.hip) on the GPU: every case of
lasso_sparse_cases at every thread count against fp64 (checked on the CPU
from the kernel's outputs), the LDS limit, and whole sparse jobs."""

import pytest
import torch

from tests import lasso_sparse_cases as lc

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(idx):
    if idx not in _CASES:
        _CASES[idx] = lc.make_case(idx)
    return _CASES[idx]


def _bits(t):
    return t.view(torch.int32)


def _run_and_check(case, lam_n, threads, label):
    from harmony_amd import ops

    args = lc.op_args(case, "cuda")
    kept = [t.clone() for t in args]
    w_out, r_out = ops.lasso_cd_sparse(*args, lam_n, _force_threads=threads)
    w_again, r_again = ops.lasso_cd_sparse(*args, lam_n,
                                           _force_threads=threads)
    assert w_out.is_cuda and r_out.is_cuda
    assert torch.equal(_bits(w_out), _bits(w_again)), label
    assert torch.equal(_bits(r_out), _bits(r_again)), label
    for a, b in zip(args, kept):                  # inputs are not mutated
        assert torch.equal(a, b), label
    return lc.check(case, lam_n, w_out.cpu(), r_out.cpu(), label)


@pytest.mark.parametrize("threads", [0, 64, 256, 1024])
@pytest.mark.parametrize("idx", range(len(lc.SHAPES)))
def test_kernel_vs_fp64(idx, threads):
    case = _case(idx)
    for lam_n in lc.lams(case["B"]):
        label = f"case {idx} threads {threads} lam_n {lam_n:g}"
        cr, rr = _run_and_check(case, lam_n, threads, label)
        print(f"{label}: coordinate error/bound {cr:.3f}, "
              f"residual error/bound {rr:.3f}")


def _golden_case():
    from harmony_amd import dataloader as dl
    from harmony_amd.mlapps.sparse_batch import SparseBatch

    row_ptr, col, val, y = dl.parse_libsvm_csr_split(str(lc.GOLDEN), 0, 1, 10)
    return lc.case_from_batch(SparseBatch(row_ptr, col, val, 10), y, 7)


@pytest.mark.parametrize("threads", [0, 64, 256, 1024])
def test_golden_sample(threads):
    case = _golden_case()
    assert bool((case["feat_ptr"][1:] - case["feat_ptr"][:-1] == 64).all())
    for lam_n in (0.0, 0.5 * 64):
        _run_and_check(case, lam_n, threads, f"golden threads {threads}")


def _limit_case(B):
    g = torch.Generator().manual_seed(B)
    lens = [B, 1, 777]
    feat_ptr = torch.tensor([0, B, B + 1, B + 778], dtype=torch.int64)
    feat_row = torch.cat([torch.randperm(B, generator=g)[:n].sort().values
                          for n in lens]).to(torch.int32)
    feat_val = torch.randn(B + 778, generator=g)
    w_in = torch.zeros(9)
    w_in[2], w_in[7] = 0.5, -1.25
    return dict(B=B, F=9, feat_ids=torch.tensor([2, 5, 8], dtype=torch.int32),
                feat_ptr=feat_ptr, feat_row=feat_row, feat_val=feat_val,
                y=torch.randn(B, generator=g), w_in=w_in,
                col_sq=lc.col_sq_of(feat_ptr, feat_val))


def test_lds_limit():
    from harmony_amd import ops

    B = ops.LASSO_SPARSE_MAX_ROWS
    assert ops._load_hip().lasso_cd_sparse_max_rows() == B
    assert B >= 16000                      # 64 KiB of LDS: about 16k rows
    for threads in (64, 256, 1024):
        _run_and_check(_limit_case(B), 0.3, threads,
                       f"B {B} threads {threads}")
    # one past it the binding refuses and the wrapper takes the torch loop
    over = _limit_case(B + 1)
    args = lc.op_args(over, "cuda")
    with pytest.raises(RuntimeError, match="too large"):
        ops._load_hip().lasso_cd_sparse(*args, 0.3, torch.empty_like(args[4]),
                                        256)
    w_out, r_out = ops.lasso_cd_sparse(*args, 0.3)
    assert w_out.is_cuda
    lc.check(over, 0.3, w_out.cpu(), r_out.cpu(), f"B {B + 1} fallback")


def test_empty_inputs_return_clones():
    from harmony_amd import ops

    ids, ptr, row, val, y, w, cs = lc.op_args(_case(1), "cuda")
    w0, r0 = ops.lasso_cd_sparse(ids[:0], ptr[:1], row[:0], val[:0], y, w,
                                 cs[:0], 0.3)
    assert torch.equal(_bits(w0), _bits(w)) and torch.equal(_bits(r0),
                                                            _bits(y))
    assert w0.data_ptr() != w.data_ptr() and r0.data_ptr() != y.data_ptr()
    w0, r0 = ops.lasso_cd_sparse(ids, torch.zeros_like(ptr), row[:0],
                                 val[:0], y[:0], w, cs, 0.3)
    assert torch.equal(_bits(w0), _bits(w)) and r0.shape == (0,)


def _run(job):
    from harmony_amd.config import RuntimeConfig
    from harmony_amd.dolphin.master import run_job
    from harmony_amd.runtime.bootstrap import init_executor

    return run_job(job, init_executor(RuntimeConfig(device="cuda"))).summary()


def test_sparse_job_gpu():
    from harmony_amd.config import JobConfig

    job = JobConfig(job_id="g_lasso_sp", app="lasso", max_num_epochs=2,
                    num_mini_batches=2,
                    app_args={"num_features": 64, "num_parts": 8,
                              "batch_size": 512, "nnz_per_row": 16,
                              "lam": 0.02, "sparse": "true"})
    s = _run(job)
    assert s["num_batches"] == 4
    assert s["mse"] < 1.0


def test_wide_sparse_job_stays_below_one_dense_batch():
    from harmony_amd.config import JobConfig

    F, B = 2 ** 20, 1024
    job = JobConfig(job_id="g_lasso_wide", app="lasso", max_num_epochs=1,
                    num_mini_batches=2,
                    app_args={"num_features": F, "num_parts": 16,
                              "batch_size": B, "nnz_per_row": 32,
                              "sparse": "true"})
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    s = _run(job)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"wide sparse lasso job: peak {peak / 2 ** 20:.0f} MiB allocated")
    assert s["num_batches"] == 2 and s["total_examples"] == 2 * B
    assert peak < B * F * 4                      # one dense batch: 4 GiB
