"""K11sL (ops/csrc/lasso_sparse_large.hip) at its first row count, through
the raw binding with the clean-window table, against the teacher-forced fp64
bounds of lasso_sparse_cases; and a sparse job whose batch reaches it."""

import pytest
import torch

from harmony_amd import ops
from tests import lasso_sparse_cases as lc

pytestmark = pytest.mark.gpu

B, F, NF = ops.LASSO_SPARSE_K11S_ROWS + 1, 1000, 61   # 61: no multiple of 16
_CASE = []


def _case():
    """61 present columns, one entry each on a row of its own, except:"""
    if _CASE:
        return _CASE[0]
    g = torch.Generator().manual_seed(5)
    cols = [[2000 + 7 * k] for k in range(NF)]
    for k in range(16):                  # a clean window of 16 on the last
        cols[k] = [B - 1 - k]            # rows, B - 1 among them
    cols[17], cols[18] = [5, 2119], [5]         # share a row inside a window
    cols[31], cols[32] = [6], [6, 2224]         # and across a boundary
    cols[33] = list(range(1000, 1065))   # 65 entries: two passes of one wave
    cols[34] = []
    cols[50] = list(range(B))            # longer than solo_len: goes alone
    feat_ptr = torch.tensor([0] + [len(c) for c in cols]).cumsum(0)
    feat_val = torch.randn(int(feat_ptr[-1]), generator=g)
    feat_val[feat_ptr[35]] = 1e-7        # col_sq clamps to 1e-9; has a weight
    ids = torch.arange(NF) * 16 + 3
    w_in = torch.zeros(F)
    w_in[ids[1::2]] = torch.randn(NF // 2, generator=g)
    w_in[0] = 0.625                      # absent from the batch
    _CASE.append(dict(
        B=B, F=F, feat_ids=ids.to(torch.int32), feat_ptr=feat_ptr,
        feat_row=torch.tensor([r for c in cols for r in c],
                              dtype=torch.int32),
        feat_val=feat_val, y=torch.randn(B, generator=g), w_in=w_in,
        col_sq=lc.col_sq_of(feat_ptr, feat_val)))
    return _CASE[0]


@pytest.mark.parametrize("lam_n", lc.lams(B))
@pytest.mark.parametrize("threads", [64, 256, 1024])
def test_kernel_vs_fp64(threads, lam_n):
    case = _case()
    args = lc.op_args(case, "cuda")
    table = ops.lasso_sparse_windows(args[1], args[2], threads // 64,
                                     ops.LASSO_SPARSE_SOLO_LEN)
    on_cpu = ops.lasso_sparse_windows(case["feat_ptr"], case["feat_row"],
                                      threads // 64,
                                      ops.LASSO_SPARSE_SOLO_LEN)
    assert table.is_cuda and torch.equal(table.cpu(), on_cpu)
    if threads == 1024:
        assert on_cpu.tolist() == [1, 0, 1, 0]

    def run(windows):
        w, r = args[5].clone(), torch.empty_like(args[4])
        ops._load_hip().lasso_cd_sparse(*args[:5], w, args[6], lam_n, r,
                                        threads, windows)
        return w.cpu(), r.cpu()

    w_out, r_out = run(table)
    w_again, r_again = run(table)
    assert torch.equal(w_out.view(torch.int32), w_again.view(torch.int32))
    assert torch.equal(r_out.view(torch.int32), r_again.view(torch.int32))
    label = f"threads {threads} lam_n {lam_n:g}"
    cr, rr = lc.check(case, lam_n, w_out, r_out, label)
    print(f"{label}: coordinate error/bound {cr:.3f}, residual {rr:.3f}")
    # every window dirty, as a zero table and as no table: the same path
    w_dirty, r_dirty = run(torch.zeros_like(table))
    lc.check(case, lam_n, w_dirty, r_dirty, label + " all dirty")
    w_none, r_none = run(None)
    assert torch.equal(w_none.view(torch.int32), w_dirty.view(torch.int32))
    assert torch.equal(r_none.view(torch.int32), r_dirty.view(torch.int32))


def test_job_reaches_the_kernel(monkeypatch):
    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.dolphin.master import run_job
    from harmony_amd.runtime.bootstrap import init_executor

    hip, calls = ops._load_hip(), []
    real = hip.lasso_cd_sparse
    monkeypatch.setattr(hip, "lasso_cd_sparse", lambda *a:
                        calls.append((a[4].shape[0], a[9], a[10]))
                        or real(*a))

    def run(device):
        job = JobConfig(job_id="g_lasso_sp_large", app="lasso",
                        max_num_epochs=1, num_mini_batches=1,
                        app_args={"num_features": 4096, "batch_size": 16500,
                                  "nnz_per_row": 4, "lam": 0.0005,
                                  "sparse": "true"})
        return run_job(job, init_executor(RuntimeConfig(device=device))) \
            .summary()

    s = run("cuda")
    (rows, threads, table), = calls
    assert rows == 16500 and threads > 64 and table.dtype == torch.uint8
    cpu = run("cpu")
    assert len(calls) == 1
    print(f"mse cuda {s['mse']!r}, cpu {cpu['mse']!r}")
    assert s["mse"] == pytest.approx(cpu["mse"], rel=1e-3)
