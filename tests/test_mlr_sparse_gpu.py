"""Sparse MLR kernels (K4s) and the sparse job on the GPU."""

import functools

import pytest
import torch

from tests import mlr_sparse_cases as mc

pytestmark = pytest.mark.gpu

GROUPS = [0, 1, 4, 64]                   # 0 = the host rule's own choice
BS = [1, 5, 67]
CS = [2, 10, 16, 17, 33]
FS = [4, 130, 2 ** 20 + 3]


def _edge_lengths(group):
    g = group or 8
    return [0, 1, g, g + 1, 200]


def _row_lengths(B, group):
    if B == 1:
        return [200]
    return (_edge_lengths(group) + [(7 * r) % 23 for r in range(B)])[:B]


@functools.lru_cache(maxsize=2)
def _table(rows, cols, seed):
    """A random [rows, cols] fp32 table on the CPU and its GPU copy, shared
    by the cases that use the same shape."""
    t = torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed))
    return t, t.cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


# B varies fastest, so consecutive cases share the cached model
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("F", FS)
def test_forward_kernel_vs_fp64(B, C, F):
    from harmony_amd import ops

    W, Wd = _table(C, F, 1000 + C)
    for group in GROUPS:
        lens = _row_lengths(B, group)
        row_ptr, col, val = mc.segments(lens, F, every=F - 1,
                                        seed=B * 100 + group,
                                        absent=0 if F > 4 else None)
        want, mag, n = mc.gather_reduce64(row_ptr, col, val, W.t())
        args = (row_ptr.cuda(), col.cuda(), val.cuda(), Wd)
        got = ops.mlr_sparse_logits(*args, _force_group=group)
        again = ops.mlr_sparse_logits(*args, _force_group=group)
        assert got.shape == (B, C) and got.dtype == torch.float32
        err = (got.cpu().double() - want).abs()
        assert bool((err <= mc.bound(n, mag)).all()), (group, float(err.max()))
        assert bool((got.cpu()[n == 0] == 0).all())      # empty rows: exact 0
        # no atomics, fixed order: two runs agree bit for bit
        assert torch.equal(_bits(got), _bits(again))


def _feature_index(B, F, group, seed):
    """A column index written down directly, so that column lengths are
    chosen freely: the every-row feature first, then 200, G+1, G, 1, 0."""
    lens = ([B] + _edge_lengths(group)[::-1])[:min(F, 6)]
    nf = len(lens)
    g = torch.Generator().manual_seed(seed)
    ids = torch.randperm(F - 1, generator=g)[:nf - 1] if F > 1 else \
        torch.zeros(0, dtype=torch.int64)
    feat_ids = torch.cat([ids, torch.tensor([F - 1])]).sort().values
    feat_ptr, feat_row, feat_val = mc.segments(lens, B, None, seed + 1)
    feat_row[:B] = torch.arange(B, dtype=torch.int32)    # present in each row
    return feat_ids.to(torch.int32), feat_ptr, feat_row, feat_val


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("F", FS)
def test_grad_kernel_vs_fp64(B, C, F):
    from harmony_amd import ops

    P, Pd = _table(B, C, 2000 + B + C)
    Cp = (C + 3) // 4 * 4
    Ppad = torch.zeros(B, Cp, device="cuda")
    Ppad[:, :C] = Pd
    for group in GROUPS:
        feat_ids, feat_ptr, feat_row, feat_val = _feature_index(
            B, F, group, B * 100 + group)
        want, mag, n = mc.gather_reduce64(feat_ptr, feat_row, feat_val, P)
        ix = (feat_ids.cuda(), feat_ptr.cuda(), feat_row.cuda(),
              feat_val.cuda())
        got = ops.mlr_sparse_grad(*ix, Pd, F, _force_group=group)
        again = ops.mlr_sparse_grad(*ix, Pd, F, _force_group=group)
        # a caller's own padded buffer, viewed as [B, C], is read in place
        padded = ops.mlr_sparse_grad(*ix, Ppad[:, :C], F, _force_group=group)
        assert got.shape == (C, F) and got.dtype == torch.float32
        ids = feat_ids.long().cuda()
        for out in (got, padded):
            err = (out[:, ids].t().cpu().double() - want).abs()
            assert bool((err <= mc.bound(n, mag)).all()), \
                (group, float(err.max()))
            # features with no entries stay exactly 0
            assert int(out.count_nonzero()) == \
                int(out[:, ids].count_nonzero())
            assert bool((out[:, ids].t().cpu()[n == 0] == 0).all())
        assert torch.equal(_bits(got), _bits(again))


def test_empty_batch():
    from harmony_amd import ops

    C, F = 10, 130
    _W, Wd = _table(C, F, 1000 + C)
    row_ptr = torch.zeros(1, dtype=torch.int64, device="cuda")
    col = torch.zeros(0, dtype=torch.int32, device="cuda")
    val = torch.zeros(0, device="cuda")
    labels = torch.zeros(0, dtype=torch.int64, device="cuda")
    p, loss, correct = ops.mlr_sparse_forward(row_ptr, col, val, Wd, labels)
    assert p.shape == (0, C) and float(loss) == 0.0 and int(correct) == 0
    g = ops.mlr_sparse_grad(col, row_ptr, col, val, p, F)
    assert g.shape == (C, F) and not bool(g.any())


def test_golden_sample():
    from harmony_amd import dataloader as dl
    from harmony_amd import ops
    from harmony_amd.mlapps.sparse_batch import SparseBatch

    F, C = 784, 10
    row_ptr, col, val, y = dl.parse_libsvm_csr_split(str(mc.GOLDEN), 0, 1, F)
    b = SparseBatch(row_ptr, col, val, F)
    bd = b.to("cuda")
    W, Wd = _table(C, F, 1000 + C)
    want, mag, n = mc.gather_reduce64(b.row_ptr, b.col, b.val, W.t())
    got = ops.mlr_sparse_logits(bd.row_ptr, bd.col, bd.val, Wd)
    assert bool(((got.cpu().double() - want).abs()
                 <= mc.bound(n, mag)).all())
    ref = ops.mlr_sparse_logits(b.row_ptr, b.col, b.val, W)
    assert torch.equal(torch.bincount(got.argmax(dim=1).cpu(), minlength=C),
                       torch.bincount(ref.argmax(dim=1), minlength=C))
    labels = y.long()
    p, _loss, correct = ops.mlr_sparse_forward(bd.row_ptr, bd.col, bd.val,
                                               Wd, labels.cuda())
    _pr, _loss_r, correct_r = ops.mlr_sparse_forward(b.row_ptr, b.col, b.val,
                                                     W, labels)
    assert int(correct) == int(correct_r)
    wantg, magg, ng = mc.gather_reduce64(b.feat_ptr, b.feat_row, b.feat_val,
                                         p.cpu())
    g = ops.mlr_sparse_grad(bd.feat_ids, bd.feat_ptr, bd.feat_row,
                            bd.feat_val, p, F)
    ids = bd.feat_ids.long()
    assert bool(((g[:, ids].t().cpu().double() - wantg).abs()
                 <= mc.bound(ng, magg)).all())
    assert int(g.count_nonzero()) == int(g[:, ids].count_nonzero())


def test_wide_sparse_job_stays_below_one_dense_batch():
    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.dolphin.master import run_job
    from harmony_amd.runtime.bootstrap import init_executor

    F, B = 2 ** 20, 1024
    job = JobConfig(job_id="sp_wide", app="mlr", max_num_epochs=1,
                    num_mini_batches=2,
                    app_args={"num_classes": 10, "num_features": F,
                              "batch_size": B, "nnz_per_row": 32,
                              "sparse": "true"})
    ctx = init_executor(RuntimeConfig(device="cuda"))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    s = run_job(job, ctx).summary()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"wide sparse job: peak {peak / 2 ** 20:.0f} MiB allocated")
    assert s["num_batches"] == 2 and s["total_examples"] == 2 * B
    assert peak < B * F * 4                      # one dense batch: 4 GiB
