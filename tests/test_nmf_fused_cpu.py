"""CPU (torch fallback) behaviour of ops.nmf_step and of the trainer that
calls it: results must be what the legacy composition gives, bit for bit."""

import torch

from harmony_amd import ops


def _problem(n=40, nnz_row=7, m_src=64, k=12, seed=0):
    g = torch.Generator().manual_seed(seed)
    nnz = n * nnz_row
    row_ptr = torch.arange(0, nnz + 1, nnz_row)
    col = 2 * torch.randint(0, m_src // 2, (nnz,), generator=g)   # even only
    vals = torch.rand(nnz, generator=g)
    uniq, col_local = torch.unique(col, return_inverse=True)
    perm = torch.argsort(col_local, stable=True)
    seg_ptr = torch.zeros(uniq.shape[0] + 1, dtype=torch.int64)
    seg_ptr[1:] = torch.bincount(col_local, minlength=uniq.shape[0]).cumsum(0)
    row_of = torch.repeat_interleave(torch.arange(n), nnz_row)
    L = torch.rand(n + 5, k, generator=g)
    table = torch.rand(m_src, k, generator=g)
    cs = (perm, seg_ptr, row_of[perm])
    return L, table, row_ptr, col, col_local, vals, uniq, cs


def _legacy(L_batch, R, row_ptr, col_local, vals, cs, step_t, lam, max_val):
    lg, rg, sq = ops.nmf_grad(L_batch, R, row_ptr, col_local, vals, lam,
                              col_sorted=cs)
    return (L_batch - step_t * lg).clamp_(0.0, max_val), rg, sq, lg


def test_nmf_step_fallback_equals_legacy_composition():
    L, table, row_ptr, col, col_local, vals, uniq, cs = _problem()
    n, lo, lam, max_val = 40, 3, 0.02, 0.8
    step_t = torch.tensor(0.05)
    want = _legacy(L[lo:lo + n], table[uniq], row_ptr, col_local, vals, cs,
                   step_t, lam, max_val)
    i32 = torch.int32
    cs32 = tuple(t.to(i32) for t in cs)
    gathered = ops.nmf_step(L, lo, n, table[uniq], row_ptr.to(i32),
                            col_local.to(i32), vals, cs32, None, step_t, lam,
                            max_val, want_lgrad=True)
    indexed = ops.nmf_step(L, lo, n, table, row_ptr.to(i32), col.to(i32),
                           vals, cs32, uniq.to(i32), step_t, lam, max_val,
                           want_lgrad=True)
    for got in (gathered, indexed):
        assert len(got) == 4
        for x, y in zip(got, want):
            assert torch.equal(x, y)
    assert len(ops.nmf_step(L, lo, n, table, row_ptr.to(i32), col.to(i32),
                            vals, cs32, uniq.to(i32), step_t, lam,
                            max_val)) == 3


def test_nmf_step_indexed_and_gathered_sgd_identical():
    """Three SGD steps on the whole table by global column id, and on the
    gathered rows by local id, leave identical L and tables."""
    from harmony_amd.et import update_functions as uf

    L, table, row_ptr, col, col_local, vals, uniq, cs = _problem(seed=1)
    n, lam, max_val, step = 40, 0.01, 1e6, 1e-3
    step_t = torch.tensor(step)
    i32 = torch.int32
    cs32 = tuple(t.to(i32) for t in cs)
    fn = uf.update_fn("nmf_sgd")
    La, Ta, Lb, Tb = L.clone(), table.clone(), L.clone(), table.clone()
    for _ in range(3):
        Ln, rg, _ = ops.nmf_step(La, 0, n, Ta, row_ptr.to(i32), col.to(i32),
                                 vals, cs32, uniq.to(i32), step_t, lam,
                                 max_val)
        La[:n] = Ln
        Ta[uniq] = fn(Ta[uniq], rg, step_size=step, max_val=max_val)
        Ln, rg, _ = ops.nmf_step(Lb, 0, n, Tb[uniq], row_ptr.to(i32),
                                 col_local.to(i32), vals, cs32, None, step_t,
                                 lam, max_val)
        Lb[:n] = Ln
        Tb[uniq] = fn(Tb[uniq], rg, step_size=step, max_val=max_val)
    assert torch.equal(La, Lb) and torch.equal(Ta, Tb)
    assert not torch.equal(Ta, table)


def test_nmf_trainer_contiguous_and_scattered_rows_match_legacy():
    """The trainer's compute phase, on a contiguous L range and on scattered
    rows, against the legacy composition on the same inputs."""
    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.mlapps import nmf
    from harmony_amd.runtime.bootstrap import init_executor

    ctx = init_executor(RuntimeConfig(device="cpu"))
    job = JobConfig(job_id="fused_cpu", app="nmf", num_mini_batches=2,
                    app_args={"num_cols": 64, "rank": 12, "nnz_per_row": 5,
                              "rows_per_batch": 32, "step_size": 1e-2,
                              "lam": 0.01})
    _, tr, provider = nmf.build(job, ctx, None)
    b1 = provider.blocks[1]
    assert b1.l_contiguous and b1.l_lo == 32
    l_rows = torch.arange(31, -1, -2)
    nnz = int(b1.row_ptr[l_rows.shape[0]])
    scattered = nmf.NMFBatch(l_rows,
                             b1.row_ptr[:l_rows.shape[0] + 1].contiguous(),
                             b1.col_idx[:nnz], b1.vals[:nnz])
    assert not scattered.l_contiguous
    for b in (b1, scattered):
        L0 = tr.L.clone()
        tr.set_batch_data(b)
        tr.pull_model()
        R = tr.R_batch.clone()
        tr.local_compute()
        L_new, rg, _, _ = _legacy(L0[b.l_rows], R, b.row_ptr, b.col_local,
                                  b.vals, b.col_sorted, tr._step_t,
                                  tr.a["lam"], tr.a["max_val"])
        want = L0.clone()
        want[b.l_rows] = L_new
        assert torch.equal(tr.L, want)
        assert torch.equal(tr.rgrad, rg)
