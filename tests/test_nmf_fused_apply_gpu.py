"""ops.nmf_step with the server update in pass B's epilogue (apply=...)
against the pair it replaces on the single-owner path, bit for bit:

    L_new, rgrad, sq = ops.nmf_step(...)                    (no apply)
    ops.scatter_apply(table, rows, rgrad, "nmf_sgd", step, max_val)

Same inputs, same process, so rgrad, L_new and the whole table (rows the
batch does not touch included) are compared with torch.equal.
"""

import pytest
import torch

from harmony_amd import ops

pytestmark = pytest.mark.gpu

TABLE_ROWS = 300
# nonzeros of the first pulled columns: an empty segment, one entry, the
# 32-lane chunk of pass B at 32 and 33, several chunks of either group width
SEG_NNZ = [0, 1, 32, 33, 200]
SRV_STEP, SRV_MAX = 0.5, 0.9


class Problem:
    """n rows over m = len(SEG_NNZ) + 6 pulled columns; the nonzeros of a
    column fall on random rows (a row may hold a column more than once).
    The pulled columns are table rows in shuffled order, a strict subset."""

    def __init__(self, n, k, seed):
        g = torch.Generator().manual_seed(seed)
        seg = SEG_NNZ + torch.randint(1, 12, (6,), generator=g).tolist()
        m = len(seg)
        col_local = torch.repeat_interleave(torch.arange(m), torch.tensor(seg))
        row = torch.randint(0, n, col_local.shape, generator=g)
        order = torch.argsort(row, stable=True)
        row, self.col_local = row[order], col_local[order]
        nnz = row.shape[0]
        self.row_ptr = torch.zeros(n + 1, dtype=torch.int64)
        self.row_ptr[1:] = torch.bincount(row, minlength=n).cumsum(0)
        perm = torch.argsort(self.col_local, stable=True)
        self.perm, self.row_sorted = perm, row[perm]
        self.seg_ptr = torch.zeros(m + 1, dtype=torch.int64)
        self.seg_ptr[1:] = torch.tensor(seg).cumsum(0)
        # dots of uniform [0, 1) vectors are near k / 4: errors of both signs
        self.vals = torch.rand(nnz, generator=g) * (k / 2)
        self.L = torch.rand(n, k, generator=g)
        self.table = torch.rand(TABLE_ROWS, k, generator=g) * SRV_MAX
        self.rows = torch.randperm(TABLE_ROWS, generator=g)[:m]
        assert not torch.equal(self.rows, self.rows.sort().values)
        self.n, self.k, self.m = n, k, m


@pytest.mark.parametrize("k", [4, 100, 130])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 257])
def test_fused_apply_equals_scatter_apply(n, k):
    p = Problem(n, k, seed=1000 * k + n)
    i32 = dict(dtype=torch.int32, device="cuda")
    row_ptr, col = p.row_ptr.to(**i32), p.col_local.to(**i32)
    cs = (p.perm.to(**i32), p.seg_ptr.to(**i32), p.row_sorted.to(**i32))
    L, vals, rows = p.L.cuda(), p.vals.cuda(), p.rows.cuda()
    t_old = p.table.cuda()
    t_new = t_old.clone()
    R = t_old[rows]                         # the pulled snapshot
    step_t = torch.tensor(1e-3, device="cuda")
    lam, max_val = 0.01, 1e6

    L_o, rg_o, _ = ops.nmf_step(L, 0, n, R, row_ptr, col, vals, cs, None,
                                step_t, lam, max_val)
    ops.scatter_apply(t_old, rows, rg_o, "nmf_sgd", SRV_STEP, SRV_MAX)
    L_n, rg_n, _ = ops.nmf_step(L, 0, n, R, row_ptr, col, vals, cs, None,
                                step_t, lam, max_val,
                                apply=(t_new, rows.to(torch.int32), SRV_STEP,
                                       SRV_MAX))
    assert torch.equal(rg_n, rg_o)
    assert torch.equal(L_n, L_o)
    assert torch.equal(t_new, t_old)
    untouched = torch.ones(TABLE_ROWS, dtype=torch.bool, device="cuda")
    untouched[rows] = False
    assert torch.equal(t_new[untouched], p.table.cuda()[untouched])
    touched = t_new[rows]
    assert not torch.equal(touched, R)
    if n >= 7:      # both clamp bounds are reached
        assert (touched == 0.0).any() and (touched == SRV_MAX).any()


def test_apply_rejects_bad_arguments():
    p = Problem(8, 100, seed=3)
    i32 = dict(dtype=torch.int32, device="cuda")
    cs = (p.perm.to(**i32), p.seg_ptr.to(**i32), p.row_sorted.to(**i32))
    table = p.table.cuda()
    rows32 = p.rows.to(**i32)
    args = (p.L.cuda(), 0, 8, table[p.rows.cuda()], p.row_ptr.to(**i32),
            p.col_local.to(**i32), p.vals.cuda(), cs, None,
            torch.tensor(1e-3, device="cuda"), 0.0, 1e6)
    with pytest.raises(RuntimeError, match="shard_row must be"):
        ops.nmf_step(*args, apply=(table, rows32[:-1], 0.1, 1.0))
    with pytest.raises(RuntimeError, match="shard must be"):
        ops.nmf_step(*args, apply=(table[:, :50].contiguous(), rows32, 0.1,
                                   1.0))
    # the table as R_src and as the shard: pass B would read what it writes
    with pytest.raises(RuntimeError, match="must not overlap"):
        ops.nmf_step(args[0], 0, 8, table, *args[4:8], rows32, *args[9:],
                     apply=(table, rows32, 0.1, 1.0))


def _run_trainer(monkeypatch, fused: bool):
    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.mlapps import nmf
    from harmony_amd.runtime.bootstrap import init_executor

    monkeypatch.setenv("HARMONY_FUSED_TAIL", "1" if fused else "0")
    ctx = init_executor(RuntimeConfig(device="cuda"))
    job = JobConfig(job_id="nmf_tail", app="nmf", num_mini_batches=2,
                    app_args={"num_cols": 96, "rank": 100, "nnz_per_row": 9,
                              "rows_per_batch": 48, "step_size": 0.05,
                              "decay_period": 1})
    tables, tr, provider = nmf.build(job, ctx, None)
    table = next(iter(tables.values()))
    assert tr._fused_tail is fused
    seen = []
    for visit in range(2):
        for b in provider.blocks:
            tr.set_batch_data(b)
            tr.pull_model()
            tr.local_compute()
            tr.push_update()
            seen.append((table.pull_all().clone(), tr.rgrad.clone(),
                         tr.L.clone()))
        tr.on_epoch_finished(visit)
    return seen


def test_trainer_two_visits_fused_equals_switched_off(monkeypatch):
    new = _run_trainer(monkeypatch, True)
    old = _run_trainer(monkeypatch, False)
    assert len(new) == len(old) == 4
    for i, (a, b) in enumerate(zip(new, old)):
        for name, x, y in zip(("table", "rgrad", "L"), a, b):
            assert torch.equal(x, y), f"{name}, step {i}"
    assert not torch.equal(new[0][0], new[3][0])
