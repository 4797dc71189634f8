"""Sparse MLR on the CPU: CSR parsers, SparseBatch, the ops' torch
references against fp64, the trainer step and whole jobs."""

import pytest
import torch

from harmony_amd import dataloader as dl
from harmony_amd import ops
from tests import mlr_sparse_cases as mc


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def _batch(csr, F):
    from harmony_amd.mlapps.sparse_batch import SparseBatch

    row_ptr, col, val, _y = csr
    return SparseBatch(row_ptr, col, val, F)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32),
                                              b.view(torch.int32))


# ----------------------------------------------------------------- parsers

def _check_parsers(path, F):
    whole = (0, 10 ** 9)
    X, y = dl.parse_libsvm(dl.read_split(path, whole), F)
    csr = dl.parse_libsvm_csr(dl.read_split(path, whole), F)
    row_ptr, col, val, ys = csr
    assert row_ptr.dtype == torch.int64 and col.dtype == torch.int32
    assert val.dtype == torch.float32 and ys.dtype == torch.float32
    assert row_ptr.shape[0] == X.shape[0] + 1 and int(row_ptr[0]) == 0
    assert _same_bits(_batch(csr, F).to_dense(), X)
    assert _same_bits(ys, y)
    # each (row, col) once, every index in range
    key = mc.seg_of(row_ptr) * F + col.long()
    assert key.unique().shape[0] == key.shape[0]
    assert bool(((col >= 0) & (col < F)).all())
    # the split entry point gives the same CSR whichever parser it picks
    for a, b in zip(dl.parse_libsvm_csr_split(path, 0, 1, F), csr):
        assert a.dtype == b.dtype and torch.equal(a, b)
    if ops.hip_available():
        with open(path, "rb") as f:
            nat = dl.parse_libsvm_csr_bytes(f.read(), F)
        for a, b in zip(nat, csr):
            assert a.dtype == b.dtype and torch.equal(a, b)
    return csr


def test_parser_equals_dense_hand_text(tmp_path):
    p = _write(tmp_path, "hand.txt", mc.HAND_TEXT)
    row_ptr, col, val, y = _check_parsers(p, mc.HAND_F)
    assert y.tolist() == [1.0, 2.0, 0.0, 1.0, 3.0]
    assert row_ptr.tolist() == [0, 2, 2, 5, 8, 10]       # row 1 is empty
    # file order kept; the repeated index 2 sits at its first position with
    # its last value; 9 >= F is gone
    assert col.tolist() == [0, 3, 5, 2, 1, 2, 4, 0, 3, 1]
    assert val[5].item() == 0.375


def test_parser_drops_negative_indices():
    lines = ["1 -1:5.0 2:1.0 -7:2.0", "0 3:4.0"]
    row_ptr, col, val, _y = dl.parse_libsvm_csr(lines, 4)
    assert row_ptr.tolist() == [0, 1, 2] and col.tolist() == [2, 3]
    if ops.hip_available():
        buf = ("\n".join(lines) + "\n").encode()
        nat = dl.parse_libsvm_csr_bytes(buf, 4)
        assert nat[0].tolist() == [0, 1, 2] and nat[1].tolist() == [2, 3]
        Xn, _ = ops._load_hip().parse_libsvm_bytes(buf, 4)
        assert _same_bits(_batch(nat, 4).to_dense(), Xn)


def test_parser_equals_dense_golden_sample():
    row_ptr, col, val, y = _check_parsers(str(mc.GOLDEN), 784)
    assert y.shape[0] == 32 and set(y.tolist()) <= set(map(float, range(10)))
    assert col.shape[0] > 32 * 50                       # ~19 % of 784 per row


def test_parser_memory_independent_of_num_features(monkeypatch):
    F = 2 ** 24
    monkeypatch.setattr(dl, "parse_libsvm", None)       # dense: not called
    g = torch.Generator().manual_seed(3)
    lines, nnz = [], 0
    for r in range(64):
        k = r % 9
        idx = torch.randint(0, F, (k,), generator=g).unique().tolist()
        nnz += len(idx)
        lines.append(f"{r % 10} " + " ".join(f"{i}:{0.5 + i % 3}"
                                             for i in idx))
    row_ptr, col, val, y = dl.parse_libsvm_csr(lines, F)
    assert (row_ptr.numel(), col.numel(), val.numel(), y.numel()) == \
        (65, nnz, nnz, 64)
    if ops.hip_available():
        nat = dl.parse_libsvm_csr_bytes(("\n".join(lines) + "\n").encode(), F)
        for a, b in zip(nat, (row_ptr, col, val, y)):
            assert a.dtype == b.dtype and torch.equal(a, b)
    b = _batch((row_ptr, col, val, y), F)
    assert b.shape == (64, F)
    total = sum(t.numel() for t in (b.feat_ids, b.feat_ptr, b.feat_row,
                                    b.feat_val))
    assert total <= 4 * nnz + 1


# ------------------------------------------------------------ column index

def _check_index(b):
    B, F = b.shape
    nnz = b.col.shape[0]
    assert b.feat_ids.dtype == torch.int32 and b.feat_row.dtype == torch.int32
    assert b.feat_ptr.dtype == torch.int64
    assert b.feat_val.dtype == torch.float32
    nf = b.feat_ids.shape[0]
    assert b.feat_ptr.shape[0] == nf + 1 and int(b.feat_ptr[0]) == 0
    assert int(b.feat_ptr[-1]) == nnz == b.feat_row.shape[0]
    assert bool((b.feat_ids[1:] > b.feat_ids[:-1]).all())
    assert bool((b.feat_ptr[1:] > b.feat_ptr[:-1]).all())   # present only
    feat_of = b.feat_ids.long()[mc.seg_of(b.feat_ptr)]
    # rows ascend within a feature <=> (feature, row) keys ascend strictly
    key_csc = feat_of * max(B, 1) + b.feat_row.long()
    assert bool((key_csc[1:] > key_csc[:-1]).all())
    # a permutation of the CSR entries: same (row, col, value) triples
    key_csr = b.col.long() * max(B, 1) + mc.seg_of(b.row_ptr)
    order = torch.argsort(key_csr)
    assert torch.equal(key_csr[order], key_csc)
    assert _same_bits(b.val[order], b.feat_val)


def _same_batch(a, b):
    assert a.shape == b.shape
    for name in ("row_ptr", "col", "val", "feat_ids", "feat_ptr",
                 "feat_row", "feat_val"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and torch.equal(x, y), name


def test_column_index_and_prefix(tmp_path):
    from harmony_amd.mlapps.sparse_batch import SparseBatch

    csr = dl.parse_libsvm_csr(
        dl.read_split(str(mc.GOLDEN), (0, 10 ** 9)), 784)
    hand = dl.parse_libsvm_csr(mc.HAND_TEXT.splitlines(), mc.HAND_F)
    for (row_ptr, col, val, _y), F in ((csr, 784), (hand, mc.HAND_F)):
        b = SparseBatch(row_ptr, col, val, F)
        _check_index(b)
        B = b.shape[0]
        for n in (0, 1, B):
            e = int(row_ptr[n])
            direct = SparseBatch(row_ptr[:n + 1], col[:e], val[:e], F)
            pre = b.prefix(n)
            assert pre.shape == (n, F)
            _same_batch(pre, direct)
            _check_index(pre)
        assert _same_bits(b.to("cpu").to_dense(), b.to_dense())


# ---------------------------------------------------- ops reference vs fp64

ROW_LENS = [0, 1, 200] + [(7 * r) % 23 for r in range(64)]     # B = 67


@pytest.mark.parametrize("C", [2, 10, 17])
def test_ops_reference_forward_vs_fp64(C):
    B, F = 67, 130
    row_ptr, col, val = mc.segments(ROW_LENS, F, every=5, seed=C, absent=11)
    W = torch.randn(C, F, generator=torch.Generator().manual_seed(100 + C))
    want, mag, n = mc.gather_reduce64(row_ptr, col, val, W.t())
    got = ops.mlr_sparse_logits(row_ptr, col, val, W)
    assert got.shape == (B, C) and got.dtype == torch.float32
    assert bool(((got.double() - want).abs() <= mc.bound(n, mag)).all())
    assert bool((got[0] == 0).all())                    # the empty row
    # same contract as the dense forward on the densified batch
    labels = torch.arange(B) % C
    p, loss, correct = ops.mlr_sparse_forward(row_ptr, col, val, W, labels)
    pd, lossd, correctd = ops.softmax_grad_ce(got, labels)
    assert torch.equal(p, pd) and torch.equal(loss, lossd)
    assert int(correct) == int(correctd)
    assert p.shape == (B, C) and loss.dim() == 0


@pytest.mark.parametrize("C", [2, 10, 17])
def test_ops_reference_grad_vs_fp64(C):
    from harmony_amd.mlapps.sparse_batch import SparseBatch

    B, F = 67, 130
    row_ptr, col, val = mc.segments(ROW_LENS, F, every=5, seed=C, absent=11)
    b = SparseBatch(row_ptr, col, val, F)
    assert 11 not in b.feat_ids.tolist()
    every = int(b.feat_ptr[b.feat_ids.tolist().index(5) + 1]
                - b.feat_ptr[b.feat_ids.tolist().index(5)])
    assert every >= B - 1                     # every row that has entries
    P = torch.randn(B, C, generator=torch.Generator().manual_seed(200 + C))
    want, mag, n = mc.gather_reduce64(b.feat_ptr, b.feat_row, b.feat_val, P)
    got = ops.mlr_sparse_grad(b.feat_ids, b.feat_ptr, b.feat_row,
                              b.feat_val, P, F)
    assert got.shape == (C, F) and got.dtype == torch.float32
    ids = b.feat_ids.long()
    err = (got[:, ids].t().double() - want).abs()
    assert bool((err <= mc.bound(n, mag)).all())
    absent = torch.ones(F, dtype=torch.bool)
    absent[ids] = False
    assert bool(absent[11]) and bool((got[:, absent] == 0).all())


def test_group_rule():
    assert ops.mlr_sparse_group(0, 0) == 1
    assert ops.mlr_sparse_group(10, 80) == 1
    assert ops.mlr_sparse_group(10, 81) == 2
    assert ops.mlr_sparse_group(16384, 16384 * 32) == 4
    assert ops.mlr_sparse_group(16384, 16384 * 256) == 32
    assert ops.mlr_sparse_group(1, 10 ** 6) == 64


# ------------------------------------------------------------ trainer step

def _build_mlr(job):
    from harmony_amd.config import RuntimeConfig
    from harmony_amd.mlapps import mlr
    from harmony_amd.runtime.bootstrap import init_executor
    from harmony_amd.runtime.control import ControlPlane

    ctx = init_executor(RuntimeConfig(device="cpu"))
    cp = ControlPlane(ctx.store, ctx.rank, ctx.world_size)
    return mlr.build(job, ctx, cp)


def _file_job(tmp_path, job_id, **kw):
    from harmony_amd.config import JobConfig

    p = _write(tmp_path, "data.txt", "\n".join(mc.job_file_lines()) + "\n")
    args = {"input": p, "num_classes": 3, "num_features": 4,
            "num_parts_per_class": 2, "step_size": 1.0, "sparse": "true"}
    return JobConfig(job_id=job_id, app="mlr", app_args=args, **kw)


def test_trainer_step_vs_fp64(tmp_path):
    from harmony_amd.mlapps.sparse_batch import SparseBatch

    job = _file_job(tmp_path, "sp_step", max_num_epochs=1,
                    num_mini_batches=1)
    _tables, trainer, provider = _build_mlr(job)
    assert provider.num_batches == 1
    x, y = provider.blocks[0]
    assert isinstance(x, SparseBatch) and x.shape == (256, 4)
    trainer.set_batch_data((x, y))
    assert trainer.num_batch_examples() == 256
    trainer.pull_model()
    trainer.local_compute()
    W = trainer._w_matrix().double()
    B, lam = 256, trainer.a["lam"]
    X = x.to_dense().double()
    z = X @ W.t()
    p = torch.softmax(z, dim=1)
    p[torch.arange(B), y] -= 1.0
    want = p.t() @ X / B + lam * W
    n_row_max = int((x.row_ptr[1:] - x.row_ptr[:-1]).max())
    col_mass = float(X.abs().sum(dim=0).max()) / B
    tol = 32 * mc.U * (B + n_row_max) * (1 + col_mass)
    err = float((trainer.grad_raw.double() - want).abs().max())
    print(f"trainer step: max err {err:.3e}, bound {tol:.3e}")
    assert tol < 1e-3           # a dropped or doubled non-zero moves > 1e-3
    assert err <= tol
    # the stopped-worker batch still gives a zero gradient
    trainer.set_batch_data((x.prefix(0), y[:0]))
    trainer.local_compute()
    assert trainer.num_batch_examples() == 0
    assert trainer.grad_raw.shape == (3, 4)
    assert not bool(trainer.grad_raw.any())


# -------------------------------------------------------------------- jobs

def test_sparse_flag_from_cli():
    from harmony_amd.config import JobConfig
    from harmony_amd.jobserver.client import _parse_flags
    from harmony_amd.mlapps import mlr

    def sparse(argv):
        _kw, app_args, _w = _parse_flags(argv)
        return mlr._is_sparse(mlr.defaults(
            JobConfig(job_id="j", app="mlr", app_args=app_args)))

    assert sparse(["-sparse", "true"]) and sparse(["-sparse", "1"])
    assert not sparse(["-sparse", "false"]) and not sparse([])


def test_sparse_job_from_file(tmp_path):
    from harmony_amd.config import RuntimeConfig
    from harmony_amd.dolphin.master import run_job
    from harmony_amd.runtime.bootstrap import init_executor

    job = _file_job(tmp_path, "sp_file_mlr", max_num_epochs=3,
                    num_mini_batches=4)
    ctx = init_executor(RuntimeConfig(device="cpu"))
    s = run_job(job, ctx).summary()
    assert s["num_batches"] == 12
    assert s["total_examples"] == 3 * 256
    assert s["accuracy"] > 0.6


def test_sparse_job_matches_dense_job(tmp_path):
    # same file, same seed, same batch order: the two paths differ only by
    # fp32 summation order, so the trained models' metrics agree closely
    from harmony_amd.config import RuntimeConfig
    from harmony_amd.dolphin.master import run_job
    from harmony_amd.runtime.bootstrap import init_executor

    ctx = init_executor(RuntimeConfig(device="cpu"))
    sp = _file_job(tmp_path, "same_id", max_num_epochs=3, num_mini_batches=4)
    s1 = run_job(sp, ctx).summary()
    de = _file_job(tmp_path, "same_id", max_num_epochs=3, num_mini_batches=4)
    de.app_args["sparse"] = "false"
    s2 = run_job(de, ctx).summary()
    assert s1["accuracy"] == s2["accuracy"]
    assert abs(s1["cross_entropy"] - s2["cross_entropy"]) < 1e-4


def test_sparse_job_synthetic():
    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.dolphin.master import run_job
    from harmony_amd.mlapps import mlr
    from harmony_amd.mlapps.sparse_batch import SparseBatch
    from harmony_amd.runtime.bootstrap import init_executor

    job = JobConfig(job_id="sp_syn", app="mlr", max_num_epochs=1,
                    num_mini_batches=3,
                    app_args={"num_classes": 5, "num_features": 4096,
                              "num_parts_per_class": 2, "batch_size": 64,
                              "nnz_per_row": 12, "sparse": "1"})
    blocks = mlr.make_batches(job, 0, torch.device("cpu"))
    again = mlr.make_batches(job, 0, torch.device("cpu"))
    other = mlr.make_batches(job, 1, torch.device("cpu"))
    assert len(blocks) == 3
    for (x, y), (x2, y2) in zip(blocks, again):
        assert isinstance(x, SparseBatch) and x.shape == (64, 4096)
        _same_batch(x, x2)                         # deterministic per rank
        assert torch.equal(y, y2)
        lens = x.row_ptr[1:] - x.row_ptr[:-1]
        assert int(lens.max()) <= 12 and int(lens.min()) >= 1
        _check_index(x)
    assert not torch.equal(blocks[0][0].col, other[0][0].col)
    ctx = init_executor(RuntimeConfig(device="cpu"))
    s = run_job(job, ctx).summary()
    assert s["num_batches"] == 3 and s["total_examples"] == 3 * 64


def test_sparse_job_set_share(tmp_path):
    from harmony_amd.dolphin.worker import WorkerTasklet
    from harmony_amd.mlapps.sparse_batch import SparseBatch
    from harmony_amd.runtime.control import ControlPlane, TaskUnitScheduler
    from harmony_amd.config import RuntimeConfig
    from harmony_amd.runtime.bootstrap import init_executor

    for share, rows in ((0.5, 32), (0.0, 0)):
        job = _file_job(tmp_path, f"sp_share_{rows}", max_num_epochs=2,
                        num_mini_batches=4)
        ctx = init_executor(RuntimeConfig(device="cpu"))
        cp = ControlPlane(ctx.store, ctx.rank, ctx.world_size)
        from harmony_amd.mlapps import mlr

        _tables, trainer, provider = mlr.build(job, ctx, cp)
        provider.set_share(share)
        for x, y in provider.epoch_iter(0):
            assert isinstance(x, SparseBatch)
            assert x.shape == (rows, 4) and y.shape[0] == rows
        tus = TaskUnitScheduler(cp, {job.job_id}, multi_job=False)
        m = WorkerTasklet(job, trainer, provider, cp, tus, ctx.rank,
                          ctx.world_size).run()
        s = m.summary()
        assert s["num_batches"] == 8
        assert s["total_examples"] == 8 * rows
