"""ops.mlr_grad_finish (the MLR step's tail in one kernel) against the chain
it replaces on the single-owner path, bit for bit:

    grad_raw = g / B + lam * W              (three tensor ops)
    delta = (-step) * grad_raw              (one)
    table.push_dense(delta)                 (ops.dense_apply, "add")

Both sides get the same g, W and table in the same process, so every
comparison is torch.equal. B = 200 is no power of two: its reciprocal is
inexact, and the kernel has to divide the way the tensor op does.
"""

import pytest
import torch

from harmony_amd import ops

pytestmark = pytest.mark.gpu

# (B, F, C, P): table rows of F/P floats; C * F = 960, 3072 (twelve blocks
# of 256 threads) and 8192 elements
SHAPES = [(64, 96, 10, 8), (200, 1024, 3, 1), (512, 512, 16, 8)]


def chain(g, W, table, B, lam, step):
    grad_raw = g / B + lam * W
    delta = (-step) * grad_raw
    ops.dense_apply(table, delta.view_as(table), "add")
    return grad_raw


@pytest.mark.parametrize("lam", [0.0, 1e-4])
@pytest.mark.parametrize("B,F,C,P", SHAPES)
def test_finish_equals_tensor_op_chain(B, F, C, P, lam):
    gen = torch.Generator().manual_seed(B + F)
    x = torch.randn(B, F, generator=gen).cuda()
    y = torch.randint(0, C, (B,), generator=gen).cuda()
    t_old = (torch.randn(C * P, F // P, generator=gen) * 0.01).cuda()
    t_new = t_old.clone()
    step = 0.01
    for visit in range(2):
        # today: the pulled model is a copy of the table
        W_old = t_old.clone().view(C, F)
        p, _, _ = ops.mlr_forward(x, W_old, y)
        g = ops.mlr_grad_gemm(p, x)
        assert g.abs().max() > 0
        want = chain(g, W_old, t_old, B, lam, step)
        # new: W is the table itself, read in place
        got = ops.mlr_grad_finish(g, t_new.view(C, F), t_new, B, lam, step)
        assert got.shape == (C, F)
        assert torch.equal(got, want), f"grad_raw, visit {visit}"
        assert torch.equal(t_new, t_old), f"table, visit {visit}"
        step *= 0.9                     # the epoch decay


def test_finish_with_a_copy_of_the_model():
    """W apart from the shard (the pulled copy) gives the same bits as W in
    place."""
    B, F, C, P = 200, 1024, 3, 1
    gen = torch.Generator().manual_seed(1)
    g = torch.randn(C, F, generator=gen).cuda()
    t_a = torch.randn(C * P, F // P, generator=gen).cuda()
    t_b = t_a.clone()
    a = ops.mlr_grad_finish(g, t_a.view(C, F), t_a, B, 1e-4, 0.01)
    b = ops.mlr_grad_finish(g, t_b.clone().view(C, F), t_b, B, 1e-4, 0.01)
    assert torch.equal(a, b) and torch.equal(t_a, t_b)


def test_finish_rejects_bad_arguments():
    g = torch.zeros(3, 8, device="cuda")
    t = torch.zeros(3, 8, device="cuda")
    with pytest.raises(RuntimeError, match="shard must hold"):
        ops.mlr_grad_finish(g, g.clone(), torch.zeros(3, 4, device="cuda"),
                            4, 0.0, 0.1)
    with pytest.raises(RuntimeError, match="B must be positive"):
        ops.mlr_grad_finish(g, g.clone(), t, 0, 0.0, 0.1)
    buf = torch.zeros(3 * 8 + 4, device="cuda")
    with pytest.raises(RuntimeError, match="the shard itself or apart"):
        ops.mlr_grad_finish(g, buf[4:].view(3, 8), buf[:24].view(3, 8), 4,
                            0.0, 0.1)


def _run_trainer(monkeypatch, fused: bool):
    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.mlapps import mlr
    from harmony_amd.runtime.bootstrap import init_executor

    monkeypatch.setenv("HARMONY_FUSED_TAIL", "1" if fused else "0")
    ctx = init_executor(RuntimeConfig(device="cuda"))
    job = JobConfig(job_id="mlr_tail", app="mlr", num_mini_batches=2,
                    app_args={"num_classes": 10, "num_features": 96,
                              "num_parts_per_class": 8, "batch_size": 200,
                              "step_size": 0.05, "decay_period": 1})
    tables, tr, provider = mlr.build(job, ctx, None)
    table = next(iter(tables.values()))
    seen = []
    for visit in range(2):
        for b in provider.blocks:
            tr.set_batch_data(b)
            tr.pull_model()
            tr.local_compute()
            tr.push_update()
            seen.append((table.pull_all().clone(), tr.grad_raw.clone()))
        tr.on_epoch_finished(visit)         # decays the step
    assert tr._fused is fused
    assert tr.step_size < 0.05
    return seen, tr.evaluate_model()


def test_trainer_two_visits_fused_equals_switched_off(monkeypatch):
    new, m_new = _run_trainer(monkeypatch, True)
    old, m_old = _run_trainer(monkeypatch, False)
    assert len(new) == len(old) == 4
    for i, ((t_n, g_n), (t_o, g_o)) in enumerate(zip(new, old)):
        assert torch.equal(g_n, g_o), f"grad_raw, step {i}"
        assert torch.equal(t_n, t_o), f"table, step {i}"
    assert not torch.equal(new[0][0], new[3][0])
    assert m_new["accuracy"] == m_old["accuracy"]
