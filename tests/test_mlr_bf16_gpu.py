"""MLR on bfloat16 training data, on the device: the K4-BF16 kernels
(ops/csrc/mlr_bf16.hip) against a float64 oracle on X.double().

Bounds. X is exact in bf16 and the kernels split W and P into three bf16
terms that sum to the float32 value, so only float32 accumulation is left:
k * 2^-24 * sum|terms| for a sum of k products in any order, doubled for
combining the accumulator chains and the split partials.
"""

import pytest
import torch

from harmony_amd import ops
from harmony_amd.config import JobConfig
from tests import heldout_cases as hc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BS, FS, CS = [1, 17, 64, 200], [32, 96, 512], [1, 10, 16]
ENTRIES = ("mlr_step_mfma", "mlr_fwd_mfma_part", "mlr_grad_mfma_part")


def make(B, F, C, seed=11):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(B, F, generator=g).bfloat16()
    W = torch.randn(C, F, generator=g)
    return X, W, torch.randint(0, C, (B,), generator=g)


def padded(M, dim):
    """M with `dim` zero-padded to 16, on the device."""
    shape = list(M.shape)
    shape[dim] = 16 - shape[dim]
    return torch.cat([M, torch.zeros(shape)], dim).contiguous().cuda()


@pytest.fixture()
def entry_calls(monkeypatch):
    """Counts the launches through the three HIP entries."""
    hip, calls = ops._load_hip(), []
    for name in ENTRIES:
        real = getattr(hip, name)
        monkeypatch.setattr(hip, name, lambda *a, _r=real, _n=name:
                            calls.append((_n, a[0].dtype, a[1].dtype))
                            or _r(*a))
    return calls


def oracle(X, W, y):
    """float64 (softmax - onehot, loss sum, correct count, gradient, logits)."""
    z = X.double() @ W.double().T
    p = torch.softmax(z, dim=1)
    p[torch.arange(len(y)), y] -= 1
    loss = (torch.logsumexp(z, dim=1) - z[torch.arange(len(y)), y]).sum()
    return p, float(loss), int((z.argmax(dim=1) == y).sum()), p.T @ X.double(), z


@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("B", BS)
def test_forward_gemm(B, F, C, largest):
    X, W, _y = make(B, F, C)
    P = torch.full((B, 16), float("nan"), device="cuda")
    ops._load_hip().mlr_fwd_mfma_part(X.cuda(), padded(W.T, 1), P, 0, B,
                                      F // 32 if largest else 1)
    got = P.cpu().double()
    bound = 2 * F * U * (X.double().abs() @ W.double().abs().T)
    assert ((got[:, :C] - X.double() @ W.double().T).abs() <= bound).all()
    assert (got[:, C:] == 0).all()


@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("B", BS)
def test_gradient_gemm(B, F, C, largest):
    X, W, _y = make(B, F, C)
    P = torch.randn(B, C, generator=torch.Generator().manual_seed(5))
    gradT = torch.zeros(16, F, device="cuda")
    # the most splits with work: one 32-row MFMA step each
    ops._load_hip().mlr_grad_mfma_part(padded(P, 1), X.cuda(), gradT, 0, B,
                                       -(-B // 32) if largest else 1)
    got = gradT.cpu().double()
    bound = 2 * B * U * (P.double().abs().T @ X.double().abs())
    assert ((got[:C] - P.double().T @ X.double()).abs() <= bound).all()
    assert (got[C:] == 0).all()


# seeds for which the precondition below holds
@pytest.mark.parametrize("B,F,C,seed", [(200, 96, 10, 12),
                                        (512, 512, 10, 2538)])
def test_step(B, F, C, seed, entry_calls):
    X, W, y = make(B, F, C, seed)
    _p, loss, correct, grad, z = oracle(X, W, y)
    # precondition: no row's argmax can flip within the forward bound
    top2 = z.topk(2, dim=1).values
    bound = 2 * F * U * (X.double().abs() @ W.double().abs().T).max(dim=1).values
    assert ((top2[:, 0] - top2[:, 1]) > 10 * bound).all()

    def errors(g, l, c):
        return (float((g.cpu().double() - grad).abs().max() / grad.abs().max()),
                abs(float(l) - loss) / abs(loss), int(c))

    got = errors(*ops.mlr_step_mfma(X.cuda(), W.cuda(), y.cuda()))
    assert [c[:2] for c in entry_calls] == [("mlr_step_mfma", torch.bfloat16)]
    xf = X.float().cuda()
    p32, l32, c32 = ops.mlr_forward(xf, W.cuda(), y.cuda())
    f32 = errors(ops.mlr_grad_gemm(p32, xf), l32, c32)
    print(f"({B}, {F}, {C}): grad rel / loss rel / correct: bf16 step {got}, "
          f"float32 default on X.float() {f32}, oracle correct {correct}")
    assert got[0] < 1e-3 and got[1] < 1e-2 and got[2] == correct


def test_runs_agree_bit_for_bit():
    X, W, y = (t.cuda() for t in make(200, 512, 10))
    first = ops.mlr_step_mfma(X, W, y, splitf=4, splitb=3)
    again = ops.mlr_step_mfma(X, W, y, splitf=4, splitb=3)
    assert all(torch.equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("B,F,C", [(100, 40, 10), (100, 64, 17)])
def test_other_shapes_take_the_tensor_ops(B, F, C, entry_calls):
    X, W, y = (t.cuda() for t in make(B, F, C))
    assert not ops.mlr_bf16_ok(X, C)
    g, loss, correct = ops.mlr_step_mfma(X, W, y)
    p, loss1, correct1 = ops.mlr_forward(X, W, y)
    g1 = ops.mlr_grad_gemm(p, X)
    assert entry_calls == []
    p32, l32, c32 = ops.mlr_forward(X.float(), W, y)
    for a, b in ((g, p32.T @ X.float()), (g1, g), (loss, l32), (loss1, l32)):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5)
    assert int(correct) == int(correct1) == int(c32)


def test_job(entry_calls):
    def job():
        return JobConfig(
            job_id="t_mlr_bf16_job", app="mlr", max_num_epochs=1,
            num_mini_batches=2, app_args={
                "num_classes": 10, "num_features": 96, "batch_size": 200,
                "num_parts_per_class": 2, "data_dtype": "bfloat16"})

    s, _trainer = hc.run(job(), device="cuda")
    # the blocks reach the step entry as bf16, W^T as float32, once per batch
    assert entry_calls == [("mlr_step_mfma", torch.bfloat16,
                            torch.float32)] * 2
    cpu, _ = hc.run(job(), device="cpu")
    print(f"cross_entropy cuda {s['cross_entropy']!r}, "
          f"cpu {cpu['cross_entropy']!r}")
    assert abs(s["cross_entropy"] - cpu["cross_entropy"]) \
        <= 1e-2 * cpu["cross_entropy"]
