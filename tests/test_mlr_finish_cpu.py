"""Argument checks of the mlr_grad_finish binding, as every launching binding
has them (tests/test_binding_checks_cpu.py): a well-formed call with CPU
tensors stops at the device check, a malformed argument is reported as
itself wherever the tensors live. And the CPU path of ops.mlr_grad_finish is
the tensor-op chain."""

import pytest
import torch

from harmony_amd import ops

pytestmark = pytest.mark.skipif(not ops.hip_available(),
                                reason="HIP extension not built")


def good():
    return dict(g=torch.zeros(3, 8), W=torch.zeros(3, 8),
                shard=torch.zeros(6, 4), B=4, lam=0.0, step=0.1)


def call(kwargs):
    return ops._load_hip().tail.mlr_grad_finish(*kwargs.values())


def test_well_formed_cpu_call_stops_at_the_device_check():
    with pytest.raises(RuntimeError, match="mlr_grad_finish: every tensor "
                       "must be on device") as e:
        call(good())
    assert "got cpu" in str(e.value)


@pytest.mark.parametrize("name,value,word", [
    ("g", torch.zeros(24), "g must be"),
    ("W", torch.zeros(3, 9), "W must be"),
    ("W", torch.zeros(3, 8, dtype=torch.float64), "W must be"),
    ("shard", torch.zeros(6, 5), "shard must hold"),
    ("shard", torch.zeros(6, 8)[:, ::2], "shard must be"),
    ("B", 0, "B must be positive"),
])
def test_malformed_argument_is_reported(name, value, word):
    kwargs = good()
    kwargs[name] = value
    with pytest.raises(RuntimeError, match="mlr_grad_finish: " + word):
        call(kwargs)


def test_cpu_path_is_the_tensor_op_chain():
    gen = torch.Generator().manual_seed(0)
    g, W = torch.randn(3, 8, generator=gen), torch.randn(3, 8, generator=gen)
    shard = W.clone().view(6, 4)
    want_grad = g / 5 + 1e-4 * W
    want_table = W + (-0.1) * want_grad
    got = ops.mlr_grad_finish(g, W, shard, 5, 1e-4, 0.1)
    assert torch.equal(got, want_grad)
    assert torch.equal(shard.view(3, 8), want_table)
