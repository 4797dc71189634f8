"""MLR app arg data_dtype=bfloat16 without a device: what the blocks hold,
the tensor-op route's result, the argument errors, and the checks of the
bf16 branch of the three HIP entries (CPU tensors never reach a launch)."""

import pytest
import torch

from harmony_amd import ops
from harmony_amd.config import JobConfig
from harmony_amd.mlapps import heldout, mlr
from tests import heldout_cases as hc

bf16, f32, i64 = torch.bfloat16, torch.float32, torch.int64


def job(**args):
    return JobConfig(job_id="t_mlr_bf16_cpu", app="mlr", max_num_epochs=2,
                     num_mini_batches=2, app_args={
                         "num_classes": 5, "num_features": 64,
                         "batch_size": 48, "num_parts_per_class": 2, **args})


def blocks(**args):
    return mlr.make_batches(job(**args), 0, torch.device("cpu"))


def test_blocks_are_bf16_and_half_the_bytes():
    half, full = blocks(data_dtype="bfloat16"), blocks()
    for (x, y), (x32, y32) in zip(half, full):
        assert x.dtype == bf16 and x32.dtype == f32 and y.dtype == i64
        assert 2 * x.numel() * x.element_size() == \
            x32.numel() * x32.element_size()
        assert torch.equal(x, x32.to(bf16)) and torch.equal(y, y32)
    x, y = mlr.reslice(half[0], 0.3)
    assert x.dtype == bf16 and x.shape == (14, 64) and y.shape == (14,)


def test_summary_equals_a_float32_run_on_rounded_data(monkeypatch):
    s, trainer = hc.run(job(data_dtype="bfloat16"))
    monkeypatch.setattr(heldout, "stored", lambda X, a: X.to(bf16).float())
    s32, trainer32 = hc.run(job())
    assert s["cross_entropy"] == s32["cross_entropy"]
    assert s["accuracy"] == s32["accuracy"]
    assert torch.equal(trainer.accessor.pull_all(),
                       trainer32.accessor.pull_all())


@pytest.mark.parametrize("args", [
    {"data_dtype": "bfloat16", "sparse": "true"}, {"data_dtype": "float16"}])
def test_unsupported_arguments_raise(args):
    with pytest.raises(ValueError, match="data_dtype"):
        hc.hand_built(job(**args))


def z(*shape, dt=f32):
    return torch.zeros(*shape, dtype=dt)


# entry -> well-formed bf16 arguments in binding order
ENTRIES = {
    "mlr_step_mfma": lambda: dict(X=z(40, 64, dt=bf16), Wt=z(64, 16),
                                  labels=z(40, dt=i64), row_block=0, C=3,
                                  splitf=2, splitb=3),
    "mlr_fwd_mfma_part": lambda: dict(X=z(40, 64, dt=bf16), Wt=z(64, 16),
                                      P=z(40, 16), off=3, n=37, splitf=2),
    "mlr_grad_mfma_part": lambda: dict(P=z(40, 16), X=z(40, 64, dt=bf16),
                                       gradT=z(16, 64), off=3, n=37,
                                       splitb=3),
}
BAD = [
    ("mlr_fwd_mfma_part", dict(X=z(40, 48, dt=bf16), Wt=z(48, 16)), "X"),
    ("mlr_grad_mfma_part", dict(X=z(40 * 64 + 1, dt=bf16)[1:].view(40, 64)),
     "X"),
    ("mlr_step_mfma", dict(row_block=64), "row_block"),
    ("mlr_fwd_mfma_part", dict(n=38), "off"),
    ("mlr_grad_mfma_part", dict(off=-1), "off"),
    ("mlr_step_mfma", dict(Wt=z(64, 8)), "Wt"),
    ("mlr_fwd_mfma_part", dict(splitf=4), "splitf"),
    ("mlr_step_mfma", dict(C=17), "C"),
]

needs_hip = pytest.mark.skipif(not ops.hip_available(),
                               reason="HIP extension not built")


@needs_hip
@pytest.mark.parametrize("op", list(ENTRIES))
def test_well_formed_bf16_call_stops_at_the_device_check(op):
    with pytest.raises(RuntimeError, match=op + ": every tensor must be on "
                       "device"):
        getattr(ops._load_hip(), op)(*ENTRIES[op]().values())


@needs_hip
@pytest.mark.parametrize("op,change,named", BAD)
def test_bf16_branch_names_the_malformed_argument(op, change, named):
    kwargs = {**ENTRIES[op](), **change}
    with pytest.raises(RuntimeError) as e:
        getattr(ops._load_hip(), op)(*kwargs.values())
    msg = str(e.value).split("\n")[0]
    assert "on device" not in msg and msg.startswith(op + ": "), msg
    assert named in msg[len(op):], msg
