"""K4 (ops/csrc/mlr.hip) and K4-MFMA (mlr_mfma.hip) on the GPU against the
float64 references of mlr_dense_cases, at the shapes where their tails,
tiles, row blocks and splits change. Bounds: the docstring of
mlr_dense_cases."""

import pytest
import torch

from tests import mlr_dense_cases as mc

pytestmark = pytest.mark.gpu


def _show(name, figs):
    print(name + ": " + ", ".join(f"{k} error {e:.3g} (bound/ratio {b:.3g})"
                                  for k, (e, b) in figs.items()))


@pytest.mark.parametrize("variant", mc.SOFTMAX_VARIANTS)
@pytest.mark.parametrize("idx", range(len(mc.SOFTMAX_SHAPES)))
def test_softmax_grad_ce(idx, variant):
    from harmony_amd import ops

    z, y = mc.softmax_case(idx, variant)
    zg = z.cuda()
    g, loss, correct = ops.softmax_grad_ce(zg, y.cuda())
    assert g.is_cuda and torch.equal(zg.cpu(), z)
    figs = mc.check_softmax(g.cpu(), loss, correct, z.double(),
                            torch.zeros(z.shape, dtype=torch.float64), y,
                            mc.ATOL_SOFTMAX, (idx, variant))
    if variant == "scale30" and z.shape[1] > 1:
        assert float(g[0, y[0]]) == -1.0
    _show(f"softmax_grad_ce {mc.SOFTMAX_SHAPES[idx]} {variant}", figs)


@pytest.mark.parametrize("shape", mc.FWD_SHAPES)
def test_mlr_fwd(shape):
    from harmony_amd import ops

    X, W, y = mc.fwd_case(*shape)
    z, dz = mc.logits_ref(X, W)
    g, loss, correct = ops._load_hip().mlr_fwd(X.cuda(), W.cuda(), y.cuda())
    figs = mc.check_softmax(g.cpu(), loss, correct, z, dz, y, mc.ATOL_FUSED,
                            shape)
    _show(f"mlr_fwd {shape}", figs)


@pytest.mark.parametrize("idx", range(len(mc.GRAD_SHAPES)))
def test_mlr_grad(idx):
    from harmony_amd import ops

    P, X, ref, bound = mc.grad_case(idx)
    got = ops._load_hip().mlr_grad(P.cuda(), X.cuda())
    err, ratio = mc.check_sum(got.cpu(), ref, bound, idx)
    print(f"mlr_grad {mc.GRAD_SHAPES[idx]}: error {err:.3g}, "
          f"error / bound {ratio:.3f}")


def _step(case, fn=None, **kw):
    from harmony_amd import ops

    fn = fn or ops.mlr_step_mfma
    X, W, y = case["X"].cuda(), case["W"].cuda(), case["y"].cuda()
    grad, loss, correct = fn(X, W, y, **kw)
    torch.cuda.synchronize()
    assert torch.equal(X.cpu(), case["X"]) and torch.equal(W.cpu(), case["W"])
    return grad.cpu(), float(loss), int(correct)


@pytest.mark.parametrize("B,F,C,rb,sf,sb", mc.STEP_CASES)
def test_mlr_step_mfma(B, F, C, rb, sf, sb):
    case = mc.step_case(B, F, C)
    out = _step(case, row_block=rb, splitf=sf, splitb=sb)
    assert out[0].shape == (C, F)
    figs = mc.check_step(out, case, (B, F, C, rb, sf, sb))
    _show(f"mlr_step_mfma {(B, F, C, rb, sf, sb)}", figs)


def test_mlr_step_mfma_reused_wt_buf_with_stale_columns():
    B, F = 192, 192
    wide, case = mc.step_case(B, F, 16), mc.step_case(B, F, 3)
    buf = torch.zeros(F, 16, device="cuda")
    mc.check_step(_step(wide, splitf=1, splitb=1, Wt_buf=buf), wide, "wide")
    assert float(buf[:, 3:].abs().min()) > 0        # stale, and not zero
    reused = _step(case, splitf=1, splitb=1, Wt_buf=buf)
    fresh = _step(case, splitf=1, splitb=1)
    mc.check_step(reused, case, "reused")
    # splits of 1: one atomic per cell onto zero, so the bits are defined
    assert torch.equal(reused[0].view(torch.int32), fresh[0].view(torch.int32))
    assert reused[2] == fresh[2]      # the loss is summed by atomics


def test_mlr_step_mfma_column_slice_of_x():
    from harmony_amd import ops

    case = mc.step_case(192, 192, 10)
    big = torch.randn(192, 320, device="cuda")
    big[:, 64:256] = case["X"].cuda()
    Xs = big[:, 64:256]
    assert not Xs.is_contiguous()
    grad, loss, correct = ops.mlr_step_mfma(Xs, case["W"].cuda(),
                                            case["y"].cuda(), row_block=64)
    mc.check_step((grad.cpu(), float(loss), int(correct)), case, "slice")


@pytest.mark.parametrize("side_stream", [False, True], ids=["default", "side"])
@pytest.mark.parametrize("rb", [64, 128])
def test_mlr_step_mfma_pipelined(rb, side_stream):
    from harmony_amd import ops

    case = mc.step_case(256, 192, 10)
    single = _step(case, row_block=rb)
    if side_stream:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            out = _step(case, ops.mlr_step_mfma_pipelined, row_block=rb)
        torch.cuda.current_stream().wait_stream(s)
    else:
        out = _step(case, ops.mlr_step_mfma_pipelined, row_block=rb)
    figs = mc.check_step(out, case, ("pipelined", rb, side_stream))
    # both lie within the bound of the float64 gradient: twice it apart
    assert bool(((out[0].double() - single[0].double()).abs()
                 <= 2 * case["bound"]).all())
    assert out[2] == single[2]
    _show(f"mlr_step_mfma_pipelined row_block {rb} "
          f"{'side' if side_stream else 'default'} stream", figs)


@pytest.mark.parametrize("rb", [256, 192, 96, 0])
def test_mlr_step_mfma_pipelined_single_stream_path(rb):
    # row_block = B, one that does not divide B, one that is no multiple of
    # 64, and none: all take mlr_step_mfma with row_block 0
    from harmony_amd import ops

    case = mc.step_case(256, 192, 10)
    out = _step(case, ops.mlr_step_mfma_pipelined, row_block=rb, splitf=1,
                splitb=1)
    mc.check_step(out, case, ("single", rb))
    same = _step(case, row_block=0, splitf=1, splitb=1)
    assert torch.equal(out[0].view(torch.int32), same[0].view(torch.int32))
