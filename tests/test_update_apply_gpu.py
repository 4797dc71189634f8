"""K3/K9 (ops/csrc/update.hip) on the GPU at every width, count, mode, dtype
and alignment of update_apply_cases, and Table on cuda against Table on cpu.
Bounds and references: the docstring of update_apply_cases."""

import pytest
import torch

from tests import update_apply_cases as uc

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32


def _scatter(shard, rows, deltas, mode, args, misalign=()):
    from harmony_amd import ops

    s = (uc.off_by_4_bytes(shard, "cuda") if "shard" in misalign
         else shard.cuda())
    d = (uc.off_by_4_bytes(deltas, "cuda") if "deltas" in misalign
         else deltas.cuda())
    ops.scatter_apply(s, rows.cuda(), d, mode, args.get("step_size", 0.0),
                      args.get("max_val", 0.0))
    assert uc.same_bits(d.cpu(), deltas)          # deltas are read only
    return s.cpu()


@pytest.mark.parametrize("dtype", [F32, I32], ids=["f32", "i32"])
@pytest.mark.parametrize("vd", uc.VDS)
def test_scatter_apply(vd, dtype):
    worst = 0.0
    for n in uc.NS:
        shard, rows, deltas = uc.scatter_case(vd, n, dtype)
        for mode in uc.MODES[dtype]:
            args = uc.args_of(mode)
            got = _scatter(shard, rows, deltas, mode, args)
            _e, ratio = uc.check_scatter(got, shard, rows, deltas, mode, args,
                                         (vd, n, mode))
            worst = max(worst, ratio)
    nmf = f"nmf_sgd error / bound {worst:.3f}, " if dtype is F32 else ""
    print(f"scatter_apply vd {vd} {dtype}: {nmf}other modes bit-equal")


@pytest.mark.parametrize("misalign", [("shard",), ("deltas",),
                                      ("shard", "deltas")],
                         ids=["shard", "deltas", "both"])
@pytest.mark.parametrize("vd", [4, 12, 256, 260])
def test_scatter_apply_base_off_by_4_bytes(vd, misalign):
    for dtype in (F32, I32):
        for mode in uc.MODES[dtype]:
            shard, rows, deltas = uc.scatter_case(vd, 40, dtype)
            args = uc.args_of(mode)
            got = _scatter(shard, rows, deltas, mode, args, misalign)
            uc.check_scatter(got, shard, rows, deltas, mode, args,
                             (vd, mode, misalign))


@pytest.mark.parametrize("vd", [1, 12, 260])
def test_scatter_apply_nan_and_inf(vd):
    shard, rows, deltas = uc.scatter_case(vd, 40, F32, True)
    for mode in ("nmf_sgd", "add"):
        args = uc.args_of(mode)
        got = _scatter(shard, rows, deltas, mode, args)
        uc.check_scatter(got, shard, rows, deltas, mode, args, (vd, mode))
        assert bool(torch.isnan(got[rows[0], 0])), mode


def test_scatter_apply_no_rows_is_a_no_op():
    for dtype in (F32, I32):
        shard, rows, deltas = uc.scatter_case(12, 0, dtype)
        for mode in uc.MODES[dtype]:
            got = _scatter(shard, rows, deltas, mode, uc.args_of(mode))
            assert uc.same_bits(got, shard), mode


@pytest.mark.parametrize("numel", uc.DENSE_NUMELS)
def test_dense_apply(numel):
    from harmony_amd import ops

    for dtype in (F32, I32):
        for mode in uc.MODES[dtype]:
            for specials in ((False, True) if dtype is F32 and numel > 1
                             and mode in ("nmf_sgd", "add") else (False,)):
                shard, delta = uc.dense_case(numel, dtype, specials)
                args = uc.args_of(mode)
                s, d = shard.cuda(), delta.cuda()
                ops.dense_apply(s, d, mode, args.get("step_size", 0.0),
                                args.get("max_val", 0.0))
                assert uc.same_bits(d.cpu(), delta)
                _e, ratio = uc.check_apply(s.cpu(), shard, delta, mode, args,
                                           (numel, mode, specials))
                if mode == "nmf_sgd":
                    print(f"dense_apply numel {numel}: nmf_sgd error / bound "
                          f"{ratio:.3f}")


@pytest.mark.parametrize("given", [True, False], ids=["args", "defaults"])
@pytest.mark.parametrize("update_fn,dtype", [
    ("add", F32), ("assign", F32), ("nmf_sgd", F32), ("lda_counts", I32)])
def test_table_on_cuda_matches_table_on_cpu(update_fn, dtype, given):
    from harmony_amd.et import update_functions as uf

    ua = uc.args_of(update_fn) if given else {}
    tg, start, keys, deltas, dense = uc.table_pair(update_fn, dtype, ua,
                                                   "cuda")
    tc = uc.table_pair(update_fn, dtype, ua, "cpu")[0]
    args = dict(zip(("step_size", "max_val"),
                    uf.fused_apply_args(update_fn, ua)))
    if update_fn == "nmf_sgd" and not given:
        # step 0.01 moves nothing past a clamp: scale so that both are met
        deltas, dense = deltas * 3e8, dense * 3e8
        start = start * 1e6
        for t in (tg, tc):
            t.put_local(torch.arange(start.shape[0], device=t.device),
                        start.to(t.device))
    tg.update_local(keys.cuda(), deltas.cuda())
    tc.update_local(keys, deltas)
    got = tg.shard.cpu()
    uc.check_scatter(got, start, keys, deltas, update_fn, args)
    _compare(got, tc.shard, start[keys], deltas, update_fn, args, keys)
    if update_fn == "nmf_sgd":
        assert float(got[keys].max()) == args["max_val"]
        assert float(got[keys].min()) == 0.0 and float(got.max()) > 0.0
    mid = got.clone()
    tc.shard.copy_(mid)
    tg.apply_update_dense_local(dense.cuda())
    tc.apply_update_dense_local(dense)
    got = tg.shard.cpu()
    uc.check_apply(got, mid, dense, update_fn, args)
    _compare(got, tc.shard, mid, dense, update_fn, args, slice(None))


def _compare(got, cpu, before, delta, update_fn, args, sel):
    if update_fn != "nmf_sgd":
        assert uc.same_bits(got, cpu)
        return
    # both lie within the bound of the float64 value: twice it apart
    step = float(torch.tensor(args["step_size"], dtype=torch.float32))
    tol = uc.EPS * (before.double().abs() + (step * delta.double()).abs())
    assert bool(((got[sel].double() - cpu[sel].double()).abs()
                 <= 2 * tol).all())


def test_table_nmf_nan_delta_stays_nan_on_both():
    for device in ("cuda", "cpu"):
        t, start, keys, deltas, dense = uc.table_pair("nmf_sgd", F32, {},
                                                      device)
        deltas = deltas.clone()
        deltas[0, 0] = float("nan")
        t.update_local(keys.to(device), deltas.to(device))
        got = t.shard.cpu()
        assert bool(torch.isnan(got[keys[0], 0])), device
        assert int(torch.isnan(got).sum()) == 1, device
        assert float(got[keys][1:].abs().max()) > 0.0, device  # not zeroed
