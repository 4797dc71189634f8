"""update_apply_cases on the CPU: the torch update functions pass the
checkers on every case, the checkers reject small corruptions, the cases hit
the edges they are built for, and the one source of kernel defaults
(update_functions.fused_apply_args) agrees with the torch functions."""

import inspect

import pytest
import torch

from harmony_amd.et import update_functions as uf
from tests import update_apply_cases as uc

F32, I32 = torch.float32, torch.int32


@pytest.mark.parametrize("dtype", [F32, I32])
@pytest.mark.parametrize("vd", uc.VDS)
def test_torch_functions_pass_on_scatter_cases(vd, dtype):
    for n in uc.NS:
        shard, rows, deltas = uc.scatter_case(vd, n, dtype)
        assert rows.unique().numel() == n and int(rows.max()) == uc.N - 1
        assert n == 1 or int(rows.min()) == 0
        for mode in uc.MODES[dtype]:
            args = uc.args_of(mode)
            got = shard.clone()
            got[rows] = uc.torch_apply(shard[rows], deltas, mode, args)
            uc.check_scatter(got, shard, rows, deltas, mode, args,
                             (vd, n, mode))


@pytest.mark.parametrize("numel", uc.DENSE_NUMELS)
def test_torch_functions_pass_on_dense_cases(numel):
    for dtype in (F32, I32):
        for mode in uc.MODES[dtype]:
            shard, delta = uc.dense_case(numel, dtype)
            args = uc.args_of(mode)
            uc.check_apply(uc.torch_apply(shard, delta, mode, args), shard,
                           delta, mode, args, (numel, mode))


def test_cases_reach_their_edges():
    shard, rows, deltas = uc.scatter_case(12, 40, F32)
    x = shard[rows].double() - 0.5 * deltas.double()
    assert bool((x < -1e-3).any()) and bool((x > 1.5 + 1e-3).any())
    shard, rows, deltas = uc.scatter_case(12, 40, I32)
    assert bool((shard[rows] + deltas < 0).any())
    shard, rows, deltas = uc.scatter_case(12, 40, F32, True)
    got = uc.torch_apply(shard[rows], deltas, "nmf_sgd", uc.NMF_ARGS)
    assert bool(torch.isnan(got[0, 0])) and float(got[-1, -1]) == 0.0
    uc.check_nmf(got, shard[rows], deltas, 0.5, 1.5)
    assert uc.off_by_4_bytes(shard, "cpu").data_ptr() % 16 == 4


def test_checkers_reject_small_corruptions():
    shard, rows, deltas = uc.scatter_case(12, 40, F32, True)
    good = uc.torch_apply(shard[rows], deltas, "nmf_sgd", uc.NMF_ARGS)
    x = shard[rows].double() - 0.5 * deltas.double()
    free = ((x > 0.1) & (x < 1.4)).nonzero()[0]
    low = (x < -0.1).nonzero()[0]

    def bad(edit):
        t = good.clone()
        edit(t)
        with pytest.raises(AssertionError):
            uc.check_nmf(t, shard[rows], deltas, 0.5, 1.5)

    def off_by_ulps(t):      # four ulps of the larger operand
        t[free[0], free[1]] += 4 * uc.EPS * 2.0

    def leaky_clamp(t):
        t[low[0], low[1]] = 1e-30

    def nan_to_zero(t):      # what fminf(fmaxf(x, 0), max) gives
        t[0, 0] = 0.0

    for edit in (off_by_ulps, leaky_clamp, nan_to_zero):
        bad(edit)
    # bit comparison: one ulp, and a touched row that was not named
    full = shard.clone()
    full[rows] = uc.torch_apply(shard[rows], deltas, "add", {})
    uc.check_scatter(full, shard, rows, deltas, "add", {})
    t = full.clone()
    r = int(rows[3])
    t[r, 5] = torch.nextafter(t[r, 5], torch.tensor(9.0))
    with pytest.raises(AssertionError):
        uc.check_scatter(t, shard, rows, deltas, "add", {})
    t = full.clone()
    other = next(i for i in range(uc.N) if i not in set(rows.tolist()))
    t[other, 11] += 1.0
    with pytest.raises(AssertionError):
        uc.check_scatter(t, shard, rows, deltas, "add", {})


def test_fused_apply_args_fall_back_to_the_torch_defaults():
    sig = inspect.signature(uf.update_fn("nmf_sgd")).parameters
    assert uf.fused_apply_args("nmf_sgd", {}) == (
        sig["step_size"].default, sig["max_val"].default) == (0.01, 1e6)
    assert uf.fused_apply_args("nmf_sgd", None) == (0.01, 1e6)
    assert uf.fused_apply_args("nmf_sgd", {"step_size": 1.0}) == (1.0, 1e6)
    assert uf.fused_apply_args("nmf_sgd", {"max_val": 2}) == (0.01, 2.0)
    assert uf.fused_apply_args(
        "nmf_sgd", {"step_size": 0.5, "max_val": 1.5, "other": 3}) == (0.5, 1.5)
    for name in ("add", "assign", "lda_counts", "min"):
        assert uf.fused_apply_args(name, {}) == (0.0, 0.0)
    # the values it returns reproduce the torch function called without them
    v, d = torch.rand(5, 3) * 2e6, torch.randn(5, 3) * 1e8
    step, top = uf.fused_apply_args("nmf_sgd", {})
    uc.check_nmf(uc.torch_apply(v, d, "nmf_sgd", {}), v, d, step, top)


@pytest.mark.parametrize("update_fn,dtype", [
    ("add", F32), ("assign", F32), ("nmf_sgd", F32), ("lda_counts", I32)])
def test_cpu_table_matches_the_reference(update_fn, dtype):
    for ua in ({}, uc.args_of(update_fn)):
        t, start, keys, deltas, dense = uc.table_pair(update_fn, dtype, ua,
                                                      "cpu")
        args = dict(zip(("step_size", "max_val"),
                        uf.fused_apply_args(update_fn, ua)))
        t.update_local(keys, deltas)
        uc.check_scatter(t.shard, start, keys, deltas, update_fn, args)
        mid = t.shard.clone()
        t.apply_update_dense_local(dense)
        uc.check_apply(t.shard, mid, dense, update_fn, args)
