"""Inputs, references and checkers for K3/K9 (ops/csrc/update.hip:
scatter_apply, dense_apply) and the Table calls that reach them.

Tolerances. add, assign and lda_counts are one float32 or int32 operation per
element, so the kernel must give the bits of the torch update function
(same_bits; a NaN is matched by any NaN, as its payload is not defined by
either side). nmf_sgd is v - step * d, which the compiler may contract to an
fma: against float64 it may be off by 2^-23 * (|v| + |step * d|), the two
roundings of the uncontracted form, and where the float64 value lies past a
clamp by more than that the result is the clamp value exactly (check_nmf).
"""

import functools

import torch

from harmony_amd.et import update_functions as uf

N = 300
VDS = [1, 3, 4, 12, 255, 256, 260, 1028]
NS = [1, 40, 257]
DENSE_NUMELS = [1, 255, 256, 257, 1600]
MODES = {torch.float32: ["add", "assign", "nmf_sgd", "lda_counts"],
         torch.int32: ["add", "assign", "lda_counts"]}
NMF_ARGS = {"step_size": 0.5, "max_val": 1.5}
EPS = 2.0 ** -23


def args_of(mode):
    return dict(NMF_ARGS) if mode == "nmf_sgd" else {}


def rows_of(n, g):
    """n unique rows of range(N) in shuffled order; N-1 always, 0 from n=2."""
    if n == 0:
        return torch.empty(0, dtype=torch.int64)
    ends = [N - 1] if n == 1 else [0, N - 1]
    mid = (torch.randperm(N - 2, generator=g) + 1)[:n - len(ends)]
    rows = torch.cat([torch.tensor(ends, dtype=torch.int64), mid])
    return rows[torch.randperm(n, generator=g)]


def values(shape, dtype, g, delta):
    """Shard values in [0, 2) or 0..4; deltas N(0, 1) or -5..4, so that
    lda_counts goes below zero and nmf_sgd passes both clamps of NMF_ARGS."""
    if dtype is torch.float32:
        return (torch.randn(shape, generator=g) if delta
                else torch.rand(shape, generator=g) * 2)
    lo, hi = (-5, 5) if delta else (0, 5)
    return torch.randint(lo, hi, shape, generator=g, dtype=dtype)


@functools.lru_cache(maxsize=None)
def scatter_case(vd, n, dtype, specials=False):
    """(shard [N, vd], rows [n], deltas [n, vd]) on the CPU; treat as
    read-only. specials: a NaN in the first delta and +inf in the last."""
    g = torch.Generator().manual_seed(1000 * vd + n)
    shard = values((N, vd), dtype, g, False)
    rows = rows_of(n, g)
    deltas = values((n, vd), dtype, g, True)
    if specials:
        deltas[0, 0] = float("nan")
        deltas[-1, -1] = float("inf")
    return shard, rows, deltas


@functools.lru_cache(maxsize=None)
def dense_case(numel, dtype, specials=False):
    g = torch.Generator().manual_seed(numel)
    shard = values((numel,), dtype, g, False)
    delta = values((numel,), dtype, g, True)
    if specials:
        delta[0] = float("nan")
        delta[-1] = float("inf")
    return shard, delta


def off_by_4_bytes(t, device):
    """A contiguous copy of t on device whose base is 4 bytes past a
    16-byte boundary."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    out = flat[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def torch_apply(values_, delta, mode, args):
    """The torch update function on clones: the new values."""
    return uf.update_fn(mode)(values_.clone(), delta.clone(), **args)


def same_bits(a, b):
    """Equal bit for bit, except that any NaN matches any NaN."""
    if not a.is_floating_point():
        return bool(torch.equal(a, b))
    nan = torch.isnan(a)
    if not torch.equal(nan, torch.isnan(b)):
        return False
    return bool(torch.equal(a.view(torch.int32)[~nan],
                            b.view(torch.int32)[~nan]))


def check_nmf(got, v, d, step_size, max_val, label=""):
    """got = clamp(v - step * d, 0, max) within the bound of the module
    docstring; returns (largest error, largest error / bound) over the
    elements where the bound is finite and the clamp is not active."""
    step = float(torch.tensor(step_size, dtype=torch.float32))
    top = float(torch.tensor(max_val, dtype=torch.float32))
    sd = step * d.double()
    x = v.double() - sd
    tol = EPS * (v.double().abs() + sd.abs())
    nan = torch.isnan(x)
    assert torch.equal(torch.isnan(got), nan), (label, "NaN kept as NaN")
    ref = x.clamp(0.0, top)
    ok = ~nan
    # 1-Lipschitz clamp: the bound holds on both sides of a clamp too
    err = (got.double() - ref).abs()
    inside = ok & torch.isfinite(tol)
    assert bool((err[inside] <= tol[inside]).all()), (
        label, float((err[inside] - tol[inside]).max()))
    active = ok & ((x <= -tol) | (x >= top + tol) | ~torch.isfinite(tol))
    assert torch.equal(got.double()[active], ref[active]), (label, "clamp")
    free = inside & ~active & (tol > 0)
    if not bool(free.any()):
        return 0.0, 0.0
    return float(err[free].max()), float((err[free] / tol[free]).max())


def check_apply(got, before, delta, mode, args, label=""):
    """got against the reference for one (values, delta) pair of any shape."""
    if mode == "nmf_sgd":
        return check_nmf(got, before, delta, args["step_size"],
                         args["max_val"], label)
    assert same_bits(got, torch_apply(before, delta, mode, args)), label
    return 0.0, 0.0


def check_scatter(got, shard, rows, deltas, mode, args, label=""):
    """Named rows against the reference, every other row bit for bit."""
    keep = torch.ones(shard.shape[0], dtype=torch.bool)
    keep[rows] = False
    assert same_bits(got[keep], shard[keep]), (label, "rows not named")
    return check_apply(got[rows], shard[rows], deltas, mode, args, label)


def table_pair(update_fn, dtype, update_args, device, value_dim=12,
               num_keys=96):
    """One-rank Table on `device` with known values, and its keys/deltas."""
    from harmony_amd.config import TableConfig
    from harmony_amd.et.table import Table

    cfg = TableConfig(table_id="edge", num_keys=num_keys, value_dim=value_dim,
                      num_blocks=8, update_fn=update_fn,
                      dtype="float32" if dtype is torch.float32 else "int32",
                      update_args=dict(update_args))
    t = Table(cfg, rank=0, world_size=1, device=torch.device(device))
    g = torch.Generator().manual_seed(7)
    start = values((num_keys, value_dim), dtype, g, False)
    keys = torch.randperm(num_keys, generator=g)[:41]
    deltas = values((41, value_dim), dtype, g, True)
    dense = values((num_keys, value_dim), dtype, g, True)
    t.put_local(torch.arange(num_keys, device=device), start.to(device))
    return t, start, keys, deltas, dense
