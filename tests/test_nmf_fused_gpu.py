"""GPU numerics of ops.nmf_step (pipelined two-pass NMF gradient with the L
update fused in) and of the row-per-group scatter_apply kernel.

Reference: a float64 torch computation written here. Yardstick: the legacy
path, ops.nmf_grad(..., col_sorted=...) plus the torch update chain. For
every output
    err(new, fp64) <= 2 * err(legacy, fp64) + 1e-6 * scale
with err = max |x - ref| and scale = max |ref|: both paths sum the same terms
in fp32 in a different order, a factor of 2 covers ordering luck, and a
dropped lane or nonzero is off by orders of magnitude more.
"""

import pytest
import torch

from harmony_amd import ops

pytestmark = pytest.mark.gpu

# nonzeros per row: ring prologue/epilogue (0..17 around the depth of 4), the
# 32/64-wide shuffle boundary, and the 4*G index-chunk boundary of both group
# widths (128 and 256), each at -1/+0/+1. 21 rows: not a multiple of the 8
# (or 4) groups per block, three blocks.
ROW_NNZ = [0, 1, 2, 3, 4, 5, 9, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129,
           255, 256, 257, 300]


class Problem:
    """A small CSR batch over a source table of m_src rows (CPU tensors).
    Columns 0..3 get segments of exactly 32, 33, 64 and 65 entries, the rest
    of the nonzeros fall on odd columns >= 5; columns 4 and m_src-2 are in
    the pulled set but have no nonzero, the other even columns are not
    pulled at all (so uniq is neither the identity nor the whole table)."""

    def __init__(self, k, row_nnz=ROW_NNZ, m_src=40, seed=0, val_scale=1.0,
                 l_extra=0, l_lo=0):
        g = torch.Generator().manual_seed(seed)
        self.k, self.n = k, len(row_nnz)
        counts = torch.tensor(row_nnz)
        nnz = int(counts.sum())
        self.row_ptr = torch.zeros(self.n + 1, dtype=torch.int64)
        self.row_ptr[1:] = counts.cumsum(0)
        fixed = [0] * 32 + [1] * 33 + [2] * 64 + [3] * 65
        fixed = fixed[:nnz]
        rest = 5 + 2 * torch.randint(0, (m_src - 5) // 2,
                                     (nnz - len(fixed),), generator=g)
        col = torch.cat([torch.tensor(fixed, dtype=torch.int64), rest])
        self.col = col[torch.randperm(nnz, generator=g)]
        self.vals = torch.rand(nnz, generator=g) * val_scale
        used = torch.unique(self.col)
        self.uniq = torch.unique(torch.cat(
            [used, torch.tensor([4, m_src - 2])]))      # empty segments
        self.col_local = torch.searchsorted(self.uniq, self.col)
        m = self.uniq.shape[0]
        perm = torch.argsort(self.col_local, stable=True)
        self.seg_ptr = torch.zeros(m + 1, dtype=torch.int64)
        self.seg_ptr[1:] = torch.bincount(self.col_local, minlength=m).cumsum(0)
        row_of = torch.repeat_interleave(torch.arange(self.n), counts)
        self.perm, self.row_sorted = perm, row_of[perm]
        self.l_lo = l_lo
        self.L_full = torch.rand(self.n + l_extra, k, generator=g)
        self.table = torch.rand(m_src, k, generator=g)

    def cuda(self):
        d = {}
        for name in ("row_ptr", "col", "vals", "uniq", "col_local", "perm",
                     "seg_ptr", "row_sorted", "L_full", "table"):
            d[name] = getattr(self, name).cuda()
        for name in ("row_ptr", "col", "uniq", "col_local", "perm",
                     "seg_ptr", "row_sorted"):
            d[name + "32"] = d[name].to(torch.int32)
        return d


def ref64(p, lam, step, max_val):
    """(L_new, rgrad, sq, lgrad) in float64 on CPU."""
    L = p.L_full[p.l_lo:p.l_lo + p.n].double()
    R = p.table[p.uniq].double()
    row_of = torch.repeat_interleave(torch.arange(p.n),
                                     p.row_ptr[1:] - p.row_ptr[:-1])
    Lr, Rr = L[row_of], R[p.col_local]
    e = (Lr * Rr).sum(1) - p.vals.double()
    ge = (2.0 * e).unsqueeze(1)
    lgrad = torch.zeros_like(L).index_add_(0, row_of, ge * Rr + 2 * lam * Lr)
    rgrad = torch.zeros_like(R).index_add_(0, p.col_local,
                                           ge * Lr + 2 * lam * Rr)
    L_new = (L - float(step) * lgrad).clamp_(0.0, max_val)
    return L_new, rgrad, (e * e).sum(), lgrad


def legacy(p, d, lam, step_t, max_val):
    L = d["L_full"][p.l_lo:p.l_lo + p.n].contiguous()
    R = d["table"][d["uniq"]]
    lg, rg, sq = ops.nmf_grad(L, R, d["row_ptr"], d["col_local"], d["vals"],
                              lam, col_sorted=(d["perm"], d["seg_ptr"],
                                               d["row_sorted"]))
    return (L - step_t * lg).clamp_(0.0, max_val), rg, sq, lg


def new(p, d, lam, step_t, max_val, indexed=True, L=None, l_lo=None):
    cs = (d["perm32"], d["seg_ptr32"], d["row_sorted32"])
    L = d["L_full"] if L is None else L
    l_lo = p.l_lo if l_lo is None else l_lo
    if indexed:
        return ops.nmf_step(L, l_lo, p.n, d["table"], d["row_ptr32"],
                            d["col32"], d["vals"], cs, d["uniq32"], step_t,
                            lam, max_val, want_lgrad=True)
    return ops.nmf_step(L, l_lo, p.n, d["table"][d["uniq"]], d["row_ptr32"],
                        d["col_local32"], d["vals"], cs, None, step_t, lam,
                        max_val, want_lgrad=True)


def check_2x(new_out, legacy_out, ref_out, what):
    for name, x, y, r in zip(("L_new", "rgrad", "sq_err", "lgrad"), new_out,
                             legacy_out, ref_out):
        x, y = x.double().cpu(), y.double().cpu()
        err_new = float((x - r).abs().max())
        err_old = float((y - r).abs().max())
        scale = float(r.abs().max())
        print(f"{what} {name}: err new {err_new:.3e} legacy {err_old:.3e} "
              f"scale {scale:.3e}")
        assert err_new <= 2 * err_old + 1e-6 * scale, (what, name)


@pytest.mark.parametrize("k", [100, 37, 4, 128, 256])
def test_nmf_step_vs_fp64(k):
    lam, max_val = 0.01, 1e6
    p = Problem(k, seed=k)
    d = p.cuda()
    step_t = torch.tensor(1e-3, device="cuda")
    out = new(p, d, lam, step_t, max_val)
    check_2x(out, legacy(p, d, lam, step_t, max_val),
             ref64(p, lam, step_t, max_val), f"k={k}")
    # with the lgrad of the same call the fused update is the torch chain
    L_new, _, _, lgrad = out
    assert torch.equal(
        L_new, (d["L_full"][:p.n] - step_t * lgrad).clamp_(0.0, max_val))


def test_nmf_step_lam_zero_and_short_rows():
    # only short rows: every row ends inside the ring's prologue/epilogue
    p = Problem(100, row_nnz=[0, 1, 2, 3, 4, 5, 9, 17, 0, 7, 16], seed=3)
    d = p.cuda()
    step_t = torch.tensor(1e-3, device="cuda")
    check_2x(new(p, d, 0.0, step_t, 1e6),
             legacy(p, d, 0.0, step_t, 1e6), ref64(p, 0.0, step_t, 1e6),
             f"short")


@pytest.mark.parametrize("k", [100, 37])
def test_nmf_step_indexed_equals_gathered(k):
    """Source table larger than the uniq set, uniq not the identity: the
    indexed form must match the gathered form bit for bit."""
    p = Problem(k, seed=11)
    assert p.uniq.shape[0] < p.table.shape[0]
    assert not torch.equal(p.uniq, torch.arange(p.uniq.shape[0]))
    d = p.cuda()
    step_t = torch.tensor(1e-3, device="cuda")
    a = new(p, d, 0.01, step_t, 1e6, indexed=True)
    b = new(p, d, 0.01, step_t, 1e6, indexed=False)
    for name, x, y in zip(("L_new", "rgrad", "sq", "lgrad"), a, b):
        if name == "sq":      # per-row atomics: order is not fixed
            assert abs(float(x) - float(y)) <= 1e-6 * abs(float(y))
        else:
            assert torch.equal(x, y), name


def test_nmf_step_L_slice_at_offset():
    p = Problem(100, seed=5, l_extra=7, l_lo=3)
    d = p.cuda()
    step_t = torch.tensor(1e-3, device="cuda")
    before = d["L_full"].clone()
    out = new(p, d, 0.01, step_t, 1e6)
    assert torch.equal(d["L_full"], before)          # the op never writes L
    check_2x(out, legacy(p, d, 0.01, step_t, 1e6),
             ref64(p, 0.01, step_t, 1e6), f"offset")
    alone = new(p, d, 0.01, step_t, 1e6,
                L=before[3:3 + p.n].contiguous(), l_lo=0)
    for x, y in zip((out[0], out[1], out[3]), (alone[0], alone[1], alone[3])):
        assert torch.equal(x, y)


def test_nmf_step_both_clamp_bounds():
    lam, max_val = 0.01, 0.9
    p = Problem(100, seed=7, val_scale=60.0)     # errors of both signs
    d = p.cuda()
    step_t = torch.tensor(0.05, device="cuda")
    r = ref64(p, lam, step_t, max_val)
    assert (r[0] == 0.0).any() and (r[0] == max_val).any()
    out = new(p, d, lam, step_t, max_val)
    check_2x(out, legacy(p, d, lam, step_t, max_val), r, f"clamp")
    assert torch.equal(
        out[0], (d["L_full"][:p.n] - step_t * out[3]).clamp_(0.0, max_val))


def test_nmf_step_unaligned_base_takes_scalar_path():
    """k % 4 == 0 but L and the table start 4 bytes off a 16-byte boundary:
    16-byte loads would fault or read wrong data, the scalar path must not."""
    p = Problem(100, seed=9)
    d = p.cuda()

    def shifted(t):
        buf = torch.empty(t.numel() + 1, device="cuda")
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    d2 = dict(d, L_full=shifted(d["L_full"]), table=shifted(d["table"]))
    step_t = torch.tensor(1e-3, device="cuda")
    check_2x(new(p, d2, 0.01, step_t, 1e6),
             legacy(p, d, 0.01, step_t, 1e6), ref64(p, 0.01, step_t, 1e6),
             f"unaligned")


def test_nmf_trainer_noncontiguous_l_rows():
    """Trainer compute with scattered L rows: gather, op, indexed write-back.
    Rows outside the batch stay as they were."""
    from harmony_amd.config import JobConfig, RuntimeConfig
    from harmony_amd.mlapps import nmf
    from harmony_amd.runtime.bootstrap import init_executor

    ctx = init_executor(RuntimeConfig(device="cuda"))
    job = JobConfig(job_id="fused_nc", app="nmf", num_mini_batches=1,
                    app_args={"num_cols": 64, "rank": 100, "nnz_per_row": 9,
                              "rows_per_batch": 48, "step_size": 1e-3})
    _, tr, provider = nmf.build(job, ctx, None)
    b0 = provider.blocks[0]
    assert b0.l_contiguous and b0.l_lo == 0
    l_rows = torch.arange(47, -1, -2, device="cuda")      # 24 rows, reversed
    nnz = int(b0.row_ptr[l_rows.shape[0]])
    b = nmf.NMFBatch(l_rows, b0.row_ptr[:l_rows.shape[0] + 1].contiguous(),
                     b0.col_idx[:nnz], b0.vals[:nnz])
    assert not b.l_contiguous
    L0 = tr.L.clone()
    tr.set_batch_data(b)
    tr.pull_model()
    R = tr.R_batch.clone()
    tr.local_compute()
    lg, rg, sq = ops.nmf_grad(L0[l_rows], R, b.row_ptr, b.col_local, b.vals,
                              tr.a["lam"], col_sorted=b.col_sorted)
    want = L0.clone()
    want[l_rows] = (L0[l_rows] - tr._step_t * lg).clamp_(0.0, tr.a["max_val"])
    untouched = torch.ones(L0.shape[0], dtype=torch.bool, device="cuda")
    untouched[l_rows] = False
    assert torch.equal(tr.L[untouched], L0[untouched])
    # a rank-100 dot of values in [0, 1) is ~25 and its fp32 summation error
    # at most ~100 * 2^-24 * 25 = 1.5e-4; lgrad sums 9 terms 2*e*R (error
    # <= 2.7e-3, times step 1e-3), an rgrad segment here ~7 terms 2*e*L
    assert torch.allclose(tr.L, want, rtol=0, atol=1e-5)
    assert torch.allclose(tr.rgrad, rg, rtol=0, atol=2e-3)


def test_nmf_ten_sgd_steps_three_ways():
    """fp64, the legacy composition (nmf_grad + torch chain + scatter_apply)
    and nmf_step on the whole table by global column id."""
    n, nnz_row, m, k = 256, 9, 300, 100
    step, max_val, lam = 1e-4, 1e6, 0.01
    p = Problem(k, row_nnz=[nnz_row] * n, m_src=m, seed=21)
    d = p.cuda()
    step_t = torch.tensor(step, device="cuda")
    cs = (d["perm"], d["seg_ptr"], d["row_sorted"])
    cs32 = (d["perm32"], d["seg_ptr32"], d["row_sorted32"])

    L64, T64 = p.L_full.double(), p.table.double()
    row_of = torch.repeat_interleave(torch.arange(n),
                                     p.row_ptr[1:] - p.row_ptr[:-1])
    L_old, T_old = d["L_full"].clone(), d["table"].clone()
    L_new, T_new = d["L_full"].clone(), d["table"].clone()
    for _ in range(10):
        Lr, Rr = L64[row_of], T64[p.col]
        ge = (2.0 * ((Lr * Rr).sum(1) - p.vals.double())).unsqueeze(1)
        lg = torch.zeros_like(L64).index_add_(0, row_of,
                                              ge * Rr + 2 * lam * Lr)
        rg = torch.zeros_like(T64).index_add_(0, p.col,
                                              ge * Lr + 2 * lam * Rr)
        L64 = (L64 - step * lg).clamp_(0.0, max_val)
        T64[p.uniq] = (T64[p.uniq] - step * rg[p.uniq]).clamp_(0.0, max_val)

        lg, rg, _ = ops.nmf_grad(L_old, T_old[d["uniq"]], d["row_ptr"],
                                 d["col_local"], d["vals"], lam,
                                 col_sorted=cs)
        L_old = (L_old - step_t * lg).clamp_(0.0, max_val)
        ops.scatter_apply(T_old, d["uniq"], rg, "nmf_sgd", step, max_val)

        Ln, rg, _ = ops.nmf_step(L_new, 0, n, T_new, d["row_ptr32"],
                                 d["col32"], d["vals"], cs32, d["uniq32"],
                                 step_t, lam, max_val)
        L_new.copy_(Ln)
        ops.scatter_apply(T_new, d["uniq"], rg, "nmf_sgd", step, max_val)
    for name, x, y, r in (("L", L_new, L_old, L64),
                          ("table", T_new, T_old, T64)):
        err_new = float((x.double().cpu() - r).abs().max())
        err_old = float((y.double().cpu() - r).abs().max())
        scale = float(r.abs().max())
        print(f"sgd10 {name}: err new {err_new:.3e} legacy {err_old:.3e}")
        assert err_new <= 2 * err_old + 1e-6 * scale, name


@pytest.mark.parametrize("n", [1, 1000])
@pytest.mark.parametrize("vd", [100, 37, 1])
@pytest.mark.parametrize("fn_name,args,dtype", [
    ("add", {}, torch.float32),
    ("assign", {}, torch.float32),
    # step 0.5: the product with a power of two is exact, so the kernel's
    # fused multiply-subtract and torch's two roundings agree bit for bit
    ("nmf_sgd", {"step_size": 0.5, "max_val": 10.0}, torch.float32),
    ("lda_counts", {}, torch.int32),
    ("add", {}, torch.int32),
])
def test_scatter_apply_bitwise(fn_name, args, dtype, vd, n):
    from harmony_amd.et import update_functions as uf

    torch.manual_seed(5)
    N = 2 * n + 3
    if dtype is torch.float32:
        shard = torch.rand(N, vd, device="cuda")
        deltas = torch.randn(n, vd, device="cuda")
    else:
        shard = torch.randint(0, 5, (N, vd), device="cuda", dtype=dtype)
        deltas = torch.randint(-5, 5, (n, vd), device="cuda", dtype=dtype)
    rows = torch.randperm(N, device="cuda")[:n]            # unsorted
    ref = shard.cpu().clone()
    ref[rows.cpu()] = uf.update_fn(fn_name)(ref[rows.cpu()], deltas.cpu(),
                                            **args)
    ops.scatter_apply(shard, rows, deltas, fn_name,
                      args.get("step_size", 0.0), args.get("max_val", 0.0))
    assert torch.equal(shard.cpu(), ref), fn_name
