"""The batched alias-table build on the GPU: a wave takes a batch of rows,
lane r runs the top-level Vose of row r. Every case compares every output
array bitwise with the torch reference on the same input: row counts around
the batch size, the grid-stride loop (workgroup cap), every K, and row
contents that send neighbouring lanes down different Vose paths."""

import functools

import pytest
import torch

from harmony_amd import ops

pytestmark = pytest.mark.gpu

BETA, V = 0.01, 1000
ROW_COUNTS = (1, 15, 16, 17, 63, 64, 65, 1027)
N_KINDS = 6


def _row_counts():
    """1, B-1, B, B+1 and many batches with a short last one, B being the
    batch size the kernel was built with; the fixed list covers B = 16, 64."""
    B = ops.lda_alias_build_batch()
    return sorted(set(ROW_COUNTS) | {max(B - 1, 1), B, B + 1})


def _rows_of_kind(kind, n, K, g):
    """n count rows of one kind; each kind sends the top-level Vose down
    another path."""
    S = K // 64
    wt = torch.zeros(n, K, dtype=torch.int32)
    if kind == 0:                       # all zero: only beta
        pass
    elif kind == 1:                     # half the segments zero
        wt = torch.randint(0, 6, (n, K), generator=g, dtype=torch.int32)
        seg = torch.rand(n, 64, generator=g).argsort(1) < 32
        wt = wt * seg.repeat_interleave(S, 1).to(torch.int32)
    elif kind == 2:                     # one large segment, 63 small
        at = torch.randint(0, K, (n,), generator=g)
        wt[torch.arange(n), at] = 10 ** 6
    elif kind == 3:                     # two large segments, 62 small
        seg = torch.rand(n, 64, generator=g).argsort(1)[:, :2]
        off = torch.randint(0, S, (n, 2), generator=g)
        for j in range(2):
            wt[torch.arange(n), seg[:, j] * S + off[:, j]] = 10 ** 6 - j * 17
    elif kind == 4:                     # all equal: top entries at 1.0
        wt += torch.randint(0, 9, (n, 1), generator=g, dtype=torch.int32)
    else:                               # small random counts
        wt = torch.randint(0, 6, (n, K), generator=g, dtype=torch.int32)
    return wt


def _mixed(rows, K, seed):
    """Rows of all kinds, shuffled, so that the lanes of one batch diverge."""
    g = torch.Generator().manual_seed(seed)
    kinds = torch.arange(rows) % N_KINDS
    kinds = kinds[torch.randperm(rows, generator=g)]
    wt = torch.zeros(rows, K, dtype=torch.int32)
    for kind in range(N_KINDS):
        idx = (kinds == kind).nonzero(as_tuple=True)[0]
        if idx.numel():
            wt[idx] = _rows_of_kind(kind, idx.numel(), K, g)
    return wt


def _nk(K, seed):
    # nearly equal topic sums: invden differs from topic to topic in its
    # last bits only, so the all-equal rows get top entries a few ulps on
    # either side of 1.0
    g = torch.Generator().manual_seed(seed)
    return torch.randint(3000, 3003, (K,), generator=g, dtype=torch.int32)


N_ROWS, N_UNIQUE = 1027, 137


@functools.lru_cache(maxsize=None)
def _case(K):
    """1027 input rows and their CPU reference, computed once per K and
    shared (never modified). A row's tables depend on that row and on the
    topic sums alone, so the reference's serial Python Vose runs over 137
    distinct rows and is expanded to the 1027 drawn from them; 137 is no
    multiple of a batch, so no two batches hold the same rows."""
    g = torch.Generator().manual_seed(K)
    uniq, nk = _mixed(N_UNIQUE, K, 100 + K), _nk(K, K)
    pick = torch.cat([torch.randperm(N_UNIQUE, generator=g),
                      torch.randint(0, N_UNIQUE, (N_ROWS - N_UNIQUE,),
                                    generator=g)])
    ref = ops.lda_alias_build(uniq, nk, BETA, V)
    ref = tuple(r[pick].contiguous() for r in ref[:6]) + (ref[6],)
    return uniq[pick].contiguous(), nk, ref


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def _assert_legacy(got, ref, n):
    names = ("prob", "alias", "top_prob", "top_alias", "qv", "qsum", "invden")
    for name, g_, r_ in zip(names, got, ref):
        want = r_ if name == "invden" else r_[:n]
        assert torch.equal(_bits(g_), _bits(want)), name


def _packed_ref(ref, n, K):
    rec, top = ops.lda_packed_alloc(n, K, "cpu")
    S = K // 64
    r = rec.view(n, 64, 4, S)
    r[:, :, 1] = ref[0][:n].view(torch.int32).view(n, 64, S)
    r[:, :, 2] = ref[4][:n].view(torch.int32).view(n, 64, S)
    r[:, :, 3] = ref[1][:n].view(n, 64, S)
    top[:, :, 0] = ref[2][:n].view(torch.int32)
    top[:, :, 1] = ref[3][:n]
    return rec, top


def _build_packed(src, src_rows, nk, n, K, cap=None, out=None):
    rec, top = out if out is not None else ops.lda_packed_alloc(n, K, "cuda")
    invden, qsum = ops.lda_alias_build_packed(
        src.cuda(), None if src_rows is None else src_rows.cuda(), nk.cuda(),
        BETA, V, rec, top, max_workgroups=cap)
    return rec, top, invden, qsum


def _assert_packed(got, ref, n, K):
    rec, top, invden, qsum = got
    rec_c, top_c = _packed_ref(ref, n, K)
    assert torch.equal(rec.cpu(), rec_c)
    assert torch.equal(top.cpu(), top_c)
    assert torch.equal(_bits(invden), _bits(ref[6]))
    assert torch.equal(_bits(qsum), _bits(ref[5][:n]))


def test_reference_rows_take_every_vose_path():
    """The inputs are what the docstring says: the CPU tables of each kind
    show the intended shape of the top table."""
    K = 256
    g = torch.Generator().manual_seed(5)
    nk = torch.full((K,), 1000, dtype=torch.int32)
    for kind, check in (
            (2, lambda tp, ta: int((ta == ta[0]).sum()) == 64),
            (4, lambda tp, ta: bool((tp == 1.0).all())),
            (0, lambda tp, ta: bool((tp == 1.0).all()))):
        wt = _rows_of_kind(kind, 1, K, g)
        ref = ops.lda_alias_build(wt, nk, BETA, V)
        assert check(ref[2][0], ref[3][0]), kind


@pytest.mark.parametrize("K", [64, 128, 256, 512])
def test_packed_build_row_counts(K):
    wt, nk, ref = _case(K)
    for n in _row_counts():
        _assert_packed(_build_packed(wt, None, nk, n, K), ref, n, K)


@pytest.mark.parametrize("K", [64, 128, 192, 256, 512])
def test_legacy_build_row_counts(K):
    wt, nk, ref = _case(K)
    for n in _row_counts():
        got = ops.lda_alias_build(wt[:n].cuda(), nk.cuda(), BETA, V)
        _assert_legacy(got, ref, n)


@pytest.mark.parametrize("cap", [3, 1])
@pytest.mark.parametrize("through_rows", [True, False])
@pytest.mark.parametrize("K", [64, 128, 256, 512])
def test_packed_build_grid_stride(K, through_rows, cap):
    n = 1027
    wt, nk, ref = _case(K)
    if through_rows:
        # the rows sit at permuted places of a larger source, as the
        # trainer's shard does
        g = torch.Generator().manual_seed(K)
        place = torch.randperm(n + 300, generator=g)[:n]
        src = torch.randint(0, 9, (n + 300, K), generator=g,
                            dtype=torch.int32)
        src[place] = wt
        got = _build_packed(src, place.to(torch.int32), nk, n, K, cap)
    else:
        got = _build_packed(wt, None, nk, n, K, cap)
    _assert_packed(got, ref, n, K)


@pytest.mark.parametrize("cap", [3, 1])
@pytest.mark.parametrize("K", [64, 192, 256, 512])
def test_legacy_build_grid_stride(K, cap):
    wt, nk, ref = _case(K)
    got = ops.lda_alias_build(wt.cuda(), nk.cuda(), BETA, V,
                              max_workgroups=cap)
    _assert_legacy(got, ref, 1027)


@pytest.mark.parametrize("K", [64, 256])
def test_build_is_repeatable(K):
    wt, nk, _ = _case(K)
    a = _build_packed(wt, None, nk, 1027, K)
    b = _build_packed(wt, None, nk, 1027, K)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))
    la = ops.lda_alias_build(wt.cuda(), nk.cuda(), BETA, V)
    lb = ops.lda_alias_build(wt.cuda(), nk.cuda(), BETA, V)
    for x, y in zip(la, lb):
        assert torch.equal(_bits(x), _bits(y))


@pytest.mark.parametrize("K", [64, 256])
def test_no_state_left_in_lds_between_batches(K):
    """One workgroup builds a batch of heavy-skew rows and then, into the
    same outputs and through the same per-wave LDS arrays, uniform rows."""
    n = 4 * max(ops.lda_alias_build_batch(), 16) + 3
    g = torch.Generator().manual_seed(9)
    nk = _nk(K, 3)
    skew = torch.cat([_rows_of_kind(2, n // 2, K, g),
                      _rows_of_kind(3, n - n // 2, K, g)])
    flat = _rows_of_kind(4, n, K, g)
    out = ops.lda_packed_alloc(n, K, "cuda")
    ref_skew = ops.lda_alias_build(skew, nk, BETA, V)
    _assert_packed(_build_packed(skew, None, nk, n, K, 1, out), ref_skew, n, K)
    ref_flat = ops.lda_alias_build(flat, nk, BETA, V)
    _assert_packed(_build_packed(flat, None, nk, n, K, 1, out), ref_flat, n, K)
    # and within one launch, through the legacy arrays too
    both = torch.cat([skew, flat])
    ref_both = tuple(torch.cat([a, b]) for a, b in
                     zip(ref_skew[:6], ref_flat[:6])) + (ref_flat[6],)
    _assert_packed(_build_packed(both, None, nk, 2 * n, K, 1), ref_both,
                   2 * n, K)
    got = ops.lda_alias_build(both.cuda(), nk.cuda(), BETA, V,
                              max_workgroups=1)
    _assert_legacy(got, ref_both, 2 * n)
