"""Packed LDA tables (K7d) on the GPU: bit-exact build, exact samples
against the legacy wave kernel where no intra-doc race exists, and integer
invariants (fused shard update included) where one does."""

import pytest
import torch

from harmony_amd import ops

pytestmark = pytest.mark.gpu

ALPHA, BETA, V = 0.1, 0.01, 1000


def _counts(rows, K, seed):
    g = torch.Generator().manual_seed(seed)
    wt = torch.randint(0, 6, (rows, K), generator=g, dtype=torch.int32)
    wt[0] = 0
    wt[1, : K // 2] = 0
    nk = wt.sum(0).to(torch.int32) + 3
    return wt, nk


@pytest.mark.parametrize("K", [64, 128, 256, 512])
@pytest.mark.parametrize("through_rows", [False, True])
def test_gpu_packed_build_equals_cpu_packed_build(K, through_rows):
    rows = 37
    wt, nk = _counts(rows + 5, K, K)
    g = torch.Generator().manual_seed(1)
    src_rows = (torch.randperm(rows + 5, generator=g)[:rows].to(torch.int32)
                if through_rows else None)
    rec_c, top_c = ops.lda_packed_alloc(rows, K, "cpu")
    inv_c, qs_c = ops.lda_alias_build_packed(wt, src_rows, nk, BETA, V,
                                             rec_c, top_c)
    rec_g, top_g = ops.lda_packed_alloc(rows, K, "cuda")
    rows_g = src_rows.cuda() if through_rows else None
    inv_g, qs_g = ops.lda_alias_build_packed(wt.cuda(), rows_g, nk.cuda(),
                                             BETA, V, rec_g, top_g)
    assert torch.equal(rec_g.cpu(), rec_c)
    assert torch.equal(top_g.cpu(), top_c)
    assert torch.equal(inv_g.cpu().view(torch.int32), inv_c.view(torch.int32))
    assert torch.equal(qs_g.cpu().view(torch.int32), qs_c.view(torch.int32))


@pytest.mark.parametrize("K", [64, 128, 256, 512])
def test_gpu_packed_build_equals_legacy_gpu_build(K):
    rows = 37
    wt, nk = _counts(rows, K, K + 1)
    wt, nk = wt.cuda(), nk.cuda()
    ref = ops.lda_alias_build(wt, nk, BETA, V)
    rec, top = ops.lda_packed_alloc(rows, K, "cuda")
    invden, qsum = ops.lda_alias_build_packed(wt, None, nk, BETA, V, rec, top)
    prob, alias, tprob, talias, qv = ops.lda_unpack_tables(rec, top)
    for got, want in ((prob, ref[0]), (alias, ref[1]), (tprob, ref[2]),
                      (talias, ref[3]), (qv, ref[4]), (qsum, ref[5]),
                      (invden, ref[6])):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def _problem(lengths, n_words, K, seed, zipf):
    """Docs of the given lengths over local words [0, n_words); counts
    consistent with a random assignment, plus background mass."""
    g = torch.Generator().manual_seed(seed)
    lengths = torch.as_tensor(lengths, dtype=torch.int64)
    D, T = lengths.shape[0], int(lengths.sum())
    offs = torch.zeros(D + 1, dtype=torch.int64)
    offs[1:] = lengths.cumsum(0)
    u = torch.rand(T, generator=g)
    w = ((u * u if zipf else u) * n_words).long().clamp_(0, n_words - 1)
    w[-1] = n_words - 1                         # the last local row is used
    tok_doc = torch.repeat_interleave(torch.arange(D), lengths)
    # sort by word within each doc, as the trainer's batches are
    order = torch.argsort(tok_doc * n_words + w, stable=True)
    w = w[order]
    z = torch.randint(0, K, (T,), generator=g, dtype=torch.int32)
    wt = torch.randint(0, 4, (n_words, K), generator=g, dtype=torch.int32)
    wt.view(-1).scatter_add_(0, w * K + z.long(),
                             torch.ones(T, dtype=torch.int32))
    nk = wt.sum(0).to(torch.int32)
    dt = torch.zeros(D, K, dtype=torch.int32)
    dt.view(-1).scatter_add_(0, tok_doc * K + z.long(),
                             torch.ones(T, dtype=torch.int32))
    return dict(offs=offs, w=w, z=z, wt=wt, nk=nk, dt=dt, tok_doc=tok_doc)


def _shard_for(pr, n_words, K, seed):
    """A table shard holding the words' rows at permuted positions, a
    summary row, and rows the batch never touches."""
    g = torch.Generator().manual_seed(seed)
    n_rows = n_words + 40
    perm = torch.randperm(n_rows, generator=g)
    row_of_local = perm[:n_words].to(torch.int32)
    summary_row = int(perm[n_words])
    shard = torch.randint(0, 9, (n_rows, K), generator=g, dtype=torch.int32)
    shard[row_of_local.long()] = pr["wt"]
    shard[summary_row] = pr["nk"]
    return shard, row_of_local, summary_row


@pytest.mark.parametrize("K", [64, 256])
def test_packed_sampler_equals_legacy_wave_without_intra_doc_race(K):
    n_docs, n_words = 1027, 300
    g = torch.Generator().manual_seed(11)
    lengths = torch.randint(0, 2, (n_docs,), generator=g)
    lengths[-1] = 1
    pr = _problem(lengths, n_words, K, 12, zipf=False)
    wt, nk = pr["wt"].cuda(), pr["nk"].cuda()
    offs, w = pr["offs"].cuda(), pr["w"].cuda()
    seed = 1234
    # legacy arrays and kernel
    prob, alias, tprob, talias, qv, _, invden = ops.lda_alias_build(
        wt, nk, BETA, V)
    z_ref, dt_ref = pr["z"].cuda(), pr["dt"].cuda()
    ops.lda_mh_wave(dt_ref, wt, invden, prob, alias, tprob, talias, qv,
                    offs, w, z_ref, ALPHA, BETA, seed)
    assert not torch.equal(z_ref.cpu(), pr["z"])     # the sweep moved tokens
    # packed, plain and fused
    shard, rol, srow = _shard_for(pr, n_words, K, 13)
    shard = shard.cuda()
    rec, top = ops.lda_packed_alloc(n_words, K, "cuda")
    inv_p, _ = ops.lda_alias_build_packed(shard, rol.cuda(), nk, BETA, V,
                                          rec, top)
    assert torch.equal(inv_p, invden)
    w32 = w.to(torch.int32)
    for fused in (False, True):
        z, dt = pr["z"].cuda(), pr["dt"].cuda()
        kw = (dict(shard=shard, row_of_local=rol.cuda(), summary_row=srow)
              if fused else {})
        ops.lda_mh_wave_packed(dt, wt, rec, top, inv_p, offs, w32, z, ALPHA,
                               BETA, seed, **kw)
        assert torch.equal(z, z_ref)
        assert torch.equal(dt, dt_ref)


def test_packed_sampler_integer_invariants_on_racy_docs():
    K, n_words = 256, 500
    lengths = [1, 63, 64, 65, 200] * 5           # 25 docs: 7 workgroups
    pr = _problem(lengths, n_words, K, 21, zipf=True)
    shard0, rol, srow = _shard_for(pr, n_words, K, 22)
    shard = shard0.cuda()
    rec, top = ops.lda_packed_alloc(n_words, K, "cuda")
    invden, _ = ops.lda_alias_build_packed(shard, rol.cuda(),
                                           pr["nk"].cuda(), BETA, V, rec, top)
    rec0, wt = rec.clone(), pr["wt"].cuda()
    z, dt = pr["z"].cuda(), pr["dt"].cuda()
    ops.lda_mh_wave_packed(dt, wt, rec, top, invden, pr["offs"].cuda(),
                           pr["w"].cuda().to(torch.int32), z, ALPHA, BETA,
                           77, shard=shard, row_of_local=rol.cuda(),
                           summary_row=srow)
    z, dt, after = z.cpu(), dt.cpu(), shard.cpu()
    old = pr["z"]
    assert int(z.min()) >= 0 and int(z.max()) < K
    assert int((z != old).sum()) > 0
    want_dt = torch.zeros_like(dt)
    want_dt.view(-1).scatter_add_(0, pr["tok_doc"] * K + z.long(),
                                  torch.ones(z.shape[0], dtype=torch.int32))
    assert torch.equal(dt, want_dt)
    # shard delta = +1 at the new topic, -1 at the old, word and summary row
    ones = torch.ones(z.shape[0], dtype=torch.int32)
    want = torch.zeros_like(shard0)
    rows = rol.long()[pr["w"]]
    for r in (rows, torch.full_like(rows, srow)):
        want.view(-1).scatter_add_(0, r * K + z.long(), ones)
        want.view(-1).scatter_add_(0, r * K + old.long(), -ones)
    assert torch.equal(after - shard0, want)
    touched = torch.zeros(shard0.shape[0], dtype=torch.bool)
    touched[rol.long()] = True
    touched[srow] = True
    assert int((~touched).sum()) == 39
    assert torch.equal(after[~touched], shard0[~touched])
    assert torch.equal(rec, rec0)                # the tables are read-only
    assert torch.equal(wt.cpu(), pr["wt"])       # and so is the snapshot
