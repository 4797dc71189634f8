"""The shared MH token step and table-row build of ops/csrc/lda_alias.hip:
every kernel shape that calls them gives the same samples where no
intra-doc race exists, the serial kernel's prefetch changes nothing, and the
legacy build is bit-exact on the run-time-S path (K = 192, S = 3) that the
packed layout does not cover."""

import functools

import pytest
import torch

from harmony_amd import ops
from tests.test_lda_packed_gpu import (ALPHA, BETA, V, _counts, _problem,
                                       _shard_for)

pytestmark = pytest.mark.gpu


def _legacy_tables(pr):
    """GPU-built legacy arrays: (prob, alias, tprob, talias, qv, invden)."""
    t = ops.lda_alias_build(pr["wt"].cuda(), pr["nk"].cuda(), BETA, V)
    return t[:5] + (t[6],)


def _sweep(fn, pr, tabs, seed, dev):
    """fn over fresh copies of the problem's z and doc_topic."""
    prob, alias, tprob, talias, qv, invden = (t.to(dev) for t in tabs)
    z, dt = pr["z"].clone().to(dev), pr["dt"].clone().to(dev)
    fn(dt, pr["wt"].to(dev), invden, prob, alias, tprob, talias, qv,
       pr["offs"].to(dev), pr["w"].to(dev), z, ALPHA, BETA, seed)
    return z.cpu(), dt.cpu()


@pytest.mark.parametrize("K", [64, 192, 256])
def test_all_kernel_shapes_agree_without_intra_doc_race(K):
    # 1027 docs of length 0 or 1: tail workgroups for 64-thread and 4-wave
    # blocks, and no two tokens share a doc-topic row
    n_docs, n_words, seed = 1027, 300, 1234
    g = torch.Generator().manual_seed(11)
    lengths = torch.randint(0, 2, (n_docs,), generator=g)
    lengths[-1] = 1
    pr = _problem(lengths, n_words, K, 12, zipf=False)
    tabs = _legacy_tables(pr)
    z_ref, dt_ref = _sweep(ops.lda_mh, pr, tabs, seed, "cuda")
    moved = int((z_ref != pr["z"]).sum())
    print(f"K={K}: moved {moved} of {z_ref.shape[0]} tokens")
    assert moved > 0
    z, dt = _sweep(ops.lda_mh_wave, pr, tabs, seed, "cuda")
    assert torch.equal(z, z_ref)
    assert torch.equal(dt, dt_ref)
    if not ops.lda_packed_supported(K):
        assert K == 192
        return
    shard, rol, srow = _shard_for(pr, n_words, K, 13)
    shard, rol = shard.cuda(), rol.cuda()
    rec, top = ops.lda_packed_alloc(n_words, K, "cuda")
    invden, _ = ops.lda_alias_build_packed(shard, rol, pr["nk"].cuda(), BETA,
                                           V, rec, top)
    assert torch.equal(invden, tabs[5])
    for fused in (False, True):
        z, dt = pr["z"].cuda(), pr["dt"].cuda()
        kw = (dict(shard=shard, row_of_local=rol, summary_row=srow)
              if fused else {})
        ops.lda_mh_wave_packed(dt, pr["wt"].cuda(), rec, top, invden,
                               pr["offs"].cuda(),
                               pr["w"].cuda().to(torch.int32), z, ALPHA, BETA,
                               seed, **kw)
        assert torch.equal(z.cpu(), z_ref)
        assert torch.equal(dt.cpu(), dt_ref)


@functools.lru_cache(maxsize=None)
def _serial_problem(K):
    lengths = [0, 1, 2, 40, 255] * 3            # 255: the longest u8 row
    pr = _problem(lengths, 300, K, 31, zipf=True)
    tabs = _legacy_tables(pr)
    # the oracle reads the same tables, so only float ties can differ
    z_cpu, _ = _sweep(ops.lda_mh, pr, tabs, 321, "cpu")
    return lengths, pr, tabs, z_cpu


@pytest.mark.parametrize("K", [64, 192])
def test_serial_kernel_prefetch_on_equals_off(K, monkeypatch):
    lengths, pr, tabs, z_cpu = _serial_problem(K)
    monkeypatch.setenv("HARMONY_LDA_MH_PREFETCH", "0")
    z_off, dt_off = _sweep(ops.lda_mh, pr, tabs, 321, "cuda")
    monkeypatch.delenv("HARMONY_LDA_MH_PREFETCH")
    z_on, dt_on = _sweep(ops.lda_mh, pr, tabs, 321, "cuda")
    assert torch.equal(z_on, z_off)
    assert torch.equal(dt_on, dt_off)
    assert torch.equal(dt_on.sum(1), torch.tensor(lengths))
    assert int((z_on != pr["z"]).sum()) > 0
    match = float((z_on == z_cpu).float().mean())
    print(f"K={K}: {match:.4f} of z equals the CPU oracle's")
    assert match >= 0.99, match


def test_legacy_build_runtime_S_bit_exact():
    K, rows = 192, 37
    wt, nk = _counts(rows, K, K)
    cpu = ops.lda_alias_build(wt, nk, BETA, V)
    gpu = ops.lda_alias_build(wt.cuda(), nk.cuda(), BETA, V)
    assert len(cpu) == len(gpu) == 7
    names = ("prob", "alias", "top_prob", "top_alias", "qv", "qsum", "invden")
    for name, c, g in zip(names, cpu, gpu):
        g = g.cpu()
        assert g.dtype == c.dtype and g.shape == c.shape, name
        diff = int((g.view(torch.int32) != c.view(torch.int32)).sum())
        print(f"{name}: {diff} of {c.numel()} words differ")
        assert diff == 0, name
