"""Packed LDA tables (K7d), CPU paths: build/unpack against the legacy
build, and the trainer against the legacy alias_wave path."""

import pytest
import torch

from harmony_amd import ops


def _counts(rows, K, seed):
    g = torch.Generator().manual_seed(seed)
    wt = torch.randint(0, 6, (rows, K), generator=g, dtype=torch.int32)
    wt[0] = 0                      # an all-zero word row
    wt[1, : K // 2] = 0            # empty segments next to full ones
    nk = wt.sum(0).to(torch.int32) + 3
    return wt, nk


@pytest.mark.parametrize("K", [64, 128, 256])
def test_packed_build_unpack_matches_legacy_build(K):
    wt, nk = _counts(9, K, K)
    ref = ops.lda_alias_build(wt, nk, 0.01, 1000)
    rec, top = ops.lda_packed_alloc(9, K, "cpu")
    invden, qsum = ops.lda_alias_build_packed(wt, None, nk, 0.01, 1000,
                                              rec, top)
    prob, alias, tprob, talias, qv = ops.lda_unpack_tables(rec, top)
    for got, want in ((prob, ref[0]), (alias, ref[1]), (tprob, ref[2]),
                      (talias, ref[3]), (qv, ref[4]), (qsum, ref[5]),
                      (invden, ref[6])):
        assert got.dtype == want.dtype
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    S = K // 64
    assert bool((rec[:, :, :S] == 0).all())       # reserved slot untouched


@pytest.mark.parametrize("K", [64, 256])
def test_packed_build_through_src_rows(K):
    wt, nk = _counts(12, K, 7)
    rows = torch.tensor([11, 0, 5, 3, 8], dtype=torch.int32)
    ref = ops.lda_alias_build(wt[rows.long()], nk, 0.01, 1000)
    rec, top = ops.lda_packed_alloc(5, K, "cpu")
    ops.lda_alias_build_packed(wt, rows, nk, 0.01, 1000, rec, top)
    prob, alias, tprob, talias, qv = ops.lda_unpack_tables(rec, top)
    assert torch.equal(prob, ref[0]) and torch.equal(alias, ref[1])
    assert torch.equal(tprob, ref[2]) and torch.equal(talias, ref[3])
    assert torch.equal(qv, ref[4])


def test_packed_unsupported_k():
    assert not ops.lda_packed_supported(192)
    assert not ops.lda_packed_supported(32)
    assert ops.lda_packed_supported(512)


def _run_trainer(packed, K, steps=3):
    from harmony_amd.config import JobConfig
    from harmony_amd.dolphin.trainer import TrainerContext
    from harmony_amd.et.table import Table
    from harmony_amd.mlapps import lda

    job = JobConfig(job_id="packed_cpu", app="lda", num_mini_batches=2,
                    app_args={"num_vocabs": 120, "num_topics": K,
                              "tokens_per_doc": 9, "docs_per_batch": 11,
                              "sampler": "alias_wave", "alias_refresh": 2,
                              "packed": packed})
    dev = torch.device("cpu")
    table = Table(lda.model_table_cfg(job, 1), 0, 1, dev, comm=None)
    blocks, local_docs = lda.make_batches(job, 0, dev, 1)
    tctx = TrainerContext(job_id=job.job_id, rank=0, world_size=1,
                          device=dev, tables={lda.MODEL_TABLE: table},
                          app_args=job.app_args)
    tr = lda.LDATrainer(tctx, local_docs, blocks)
    tr.initialize()
    zs = []
    for i in range(steps):
        tr.set_batch_data(blocks[i % len(blocks)])
        tr.pull_model()
        tr.local_compute()
        tr.push_update()
        zs.append(tr._new_z.clone())
    return zs, tr.doc_topic.clone(), table.shard.clone()


@pytest.mark.parametrize("K", [64, 256])
def test_trainer_packed_equals_legacy_path_on_cpu(K):
    # the CPU fallback of both paths is the serial sampler: exact equality
    z0, dt0, sh0 = _run_trainer(False, K)
    z1, dt1, sh1 = _run_trainer(True, K)
    for a, b in zip(z0, z1):
        assert torch.equal(a, b)
    assert torch.equal(dt0, dt1)
    assert torch.equal(sh0, sh1)
    assert int(sh1.sum()) == 2 * int(dt1.sum())   # word rows + summary row


def test_trainer_k192_keeps_legacy_arrays():
    zs, dt, sh = _run_trainer(True, 192, steps=1)
    assert int(zs[0].max()) < 192 and int(dt.sum()) > 0
