"""LDA held-out perplexity on the device: kernel K7e (ops/csrc/lda_foldin.hip)
against the fp64 oracle of lda_foldin_cases.py with the assertions of
test_lda_foldin_cpu.py, its determinism, its 64-bit row offsets, and one
alias_wave job with test_data_path."""

import math

import pytest
import torch

from harmony_amd import ops
from tests import heldout_cases as hc
from tests import lda_foldin_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shape_pairs():
    return fc.split_pairs(fc.shape_docs())


@pytest.fixture()
def kernel_calls(monkeypatch):
    """Counts the launches of the HIP entry point."""
    assert ops.hip_available()
    calls = []
    real = ops._hip.lda_foldin
    monkeypatch.setattr(ops._hip, "lda_foldin",
                        lambda *a: calls.append(1) or real(*a))
    return calls


@pytest.mark.parametrize("K", fc.SHAPE_KS)
def test_one_step_chain(K, shape_pairs, kernel_calls):
    fc.check_chain(fc.random_table(K), shape_pairs, "cuda", "shapes")
    assert len(kernel_calls) == 6


def test_end_to_end_error_is_reported(shape_pairs):
    for K in (8, 320, 1024):
        te, le = fc.end_to_end_error(fc.random_table(K), shape_pairs, "cuda")
        assert math.isfinite(te) and math.isfinite(le)


def test_one_document_and_none(kernel_calls):
    docs = fc.shape_docs()
    for d in (1, 9):
        fc.check_chain(fc.random_table(96), fc.split_pairs(docs[d:d + 1]),
                       "cuda", f"doc {d}")
    assert len(kernel_calls) == 12
    theta, ll = fc.run_op(fc.random_table(96), fc.split_pairs([]), 20, "cuda")
    assert theta.shape == (0, 96) and ll.shape == (0,)
    assert len(kernel_calls) == 12              # D = 0: no launch


def test_topics_beyond_the_kernel_limit_take_the_tensor_ops(shape_pairs,
                                                            kernel_calls):
    theta, ll = fc.run_op(fc.random_table(2048), shape_pairs, 2, "cuda")
    assert kernel_calls == []
    want_t, want_l = fc.run_op(fc.random_table(2048), shape_pairs, 2, "cpu")
    assert torch.allclose(theta, want_t, rtol=1e-4, atol=0)
    assert torch.allclose(ll, want_l, rtol=1e-4, atol=0)


@pytest.mark.parametrize("name", ["threes", "zeros"])
def test_equal_rows_give_perplexity_v(name, shape_pairs):
    fc.check_perplexity_is_v(fc.equal_rows_tables()[name], shape_pairs,
                             "cuda")


def test_planted_table():
    pairs = fc.split_pairs(fc.planted_docs(13, 24, seed=99))
    ppl = {}
    for it in (0, 20):
        _theta, ll = fc.run_op(fc.planted_table(), pairs, it, "cuda")
        ppl[it] = math.exp(-float(ll.double().sum()) / (13 * 12))
    print(f"planted table: perplexity {ppl}")
    assert 16 <= ppl[20] < fc.V and ppl[20] < ppl[0]


@pytest.mark.parametrize("K", [96, 576])
def test_runs_and_document_orders_agree_bit_for_bit(K):
    docs = fc.shape_docs()
    table = fc.random_table(K)
    theta, ll = fc.run_op(table, fc.split_pairs(docs), 20, "cuda")
    again = fc.run_op(table, fc.split_pairs(docs), 20, "cuda")
    assert torch.equal(theta, again[0]) and torch.equal(ll, again[1])
    back = fc.run_op(table, fc.split_pairs(docs[::-1]), 20, "cuda")
    assert torch.equal(back[0].flip(0), theta)
    assert torch.equal(back[1].flip(0), ll)
    alone = fc.run_op(table, fc.split_pairs(docs[4:5]), 20, "cuda")
    assert torch.equal(alone[0][0], theta[4]) and alone[1][0] == ll[4]


def test_row_offsets_are_64_bit():
    """V = 2^21 + 1, K = 1024: the top word rows start past 2^31 elements.
    On an all-zero table every scored token has probability 1/V."""
    nv, K = 2 ** 21 + 1, 1024
    free, _total = torch.cuda.mem_get_info()
    if free < 16 * 2 ** 30:
        pytest.skip(f"needs 16 GB of free device memory, {free >> 30} free")
    g = torch.Generator().manual_seed(5)
    docs = [(nv - 16 + torch.randint(0, 16, (n,), generator=g)).tolist()
            for n in (2, 9, 24, 40, 64)]
    for doc in docs:                    # the one row that starts at 2^31
        doc[0] = doc[1] = nv - 1
    assert (nv - 1) * K >= 2 ** 31
    pairs = fc.split_pairs(docs, device="cuda")
    table = torch.zeros(nv + 1, K, dtype=torch.int32, device="cuda")
    try:
        fc.check_perplexity_is_v(table, pairs, "cuda", num_vocabs=nv)
    finally:
        del table
        torch.cuda.empty_cache()        # 8.6 GB back to the device


def test_metric_in_the_job_summary(tmp_path, kernel_calls):
    train, test, held = fc.planted_files(tmp_path)
    job = fc.lda_job("t_fold_job_gpu", train, test, sampler="alias_wave",
                     num_topics=64, num_vocabs=512)
    s, trainer = hc.run(job, device="cuda")
    assert trainer.test_set.obs_word.device.type == "cuda"
    assert len(kernel_calls) == 1
    assert s["test_examples"] == 13 and s["test_tokens"] == 13 * 12
    want, total = fc.recomputed(trainer, held)
    print(f"test_perplexity {s['test_perplexity']!r}, recomputed {want!r}")
    assert s["test_perplexity"] == want
    assert s["test_log_likelihood"] == total
    assert s["test_perplexity"] < 512
