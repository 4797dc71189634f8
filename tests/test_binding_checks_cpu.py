"""Argument checks of the raw HIP bindings, exercised with CPU tensors only.

Every binding checks metadata first and "on device" last, so a well-formed
CPU call stops at the device check and a malformed one at its own check:
nothing here can reach a kernel launch.
"""

import pytest
import torch

from harmony_amd import ops

pytestmark = pytest.mark.skipif(not ops.hip_available(),
                                reason="HIP extension not built")

i32, i64, f32, u8 = torch.int32, torch.int64, torch.float32, torch.uint8


def z(*shape, dt=f32):
    return torch.zeros(*shape, dtype=dt)


def padded(rows, c, ld):
    """[rows, c] view with unit inner stride and row stride ld."""
    return z(rows, ld)[:, :c]


K = 64          # the LDA samplers need K % 64 == 0
D, N, V = 2, 4, 3   # two documents of two tokens over three words


def lda_tables():
    return dict(prob=z(V, K), alias=z(V, K, dt=i32), top_prob=z(V, 64),
                top_alias=z(V, 64, dt=i32), qv=z(V, K))


def mh_args():
    t = lda_tables()
    return dict(doc_topic=z(D, K, dt=i32), word_topic=z(V, K, dt=i32),
                invden=z(K), prob=t["prob"], alias=t["alias"],
                top_prob=t["top_prob"], top_alias=t["top_alias"], qv=t["qv"],
                doc_offsets=z(D + 1, dt=i64), word_ids=z(N, dt=i64),
                assignments=z(N, dt=i32), alpha=0.1, beta=0.01, seed=1)


MH_BAD = [
    ("doc_topic", z(D, K + 1, dt=i32)),          # K % 64 != 0
    ("prob", z(V, K - 1)), ("alias", z(V + 1, K, dt=i32)),
    ("top_prob", z(V, 32)), ("top_alias", z(V + 1, 64, dt=i32)),
    ("qv", z(V + 1, K)), ("word_topic", z(V - 1, K, dt=i32)),
    ("word_topic", z(V, K)), ("invden", z(K + 1)),
    ("doc_offsets", z(D, dt=i64)), ("assignments", z(N + 1, dt=i32)),
    ("word_ids", z(N, dt=i32)),
]

# entry -> (well-formed keyword arguments in binding order,
#           [(argument to replace, bad value[, name the error carries])])
ENTRIES = {
    "mlr_softmax_grad": (lambda: dict(logits=z(2, 3), labels=z(2, dt=i64)), [
        ("labels", z(3, dt=i64)), ("labels", z(2, dt=i32)),
        ("logits", z(6)), ("logits", z(2, 6)[:, ::2])]),
    "mlr_fwd": (lambda: dict(X=z(2, 4), W=z(3, 4), labels=z(2, dt=i64)), [
        ("W", z(3, 5)), ("labels", z(1, dt=i64)), ("X", z(2, 4, dt=i32))]),
    "mlr_grad": (lambda: dict(P=z(2, 3), X=z(2, 4)), [
        ("P", z(3, 3)), ("P", z(2, 17)), ("X", z(8))]),
    "mlr_step_mfma": (lambda: dict(X=z(64, 64), Wt=z(64, 16),
                                   labels=z(64, dt=i64), row_block=0, C=3,
                                   splitf=1, splitb=1), [
        ("Wt", z(64, 8)), ("labels", z(63, dt=i64)),
        ("row_block", 32, "row_block"), ("C", 17, "C"),
        ("splitf", 2, "splitf"), ("splitb", 2, "splitb")]),
    "mlr_fwd_mfma_part": (lambda: dict(X=z(64, 64), Wt=z(64, 16), P=z(64, 16),
                                       off=0, n=64, splitf=1), [
        ("Wt", z(32, 16)), ("P", z(32, 16)), ("off", 64, "off"),
        ("n", 32, "n"), ("splitf", 2, "splitf")]),
    "mlr_softmax_part": (lambda: dict(P=z(64, 16), labels=z(64, dt=i64),
                                      loss=z(1), correct=z(1, dt=i32), off=0,
                                      n=64, C=3), [
        ("labels", z(32, dt=i64)), ("loss", z(2)), ("correct", z(1)),
        ("n", 128, "n"), ("C", 17, "C")]),
    "mlr_grad_mfma_part": (lambda: dict(P=z(64, 16), X=z(64, 64),
                                        gradT=z(16, 64), off=0, n=64,
                                        splitb=1), [
        ("P", z(64, 8)), ("gradT", z(16, 32)), ("off", 1, "off"),
        ("splitb", 2, "splitb")]),
    "nmf_grad": (lambda: dict(L=z(2, 4), R=z(3, 4), row_ptr=z(3, dt=i64),
                              col_idx=z(5, dt=i64), vals=z(5), lam=0.1), [
        ("R", z(3, 5)), ("row_ptr", z(2, dt=i64)), ("vals", z(4)),
        ("col_idx", z(5, dt=i32))]),
    "nmf_grad_twopass": (lambda: dict(
        L=z(2, 4), R=z(3, 4), row_ptr=z(3, dt=i64), col_idx=z(5, dt=i64),
        vals=z(5), perm=z(5, dt=i64), seg_ptr=z(4, dt=i64),
        row_sorted=z(5, dt=i64), lam=0.1), [
        ("vals", z(4)), ("col_idx", z(5, 1, dt=i64)), ("perm", z(6, dt=i64)),
        ("row_sorted", z(4, dt=i64)), ("seg_ptr", z(3, dt=i64)),
        ("row_ptr", z(4, dt=i64)), ("R", z(3, 8))]),
    "nmf_step": (lambda: dict(
        L=z(4, 4), l_lo=1, n=2, R_src=z(3, 4), row_ptr=z(3, dt=i32),
        col=z(5, dt=i32), vals=z(5), perm=z(5, dt=i32), seg_ptr=z(4, dt=i32),
        row_sorted=z(5, dt=i32), rsrc_of=None, step=z(()), lam=0.1,
        max_val=1.0, want_lgrad=False), [
        ("R_src", z(3, 5)), ("R_src", z(2, 4)), ("l_lo", 3, "l_lo"),
        ("row_ptr", z(4, dt=i32)), ("col", z(5, dt=i64)), ("vals", z(6)),
        ("perm", z(4, dt=i32)), ("row_sorted", z(6, dt=i32)),
        ("rsrc_of", z(2, dt=i32)), ("step", z(2))]),
    "lda_gibbs": (lambda: dict(
        doc_topic=z(D, K, dt=i32), word_topic=z(V, K, dt=i32),
        topic_sum=z(K, dt=i32), doc_offsets=z(D + 1, dt=i64),
        word_ids=z(N, dt=i64), assignments=z(N, dt=i32), alpha=0.1, beta=0.01,
        num_vocabs=V, seed=1), [
        ("word_topic", z(V, K + 1, dt=i32)), ("topic_sum", z(K - 1, dt=i32)),
        ("doc_offsets", z(D, dt=i64)), ("assignments", z(N - 1, dt=i32)),
        ("doc_topic", z(D * K, dt=i32)), ("word_ids", z(N, dt=i32))]),
    "lda_apply_pairs": (lambda: dict(shard=z(V + 1, K, dt=i32),
                                     rows=z(N, dt=i64), old_t=z(N, dt=i32),
                                     new_t=z(N, dt=i32)), [
        ("shard", z((V + 1) * K, dt=i32)), ("old_t", z(N + 1, dt=i32)),
        ("new_t", z(N - 1, dt=i32)), ("rows", z(N, dt=i32))]),
    "lda_apply_all": (lambda: dict(shard=z(V + 1, K, dt=i32),
                                   word_rows=z(N, dt=i64), old_t=z(N, dt=i32),
                                   new_t=z(N, dt=i32), summary_row=V), [
        ("shard", z(K, dt=i32)), ("old_t", z(N + 1, dt=i32)),
        ("new_t", z(N - 1, dt=i32)), ("summary_row", V + 1, "summary_row"),
        ("summary_row", -1, "summary_row")]),
    "lda_alias_build": (lambda: dict(word_topic=z(V, K, dt=i32),
                                     topic_sum=z(K, dt=i32), beta=0.01,
                                     num_vocabs=V, max_workgroups=None), [
        ("word_topic", z(V, K + 1, dt=i32), "K % 64"),
        ("topic_sum", z(K + 1, dt=i32)), ("word_topic", z(V, K))]),
    "lda_mh": (mh_args, MH_BAD),
    "lda_mh_wave": (mh_args, MH_BAD),
    "lda_alias_build_packed": (lambda: dict(
        src=z(V, K, dt=i32), src_rows=None, topic_sum=z(K, dt=i32), beta=0.01,
        num_vocabs=V, rec=z(V, 64, 4, dt=i32), top=z(V, 64, 2, dt=i32),
        max_workgroups=None), [
        ("rec", z(V, 64, 5, dt=i32)), ("top", z(V + 1, 64, 2, dt=i32)),
        ("topic_sum", z(K + 1, dt=i32)),
        ("src", z(V - 1, K, dt=i32)), ("src_rows", z(V + 1, dt=i32))]),
    "lda_mh_wave_packed": (lambda: dict(
        doc_topic=z(D, K, dt=i32), word_topic=z(V + 2, K, dt=i32),
        rec=z(V, 64, 4, dt=i32), top=z(V, 64, 2, dt=i32), invden=z(K),
        doc_offsets=z(D + 1, dt=i64), word_ids=z(N, dt=i32),
        assignments=z(N, dt=i32), alpha=0.1, beta=0.01, seed=1,
        shard=z(V + 1, K, dt=i32), row_of_local=z(V, dt=i32),
        summary_row=V), [
        ("doc_topic", z(D, 2 * K, dt=i32)), ("invden", z(K - 1)),
        ("doc_offsets", z(D + 2, dt=i64)), ("assignments", z(N + 1, dt=i32)),
        ("word_topic", z(V - 1, K, dt=i32)),
        ("shard", z(V + 1, 2 * K, dt=i32)),
        ("row_of_local", z(V + 1, dt=i32)), ("row_of_local", None),
        ("summary_row", V + 1, "summary_row")]),
    "lda_foldin": (lambda: dict(
        word_topic=z(V, K, dt=i32), topic_sum=z(K, dt=i32),
        obs_ptr=z(D + 1, dt=i64), obs_word=z(N, dt=i64),
        obs_cnt=z(N, dt=i32), sc_ptr=z(D + 1, dt=i64), sc_word=z(N, dt=i64),
        sc_cnt=z(N, dt=i32), alpha=0.1, beta=0.01, num_vocabs=V, iters=2), [
        ("topic_sum", z(K + 1, dt=i32)), ("word_topic", z(V - 1, K, dt=i32)),
        ("sc_ptr", z(D, dt=i64)), ("obs_cnt", z(N + 1, dt=i32)),
        ("sc_cnt", z(N - 1, dt=i32)), ("obs_word", z(N, dt=i32)),
        ("iters", -1, "iters")]),
    "lasso_cd": (lambda: dict(Xt=z(3, 2), r=z(2), w=z(3), col_sq=z(3),
                              lam_n=0.1), [
        ("r", z(3)), ("w", z(2)), ("col_sq", z(4)), ("Xt", z(6))]),
    "lasso_cd_sparse": (lambda: dict(
        feat_ids=z(2, dt=i32), feat_ptr=z(3, dt=i64), feat_row=z(4, dt=i32),
        feat_val=z(4), y=z(2), w=z(5), col_sq=z(2), lam_n=0.1, r_out=z(2),
        threads=64), [
        ("feat_ptr", z(2, dt=i64)), ("feat_val", z(3)), ("r_out", z(3)),
        ("col_sq", z(3)), ("feat_row", z(4, dt=i64)),
        ("threads", 128, "threads"), ("threads", 100, "threads")]),
    "gbt_hist": (lambda: dict(bins=z(3, 2, dt=i32), resid=z(3),
                              node=z(3, dt=i32), cnt=z(2, 2, 4),
                              sum=z(2, 2, 4)), [
        ("resid", z(2)), ("node", z(4, dt=i32)), ("cnt", z(2, 3, 4)),
        ("sum", z(2, 2, 5)), ("bins", z(3, 2, dt=i64))]),
    "gbt_best_split": (lambda: dict(cnt=z(2, 3, 4), s=z(2, 3, 4),
                                    ftype=z(3, dt=i32), lam=1.0), [
        ("s", z(2, 3, 5)), ("ftype", z(2, dt=i32)), ("cnt", z(2, 12))]),
    "gbt_hist_sparse": (lambda: dict(
        feat_ptr=z(3, dt=i64), feat_row=z(4, dt=i32), feat_bin=z(4, dt=i32),
        feat_idx=z(4, dt=i32), zero_bin=z(2, dt=i32), resid=z(3),
        node=z(3, dt=i32), node_cnt=z(2), node_sum=z(2), nb=4), [
        ("feat_bin", z(3, dt=i32)), ("feat_idx", z(5, dt=i32)),
        ("zero_bin", z(3, dt=i32)), ("node", z(2, dt=i32)),
        ("node_sum", z(3)), ("resid", z(3, dt=torch.float64))]),
    "gbt_forest_predict": (lambda: dict(
        bins=z(3, 2, dt=i64), forest=z(2, 5, dt=i32), depth=1, step_size=0.1,
        F=2, keys=None, key_bin=None, row_ptr=None), [
        ("bins", z(3, 3, dt=i64)), ("forest", z(2, 6, dt=i32)),
        ("forest", z(12, dt=i32)), ("depth", 0, "depth")]),
    "scatter_apply": (lambda: dict(shard=z(4, 3), rows=z(2, dt=i64),
                                   deltas=z(2, 3), mode=0, step=0.0,
                                   maxval=0.0), [
        ("deltas", z(3, 3)), ("deltas", z(2, 4)), ("deltas", z(2, 3, dt=i32)),
        ("rows", z(2, dt=i32)), ("shard", z(4, 3, dt=torch.float64))]),
    "dense_apply": (lambda: dict(shard=z(4, 3), delta=z(4, 3), mode=0,
                                 step=0.0, maxval=0.0), [
        ("delta", z(4, 4)), ("delta", z(4, 3, dt=i32)),
        ("shard", z(4, 6)[:, ::2])]),
    "os_gather": (lambda: dict(ptr=64, idx=z(2, dt=i64), k=3, dtype_i32=0), [
        ("idx", z(2, dt=i32)), ("k", 0, "k")]),
    "os_scatter_add": (lambda: dict(ptr=64, idx=z(2, dt=i64), delta=z(2, 3)), [
        ("delta", z(3, 3)), ("delta", z(6)), ("idx", z(2, dt=i32))]),
    "os_ring_reserve": (lambda: dict(base=64, W=2, cap=4, vd=3, writer=1, n=2,
                                     scratch=z(1, dt=i64)), [
        ("writer", 2, "writer"), ("scratch", z(1, dt=i32)),
        ("scratch", z(0, dt=i64))]),
    "os_ring_read_head": (lambda: dict(base=64, W=2, cap=4, vd=3, writer=1,
                                       scratch=z(2, dt=i64)), [
        ("writer", -1, "writer"), ("scratch", z(2))]),
    "os_ring_push": (lambda: dict(base=64, W=2, cap=4, vd=3, writer=0,
                                  seq_base=z(1, dt=i64), keys=z(2, dt=i64),
                                  deltas=z(2, 3)), [
        ("deltas", z(2, 4)), ("deltas", z(3, 3)), ("keys", z(2, dt=i32)),
        ("seq_base", z(1, dt=i32))]),
    "pregel_pull": (lambda: dict(
        in_ptr=z(4, dt=i64), in_src=z(5, dt=i32), in_w=z(5), w_const=1.0,
        vert_msg=z(3), send_mask=z(3, dt=u8), combiner=1, add_weight=True,
        group=4), [
        ("in_w", z(4)), ("send_mask", z(4, dt=u8)), ("send_mask", z(3)),
        ("vert_msg", z(3, 1)), ("in_src", z(5, dt=i64)),
        ("combiner", 2, "combiner"), ("group", 3, "group"),
        ("group", 128, "group")]),
    "pregel_push": (lambda: dict(
        out_ptr=z(4, dt=i64), out_row=z(5, dt=i32), out_w=z(5), w_const=1.0,
        vert_msg=z(3), frontier=z(2, dt=i32), send_mask=z(3, dt=u8),
        num_rows=3, add_weight=True, edges_hint=-1), [
        ("vert_msg", z(4)), ("out_w", z(6)), ("send_mask", z(2, dt=u8)),
        ("frontier", z(2, dt=i64)), ("num_rows", -1, "num_rows")]),
    "mlr_sparse_fwd": (lambda: dict(
        row_ptr=z(3, dt=i64), col=z(4, dt=i32), val=z(4), Wt=z(5, 4), C=3,
        group=2), [
        ("val", z(5)), ("Wt", z(5, 8), "Wt"), ("Wt", z(5, 3), "Wt"),
        ("Wt", z(6, 8)[1:, :4]), ("Wt", z(21)[1:].view(5, 4), "Wt"),
        ("col", z(4, dt=i64)), ("row_ptr", z(3, 1, dt=i64)),
        ("group", 3, "group"), ("group", 0, "group")]),
    "mlr_sparse_grad": (lambda: dict(
        feat_ids=z(2, dt=i32), feat_ptr=z(3, dt=i64), feat_row=z(4, dt=i32),
        feat_val=z(4), P=padded(3, 3, 4), F=5, group=2), [
        ("feat_ptr", z(2, dt=i64)), ("feat_val", z(3)),
        ("P", z(3, 3), "P"),                         # row stride 3
        ("P", z(3, 8)[:, ::2]),                      # inner stride 2
        ("P", z(13)[1:].view(3, 4)[:, :3], "P"),     # misaligned base
        ("P", z(3, 4, dt=torch.float64)), ("F", -1, "F"),
        ("group", 6, "group")]),
}

CASES = [(op, i) for op, (_, bad) in ENTRIES.items() for i in range(len(bad))]


def call(op, kwargs):
    return getattr(ops._load_hip(), op)(*kwargs.values())


def test_every_launching_binding_is_listed():
    out_of_scope = ("parse_", "os_ipc_", "os_stream_", "os_cu_masked_stream",
                    "os_ring_bytes", "os_shard_alloc", "os_ring_drain")
    hip = ops._load_hip()
    names = [n for n in dir(hip) if not n.startswith("_")
             and callable(getattr(hip, n)) and not n.startswith(out_of_scope)
             and not n.endswith(("_max_rows", "_max_cells", "_max_depth",
                                 "_max_topics", "_lds_words", "_build_batch"))]
    assert sorted(names) == sorted(ENTRIES)


@pytest.mark.parametrize("op", list(ENTRIES))
def test_well_formed_cpu_call_stops_at_the_device_check(op):
    with pytest.raises(RuntimeError, match=op + ": every tensor must be on "
                       "device") as e:
        call(op, ENTRIES[op][0]())
    assert "got cpu" in str(e.value)


@pytest.mark.parametrize("op,i", CASES,
                         ids=[f"{op}-{i}" for op, i in CASES])
def test_malformed_argument_is_named(op, i):
    good, bad = ENTRIES[op]
    arg, value, *named = bad[i]
    kwargs = good()
    assert arg in kwargs
    kwargs[arg] = value
    with pytest.raises(RuntimeError) as e:
        call(op, kwargs)
    msg = str(e.value).split("\n")[0]
    assert "on device" not in msg, msg
    assert msg.startswith(op + ": "), msg
    assert (named[0] if named else arg) in msg[len(op):], msg
