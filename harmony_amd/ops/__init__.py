"""Compute ops: CDNA4 HIP kernels with fp32 torch reference implementations.

Dispatch policy:
  * CPU tensors -> torch reference implementation (also the numerics oracle).
  * CUDA (ROCm) tensors -> the in-tree HIP extension `_hip_ops`. If the
    extension is missing on a GPU machine this raises immediately — a silent
    eager fallback would invalidate every GPU benchmark (and the round-end
    "native code not loaded" check).
Set HARMONY_FORCE_TORCH_OPS=1 to force the torch path on GPU (debug only).

Kernel inventory (reference hot loops):
  K1  nmf_grad            NMFTrainer.java:328-367
  K3  (fused in push)     NMFETModelUpdateFunction.java:48-52
  K4  mlr softmax+grad    MLRTrainer.java:374-398,475-489
  K4s mlr_sparse_fwd/grad MLRTrainer.java:374-398 over SparseVector rows
  K7  lda_gibbs           SparseLDASampler.java:141-274
  K7e lda_foldin          held-out document completion (TestDataProvider)
  K9  scatter-apply       LDAETModelUpdateFunction.java:43-64
  K10 gbt_hist            GBTTrainer.java:244+ (histogram method)
  K10b gbt_best_split     GBTTrainer.java bestSplitRealFeature/LabelFeature
  K10s gbt_hist_sparse    K10 over SparseVector samples (GBTETDataParser)
  K10p gbt_forest_predict GBTTrainer.java predictByTree over the whole forest
  K11 lasso_cd            LassoTrainer.java:164-190
  K11s lasso_cd_sparse    LassoTrainer.java:164-208 over SparseVector columns
  K12 loss reductions     NMFTrainer.java:414-456 etc.
  K13 pregel_pull         pregel MessageManager.addMessage + MessageCombiner
  K13p pregel_push        K13 along the out-edges of the sending vertices only
                          (ComputationCallable.java:36 runs woken vertices)
"""

from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

_hip = None
_hip_err: Optional[str] = None


def _load_hip():
    global _hip, _hip_err
    if _hip is not None or _hip_err is not None:
        return _hip
    try:
        from harmony_amd.ops import _hip_ops  # built in-tree by setup_ops.py

        _hip = _hip_ops
    except ImportError:
        try:
            import importlib.util
            from pathlib import Path

            cands = list(Path(__file__).parent.glob("_hip_ops*.so"))
            if cands:
                spec = importlib.util.spec_from_file_location("_hip_ops", cands[0])
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                _hip = mod
            else:
                _hip_err = "harmony_amd/ops/_hip_ops*.so not built " \
                           "(run: python setup_ops.py build)"
        except Exception as e:  # noqa: BLE001
            _hip_err = str(e)
    return _hip


def hip_available() -> bool:
    return _load_hip() is not None


def _use_hip(t: torch.Tensor) -> bool:
    if t.device.type != "cuda":
        return False
    if os.environ.get("HARMONY_FORCE_TORCH_OPS") == "1":
        return False
    if _load_hip() is None:
        raise RuntimeError(
            f"GPU tensor but HIP extension not available: {_hip_err}. "
            "Refusing silent eager fallback on a GPU machine.")
    return True


# ---------------------------------------------------------------------------
# K4: MLR fused softmax + label-subtract + CE/accuracy
# ---------------------------------------------------------------------------

def mlr_forward(X: torch.Tensor, W: torch.Tensor, labels: torch.Tensor
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """MLR forward: logits = X @ W^T (rocBLAS), then the fused
    softmax + label-subtract + CE/accuracy kernel (K4).
    Returns (p - onehot [B,C], loss_sum, n_correct)."""
    # Measured (scripts/mlr_ab.py, isolated A/B on MI355X): rocBLAS X@W^T is
    # near the HBM floor (0.204 ms at 16k x 16k x 10) — the custom fused
    # kernel (0.685 ms) only looked competitive against concurrency-inflated
    # profile times. GEMM + the small fused softmax kernel is the fast path;
    # mlr_fwd stays available for C<=16 regression testing.
    return softmax_grad_ce(X @ W.t(), labels)


def mlr_grad_gemm(P: torch.Tensor, X: torch.Tensor) -> torch.Tensor:
    """grad = P^T @ X. rocBLAS measured 0.212 ms vs the custom B-tile kernel's
    0.520 ms (scripts/mlr_ab.py) — Tensile's split-K wins this shape."""
    return P.t() @ X


def mlr_step_ok(X: torch.Tensor, C: int) -> bool:
    """Shapes the fused MFMA step kernel supports (see mlr_mfma.hip)."""
    B, F = X.shape
    return (C <= 16 and F % 64 == 0 and B % 64 == 0
            and X.dtype == torch.float32)


def _pow2_div(limit: int, n: int) -> int:
    """Largest power of two <= limit that divides n."""
    p = 1
    while p * 2 <= limit and n % (p * 2) == 0:
        p *= 2
    return p


def mlr_step_mfma(X: torch.Tensor, W: torch.Tensor, labels: torch.Tensor,
                  row_block: int = 0, splitf: Optional[int] = None,
                  splitb: Optional[int] = None,
                  Wt_buf: Optional[torch.Tensor] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One fused MLR step on the gfx950 matrix cores (K4-MFMA,
    ops/csrc/mlr_mfma.hip): logits = X @ W^T via v_mfma_f32_16x16x4_f32,
    in-kernel softmax - onehot, grad = P^T @ X via MFMA with split-B
    atomics. With row_block > 0 the fwd/grad pair runs per row block so the
    grad pass re-reads X from the Infinity Cache (the step is X-bandwidth
    bound). Returns (grad [C,F], loss_sum, n_correct) — exact-f32 MFMA
    numerics (a k-ordered fmaf chain).

    Replaces reference MLRTrainer.java:374-398 + :475-489 + the rocBLAS
    GEMM pair (measured A/B: scripts/mlr_mfma_ab.py)."""
    C, F = W.shape
    if not _use_hip(X):                # CPU oracle path
        p, loss, correct = mlr_forward(X, W, labels)
        return mlr_grad_gemm(p, X), loss, correct
    B = X.shape[0]
    rows = row_block if row_block > 0 else B
    if splitf is None:
        # target ~512 workgroups per launch (2 blocks/CU on 256 CUs) —
        # the sweep's optimum on the bench shape (scripts/mlr_mfma_ab.py)
        splitf = _pow2_div(max(1, 512 // (rows // 64)), F // 64)
    if splitb is None:
        splitb = _pow2_div(max(1, 512 // (F // 64)), rows // 64)
    if Wt_buf is None:
        Wt_buf = torch.zeros((F, 16), dtype=X.dtype, device=X.device)
    Wt_buf[:, :C] = W.t()
    gradT, loss, correct = _hip.mlr_step_mfma(
        X.contiguous(), Wt_buf, labels.contiguous(), row_block, C,
        splitf, splitb)
    return gradT[:C], loss[0], correct[0].to(torch.int64)


_mlr_aux_streams = {}


def mlr_step_mfma_pipelined(X: torch.Tensor, W: torch.Tensor,
                            labels: torch.Tensor, row_block: int = 2048,
                            splitf: Optional[int] = None,
                            splitb: Optional[int] = None,
                            Wt_buf: Optional[torch.Tensor] = None
                            ) -> Tuple[torch.Tensor, torch.Tensor,
                                       torch.Tensor]:
    """Row-blocked K4-MFMA step with a two-stream software pipeline:
    fwd+softmax of block i+1 (stream A) overlaps grad of block i (stream
    B). The grad pass then re-reads its X block from the 256 MiB Infinity
    Cache while fwd streams the next block from HBM — the step's HBM
    traffic drops from 2 passes over X toward 1 (the step is X-bandwidth
    bound). Falls back to the single-stream path when shapes don't block
    evenly."""
    C, F = W.shape
    if not _use_hip(X):
        return mlr_step_mfma(X, W, labels)
    B = X.shape[0]
    if row_block <= 0 or B % row_block or row_block % 64 or B == row_block:
        return mlr_step_mfma(X, W, labels, row_block=0, splitf=splitf,
                             splitb=splitb, Wt_buf=Wt_buf)
    if splitf is None:
        splitf = _pow2_div(max(1, 512 // (row_block // 64)), F // 64)
    if splitb is None:
        splitb = _pow2_div(max(2, 1024 // (F // 64)), row_block // 64)
    if Wt_buf is None:
        Wt_buf = torch.zeros((F, 16), dtype=X.dtype, device=X.device)
    Wt_buf[:, :C] = W.t()
    dev = X.device
    key = dev.index
    aux = _mlr_aux_streams.get(key)
    if aux is None:
        aux = (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev))
        _mlr_aux_streams[key] = aux
    sA, sB = aux
    X = X.contiguous()
    labels = labels.contiguous()
    P = torch.zeros((B, 16), dtype=X.dtype, device=dev)
    gradT = torch.zeros((16, F), dtype=X.dtype, device=dev)
    loss = torch.zeros((1,), dtype=X.dtype, device=dev)
    correct = torch.zeros((1,), dtype=torch.int32, device=dev)
    cur = torch.cuda.current_stream(dev)
    start = torch.cuda.Event()
    start.record(cur)
    sA.wait_event(start)
    sB.wait_event(start)
    for off in range(0, B, row_block):
        ev = torch.cuda.Event()
        with torch.cuda.stream(sA):
            _hip.mlr_fwd_mfma_part(X, Wt_buf, P, off, row_block, splitf)
            _hip.mlr_softmax_part(P, labels, loss, correct, off, row_block,
                                  C)
            ev.record(sA)
        sB.wait_event(ev)
        with torch.cuda.stream(sB):
            _hip.mlr_grad_mfma_part(P, X, gradT, off, row_block, splitb)
    endA, endB = torch.cuda.Event(), torch.cuda.Event()
    endA.record(sA)
    endB.record(sB)
    cur.wait_event(endA)
    cur.wait_event(endB)
    for t in (X, Wt_buf, P, gradT, loss, correct, labels):
        t.record_stream(sA)
        t.record_stream(sB)
    return gradT[:C], loss[0], correct[0].to(torch.int64)


def softmax_grad_ce(logits: torch.Tensor, labels: torch.Tensor
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Row softmax with log-sum-exp guard; returns (p - onehot(label),
    sum of CE loss, #correct). Fuses reference MLRTrainer predict/softmax
    (:475-489) + label subtract (:374-398) + CE/accuracy metrics."""
    if _use_hip(logits):
        return _hip.mlr_softmax_grad(logits.contiguous(), labels.contiguous())
    z = logits.float()
    m = z.max(dim=1, keepdim=True).values
    e = torch.exp(z - m)
    s = e.sum(dim=1, keepdim=True)
    p = e / s
    lse = m.squeeze(1) + torch.log(s.squeeze(1))
    loss = (lse - z.gather(1, labels.view(-1, 1)).squeeze(1)).sum()
    correct = (z.argmax(dim=1) == labels).sum()
    grad = p
    grad.scatter_add_(1, labels.view(-1, 1),
                      torch.full((z.shape[0], 1), -1.0, device=z.device))
    return grad.to(logits.dtype), loss, correct


# ---------------------------------------------------------------------------
# K4s: sparse MLR — CSR forward and column-index gradient (gather-reduce)
# ---------------------------------------------------------------------------

def mlr_sparse_group(num_segments: int, num_entries: int) -> int:
    """Lanes that cooperate on one segment (a row in the forward, a present
    feature in the gradient) of the K4s kernel: the smallest power of two >=
    an eighth of the mean segment length, clamped to 1..64. K13's rule with
    up to 8 entries per lane instead of 1: an entry here costs a Cp-float
    row fetch and every doubling of the group adds Cp shuffles per segment.
    Measured against forced groups it picks the fastest or a near-fastest
    group at 1.3, 32, 150 and 780 entries per segment, and one up to 1.4x
    off the fastest at 254 (profiles/mlr_sparse_ab.md). A function of the
    batch alone, so a batch always runs with the same summation order."""
    mean = num_entries / max(1, num_segments)
    g = 1
    while g < 64 and g * 8 < mean:
        g *= 2
    return g


def mlr_sparse_wt(W: torch.Tensor, out: Optional[torch.Tensor] = None
                  ) -> torch.Tensor:
    """The model transposed and padded for the K4s forward: [F, Cp] float32,
    Cp = C rounded up to a multiple of 4, pad columns zero. `out` is a
    persistent buffer from an earlier call (its pad columns stay zero)."""
    C, F = W.shape
    if out is None:
        out = torch.zeros((F, (C + 3) // 4 * 4), dtype=torch.float32,
                          device=W.device)
    out[:, :C] = W.t()
    return out


def mlr_sparse_logits(row_ptr: torch.Tensor, col: torch.Tensor,
                      val: torch.Tensor, W: torch.Tensor,
                      Wt_buf: Optional[torch.Tensor] = None,
                      _force_group: int = 0) -> torch.Tensor:
    """logits [B, C] = X @ W^T for a CSR batch X (row_ptr int64 [B+1],
    col int32 [nnz], val float32 [nnz]) and the model W [C, F], touching
    only the batch's non-zeros (K4s forward, ops/csrc/mlr_sparse.hip;
    reference MLRTrainer.java:374-398 over SparseVector rows). A row with
    no entries gives zeros; entries whose column lies outside [0, F) are
    skipped.

    On GPU the kernel reads W through mlr_sparse_wt's layout; Wt_buf is the
    caller's persistent buffer for it (filled here), else one is allocated.
    CPU tensors (and HARMONY_FORCE_TORCH_OPS=1) take the torch reference
    below, which is also the kernel's test oracle. _force_group is for
    tests: it overrides the lanes-per-row choice of mlr_sparse_group."""
    C, F = W.shape
    B = row_ptr.shape[0] - 1
    if _use_hip(W):
        if B == 0:
            return torch.empty((0, C), dtype=torch.float32, device=W.device)
        group = _force_group or mlr_sparse_group(B, col.shape[0])
        Wt = mlr_sparse_wt(W, Wt_buf)
        return _hip.mlr_sparse_fwd(row_ptr.contiguous(), col.contiguous(),
                                   val.contiguous(), Wt, int(C), int(group))
    dev = W.device
    row = torch.repeat_interleave(torch.arange(B, device=dev),
                                  row_ptr[1:] - row_ptr[:-1])
    c = col.long()
    ok = (c >= 0) & (c < F)
    row, c, v = row[ok], c[ok], val[ok]
    logits = torch.zeros((B, C), dtype=torch.float32, device=dev)
    logits.index_add_(0, row, v.unsqueeze(1) * W.float().t()[c])
    return logits


def mlr_sparse_forward(row_ptr: torch.Tensor, col: torch.Tensor,
                       val: torch.Tensor, W: torch.Tensor,
                       labels: torch.Tensor,
                       Wt_buf: Optional[torch.Tensor] = None,
                       _force_group: int = 0
                       ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Sparse MLR forward: mlr_sparse_logits, then the fused softmax +
    label-subtract + CE/accuracy kernel (K4). Same return contract as
    mlr_forward: (p - onehot [B, C], loss_sum, n_correct)."""
    return softmax_grad_ce(
        mlr_sparse_logits(row_ptr, col, val, W, Wt_buf, _force_group),
        labels)


def mlr_sparse_grad(feat_ids: torch.Tensor, feat_ptr: torch.Tensor,
                    feat_row: torch.Tensor, feat_val: torch.Tensor,
                    P: torch.Tensor, F: int, _force_group: int = 0
                    ) -> torch.Tensor:
    """grad [C, F] = P^T @ X through the batch's static column index (K4s
    gradient): feat_ids int32 [nf] the distinct present columns ascending,
    feat_ptr int64 [nf+1], feat_row int32 [nnz] / feat_val float32 [nnz]
    the entries of each feature with rows ascending. G[c, f] =
    sum_e feat_val[e] * P[feat_row[e], c]; absent features stay exactly 0.
    No atomics, so the result is bitwise reproducible. The kernel reads P
    rows with 16-byte loads, so a P whose row stride is no multiple of 4
    floats is first copied into a padded [B, Cp] buffer (measured faster
    than scalar loads, the copy included). Entries whose row lies outside
    [0, B), and features outside [0, F), are skipped.

    CPU tensors (and HARMONY_FORCE_TORCH_OPS=1) take the torch reference
    below. _force_group overrides the lanes-per-feature choice (tests)."""
    B, C = P.shape
    nf = feat_ids.shape[0]
    if _use_hip(P):
        if B == 0 or nf == 0:
            return torch.zeros((C, F), dtype=torch.float32, device=P.device)
        group = _force_group or mlr_sparse_group(nf, feat_row.shape[0])
        Cp = (C + 3) // 4 * 4
        if (P.dtype != torch.float32 or P.stride(1) != 1 or P.stride(0) % 4
                or P.stride(0) < Cp or P.data_ptr() % 16):
            Ppad = torch.zeros((B, Cp), dtype=torch.float32, device=P.device)
            Ppad[:, :C] = P
            P = Ppad[:, :C]
        return _hip.mlr_sparse_grad(
            feat_ids.contiguous(), feat_ptr.contiguous(),
            feat_row.contiguous(), feat_val.contiguous(), P, int(F),
            int(group))
    dev = P.device
    seg = torch.repeat_interleave(torch.arange(nf, device=dev),
                                  feat_ptr[1:] - feat_ptr[:-1])
    r = feat_row.long()
    ok = (r >= 0) & (r < B)
    seg, r, v = seg[ok], r[ok], feat_val[ok]
    per_feat = torch.zeros((nf, C), dtype=torch.float32, device=dev)
    per_feat.index_add_(0, seg, v.unsqueeze(1) * P.float()[r])
    G = torch.zeros((C, F), dtype=torch.float32, device=dev)
    f = feat_ids.long()
    okf = (f >= 0) & (f < F)
    G[:, f[okf]] = per_feat[okf].t()
    return G


# ---------------------------------------------------------------------------
# K1: NMF gradient over a sparse batch (CSR by row)
# ---------------------------------------------------------------------------

def nmf_grad(L: torch.Tensor, R: torch.Tensor, row_ptr: torch.Tensor,
             col_idx: torch.Tensor, vals: torch.Tensor, lam: float,
             col_sorted=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """For each nonzero (i, j, v): e = L_i . R_j - v;
    lgrad_i += 2 e R_j, rgrad_j += 2 e L_i; plus L2 terms 2*lam*{L_i,R_j}
    per nonzero (reference NMFTrainer.updateGradient:328-367).
    L: [n_rows, k], CSR over rows: row_ptr [n_rows+1], col_idx/vals [nnz]
    (col_idx indexes R's rows). Returns (lgrad, rgrad, sq_err_sum).

    col_sorted: optional static precompute (perm, seg_ptr, row_sorted) — the
    column-sorted view of the nonzeros (seg_ptr covers ALL R rows) — enables
    the atomic-free two-pass kernel on GPU."""
    if _use_hip(L):
        if col_sorted is not None:
            perm, seg_ptr, row_sorted = col_sorted
            return tuple(_hip.nmf_grad_twopass(
                L.contiguous(), R.contiguous(), row_ptr.contiguous(),
                col_idx.contiguous(), vals.contiguous(), perm.contiguous(),
                seg_ptr.contiguous(), row_sorted.contiguous(), float(lam)))
        return tuple(_hip.nmf_grad(L.contiguous(), R.contiguous(),
                                   row_ptr.contiguous(), col_idx.contiguous(),
                                   vals.contiguous(), float(lam)))
    row_idx = torch.repeat_interleave(
        torch.arange(L.shape[0], device=L.device),
        row_ptr[1:] - row_ptr[:-1])
    Lr = L[row_idx]                       # [nnz, k]
    Rr = R[col_idx]
    e = (Lr * Rr).sum(dim=1) - vals       # [nnz]
    ge = (2.0 * e).unsqueeze(1)
    lcontrib = ge * Rr + 2.0 * lam * Lr
    rcontrib = ge * Lr + 2.0 * lam * Rr
    lgrad = torch.zeros_like(L)
    rgrad = torch.zeros_like(R)
    lgrad.index_add_(0, row_idx, lcontrib)
    rgrad.index_add_(0, col_idx, rcontrib)
    return lgrad, rgrad, (e * e).sum()


def nmf_step(L: torch.Tensor, l_lo: int, n: int, R_src: torch.Tensor,
             row_ptr: torch.Tensor, col: torch.Tensor, vals: torch.Tensor,
             col_sorted, rsrc_of: Optional[torch.Tensor],
             step: torch.Tensor, lam: float, max_val: float,
             want_lgrad: bool = False):
    """One NMF compute phase on the batch L[l_lo:l_lo+n]: the two-pass
    gradient of nmf_grad(col_sorted=...) plus the worker-side update
    L_new = clamp(L_batch - step * lgrad, 0, max_val) in the same kernel.

    col [nnz] names, per nonzero, a row of R_src; col_sorted = (perm,
    seg_ptr, row_sorted) is the column-sorted view with one segment per
    rgrad row; rsrc_of [n_uniq] maps an rgrad row to its R_src row (None:
    rgrad row j is R_src row j). So R_src is either the gathered
    [n_uniq, k] tensor with local col, or any larger table with rsrc_of.
    Index tensors are int32 on GPU. step is a 0-dim float tensor on L's
    device. L is not modified.
    Returns (L_new [n, k], rgrad [n_uniq, k], sq_err_sum[, lgrad])."""
    perm, seg_ptr, row_sorted = col_sorted
    if _use_hip(L):
        return tuple(_hip.nmf_step(
            L.contiguous(), int(l_lo), int(n), R_src.contiguous(), row_ptr,
            col, vals.contiguous(), perm, seg_ptr, row_sorted, rsrc_of, step, float(lam), float(max_val),
            bool(want_lgrad)))
    L_batch = L[l_lo:l_lo + n]
    lgrad, rgrad, sq = nmf_grad(L_batch, R_src, row_ptr.long(), col.long(),
                                vals, lam)
    if rsrc_of is not None:
        rgrad = rgrad[rsrc_of.long()]
    else:
        rgrad = rgrad[:seg_ptr.shape[0] - 1]
    L_new = (L_batch - step * lgrad).clamp_(0.0, max_val)
    if want_lgrad:
        return L_new, rgrad, sq, lgrad
    return L_new, rgrad, sq


# ---------------------------------------------------------------------------
# K7: LDA collapsed Gibbs sampling over a doc block
# ---------------------------------------------------------------------------

def lda_gibbs(doc_topic: torch.Tensor, word_topic: torch.Tensor,
              topic_sum: torch.Tensor, doc_offsets: torch.Tensor,
              word_ids: torch.Tensor, assignments: torch.Tensor,
              alpha: float, beta: float, num_vocabs: int, seed: int
              ) -> torch.Tensor:
    """One Gibbs sweep over the batch's tokens; returns new assignments.

    doc_topic: [n_docs, K] int32 (updated in place),
    word_topic: [n_words_in_batch, K] (pulled rows, LOCAL indices; treated as
    fixed within the sweep — batch-stale counts, see mlapps/lda.py),
    topic_sum: [K], doc_offsets: [n_docs+1] CSR over tokens, word_ids: local
    word index per token, assignments: [n_tokens] int32 (updated in place).

    p(k) ∝ (n_dk + α) (n_wk + β) / (n_k + V β)
    (reference SparseLDASampler.java:141-274's s/r/q bucket decomposition is a
    CPU sparsity optimization; on CDNA4 the dense K-way distribution is
    computed by a wave per document — see ops/csrc/lda.hip.)

    The torch path mirrors the device kernel: same counter-based RNG keyed by
    (seed, token index), same float32 probability terms, same "first k with
    cumsum > u" draw — CPU and GPU agree except at float summation-order
    tie-breaks (tests require >=99% identical samples + exact invariants)."""
    if _use_hip(word_topic):
        return _hip.lda_gibbs(doc_topic, word_topic, topic_sum, doc_offsets,
                              word_ids, assignments, float(alpha), float(beta),
                              int(num_vocabs), int(seed))
    from harmony_amd.ops.rng import rng_uniform

    n_docs = doc_topic.shape[0]
    inv_den = (1.0 / (topic_sum.float() + num_vocabs * beta)).float()   # [K]
    # Lockstep over token positions: docs advance one token per step so the
    # per-doc sequential dependency (n_dk) is honored while steps stay
    # vectorized over docs.
    lengths = doc_offsets[1:] - doc_offsets[:-1]
    max_len = int(lengths.max()) if n_docs else 0
    for pos in range(max_len):
        active = (lengths > pos).nonzero(as_tuple=True)[0]
        tok = doc_offsets[active] + pos
        w = word_ids[tok].long()
        old = assignments[tok].long()
        ar = torch.arange(active.shape[0])
        dt = doc_topic[active]
        dt[ar, old] -= 1
        probs = ((dt.float() + alpha) * (word_topic[w].float() + beta)
                 * inv_den)                                  # [n_active, K]
        tot = probs.sum(dim=1)
        u = rng_uniform(seed & 0xFFFFFFFF, tok.long()) * tot
        cdf = probs.cumsum(dim=1)
        new = torch.searchsorted(cdf, u.unsqueeze(1).to(cdf.dtype),
                                 right=True).squeeze(1)
        bad = new >= probs.shape[1]
        new = torch.where(bad, old, new)                     # numeric edge
        dt[ar, new] += 1
        doc_topic[active] = dt
        assignments[tok] = new.to(assignments.dtype)
    return assignments


def lda_apply_pairs(shard: torch.Tensor, rows: torch.Tensor,
                    old_t: torch.Tensor, new_t: torch.Tensor) -> None:
    """Apply (row, old_topic, new_topic) ±1 count pairs to the word-topic
    shard (the reference's TopicChanges wire format — 12 B per changed token
    instead of a dense K-int row per touched word)."""
    if _use_hip(shard):
        _hip.lda_apply_pairs(shard, rows.contiguous(),
                             old_t.contiguous(), new_t.contiguous())
        return
    K = shard.shape[1]
    flat = shard.view(-1)
    ones = torch.ones(rows.shape[0], dtype=shard.dtype, device=shard.device)
    flat.scatter_add_(0, rows * K + old_t.long(), -ones)
    flat.scatter_add_(0, rows * K + new_t.long(), ones)


def _butterfly_sum64(x: torch.Tensor) -> torch.Tensor:
    """Bitwise replica of the wave64 shfl_xor butterfly sum over dim -1."""
    idx = torch.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        x = x + x[..., idx ^ m]
    return x[..., 0]


def _vose_serial(pr, al, lk, n):
    """Python replica of the device vose_serial (same order)."""
    small_top, large_top = -1, -1
    for k in range(n - 1, -1, -1):
        if float(pr[k]) < 1.0:
            lk[k] = small_top
            small_top = k
        else:
            lk[k] = large_top
            large_top = k
    while small_top >= 0 and large_top >= 0:
        sm = small_top
        small_top = lk[sm]
        lg = large_top
        al[sm] = lg
        # float32 at every step, as on the device: summed in double and
        # rounded once, the remainder can land one ulp off the kernel's
        rem_t = (pr[lg] + pr[sm]) - 1.0
        pr[lg] = rem_t
        rem = float(rem_t)
        large_top = lk[lg]
        if rem < 1.0:
            lk[lg] = small_top
            small_top = lg
        else:
            lk[lg] = large_top
            large_top = lg
    while large_top >= 0:
        lg = large_top
        large_top = lk[lg]
        pr[lg] = 1.0
        al[lg] = lg
    while small_top >= 0:
        sm = small_top
        small_top = lk[sm]
        pr[sm] = 1.0
        al[sm] = sm


def lda_alias_build(word_topic: torch.Tensor, topic_sum: torch.Tensor,
                    beta: float, num_vocabs: int):
    """Two-level per-word alias tables over the (batch-stale) word factor
    q_w(k) = (n_wk + b)/(n_k + V b): a 64-entry top alias over lane-segment
    masses + per-segment aliases (exact — see ops/csrc/lda_alias.hip).
    Returns (prob, alias, top_prob, top_alias, qsum, invden). Construction
    is deterministic and float-order-matched to the device kernel
    (butterfly total, ascending serial segment sums) so CPU and GPU build
    bit-identical tables."""
    if _use_hip(word_topic):
        return tuple(_hip.lda_alias_build(word_topic.contiguous(),
                                          topic_sum.contiguous(),
                                          float(beta), int(num_vocabs)))
    rows, K = word_topic.shape
    W = 64
    assert K % W == 0, "alias sampler requires K % 64 == 0"
    S = K // W
    invden = (1.0 / (topic_sum.float() + num_vocabs * beta)).contiguous()
    c = word_topic.float() + beta
    p = c * invden                                       # [rows, K]
    pseg = p.view(rows, W, S)
    # the kernel accumulates the segment mass with a fused multiply-add
    # (c * invden is not rounded before the add); a float32 product is exact
    # in double, so one double add rounded to float32 reproduces it
    cseg = c.view(rows, W, S).double()
    iseg = invden.view(W, S).double()
    seg_mass = torch.zeros(rows, W)
    for i in range(S):                                   # ascending = kernel
        seg_mass = (cseg[:, :, i] * iseg[:, i] + seg_mass.double()).float()
    total = _butterfly_sum64(seg_mass)
    qv = (p * (1.0 / total).unsqueeze(1)).contiguous()   # encoded density
    # tensor / tensor: torch evaluates `S / seg_mass` as reciprocal * S,
    # which rounds twice and differs from the kernel's one division unless
    # S is a power of two
    sscale = torch.where(seg_mass > 0,
                         torch.full_like(seg_mass, float(S)) / seg_mass,
                         torch.zeros_like(seg_mass))
    prob = (pseg * sscale.unsqueeze(2)).reshape(rows, K).contiguous()
    alias = torch.empty((rows, K), dtype=torch.int32)
    top_prob = (seg_mass * W / total.unsqueeze(1)).contiguous()
    top_alias = torch.empty((rows, W), dtype=torch.int32)
    lk = [0] * max(K, W)
    for r in range(rows):
        for g in range(W):
            _vose_serial(prob[r, g * S:(g + 1) * S],
                         alias[r, g * S:(g + 1) * S], lk, S)
        _vose_serial(top_prob[r], top_alias[r], lk, W)
    return prob, alias, top_prob, top_alias, qv, total, invden


def lda_mh_wave(doc_topic: torch.Tensor, word_topic: torch.Tensor,
                invden: torch.Tensor, prob: torch.Tensor,
                alias: torch.Tensor, top_prob: torch.Tensor,
                top_alias: torch.Tensor, qv: torch.Tensor,
                doc_offsets: torch.Tensor, word_ids: torch.Tensor,
                assignments: torch.Tensor, alpha: float, beta: float,
                seed: int) -> torch.Tensor:
    """Wave-per-doc MH sweep (K7c): 64 lanes cooperate on each doc with
    the doc-topic row shared in LDS via atomics — within-doc token
    updates are approximately parallel (acceptance may read slightly
    stale counts; standard GPU-LDA relaxation, convergence validated by
    scripts/lda_convergence.py). On CPU this falls back to the SERIAL
    sampler: the wave kernel's interleaving is hardware-scheduling
    dependent, so there is no bit-exact oracle — the two are compared
    statistically, not elementwise."""
    if _use_hip(word_topic):
        return _hip.lda_mh_wave(doc_topic, word_topic, invden, prob, alias,
                                top_prob, top_alias, qv, doc_offsets,
                                word_ids, assignments, float(alpha),
                                float(beta), int(seed))
    return lda_mh(doc_topic, word_topic, invden, prob, alias, top_prob,
                  top_alias, qv, doc_offsets, word_ids, assignments,
                  alpha, beta, seed)


def lda_mh(doc_topic: torch.Tensor, word_topic: torch.Tensor,
           invden: torch.Tensor, prob: torch.Tensor, alias: torch.Tensor,
           top_prob: torch.Tensor, top_alias: torch.Tensor,
           qv: torch.Tensor, doc_offsets: torch.Tensor,
           word_ids: torch.Tensor, assignments: torch.Tensor, alpha: float,
           beta: float, seed: int) -> torch.Tensor:
    """One Metropolis-Hastings alias sweep (K7b; proposal/acceptance
    derivation in ops/csrc/lda_alias.hip). Same stationary distribution as
    the exact sampler under the batch-stale word-topic snapshot; O(1) per
    token. Torch path mirrors the kernel's RNG and float math."""
    if _use_hip(word_topic):
        return _hip.lda_mh(doc_topic, word_topic, invden, prob, alias,
                           top_prob, top_alias, qv, doc_offsets, word_ids,
                           assignments, float(alpha), float(beta), int(seed))
    from harmony_amd.ops.rng import rng_uniform

    K = word_topic.shape[1]
    W = 64
    S = K // W
    lengths = doc_offsets[1:] - doc_offsets[:-1]
    n_docs = doc_topic.shape[0]
    max_len = int(lengths.max()) if n_docs else 0
    aK = alpha * K
    for pos in range(max_len):
        active = (lengths > pos).nonzero(as_tuple=True)[0]
        tok = doc_offsets[active] + pos
        w = word_ids[tok].long()
        s = assignments[tok].long()
        ar = torch.arange(active.shape[0])
        dt = doc_topic[active]
        dt[ar, s] -= 1
        c0 = (tok * 8).long()
        sd = seed & 0xFFFFFFFF
        # word proposal: two-level alias draw
        u1 = rng_uniform(sd, c0) * W
        gb = u1.long().clamp_(max=W - 1)
        g = torch.where(u1 - gb.float() < top_prob[w, gb], gb,
                        top_alias[w, gb].long())
        u2 = rng_uniform(sd, c0 + 6) * S
        eb = u2.long().clamp_(max=S - 1)
        ecol = g * S + eb
        t1 = g * S + torch.where(u2 - eb.float() < prob[w, ecol], eb,
                                 alias[w, ecol].long())
        # stale-table-safe acceptance: pi from the CURRENT snapshot, q from
        # the table's encoded density (cancels when the table is fresh)
        pi_s = (dt[ar, s].float() + alpha) * \
            (word_topic[w, s].float() + beta) * invden[s]
        pi_t = (dt[ar, t1].float() + alpha) * \
            (word_topic[w, t1].float() + beta) * invden[t1]
        a1 = (pi_t * qv[w, s]) / (pi_s * qv[w, t1])
        s = torch.where(rng_uniform(sd, c0 + 1) < a1, t1, s)
        # doc proposal
        Ld = lengths[active].float()
        uni = rng_uniform(sd, c0 + 2) < (aK / (aK + Ld))
        t_uni = (rng_uniform(sd, c0 + 3) * K).long().clamp_(max=K - 1)
        j = doc_offsets[active] + (rng_uniform(sd, c0 + 4) * Ld).long()
        j = torch.minimum(j, doc_offsets[active] + lengths[active] - 1)
        t_copy = torch.where(j == tok, s, assignments[j].long())
        t2 = torch.where(uni, t_uni, t_copy)
        nds = dt[ar, s].float()
        ndt = dt[ar, t2].float()
        qs = nds + 1.0 + alpha
        qt = ndt + (t2 == s).float() + alpha
        pis = (nds + alpha) * (word_topic[w, s].float() + beta) * invden[s]
        pit = (ndt + alpha) * (word_topic[w, t2].float() + beta) * invden[t2]
        a2 = (pit * qs) / (pis * qt)
        s = torch.where(rng_uniform(sd, c0 + 5) < a2, t2, s)
        dt[ar, s] += 1
        doc_topic[active] = dt
        assignments[tok] = s.to(assignments.dtype)
    return assignments


def lda_apply_all(shard, word_rows, old_t, new_t, summary_row: int) -> None:
    """Fused single-owner update: per token, if the topic changed, apply
    ±1 to the word row and the summary row (K9; replaces the whole
    nonzero/gather/bincount/scatter pipeline on the local path)."""
    if _use_hip(shard):
        _hip.lda_apply_all(shard, word_rows.contiguous(), old_t.contiguous(),
                           new_t.contiguous(), int(summary_row))
        return
    changed = (old_t != new_t)
    rows = word_rows[changed]
    o = old_t[changed].long()
    nw = new_t[changed].long()
    K = shard.shape[1]
    flat = shard.view(-1)
    ones = torch.ones(rows.shape[0], dtype=shard.dtype, device=shard.device)
    flat.scatter_add_(0, rows * K + o, -ones)
    flat.scatter_add_(0, rows * K + nw, ones)
    srow = summary_row * K
    flat.scatter_add_(0, srow + o, -ones)
    flat.scatter_add_(0, srow + nw, ones)


# ---------------------------------------------------------------------------
# K7e: held-out fold-in (document completion) against the frozen table
# ---------------------------------------------------------------------------

LDA_FOLDIN_MAX_TOPICS = 1024        # ops/csrc/lda_foldin.hip: 64 lanes x 16
_FOLDIN_CHUNK_ELEMS = 1 << 22       # torch path: floats per [pairs, K] chunk


def _foldin_check(ptr: torch.Tensor, word: torch.Tensor, cnt: torch.Tensor,
                  num_vocabs: int) -> torch.Tensor:
    ok = (ptr[0] == 0) & (ptr[-1] == word.shape[0]) \
        & (ptr[1:] >= ptr[:-1]).all()
    if word.shape[0]:
        ok = ok & (word.min() >= 0) & (word.max() < num_vocabs)
    if cnt.shape[0] != word.shape[0]:
        raise ValueError("lda_foldin: one count per (word, count) pair")
    return ok


def lda_foldin(word_topic: torch.Tensor, topic_sum: torch.Tensor,
               obs_ptr: torch.Tensor, obs_word: torch.Tensor,
               obs_cnt: torch.Tensor, sc_ptr: torch.Tensor,
               sc_word: torch.Tensor, sc_cnt: torch.Tensor,
               alpha: float, beta: float, num_vocabs: int, iters: int
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fold held-out documents in against the frozen model and score them
    (K7e, ops/csrc/lda_foldin.hip): (theta float32 [D, K], ll float32 [D]).

    word_topic: int32 [>= num_vocabs, K], contiguous (the [:V] view of the
    pulled table qualifies), topic_sum: int32 [K]; both are read as they
    are, no float copy of the table is made. Document d owns the (word,
    count) pairs obs_ptr[d]:obs_ptr[d+1] of obs_word (int64) / obs_cnt
    (int32), its observed half, and the pairs sc_ptr[d]:sc_ptr[d+1] of
    sc_word / sc_cnt, its scored half; the ptr tensors are int64 [D + 1].

      phi[w,k] = (n_wk + beta) / (n_k + V beta),         theta^0_k = 1/K
      iters times:  m_k = sum_obs c theta_k phi[w,k] / sum_j theta_j phi[w,j]
                    theta_k = (m_k + alpha) / (N_obs + K alpha)
      ll = sum_scored c log sum_k theta_k phi[w,k]

    All of it in float32, pairs in their stored order. The kernel couples no
    two documents, so its result for a document is bitwise the same wherever
    the document stands in the batch. CPU tensors, HARMONY_FORCE_TORCH_OPS=1
    and K > LDA_FOLDIN_MAX_TOPICS take the tensor ops below, in chunks of
    pairs, so that no [all_pairs, K] tensor is built; on a GPU their
    index_add_ sums in no fixed order. D = 0 returns empty tensors without a
    launch. A word id outside [0, num_vocabs) raises ValueError."""
    K = int(word_topic.shape[1])
    D = int(obs_ptr.shape[0]) - 1
    dev = word_topic.device
    if D < 0 or sc_ptr.shape[0] != D + 1:
        raise ValueError("lda_foldin: obs_ptr and sc_ptr must be [D + 1]")
    if word_topic.shape[0] < num_vocabs or topic_sum.shape[0] != K:
        raise ValueError("lda_foldin: word_topic [>= num_vocabs, K] and "
                         "topic_sum [K] expected")
    if iters < 0:
        raise ValueError("lda_foldin: iters must be >= 0")
    if D == 0:
        return (torch.empty(0, K, dtype=torch.float32, device=dev),
                torch.empty(0, dtype=torch.float32, device=dev))
    if not bool(_foldin_check(obs_ptr, obs_word, obs_cnt, num_vocabs)
                & _foldin_check(sc_ptr, sc_word, sc_cnt, num_vocabs)):
        raise ValueError("lda_foldin: a word id outside [0, num_vocabs) or "
                         "pair offsets that do not match the pair arrays")
    if _use_hip(word_topic) and K <= LDA_FOLDIN_MAX_TOPICS:
        theta, ll = _hip.lda_foldin(
            word_topic, topic_sum.contiguous(), obs_ptr.contiguous(),
            obs_word.contiguous(), obs_cnt.contiguous(), sc_ptr.contiguous(),
            sc_word.contiguous(), sc_cnt.contiguous(), float(alpha),
            float(beta), int(num_vocabs), int(iters))
        return theta, ll

    invden = 1.0 / (topic_sum.float() + num_vocabs * beta)          # [K]
    docs = torch.arange(D, device=dev)
    obs_doc = torch.repeat_interleave(docs, obs_ptr[1:] - obs_ptr[:-1])
    sc_doc = torch.repeat_interleave(docs, sc_ptr[1:] - sc_ptr[:-1])
    n_obs = torch.zeros(D, dtype=torch.int64, device=dev).index_add_(
        0, obs_doc, obs_cnt.long())
    den = (n_obs.float() + float(K) * alpha).unsqueeze(1)
    step = max(1, _FOLDIN_CHUNK_ELEMS // K)

    def terms(ti, word, doc, lo):
        """theta_k phi[w,k] of the pairs lo:lo+step and their totals."""
        val = ti[doc[lo:lo + step]] * \
            (word_topic[word[lo:lo + step]].float() + beta)
        return val, val.sum(dim=1)

    one = torch.ones((), dtype=torch.float32, device=dev)
    theta = (one / torch.tensor(float(K), dtype=torch.float32, device=dev)
             ).expand(D, K).contiguous()
    for _ in range(int(iters)):
        ti = theta * invden
        m = torch.zeros(D, K, dtype=torch.float32, device=dev)
        for lo in range(0, obs_word.shape[0], step):
            val, tot = terms(ti, obs_word, obs_doc, lo)
            scale = obs_cnt[lo:lo + step].float() / tot
            m.index_add_(0, obs_doc[lo:lo + step], val * scale.unsqueeze(1))
        theta = (m + alpha) / den
    ti = theta * invden
    ll = torch.zeros(D, dtype=torch.float32, device=dev)
    for lo in range(0, sc_word.shape[0], step):
        _val, tot = terms(ti, sc_word, sc_doc, lo)
        ll.index_add_(0, sc_doc[lo:lo + step],
                      sc_cnt[lo:lo + step].float() * torch.log(tot))
    return theta, ll


# K7d: packed per-segment tables for the wave sampler. rec[rows][64][4*S]
# int32 holds {reserved[S] | prob[S] | qv[S] | alias[S]} per (word, lane
# segment), S = K/64; top[rows][64][2] int32 holds {top_prob, top_alias}.
# Float fields are stored as their bits. The counts stay in the dense
# pulled snapshot (profiles/r04_lda_step.md: a count slot in the record,
# refreshed every step, lost to it).
LDA_PACKED_S = (1, 2, 4, 8)


def lda_packed_supported(num_topics: int) -> bool:
    return num_topics % 64 == 0 and num_topics // 64 in LDA_PACKED_S


def lda_packed_alloc(rows: int, num_topics: int, device):
    """Zeroed (rec, top) for `rows` words."""
    assert lda_packed_supported(num_topics), num_topics
    S = num_topics // 64
    rec = torch.zeros(rows, 64, 4 * S, dtype=torch.int32, device=device)
    top = torch.zeros(rows, 64, 2, dtype=torch.int32, device=device)
    return rec, top


def _rows32(src_rows):
    if src_rows is None:
        return None
    return src_rows.to(torch.int32).contiguous()


def lda_alias_build_packed(src: torch.Tensor, src_rows, topic_sum,
                           beta: float, num_vocabs: int, rec: torch.Tensor,
                           top: torch.Tensor):
    """lda_alias_build over rows `src[src_rows]` (or `src[:rows]` when
    src_rows is None; the former reads a table shard in place), written
    into the packed tables. Stored values are bit-identical to
    lda_alias_build's. Returns (invden, qsum)."""
    if _use_hip(src):
        return tuple(_hip.lda_alias_build_packed(
            src, _rows32(src_rows), topic_sum.contiguous(), float(beta),
            int(num_vocabs), rec, top))
    rows, S = rec.shape[0], rec.shape[2] // 4
    wt = src[src_rows.long()] if src_rows is not None else src[:rows]
    prob, alias, tprob, talias, qv, qsum, invden = lda_alias_build(
        wt, topic_sum, beta, num_vocabs)
    r = rec.view(rows, 64, 4, S)
    r[:, :, 1] = prob.view(torch.int32).view(rows, 64, S)
    r[:, :, 2] = qv.view(torch.int32).view(rows, 64, S)
    r[:, :, 3] = alias.view(rows, 64, S)
    top[:, :, 0] = tprob.view(torch.int32)
    top[:, :, 1] = talias
    return invden, qsum


def lda_unpack_tables(rec: torch.Tensor, top: torch.Tensor):
    """The legacy arrays held by the packed tables:
    (prob, alias, top_prob, top_alias, qv)."""
    rows, S = rec.shape[0], rec.shape[2] // 4
    K = 64 * S
    r = rec.view(rows, 64, 4, S)

    def field(i):
        return r[:, :, i].reshape(rows, K).contiguous()

    return (field(1).view(torch.float32), field(3),
            top[:, :, 0].contiguous().view(torch.float32),
            top[:, :, 1].contiguous(), field(2).view(torch.float32))


def lda_mh_wave_packed(doc_topic: torch.Tensor, word_topic: torch.Tensor,
                       rec: torch.Tensor, top: torch.Tensor,
                       invden: torch.Tensor, doc_offsets: torch.Tensor,
                       word_ids: torch.Tensor, assignments: torch.Tensor,
                       alpha: float, beta: float, seed: int, shard=None,
                       row_of_local=None,
                       summary_row: int = -1) -> torch.Tensor:
    """lda_mh_wave reading the packed tables (word_ids int32). With `shard`
    the sweep also applies every changed token's -1/+1 to
    shard[row_of_local[word]] and to shard[summary_row] (what lda_apply_all
    does from an old/new copy of the assignments): it samples from the
    snapshot word_topic, never from the shard, so the result is the same.
    On CPU this is the serial sampler over the unpacked tables, as for
    lda_mh_wave."""
    if _use_hip(rec):
        return _hip.lda_mh_wave_packed(
            doc_topic, word_topic, rec, top, invden, doc_offsets, word_ids,
            assignments, float(alpha), float(beta), int(seed), shard,
            _rows32(row_of_local) if shard is not None else None,
            int(summary_row))
    prob, alias, tprob, talias, qv = lda_unpack_tables(rec, top)
    old = assignments.clone() if shard is not None else None
    lda_mh(doc_topic, word_topic, invden, prob, alias, tprob, talias, qv,
           doc_offsets, word_ids.long(), assignments, alpha, beta, seed)
    if shard is not None:
        lda_apply_all(shard, row_of_local.long()[word_ids.long()], old,
                      assignments, summary_row)
    return assignments


# ---------------------------------------------------------------------------
# K3/K9: fused owner-side update application ("server" compute)
# ---------------------------------------------------------------------------

# update-function name (et.update_functions) -> device kernel mode
_APPLY_MODES = {"add": 0, "assign": 1, "nmf_sgd": 2, "lda_counts": 3}


def gbt_hist(bins: torch.Tensor, resid: torch.Tensor, node: torch.Tensor,
             n_nodes: int, num_bins: int
             ) -> Tuple[torch.Tensor, torch.Tensor]:
    """GBT level histogram (K10): per-(node, feature, bin) sample counts and
    residual sums for one tree level. Reference GBTTrainer.java:244+ scans
    sorted raw values per node/feature on the CPU; the GPU histogram method
    (pre-quantized bins) is the standard redesign. Returns (cnt, sum),
    each float32 [n_nodes, F, num_bins]."""
    B, F = bins.shape
    if _use_hip(bins) and n_nodes * num_bins <= 8192:
        cnt = torch.zeros(n_nodes, F, num_bins, device=bins.device)
        s = torch.zeros_like(cnt)
        _hip.gbt_hist(bins.int().contiguous(), resid.float().contiguous(),
                      node.int().contiguous(), cnt, s)
        return cnt, s
    idx = (node.long().unsqueeze(1) * F * num_bins
           + torch.arange(F, device=bins.device) * num_bins + bins)
    cnt = torch.zeros(n_nodes * F * num_bins, device=bins.device)
    s = torch.zeros_like(cnt)
    cnt.scatter_add_(0, idx.reshape(-1),
                     torch.ones(B, 1, device=bins.device).expand(B, F)
                     .reshape(-1))
    s.scatter_add_(0, idx.reshape(-1),
                   resid.float().unsqueeze(1).expand(B, F).reshape(-1))
    return (cnt.view(n_nodes, F, num_bins), s.view(n_nodes, F, num_bins))


GBT_HIST_MAX_CELLS = 8192    # K10 / K10s: n_nodes * nb cells per feature in LDS


def gbt_hist_sparse(feat_ptr: torch.Tensor, feat_row: torch.Tensor,
                    feat_bin: torch.Tensor, feat_idx: torch.Tensor,
                    zero_bin: torch.Tensor, resid: torch.Tensor,
                    node: torch.Tensor, n_nodes: int, num_bins: int
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """GBT level histogram over a binned sparse batch (K10s,
    ops/csrc/gbt_hist_sparse.hip). The first five arguments are the column
    side of a mlapps.sparse_bins.SparseBins: feat_ptr int64 [nf+1],
    feat_row / feat_bin / feat_idx int32 [nnz] (row, bin and compact feature
    index of every entry, grouped by feature), zero_bin int32 [nf] (the bin
    of an absent entry). resid [B]; node [B] level-local node per sample.
    Returns (cnt, sum), each float32 [n_nodes, nf, num_bins], over the
    PRESENT features in feat_ids order.

    Formula: the entries are scatter-added into their (node, feature, bin)
    cells; then every (node, feature) adds node_cnt - sum_b cnt and
    node_sum - sum_b sum into the feature's zero bin, where node_cnt and
    node_sum are the per-node sample count and residual sum (one scatter
    here). That is the share of the samples with no entry in the column.

    CPU tensors, HARMONY_FORCE_TORCH_OPS=1 and levels wider than
    n_nodes * num_bins = 8192 take the tensor ops below, which compute the
    same formula and are the kernel's test oracle. nf == 0 launches nothing.
    """
    dev = resid.device
    nf = feat_ptr.shape[0] - 1
    resid = resid.float().contiguous()
    node_l = node.long()
    node_cnt = torch.zeros(n_nodes, device=dev).scatter_add_(
        0, node_l, torch.ones_like(resid))
    node_sum = torch.zeros(n_nodes, device=dev).scatter_add_(
        0, node_l, resid)
    if _use_hip(resid) and n_nodes * num_bins <= GBT_HIST_MAX_CELLS:
        cnt, s = _hip.gbt_hist_sparse(
            feat_ptr.contiguous(), feat_row.contiguous(),
            feat_bin.contiguous(), feat_idx.contiguous(),
            zero_bin.contiguous(), resid, node.int().contiguous(),
            node_cnt, node_sum, int(num_bins))
        return cnt, s
    rows = feat_row.long()
    cell = ((node_l[rows] * nf + feat_idx.long()) * num_bins
            + feat_bin.long())
    cnt = torch.zeros(n_nodes * nf * num_bins, device=dev)
    s = torch.zeros_like(cnt)
    cnt.scatter_add_(0, cell, torch.ones(cell.shape[0], device=dev))
    s.scatter_add_(0, cell, resid[rows])
    cnt = cnt.view(n_nodes, nf, num_bins)
    s = s.view(n_nodes, nf, num_bins)
    zb = zero_bin.long().view(1, nf, 1).expand(n_nodes, nf, 1)
    cnt.scatter_add_(2, zb, node_cnt.view(-1, 1, 1)
                     - cnt.sum(dim=2, keepdim=True))
    s.scatter_add_(2, zb, node_sum.view(-1, 1, 1)
                   - s.sum(dim=2, keepdim=True))
    return cnt, s


GBT_NO_CANDIDATE = -1e30     # gain of an invalid split candidate
GBT_MIN_GAIN = 1e-12         # a split must gain more than this
GBT_SPLIT_MAX_BINS = 64      # K10b: one lane per bin or category


def gbt_best_split(cnt: torch.Tensor, s: torch.Tensor, ftype: torch.Tensor,
                   lam: float) -> Tuple[torch.Tensor, torch.Tensor,
                                        torch.Tensor, torch.Tensor]:
    """Best split per node of one tree level from its K10 histograms (K10b,
    ops/csrc/gbt_split.hip; reference GBTTrainer.java bestSplitRealFeature /
    bestSplitLabelFeature). cnt, s: float32 [n_nodes, F, nb]; ftype: int32
    [F], 0 = continuous, non-zero = categorical.
    Returns (feature int32, threshold int32, mask int64, gain float32), each
    [n_nodes].

    Continuous feature: candidates b = 0..nb-2, left = bins <= b. Categorical
    feature: the live categories (cnt > 0) ordered by mean s / cnt ascending,
    ties by category id; candidates p = 1..L-1, left = the first p of that
    order, and the mask holds exactly the bits of the others. A candidate is
    valid iff both sides have cnt > 0. gain = sl^2/(cl+lam) + sr^2/(cr+lam)
    - stot^2/(ctot+lam); the best is the largest over all features and
    candidates, ties to the lowest feature, then the lowest candidate. A
    continuous winner gives threshold = b, mask = 0; a categorical one
    threshold = -2. No valid candidate, or a best gain <= 1e-12, gives
    feature 0, threshold -1, mask 0, gain 0.

    CPU tensors, HARMONY_FORCE_TORCH_OPS=1 and nb > 64 take the tensor ops
    below, which are the kernel's test oracle."""
    n_nodes, F, nb = cnt.shape
    if _use_hip(cnt) and nb <= GBT_SPLIT_MAX_BINS:
        return tuple(_hip.gbt_best_split(
            cnt.contiguous(), s.contiguous(),
            ftype.to(device=cnt.device, dtype=torch.int32).contiguous(),
            float(lam)))
    dev = cnt.device
    if nb < 2:
        no = torch.zeros(n_nodes, dtype=torch.int32, device=dev)
        return (no, no - 1, no.long(), no.float())
    cat = (ftype.to(dev) != 0).view(1, F, 1)
    live = cnt > 0
    ident = torch.arange(nb, device=dev).expand(n_nodes, F, nb)
    # (mean, id) order of the live categories, dead ones behind them
    mean = torch.where(live, s / cnt, torch.full_like(s, float("inf")))
    order = torch.where(cat, mean.sort(dim=2, stable=True).indices, ident)
    ccum = cnt.gather(2, order).cumsum(dim=2)
    scum = s.gather(2, order).cumsum(dim=2)
    ctot, stot = ccum[:, :, -1:], scum[:, :, -1:]
    cl, sl = ccum[:, :, :-1], scum[:, :, :-1]
    cr, sr = ctot - cl, stot - sl
    gain = (sl * sl / (cl + lam) + sr * sr / (cr + lam)
            - stot * stot / (ctot + lam))
    gain = torch.where((cl > 0) & (cr > 0), gain,
                       torch.full_like(gain, GBT_NO_CANDIDATE))
    flat = gain.reshape(n_nodes, -1)
    best_gain = flat.max(dim=1).values
    pos = torch.arange(flat.shape[1], device=dev).expand_as(flat)
    best = torch.where(flat == best_gain.unsqueeze(1), pos,
                       torch.full_like(pos, flat.shape[1])).min(dim=1).values
    bf = best // (nb - 1)
    bp = best % (nb - 1)
    split = best_gain > GBT_MIN_GAIN
    wcat = split & cat.view(F)[bf]
    # right side of the winner: live categories ranked behind candidate bp
    sel = bf.view(n_nodes, 1, 1).expand(n_nodes, 1, nb)
    rank = torch.empty_like(order).scatter_(2, order, ident)
    right = (live.gather(1, sel).squeeze(1)
             & (rank.gather(1, sel).squeeze(1) > bp.unsqueeze(1)))
    # distinct bits, so the sum is their union (bit 63 is the sign bit); a
    # category id above 63 has no bit and always goes left
    ids = torch.arange(nb, device=dev)
    bit = (torch.ones(nb, dtype=torch.int64, device=dev)
           << ids.clamp(max=63)) * (ids < 64)
    mask = (right.long() * bit).sum(dim=1)
    zero = torch.zeros_like(best)
    return (torch.where(split, bf, zero).to(torch.int32),
            torch.where(wcat, zero - 2,
                        torch.where(split, bp, zero - 1)).to(torch.int32),
            torch.where(wcat, mask, zero),
            torch.where(split, best_gain, torch.zeros_like(best_gain)))


GBT_PREDICT_MAX_DEPTH = 8       # K10p: deeper trees take the torch loop
GBT_PREDICT_LDS_WORDS = 8192    # K10p: words of staged trees per LDS group


def gbt_predict_group_trees(row_len: int) -> int:
    """Trees K10p stages in LDS at a time, for rows of row_len words as the
    kernel sees them (a SparseBins batch adds 2^d - 1 words to a row)."""
    return GBT_PREDICT_LDS_WORDS // row_len


def gbt_forest_check(forest: torch.Tensor, depth: int, num_features: int
                     ) -> torch.Tensor:
    """The host copy of a packed forest (gbt.encode_trees), checked: int32
    [T, row] with a row length that fits `depth` (with or without the mask
    words) and every feature index in 0 .. num_features - 1, else
    ValueError. A restored forest may come from a job with another F; it
    must never become an out-of-bounds read."""
    ni = (1 << depth) - 1
    base = 1 + 2 * ni + (1 << depth)
    host = forest.cpu()
    if host.dim() != 2 or host.dtype != torch.int32 or \
            host.shape[1] not in (base, base + 2 * ni):
        raise ValueError(
            f"packed forest {tuple(host.shape)} {host.dtype}: a depth-"
            f"{depth} row has {base} or {base + 2 * ni} int32 words")
    feat = host[:, 1:1 + ni]
    if feat.numel() and (int(feat.min()) < 0
                         or int(feat.max()) >= num_features):
        raise ValueError(
            f"packed forest: feature index {int(feat.min())}.."
            f"{int(feat.max())} outside 0..{num_features - 1}")
    return host


def gbt_forest_predict(bins, forest: torch.Tensor, depth: int,
                       step_size: float) -> torch.Tensor:
    """step_size * the prediction of a packed forest for binned rows (K10p,
    ops/csrc/gbt_predict.hip): float32 [B]. bins: dense int64 [B, F] bins or
    a mlapps.sparse_bins.SparseBins; forest: the int32 [T, row] tensor of
    gbt.encode_trees, on any device (it is checked on the host by
    gbt_forest_check before anything is launched, then copied once).

    Formula, GBTTrainer._forest_pred from an empty cache: pred = 0, then for
    each tree in forest order pred = pred + fp32(step_size) * leaf, one
    rounded multiply and one rounded add per tree; the leaf is found by
    gbt._route_right per level. A SparseBins row uses SparseBins.bin_of.

    CPU tensors, HARMONY_FORCE_TORCH_OPS=1 and depth > 8 take the torch loop
    below (GBTree.predict_bins per tree), which is the kernel's test oracle;
    the kernel's result is bit-identical to it."""
    from harmony_amd.mlapps.sparse_bins import SparseBins

    B, F = bins.shape
    dev = bins.device
    host = gbt_forest_check(forest, depth, F)
    T = host.shape[0]
    if not (_use_hip(bins.keys if isinstance(bins, SparseBins) else bins)
            and depth <= GBT_PREDICT_MAX_DEPTH):
        from harmony_amd.mlapps.gbt import decode_trees

        pred = torch.zeros(B, dtype=torch.float32, device=dev)
        for _key, tree in decode_trees(host, depth):
            pred = pred + step_size * tree.predict_bins(bins)
        return pred
    if B == 0 or T == 0:
        return torch.zeros(B, dtype=torch.float32, device=dev)
    packed = host.to(dev)
    if not isinstance(bins, SparseBins):
        return _hip.gbt_forest_predict(
            bins.long().contiguous(), packed, int(depth), float(step_size),
            int(F), None, None, None)
    # per (tree, node), independent of the row: the zero bin of the node's
    # feature, 0 for a feature absent from the batch (SparseBins.bin_of)
    ni = (1 << depth) - 1
    feat = packed[:, 1:1 + ni].long()
    ids = bins.feat_ids.long()
    nf = ids.shape[0]
    if nf:
        k = torch.searchsorted(ids, feat).clamp_(max=nf - 1)
        zb = torch.where(ids[k] == feat, bins.zero_bin[k],
                         torch.zeros_like(bins.zero_bin[k]))
    else:
        zb = torch.zeros_like(feat, dtype=torch.int32)
    row_ptr = torch.searchsorted(
        bins.keys, torch.arange(B + 1, dtype=torch.int64, device=dev) * F)
    return _hip.gbt_forest_predict(
        None, torch.cat([packed, zb.to(torch.int32)], dim=1).contiguous(),
        int(depth), float(step_size), int(F), bins.keys.contiguous(),
        bins.key_bin.contiguous(), row_ptr)


def lasso_cd(X: torch.Tensor, r: torch.Tensor, w: torch.Tensor,
             col_sq: torch.Tensor, lam_n: float
             ) -> Tuple[torch.Tensor, torch.Tensor]:
    """One full cyclic coordinate-descent sweep (K11): for each coordinate
    the closed-form soft-threshold update (reference LassoTrainer.java:
    164-190), residual maintained incrementally. Returns (w_new, r_new);
    inputs are not mutated. GPU: single persistent workgroup, residual in
    LDS (ops/csrc/lasso.hip); CPU: the tensor-op loop."""
    F = X.shape[1]
    w = w.clone()
    r = r.clone()
    if _use_hip(X) and X.shape[0] + 17 <= 16384:
        Xt = getattr(X, "_harmony_xt", None)
        if Xt is None:
            Xt = X.t().contiguous()
            X._harmony_xt = Xt          # batches are static per block
        _hip.lasso_cd(Xt, r, w, col_sq.contiguous(), float(lam_n))
        return w, r
    for i in range(F):
        xi = X[:, i]
        c = xi @ r + w[i] * col_sq[i]
        wn = (torch.clamp(c.abs() - lam_n, min=0.0) * torch.sign(c)
              / col_sq[i])
        r = r + xi * (w[i] - wn)
        w[i] = wn
    return w, r


# ---------------------------------------------------------------------------
# K11s: Lasso CD sweep over a sparse batch's column index
# ---------------------------------------------------------------------------

LASSO_ZERO_THRESHOLD = 1e-9
# rows K11s keeps in LDS (64 KiB less its scratch; the binding checks it)
LASSO_SPARSE_MAX_ROWS = 16384 - 176


def lasso_sparse_threads(nf: int, nnz: int) -> int:
    """Threads of the one K11s workgroup, from the mean column length
    nnz / nf: 64 up to a mean of 64 entries, 256 up to 512, else 1024.
    One wave has no cross-wave partials and no hardware barrier per
    coordinate, which is what a column of a few entries pays for; wider
    workgroups win only once a column is long enough to amortise them
    (measured against forced thread counts: profiles/lasso_sparse_ab.md).
    A function of the batch alone, so a batch always runs with the same
    summation order."""
    mean = nnz / max(1, nf)
    if mean <= 64:
        return 64
    if mean <= 512:
        return 256
    return 1024


def lasso_cd_sparse(feat_ids: torch.Tensor, feat_ptr: torch.Tensor,
                    feat_row: torch.Tensor, feat_val: torch.Tensor,
                    y: torch.Tensor, w: torch.Tensor, col_sq: torch.Tensor,
                    lam_n: float, _force_threads: int = 0
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """One full cyclic coordinate-descent sweep over the features PRESENT in
    a sparse batch (K11s, ops/csrc/lasso_sparse.hip; reference
    LassoTrainer.java:164-208 over SparseVector columns). The batch is given
    by its column index (SparseBatch): feat_ids int32 [nf] ascending,
    feat_ptr int64 [nf+1], feat_row int32 [nnz] (each row at most once per
    feature), feat_val float32 [nnz]; y [B], w [F], col_sq [nf] the
    per-present-feature sum of squares.

    r = y, then r[row] -= val * w for each present feature with w != 0, in
    feature order. Then for each present feature k in order, f = feat_ids[k]:
        c  = sum_e val[e] * r[row[e]] + w[f] * col_sq[k]
        wn = sign(c) * max(|c| - lam_n, 0) / col_sq[k]
        r[row[e]] += val[e] * (w[f] - wn);  w[f] = wn
    A feature with no entries, or with col_sq[k] <= 1e-9, is skipped and
    keeps its weight (upstream: `continue`), as does every feature absent
    from the batch. Returns (w_new, r_new) with r_new = y - X w_new; inputs
    are not mutated.

    CPU tensors, HARMONY_FORCE_TORCH_OPS=1 and batches above
    LASSO_SPARSE_MAX_ROWS take the torch loop below, which is the reference
    implementation. _force_threads overrides lasso_sparse_threads (tests)."""
    B, nf = y.shape[0], feat_ids.shape[0]
    w = w.clone()
    if B == 0 or nf == 0:
        return w, y.clone()
    if _use_hip(y) and B <= LASSO_SPARSE_MAX_ROWS:
        threads = _force_threads or lasso_sparse_threads(
            nf, feat_row.shape[0])
        r = torch.empty_like(y)
        _hip.lasso_cd_sparse(
            feat_ids.contiguous(), feat_ptr.contiguous(),
            feat_row.contiguous(), feat_val.contiguous(), y.contiguous(), w,
            col_sq.contiguous(), float(lam_n), r, int(threads))
        return w, r
    r = y.clone()
    ids = feat_ids.tolist()
    ptr = feat_ptr.tolist()
    rows = feat_row.long()
    live = (w[feat_ids.long()] != 0).tolist()
    for k, f in enumerate(ids):
        if live[k] and ptr[k + 1] > ptr[k]:
            sl = slice(ptr[k], ptr[k + 1])
            r[rows[sl]] -= feat_val[sl] * w[f]
    ok = ((col_sq > LASSO_ZERO_THRESHOLD)
          & (feat_ptr[1:] > feat_ptr[:-1])).tolist()
    for k, f in enumerate(ids):
        if not ok[k]:
            continue
        sl = slice(ptr[k], ptr[k + 1])
        rw, v = rows[sl], feat_val[sl]
        c = v @ r[rw] + w[f] * col_sq[k]
        wn = (torch.clamp(c.abs() - lam_n, min=0.0) * torch.sign(c)
              / col_sq[k])
        r[rw] += v * (w[f] - wn)
        w[f] = wn
    return w, r


def fused_apply_supported(update_fn_name: str) -> bool:
    return update_fn_name in _APPLY_MODES


def scatter_apply(shard: torch.Tensor, rows: torch.Tensor,
                  deltas: torch.Tensor, update_fn_name: str,
                  step_size: float = 0.0, max_val: float = 0.0) -> None:
    """shard[rows] = f(shard[rows], deltas) in one kernel (GPU only)."""
    assert _use_hip(shard), "scatter_apply is the GPU fused path"
    _hip.scatter_apply(shard, rows.contiguous(), deltas.contiguous(),
                       _APPLY_MODES[update_fn_name], float(step_size),
                       float(max_val))


def dense_apply(shard: torch.Tensor, delta: torch.Tensor,
                update_fn_name: str, step_size: float = 0.0,
                max_val: float = 0.0) -> None:
    assert _use_hip(shard), "dense_apply is the GPU fused path"
    _hip.dense_apply(shard, delta.contiguous(), _APPLY_MODES[update_fn_name],
                     float(step_size), float(max_val))


# ---------------------------------------------------------------------------
# K13: Pregel pull (send + combine over a static inverted edge index)
# ---------------------------------------------------------------------------

_PULL_COMBINERS = {"add": 0, "min": 1}


def pregel_pull_group(num_rows: int, num_in_edges: int) -> int:
    """Lanes that cooperate on one row in the K13 kernel: the smallest power
    of two >= the graph's mean in-degree, clamped to 1..64. A function of
    the graph alone, so a graph always runs with the same summation order."""
    mean = num_in_edges / max(1, num_rows)
    g = 1
    while g < 64 and g < mean:
        g *= 2
    return g


def pregel_pull(in_ptr: torch.Tensor, in_src: torch.Tensor,
                in_w: Optional[torch.Tensor], w_const: float,
                vert_msg: torch.Tensor, send_mask: Optional[torch.Tensor],
                combiner: str, add_weight: bool, _force_group: int = 0
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """One superstep's message send + combine as a gather-reduce (K13,
    ops/csrc/pregel.hip; replaces reference MessageManager.addMessage with a
    MessageCombiner). The pull index lists, for each of R destination rows,
    its sources: in_ptr int64 [R+1], in_src int32 [Ein] (local source
    index), in_w float32 [Ein] or None.

    out[r] combines, over the in-edges e of row r whose source is sending,
    vert_msg[src] (+ in_w[e], or w_const when in_w is None, if add_weight);
    the combiner's identity (0 for add, +inf for min) when nothing is sent.
    flag[r] = 1 iff at least one in-edge's source was sending. send_mask
    (uint8/bool [n_local]) None means every source sends.
    Returns (out float32 [R], flag uint8 [R]).

    CPU tensors (and HARMONY_FORCE_TORCH_OPS=1) take the torch reference
    below, which is also the kernel's test oracle. _force_group is for tests:
    it overrides the lanes-per-row choice of pregel_pull_group."""
    mode = _PULL_COMBINERS[combiner]
    R = in_ptr.shape[0] - 1
    if _use_hip(vert_msg):
        group = _force_group or pregel_pull_group(R, in_src.shape[0])
        mask = None
        if send_mask is not None:
            mask = (send_mask.view(torch.uint8)
                    if send_mask.dtype == torch.bool
                    else send_mask.to(torch.uint8)).contiguous()
        out, flag = _hip.pregel_pull(
            in_ptr.contiguous(), in_src.contiguous(),
            None if in_w is None else in_w.contiguous(), float(w_const),
            vert_msg.contiguous(), mask, mode, bool(add_weight), int(group))
        return out, flag
    dev = vert_msg.device
    counts = in_ptr[1:] - in_ptr[:-1]
    row = torch.repeat_interleave(torch.arange(R, device=dev), counts)
    src = in_src.long()
    v = vert_msg[src]
    if add_weight:
        v = v + (in_w if in_w is not None else w_const)
    if send_mask is not None:
        sending = send_mask[src].bool()
        row, v = row[sending], v[sending]
    flag = torch.zeros(R, dtype=torch.uint8, device=dev)
    flag[row] = 1
    if mode == 1:
        out = torch.full((R,), float("inf"), dtype=vert_msg.dtype, device=dev)
        out.scatter_reduce_(0, row, v, reduce="amin", include_self=True)
    else:
        out = torch.zeros(R, dtype=vert_msg.dtype, device=dev)
        out.index_add_(0, row, v)
    return out, flag


# ---------------------------------------------------------------------------
# K13p: Pregel push (send + combine along the frontier's out-edges)
# ---------------------------------------------------------------------------

def pregel_push(out_ptr: torch.Tensor, out_row: torch.Tensor,
                out_w: Optional[torch.Tensor], w_const: float,
                vert_msg: torch.Tensor, frontier: torch.Tensor,
                num_rows: int, combiner: str, add_weight: bool,
                send_mask: Optional[torch.Tensor] = None,
                _edges_hint: int = -1) -> Tuple[torch.Tensor, torch.Tensor]:
    """One superstep's message send + combine along the out-edges of the
    sending vertices only (K13p, ops/csrc/pregel_push.hip): pregel_pull's
    result at the cost of the frontier's edges instead of the whole index.

    The local out-CSR in original edge order: out_ptr int64 [n_local+1],
    out_row int32 [E], out_w float32 [E] or None. out_row[e] is the
    destination ROW in the pull index's row space (0..n_local-1 local
    vertices, n_local + position in remote_keys for remote ones; see
    pregel.engine.build_push_index). frontier int32 [nf]: local indices of
    the sending vertices; a repeated entry is harmless (min is idempotent).
    send_mask (uint8/bool [n_local], optional) narrows the frontier to the
    entries whose vertex it marks: a caller that holds a mask on the device
    passes frontier = all vertices with it and needs neither a compaction
    nor a host read of the frontier's size.

    out[r] = min over the edges e of frontier vertices that end in row r of
    vert_msg[src] (+ out_w[e], or w_const when out_w is None, if
    add_weight), each one rounded float32 add as in K13; +inf when there is
    none. flag[r] = 1 iff at least one such edge exists (even when its value
    is +inf). So the result equals pregel_pull on the inverted index with
    send_mask = the indicator of frontier, value for value.
    Returns (out float32 [num_rows], flag uint8 [num_rows]).

    combiner must be "min": the kernel combines with integer atomics on the
    float's bits, whose result does not depend on arrival order; "add" would
    need float atomic adds and lose K13's bitwise reproducibility, and
    raises ValueError. NaN messages are unspecified (K13's fminf drops
    them). A frontier id outside [0, n_local) and a row outside
    [0, num_rows) are skipped, edge ranges are clamped to [0, E]; nf == 0 or
    num_rows == 0 launches nothing.

    CPU tensors (and HARMONY_FORCE_TORCH_OPS=1) take the torch reference
    below (a scatter_reduce_ amin over the frontier's edges), which is also
    the kernel's test oracle. _edges_hint: the caller's count of frontier
    edges, if it has one; it only sizes the kernel's grid."""
    if combiner != "min":
        raise ValueError(
            f"pregel_push supports the min combiner only, got {combiner!r}: "
            "a pushed add needs float atomics, whose sum depends on arrival "
            "order")
    R = int(num_rows)
    if _use_hip(vert_msg):
        mask = None
        if send_mask is not None:
            mask = (send_mask.view(torch.uint8)
                    if send_mask.dtype == torch.bool
                    else send_mask.to(torch.uint8)).contiguous()
        out, flag = _hip.pregel_push(
            out_ptr.contiguous(), out_row.contiguous(),
            None if out_w is None else out_w.contiguous(), float(w_const),
            vert_msg.contiguous(), frontier.to(torch.int32).contiguous(),
            mask, R, bool(add_weight), int(_edges_hint))
        return out, flag
    dev = vert_msg.device
    n_local = out_ptr.shape[0] - 1
    n_edges = out_row.shape[0]
    out = torch.full((R,), float("inf"), dtype=torch.float32, device=dev)
    flag = torch.zeros(R, dtype=torch.uint8, device=dev)
    f = frontier.long()
    f = f[(f >= 0) & (f < n_local)]
    if send_mask is not None:
        f = f[send_mask.bool()[f]]
    if f.numel() == 0 or R == 0:
        return out, flag
    beg = out_ptr[f].clamp(0, n_edges)
    end = out_ptr[f + 1].clamp(0, n_edges)
    cnt = (end - beg).clamp_min(0)
    fptr = torch.cumsum(cnt, 0) - cnt
    total = int(cnt.sum())
    src = torch.repeat_interleave(f, cnt)
    e = (torch.arange(total, device=dev)
         - torch.repeat_interleave(fptr, cnt)
         + torch.repeat_interleave(beg, cnt))
    row = out_row[e].long()
    v = vert_msg[src].float()
    if add_weight:
        v = v + (out_w[e] if out_w is not None else w_const)
    ok = (row >= 0) & (row < R)
    row, v = row[ok], v[ok]
    flag[row] = 1
    out.scatter_reduce_(0, row, v, reduce="amin", include_self=True)
    return out, flag


# ---------------------------------------------------------------------------
# segment / scatter helpers
# ---------------------------------------------------------------------------

def segment_sum(keys: torch.Tensor, deltas: torch.Tensor
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Aggregate duplicate keys -> (unique_keys, summed deltas)."""
    uniq, inv = torch.unique(keys, return_inverse=True)
    out = torch.zeros((uniq.shape[0], deltas.shape[1]), dtype=deltas.dtype,
                      device=deltas.device)
    out.index_add_(0, inv, deltas)
    return uniq, out
