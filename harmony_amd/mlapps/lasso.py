"""Lasso — cyclic coordinate descent on the PS.

Reference: dolphin/mlapps/lasso/LassoTrainer.java:164-190 — model is
partitioned partIdx -> weight Vector(featuresPerPartition), workers pull all
partitions each batch (:292); per coordinate i the closed-form update
optimal_i = dot(x_i, y - sum_{j!=i} x_j w_j) / dot(x_i, x_i) followed by a
soft-threshold by lambda (ZERO_THRESHOLD 1e-9 at :61); server applies vector
add (LassoETModelUpdateFunction.java:33).

MI355X shape: the residual r = y - Xw is maintained incrementally so each
coordinate step is two rocBLAS dot/axpy column ops on the device-resident
batch; the full sweep stays on the GPU (F small relative to batch).

App args: num_features, num_parts, batch_size, lam, step_size(unused),
noise, density; sparse (default false) and nnz_per_row (synthetic sparse
generator, default 32); test_data_path (mlapps/heldout.py; reference
TestDataProvider): a held-out file read whole by every rank in build(), cut
into blocks of at most batch_size rows; evaluate_test() reports test_mse and
test_examples for the final model and for every offline checkpoint.

sparse=true keeps every batch as a SparseBatch (CSR + static column index),
as the reference does (LassoETParser createSparse, horzcatVecSparse at
LassoTrainer.java:273-283), and runs the K11s sweep (ops/csrc/
lasso_sparse.hip) over the features PRESENT in the batch: memory and time
follow the non-zeros, not B * F, so num_features may be far wider than a row
is long. Pull and push stay dense ([P, F/P]).

The two paths differ on purpose in one place. The sparse sweep skips a
feature that has no entries in the batch (or whose column mass is <= 1e-9)
and keeps its weight, as the reference does (LassoTrainer.java:199-208,
`continue`). The dense sweep visits every feature: an all-zero column has
c = w * 1e-9 after the clamp of col_sq, so the soft-threshold drives that
weight to 0. On data where every column is present in every batch the two
compute the same thing up to fp32 summation order.
"""

from __future__ import annotations

import torch

from harmony_amd.config import JobConfig, TableConfig
from harmony_amd.dolphin.data_provider import TrainingDataProvider
from harmony_amd.dolphin.model_accessor import accessor_for, build_ps_table
from harmony_amd.dolphin.trainer import Trainer, TrainerContext
from harmony_amd.mlapps import heldout
from harmony_amd.mlapps.sparse_batch import (SparseBatch, csr_row_blocks,
                                             drop_repeats, is_sparse,
                                             reslice)
from harmony_amd.utils import stable_seed
from harmony_amd import ops

MODEL_TABLE = "lasso_model"
ZERO_THRESHOLD = 1e-9


def defaults(job: JobConfig) -> dict:
    a = dict(num_features=256, num_parts=16, batch_size=2048, lam=0.05,
             noise=0.1, density=0.25, sparse="false", nnz_per_row=32)
    a.update(job.app_args)
    return a


_is_sparse = is_sparse


def model_table_cfg(job: JobConfig, world_size: int) -> TableConfig:
    a = defaults(job)
    P = a["num_parts"]
    assert a["num_features"] % P == 0
    return TableConfig(
        table_id=f"{job.job_id}/{MODEL_TABLE}",
        num_keys=P,
        value_dim=a["num_features"] // P,
        dtype="float32",
        num_blocks=P,
        update_fn="add",
        init_fn="zeros",
    )


def make_batches(job: JobConfig, rank: int, device: torch.device,
                 world_size: int = 1):
    a = defaults(job)
    F = a["num_features"]
    if _is_sparse(a):
        return _make_sparse_batches(job, a, rank, device, world_size)
    if job.app_args.get("input"):
        # sample_lasso rows "label idx:val ..." (reference LassoParser)
        from harmony_amd import dataloader as dl

        X, y = dl.parse_libsvm_split(job.app_args["input"], rank,
                                     world_size, F)
        n_blocks = max(1, job.num_worker_blocks or job.num_mini_batches)
        return [(xb.to(device), yb.to(device)) for xb, yb in
                zip(torch.chunk(X, n_blocks), torch.chunk(y, n_blocks))], None
    g = torch.Generator().manual_seed(stable_seed(job.job_id, "data", rank))
    # sparse ground-truth weights
    w_true = torch.randn(F, generator=g)
    mask = torch.rand(F, generator=g) < a["density"]
    w_true = w_true * mask
    blocks = []
    n_blocks = job.num_worker_blocks or job.num_mini_batches
    for _ in range(n_blocks):
        X = torch.randn(a["batch_size"], F, generator=g)
        y = X @ w_true + a["noise"] * torch.randn(a["batch_size"], generator=g)
        blocks.append((X.to(device), y.to(device)))
    return blocks, w_true


def _make_sparse_batches(job: JobConfig, a: dict, rank: int,
                         device: torch.device, world_size: int):
    """make_batches for sparse=true: the same block structure as the dense
    branch, every block a (SparseBatch, y) pair. No tensor with B*F elements
    is built on either path."""
    F = int(a["num_features"])
    if a.get("input"):
        from harmony_amd import dataloader as dl

        row_ptr, col, val, y = dl.parse_libsvm_csr_split(
            a["input"], rank, world_size, F)
        n_blocks = max(1, job.num_worker_blocks or job.num_mini_batches)
        return [(SparseBatch(*csr, F).to(device), y[lo:hi].to(device))
                for lo, hi, *csr in csr_row_blocks(row_ptr, col, val,
                                                   y.shape[0], n_blocks)
                ], None
    B = int(a["batch_size"])
    k = max(1, min(int(a["nnz_per_row"]), F))
    g = torch.Generator().manual_seed(stable_seed(job.job_id, "data", rank))
    w_true = torch.randn(F, generator=g)
    mask = torch.rand(F, generator=g) < a["density"]
    w_true = w_true * mask
    blocks = []
    n_blocks = job.num_worker_blocks or job.num_mini_batches
    for _ in range(n_blocks):
        cols = torch.randint(0, F, (B, k), generator=g).sort(dim=1).values
        keep, row_ptr = drop_repeats(cols)
        vals = torch.randn(B, k, generator=g) * keep
        y = (vals * w_true[cols]).sum(dim=1) \
            + a["noise"] * torch.randn(B, generator=g)
        x =SparseBatch(row_ptr, cols[keep].to(torch.int32), vals[keep], F)
        blocks.append((x.to(device), y.to(device)))
    return blocks, w_true


def _sparse_col_sq(X: SparseBatch) -> torch.Tensor:
    """Per-present-feature sum of squares, clamped as the dense path's;
    computed once and kept on the batch (a block is static, and prefix()
    builds a new batch, so the cache cannot go stale)."""
    col_sq = getattr(X, "_harmony_colsq", None)
    if col_sq is None:
        nf = X.feat_ids.shape[0]
        seg = torch.repeat_interleave(
            torch.arange(nf, device=X.device),
            X.feat_ptr[1:] - X.feat_ptr[:-1])
        # summed in fp64 and rounded once: the device index_add_ is atomic,
        # and its order must not show in the fp32 value
        v = X.feat_val.double()
        col_sq = torch.zeros(nf, dtype=torch.float64, device=X.device)
        col_sq.index_add_(0, seg, v * v)
        col_sq = col_sq.float().clamp_min(ZERO_THRESHOLD)
        X._harmony_colsq = col_sq
    return col_sq


class LassoTrainer(Trainer):
    def __init__(self, ctx: TrainerContext):
        super().__init__(ctx)
        self.a = defaults(JobConfig(job_id=ctx.job_id, app="lasso",
                                    app_args=ctx.app_args))
        self.accessor = accessor_for(ctx.table(MODEL_TABLE))
        self._loss = torch.zeros(())

    def pull_model(self) -> None:
        self.w = self.accessor.pull_all()[:self.a["num_parts"]].reshape(-1)

    def local_compute(self) -> None:
        X, y = self.batch
        if X.shape[0] == 0:      # stopped worker: no work, zero delta
            self.delta = torch.zeros_like(self.w)
            self._loss = torch.zeros(())
            return
        F = X.shape[1]
        lam_n = self.a["lam"] * X.shape[0]
        if isinstance(X, SparseBatch):
            # one K11s sweep over the batch's present features; the
            # residual is built inside the op
            w, r = ops.lasso_cd_sparse(X.feat_ids, X.feat_ptr, X.feat_row,
                                       X.feat_val, y, self.w,
                                       _sparse_col_sq(X), lam_n)
            self.delta = w - self.w
            self._loss = (r * r).mean()
            return
        r = y - X @ self.w                     # residual
        col_sq = getattr(X, "_harmony_colsq", None)
        if col_sq is None:
            col_sq = (X * X).sum(dim=0).clamp_min(ZERO_THRESHOLD)
            X._harmony_colsq = col_sq          # batches are static per block
        # full cyclic sweep in one persistent kernel on GPU (K11); the torch
        # path queues F small device ops asynchronously (no host syncs)
        w, r = ops.lasso_cd(X, r, self.w, col_sq, lam_n)
        _ = F
        self.delta = w - self.w
        self._loss = (r * r).mean()          # device scalar; no batch sync

    def push_update(self) -> None:
        P = self.a["num_parts"]
        self.accessor.push_dense(self.delta.reshape(P, -1))

    def evaluate_model(self):
        return {"mse": float(self._loss)}

    def evaluate_test(self):
        """test_mse of y - Xw over the held-out blocks, for the model as
        pulled now (a collective). Nothing of the training state (self.w,
        _loss) is touched. The squared residuals are summed in fp64 over all
        blocks and divided once."""
        if not self.test_blocks:
            return {}
        w = self.accessor.pull_all()[:self.a["num_parts"]].reshape(-1)
        sq = torch.zeros((), dtype=torch.float64, device=w.device)
        n = 0
        for X, y in self.test_blocks:
            if isinstance(X, SparseBatch):
                # follow the non-zeros: a row's sum in fp64, rounded once to
                # fp32, so the order of the device's atomic index_add_ does
                # not show in the value (as in _sparse_col_sq)
                B = X.shape[0]
                row = torch.repeat_interleave(
                    torch.arange(B, device=X.device),
                    X.row_ptr[1:] - X.row_ptr[:-1])
                xw = torch.zeros(B, dtype=torch.float64, device=X.device)
                xw.index_add_(0, row,
                              X.val.double() * w.double()[X.col.long()])
                r = y - xw.float()
            else:
                r = y - X @ w
            sq += (r.double() * r.double()).sum()
            n += y.shape[0]
        return {"test_mse": float(sq) / n, "test_examples": float(n)}

    def num_batch_examples(self) -> int:
        return self.batch[0].shape[0]


def build(job: JobConfig, ctx, cp):
    # before anything else: a missing test file fails the job at once
    test_blocks = heldout.row_blocks(defaults(job), ctx.device)
    cfg = model_table_cfg(job, ctx.world_size)
    table = build_ps_table(job, cfg, ctx, cp)
    blocks, _ = make_batches(job, ctx.rank, ctx.device, ctx.world_size)
    tctx = TrainerContext(job_id=job.job_id, rank=ctx.rank,
                          world_size=ctx.world_size, device=ctx.device,
                          tables={MODEL_TABLE: table}, app_args=job.app_args)
    trainer = LassoTrainer(tctx)
    trainer.test_blocks = test_blocks
    provider = TrainingDataProvider(reslice=reslice, local_blocks=blocks)
    return {MODEL_TABLE: table}, trainer, provider
