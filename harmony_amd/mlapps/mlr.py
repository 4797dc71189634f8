"""MLR — multinomial (softmax) logistic regression on the PS.

Reference: dolphin/mlapps/mlr/MLRTrainer.java — the model is partitioned as
key = classIdx*numPartitionsPerClass + partIdx -> Vector(featuresPerPartition)
and workers pull ALL partitions each mini-batch (MLRTrainer.java:185-187);
per sample p = softmax(Wx) with a log-sum-exp guard (:475-489), gradient
grad_j -= stepSize * p_j * x (+L2) accumulated densely (:374-398); the server
applies old.addi(delta) (MLRETModelUpdateFunction.java:60-62).

MI355X shape: the whole per-batch math is (batch x F) @ (F x C) GEMM on the
matrix cores + a fused row-softmax/label-subtract kernel + the outer-product
gradient GEMM; pull-all = all-gather, dense push = reduce-scatter with the
add-update epilogue. GEMMs go to rocBLAS (torch.matmul); the softmax+grad
scaling is the fused HIP kernel `mlr_softmax_grad` (ops/csrc/mlr.hip).

App args: num_classes, num_features, num_parts_per_class, batch_size,
step_size, lambda (L2), dtype; sparse (default false) keeps every batch as a
SparseBatch (CSR + static column index) and runs the K4s gather-reduce
kernels (ops/csrc/mlr_sparse.hip) instead of the dense GEMM pair, so the
input's feature space may be far wider than a row is long; nnz_per_row sizes
the synthetic sparse generator; test_data_path (mlapps/heldout.py; reference
TestDataProvider): a held-out file read whole by every rank in build(), cut
into blocks of at most batch_size rows; evaluate_test() reports
test_cross_entropy, test_accuracy and test_examples for the final model and
for every offline checkpoint.
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
from harmony_amd import ops

MODEL_TABLE = "mlr_model"


def defaults(job: JobConfig) -> dict:
    a = dict(num_classes=10, num_features=1024, num_parts_per_class=8,
             batch_size=4096, step_size=0.01, lam=1e-4, dtype="float32",
             decay_rate=0.9, decay_period=5, sparse="false", nnz_per_row=32)
    a.update(job.app_args)
    return a


_is_sparse = is_sparse


def model_table_cfg(job: JobConfig, world_size: int) -> TableConfig:
    a = defaults(job)
    P = a["num_parts_per_class"]
    assert a["num_features"] % P == 0
    return TableConfig(
        table_id=f"{job.job_id}/{MODEL_TABLE}",
        num_keys=a["num_classes"] * P,
        value_dim=a["num_features"] // P,
        dtype=a["dtype"],
        # one key per block (a partition row IS the unit of placement, as in
        # the reference's per-partition table entries) -> no keyspace padding,
        # clean [C*P, F/P] <-> [C, F] views.
        num_blocks=a["num_classes"] * P,
        update_fn="add",
        init_fn="gaussian",
        init_args={"std": 0.01},
    )


def make_batches(job: JobConfig, rank: int, device: torch.device,
                 world_size: int = 1):
    """One block = one mini-batch (reference ETTrainingDataProvider).
    With app_args['input'] (reference -input flag): load this rank's split of
    a sample_mlr-format file; otherwise synthetic per-class gaussian blobs,
    deterministic per (job, rank)."""
    a = defaults(job)
    if _is_sparse(a):
        return _make_sparse_batches(job, a, rank, device, world_size)
    if a.get("input") or job.app_args.get("input"):
        from harmony_amd import dataloader as dl

        X, y = dl.parse_libsvm_split(job.app_args["input"], rank,
                                     world_size, a["num_features"])
        n_blocks = max(1, job.num_worker_blocks or job.num_mini_batches)
        xs = torch.chunk(X, n_blocks)
        ys = torch.chunk(y.long(), n_blocks)
        return [(x.to(device), yy.to(device)) for x, yy in zip(xs, ys)]
    C, F, B = a["num_classes"], a["num_features"], a["batch_size"]
    from harmony_amd.utils import stable_seed

    g = torch.Generator().manual_seed(stable_seed(job.job_id, rank))
    centers = torch.randn(C, F, generator=g) * 0.5
    blocks = []
    n_blocks = job.num_worker_blocks or job.num_mini_batches
    for _ in range(n_blocks):
        y = torch.randint(0, C, (B,), generator=g)
        x = centers[y] + torch.randn(B, F, generator=g)
        blocks.append((x.to(device), y.to(device)))
    return blocks


def _make_sparse_batches(job: JobConfig, a: dict, rank: int,
                         device: torch.device, world_size: int):
    """make_batches for sparse=true: the same block structure as the dense
    branch, every block a (SparseBatch, labels) pair. No tensor with B*F
    elements is built on either path."""
    F = int(a["num_features"])
    n_blocks = max(1, job.num_worker_blocks or job.num_mini_batches)
    blocks = []
    if a.get("input"):
        from harmony_amd import dataloader as dl

        row_ptr, col, val, y = dl.parse_libsvm_csr_split(
            a["input"], rank, world_size, F)
        for lo, hi, *csr in csr_row_blocks(row_ptr, col, val, y.shape[0],
                                           n_blocks):
            blocks.append((SparseBatch(*csr, F).to(device),
                           y[lo:hi].long().to(device)))
        return blocks
    C, B = a["num_classes"], a["batch_size"]
    k = max(1, min(int(a["nnz_per_row"]), F))
    from harmony_amd.utils import stable_seed

    g = torch.Generator().manual_seed(stable_seed(job.job_id, rank))
    centers = torch.randn(C, F, generator=g) * 0.5
    for _ in range(n_blocks):
        y = torch.randint(0, C, (B,), generator=g)
        cols = torch.randint(0, F, (B, k), generator=g).sort(dim=1).values
        keep, row_ptr = drop_repeats(cols)
        vals = centers[y.unsqueeze(1), cols] + torch.randn(B, k, generator=g)
        x = SparseBatch(row_ptr, cols[keep].to(torch.int32), vals[keep], F)
        blocks.append((x.to(device), y.to(device)))
    return blocks


class MLRTrainer(Trainer):
    def __init__(self, ctx: TrainerContext):
        super().__init__(ctx)
        self.a = defaults(JobConfig(job_id=ctx.job_id, app="mlr",
                                    app_args=ctx.app_args))
        # async mode (app arg one_sided=true): pull/push are direct xGMI
        # kernels; the worker never issues a collective
        self.accessor = accessor_for(ctx.table(MODEL_TABLE))
        self.step_size = self.a["step_size"]
        self.W = None          # [C*P, F/P] pulled model
        # hipGraph capture of the compute phase (static per block); the
        # pulled model lands in a stable buffer so graphs see fixed pointers
        import os

        from harmony_amd.utils.graphs import GraphRunner

        # measured on MI355X: graph replay was neutral in the 3-job bench
        # and slightly SLOWER per-app (kernels are large; launches were not
        # the bottleneck) — opt-in via HARMONY_GRAPHS=1
        self._graphs = GraphRunner(
            enabled=ctx.device.type == "cuda"
            and os.environ.get("HARMONY_GRAPHS") == "1")
        self._W_buf = None
        self._bodies = {}
        # device-resident accumulators (no per-batch host syncs)
        self._loss_sum = torch.zeros((), device=ctx.device)
        self._loss_n = 0
        self._correct = torch.zeros((), dtype=torch.int64, device=ctx.device)

    def _w_matrix(self) -> torch.Tensor:
        C, F = self.a["num_classes"], self.a["num_features"]
        return self.W.view(C, F)

    def _wt_buf(self) -> torch.Tensor:
        # persistent padded W^T staging buffer for the MFMA step kernel
        if getattr(self, "_wt", None) is None:
            F = self.a["num_features"]
            self._wt = torch.zeros((F, 16), dtype=torch.float32,
                                   device=self.ctx.device)
        return self._wt

    def _sparse_wt_buf(self):
        # persistent [F, Cp] W^T buffer for the K4s forward, refilled from
        # the pulled model once per batch; the CPU reference reads W itself
        if self.ctx.device.type != "cuda":
            return None
        if getattr(self, "_sparse_wt", None) is None:
            C, F = self.a["num_classes"], self.a["num_features"]
            self._sparse_wt = torch.zeros((F, (C + 3) // 4 * 4),
                                          dtype=torch.float32,
                                          device=self.ctx.device)
        return self._sparse_wt

    def _sparse_compute(self, x: SparseBatch, y: torch.Tensor) -> None:
        # same math as the dense body with both GEMMs replaced by the K4s
        # gather-reduces; graphs and the MFMA path do not apply here
        W = self._w_matrix()
        F = self.a["num_features"]
        p, loss, correct = ops.mlr_sparse_forward(
            x.row_ptr, x.col, x.val, W, y, Wt_buf=self._sparse_wt_buf())
        g = ops.mlr_sparse_grad(x.feat_ids, x.feat_ptr, x.feat_row,
                                x.feat_val, p, F)            # [C, F]
        self.grad_raw = g / x.shape[0] + self.a["lam"] * W
        self._loss_sum += loss
        self._correct += correct
        self._loss_n += x.shape[0]

    def pull_model(self) -> None:
        C, P = self.a["num_classes"], self.a["num_parts_per_class"]
        pulled = self.accessor.pull_all()[:C * P]
        if self._W_buf is None:
            self._W_buf = pulled.clone()
        else:
            self._W_buf.copy_(pulled)
        self.W = self._W_buf

    def local_compute(self) -> None:
        x, y = self.batch
        if x.shape[0] == 0:       # stopped worker: zero grad, no forward
            self.grad_raw = torch.zeros_like(self._w_matrix())
            return
        if isinstance(x, SparseBatch):
            self._sparse_compute(x, y)
            return
        key = id(self.batch)
        body = self._bodies.get(key)
        if body is None:
            W = self._w_matrix()                   # [C, F] view of W_buf
            import os as _os

            # default: rocBLAS pair (measured at the fetch roofline and
            # 4% faster than the in-tree MFMA kernels both isolated and
            # in-bench — profiles/r02_mlr_mfma.md); HARMONY_MLR_MFMA=1
            # switches to the hand-written K4-MFMA path
            use_mfma = (x.device.type == "cuda"
                        and ops.mlr_step_ok(x, self.a["num_classes"])
                        and _os.environ.get("HARMONY_MLR_MFMA", "0") == "1")
            rb = int(_os.environ.get("HARMONY_MLR_RB", "0"))
            if rb and (x.shape[0] % rb or rb % 64):
                rb = 0

            if use_mfma:
                # fused fwd+softmax+grad on f32 MFMA, L3 row-blocked
                # (K4-MFMA, ops/csrc/mlr_mfma.hip; A/B scripts/mlr_mfma_ab.py)
                def body(x=x, y=y, W=W, rb=rb):
                    g, loss, correct = ops.mlr_step_mfma(
                        x, W, y, row_block=rb, Wt_buf=self._wt_buf())
                    self.grad_raw = g / x.shape[0] + self.a["lam"] * W
                    self._loss_sum += loss
                    self._correct += correct
            else:
                def body(x=x, y=y, W=W):
                    # forward GEMM + fused softmax + grad GEMM
                    p, loss, correct = ops.mlr_forward(x, W, y)
                    g = ops.mlr_grad_gemm(p, x)        # [C, F]
                    self.grad_raw = g / x.shape[0] + self.a["lam"] * W
                    self._loss_sum += loss
                    self._correct += correct

            self._bodies[key] = body
        self._graphs.run(key, body, state=(self._loss_sum, self._correct))
        self._loss_n += x.shape[0]

    def push_update(self) -> None:
        C, P = self.a["num_classes"], self.a["num_parts_per_class"]
        # step size applied OUTSIDE the graph (it decays over epochs)
        delta = (-self.step_size) * self.grad_raw
        self.accessor.push_dense(delta.view(C * P, -1))

    def on_epoch_finished(self, epoch: int) -> None:
        if (epoch + 1) % self.a["decay_period"] == 0:
            self.step_size *= self.a["decay_rate"]

    def evaluate_model(self):
        if not self._loss_n:
            return {}
        out = {"cross_entropy": float(self._loss_sum) / self._loss_n,
               "accuracy": float(self._correct) / self._loss_n}
        self._loss_sum = torch.zeros((), device=self.ctx.device)
        self._correct = torch.zeros((), dtype=torch.int64,
                                    device=self.ctx.device)
        self._loss_n = 0
        return out

    def evaluate_test(self):
        """Cross entropy and accuracy of the model as pulled now (a
        collective) on the held-out blocks, by the forward kernels alone:
        loss and correct counts are summed over the blocks and divided
        once. The pulled model stays local, so W, the accumulators of
        evaluate_model() and the graph buffers are untouched."""
        if not self.test_blocks:
            return {}
        C, P = self.a["num_classes"], self.a["num_parts_per_class"]
        W = self.accessor.pull_all()[:C * P].reshape(
            C, self.a["num_features"])
        loss = torch.zeros((), dtype=torch.float64, device=W.device)
        correct = torch.zeros((), dtype=torch.int64, device=W.device)
        n = 0
        for x, y in self.test_blocks:
            if isinstance(x, SparseBatch):
                _p, l, c = ops.mlr_sparse_forward(
                    x.row_ptr, x.col, x.val, W, y,
                    Wt_buf=self._sparse_wt_buf())
            else:
                _p, l, c = ops.mlr_forward(x, W, y)
            loss += l
            correct += c
            n += x.shape[0]
        return {"test_cross_entropy": float(loss) / n,
                "test_accuracy": float(correct) / n,
                "test_examples": float(n)}

    def num_batch_examples(self) -> int:
        return self.batch[0].shape[0]


def build(job: JobConfig, ctx, cp):
    # before anything else: a missing test file fails the job at once
    test_blocks = heldout.row_blocks(defaults(job), ctx.device,
                                     label_dtype=torch.int64)
    cfg = model_table_cfg(job, ctx.world_size)
    table = build_ps_table(job, cfg, ctx, cp)
    tctx = TrainerContext(job_id=job.job_id, rank=ctx.rank,
                          world_size=ctx.world_size, device=ctx.device,
                          tables={MODEL_TABLE: table}, app_args=job.app_args)
    trainer = MLRTrainer(tctx)
    trainer.test_blocks = test_blocks
    provider = TrainingDataProvider(reslice=reslice, local_blocks=
        make_batches(job, ctx.rank, ctx.device, ctx.world_size))
    return {MODEL_TABLE: table}, trainer, provider
