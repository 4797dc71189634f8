"""Shared jobs, files and fp64 evaluations for the held-out test-data tests
(test_heldout_cpu.py, test_heldout_gpu.py).

Bounds. With u = 2^-24, an fp32 sum of k products differs from the exact sum
by at most k * u * sum|terms| to first order in any order; a residual
y - sum(x w) has k + 1 terms, one more rounding for the subtraction, and the
factor 2 covers the fp32 rounding of the inputs: 2 (k + 2) u sum|terms| per
residual, k the row's entry count (the form of mlr_sparse_cases.bound).
Through the mean of squares: |r'^2 - r^2| <= 2 |r| e + e^2. Nothing here is
tuned to an implementation.
"""

import math
from pathlib import Path

import torch

from harmony_amd import mlapps
from harmony_amd.config import JobConfig, RuntimeConfig
from harmony_amd.mlapps import gbt
from harmony_amd.mlapps.sparse_bins import SparseBins
from harmony_amd.utils import stable_seed

U = 2.0 ** -24
GOLDEN = Path(__file__).parent / "golden"
LASSO_TRAIN = GOLDEN / "lasso" / "sample_lasso_64"
LASSO_TEST = GOLDEN / "lasso" / "sample_lasso_test"
MLR_TRAIN = GOLDEN / "mlr" / "sample_mlr_32"
MLR_TEST = GOLDEN / "mlr" / "sample_mlr_test_16"
LASSO_F, MLR_F, MLR_C = 10, 784, 10


def data_rows(path):
    """(y float64 [n], X float64 [n, F] by a plain line parse, entry counts):
    independent of the project's parsers. Comment and blank lines skipped."""
    F = LASSO_F if "lasso" in str(path) else MLR_F
    ys, rows = [], []
    for line in Path(path).read_text().splitlines():
        line = line.strip()
        if not line or line.startswith("#"):
            continue
        parts = line.split()
        ys.append(float(parts[0]))
        row = torch.zeros(F, dtype=torch.float64)
        for p in parts[1:]:
            i, v = p.split(":")
            row[int(i)] = float(v)
        rows.append(row)
    X = torch.stack(rows)
    return torch.tensor(ys, dtype=torch.float64), X, (X != 0).sum(dim=1)


def run(job, device="cpu"):
    """run_job on one rank: (summary, trainer)."""
    from harmony_amd.dolphin.master import run_job
    from harmony_amd.runtime.bootstrap import init_executor

    app = mlapps.get_app(job.app)
    real = app.build
    seen = {}

    def build(*args):
        out = real(*args)
        seen["trainer"] = out[1]
        return out

    app.build = build
    try:
        s = run_job(job, init_executor(RuntimeConfig(device=device))).summary()
    finally:
        app.build = real
    return s, seen["trainer"]


def hand_built(job, device="cpu"):
    """(tables, trainer, provider) of app.build, for hand-driven batches."""
    from harmony_amd.runtime.bootstrap import init_executor
    from harmony_amd.runtime.control import ControlPlane

    ctx = init_executor(RuntimeConfig(device=device))
    cp = ControlPlane(ctx.store, ctx.rank, ctx.world_size)
    return mlapps.get_app(job.app).build(job, ctx, cp)


def lasso_job(job_id, sparse, test=LASSO_TEST, **kw):
    args = {"input": str(LASSO_TRAIN), "num_features": LASSO_F,
            "num_parts": 5, "lam": 0.5, "sparse": sparse}
    if test is not None:
        args["test_data_path"] = str(test)
    kw.setdefault("max_num_epochs", 2)
    return JobConfig(job_id=job_id, app="lasso", num_mini_batches=2,
                     app_args=args, **kw)


def mlr_job(job_id, sparse, test=MLR_TEST, **kw):
    args = {"input": str(MLR_TRAIN), "num_features": MLR_F,
            "num_classes": MLR_C, "num_parts_per_class": 2,
            "step_size": 0.05, "sparse": sparse}
    if test is not None:
        args["test_data_path"] = str(test)
    kw.setdefault("max_num_epochs", 3)
    return JobConfig(job_id=job_id, app="mlr", num_mini_batches=2,
                     app_args=args, **kw)


def lasso_mse64(w, path=LASSO_TEST):
    """fp64 test mse for weights w, and the bound on an fp32 evaluation."""
    y, X, k = data_rows(path)
    w = w.detach().cpu().double()
    r = y - X @ w
    e = 2.0 * (k.double() + 2) * U * (y.abs() + X.abs() @ w.abs())
    return float((r * r).mean()), float((2 * r.abs() * e + e * e).mean())


def mlr_eval64(W, path=MLR_TEST):
    """From weights W [C, F]: fp64 logits, the per-row bound e on an fp32
    logit (2 (k + 2) u sum|terms|, the largest over the classes), labels."""
    y, X, k = data_rows(path)
    W = W.detach().cpu().double()
    z = X @ W.t()
    e = (2.0 * (k.double() + 2) * U).unsqueeze(1) * (X.abs() @ W.abs().t())
    return z, e.max(dim=1).values, y.long()


# ------------------------------------------------------------------- GBT

GBT_F, GBT_B = 8, 256


def gbt_job(job_id, test, **kw):
    args = {"num_features": GBT_F, "batch_size": GBT_B, "num_bins": 16,
            "max_depth": 3, "step_size": 0.3, "nnz_per_row": 5,
            "test_data_path": str(test)}
    args.update(kw)
    if test is None:
        del args["test_data_path"]
    return JobConfig(job_id=job_id, app="gbt", max_num_epochs=3,
                     num_mini_batches=2, app_args=args)


def write_libsvm(path, X, y, mask=None):
    """Rows "label idx:value ..." of X where mask (default: everywhere);
    %.9g keeps every float32 exactly."""
    lines = []
    for i in range(X.shape[0]):
        cols = range(X.shape[1]) if mask is None else \
            mask[i].nonzero().flatten().tolist()
        ent = " ".join(f"{j}:{float(X[i, j]):.9g}" for j in cols)
        lines.append(f"{float(y[i]):.9g} {ent}".rstrip())
    Path(path).write_text("\n".join(lines) + "\n")
    return str(path)


def gbt_test_data(job_id, mode, seed=4242, n=200):
    """Held-out (X, y, mask) for the synthetic job `job_id`. mode "dense":
    the dense generator of gbt.make_batches with its own weights (the first
    draw of the job's data generator) and other samples; the other modes
    need valid rows only: "cat" makes the last two columns category ids,
    "sparse" keeps about half of the entries, "multiclass" labels 0..2."""
    F = GBT_F
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, F, generator=g)
    mask = None
    if mode == "dense":
        gw = torch.Generator().manual_seed(stable_seed(job_id, "data", 0))
        w = torch.randn(F, generator=gw)
        y = X @ w + torch.sin(3 * X[:, 0]) * 2 \
            + 0.1 * torch.randn(n, generator=g)
        return X, y, mask
    if mode in ("cat", "sparse"):
        X[:, F - 2:] = torch.randint(0, 8, (n, 2), generator=g).float()
    y = X[:, 0] * 2 - X[:, 1] + (X[:, F - 1] % 3 == 1).float() * 3
    if mode == "sparse":
        mask = torch.rand(n, F, generator=g) < 0.5
        mask[0] = False                     # a row without entries
        y = (X * mask)[:, 0] * 2 - (X * mask)[:, 1]
    if mode == "multiclass":
        y = torch.randint(0, 3, (n,), generator=g).float()
    return X, y, mask


def gbt_recomputed(trainer):
    """The test metric from the trainer's final forest(s) by the predict_bins
    loop over its test bins, run on the CPU; the last reduction runs on the
    trainer's device, as evaluate_test's does (a mean's order is the
    device's own, the predictions are compared bit for bit)."""
    bins, y = trainer.test_blocks[0]
    cpu_bins = bins.to("cpu")
    step = trainer.a["step_size"]
    like = torch.zeros(y.shape[0])

    def loop(forest):
        return gbt.GBTTrainer._forest_pred({}, "k", forest, cpu_bins, like,
                                           step).to(y.device)

    if trainer.a["objective"] == "multiclass":
        cls = torch.stack([loop(f) for f in trainer.forests],
                          dim=1).argmax(dim=1)
        return float((cls != y.long()).float().mean())
    resid = y - loop(trainer.forest)
    return float((resid * resid).mean())


def check_mlr(s, trainer):
    assert s["test_examples"] == 16
    W = trainer.accessor.pull_all()[:MLR_C * 2].reshape(MLR_C,
                                                           MLR_F)
    z, e, y = mlr_eval64(W)
    top2 = z.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2 * e
    unsure = int((~sure).sum())
    correct = int(((z.argmax(dim=1) == y) & sure).sum())
    got = s["test_accuracy"] * 16
    print(f"accuracy {s['test_accuracy']}, sure rows correct {correct}, "
          f"rows left out {unsure}, train accuracy {s['accuracy']}")
    assert unsure <= 1
    assert got == round(got) and correct <= got <= correct + unsure
    # cross entropy: lse - z_y per row. Each logit is within e, so lse and
    # z_y are; m + log(sum of C exps <= 1) in fp32 adds a few roundings of
    # terms of that size: 2 (C + 2) u (|lse| + |z_y|). Then the fp32 sum of
    # the 16 rows: 2 n u sum|ce|.
    lse = torch.logsumexp(z, dim=1)
    zy = z.gather(1, y.view(-1, 1)).squeeze(1)
    ce = lse - zy
    per_row = 2 * e + 2 * (MLR_C + 2) * U * (lse.abs() + zy.abs())
    bound = float(per_row.sum() + 2 * 16 * U * ce.abs().sum()) / 16
    want = float(ce.mean())
    print(f"cross entropy {s['test_cross_entropy']!r}, fp64 {want!r}, "
          f"error {abs(s['test_cross_entropy'] - want):.3e}, "
          f"bound {bound:.3e}")
    assert abs(s["test_cross_entropy"] - want) <= bound


GBT_MODES = {
    "dense": ("dense", {}),
    "sparse": ("sparse", {"sparse": "true"}),
    "cat": ("cat", {"num_categorical": 2, "num_categories": 8}),
    "multiclass": ("multiclass", {"objective": "multiclass",
                                  "num_classes": 3}),
}


def run_gbt(mode, tmp_path, device="cpu"):
    data_mode, kw = GBT_MODES[mode]
    job_id = f"t_ho_gbt_{mode}_{device}"
    X, y, mask = gbt_test_data(job_id, data_mode)
    path = write_libsvm(tmp_path / "held_out", X, y, mask)
    s, trainer = run(gbt_job(job_id, path, **kw), device)
    return s, trainer, (X, y, mask)


def check_gbt(mode, s, trainer, X, y, mask):
    key = "test_error_rate" if mode == "multiclass" else "test_mse"
    assert s["test_examples"] == 200 and len(trainer.test_blocks) == 1
    bins, yt = trainer.test_blocks[0]
    assert isinstance(bins, SparseBins) == (mode == "sparse")
    assert torch.equal(yt.cpu(), y)
    ftypes = trainer.feature_types
    ftypes = None if ftypes is None else ftypes.cpu()
    assert (ftypes is not None) == (mode == "cat")
    # binned exactly as a training block is
    if mode == "sparse":
        want_bins = gbt.quantize(X * mask, 16, ftypes)
        assert torch.equal(bins.to("cpu").to_dense_bins(), want_bins)
    else:
        assert torch.equal(bins.cpu(), gbt.quantize(X, 16, ftypes))
    n_trees = 3 * 6 if mode == "multiclass" else 6
    assert s["num_trees"] == n_trees
    want = gbt_recomputed(trainer)
    print(f"{mode}: {key} {s[key]!r}, recomputed {want!r}")
    assert s[key] == want and math.isfinite(want)
    if mode == "dense":
        empty = float((y * y).mean())
        print(f"dense: test_mse {s[key]:.4f}, empty forest {empty:.4f}, "
              f"train mse {s['mse']:.4f}")
        assert s[key] < empty
    if mode == "cat":
        assert any(-2 in t.threshold for t in trainer.forest)
