"""The driver depends on bench.py's JSON line contract — lock it down."""

import json
import subprocess
import sys
from pathlib import Path

REPO = str(Path(__file__).resolve().parents[1])


def test_bench_json_contract():
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
         "--nmf-cols", "512", "--nmf-rows-per-batch", "64",
         "--nmf-nnz-per-row", "8", "--mlr-features", "64",
         "--mlr-batch", "64", "--lda-vocab", "500",
         "--lda-docs-per-batch", "32", "--lda-tokens-per-doc", "8"],
        capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.strip().splitlines()[-1]
    d = json.loads(line)
    assert d["metric"] == "aggregate_examples_per_sec_3job"
    assert isinstance(d["value"], float) and d["value"] > 0
    assert d["unit"] == "examples/s"
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["ms_per_step"] > 0 and d["makespan_sec"] > 0
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["vs_baseline"] is None          # no published baseline
    assert d["dtype"] == "fp32" and d["data"] == "synthetic"
    cfg = d["config"]
    assert "nmf" in cfg and "mlr" in cfg and "lda" in cfg
    assert cfg["parallelism"] == "ps-dp1"
    assert cfg["global_batch"] > 0
    # value is the WHOLE-JOB aggregate: examples per step x steps / elapsed
    assert abs(d["value"] * d["makespan_sec"]
               - cfg["global_batch"] * d["steps"]) < 1e-3 * d["value"]


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last step's arrays as float32 .npy, the
    same from run to run (seeded inputs, fixed step count); --full is
    accepted and leaves the result line's contract alone."""
    import numpy as np

    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        out = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--device", "cpu",
             "--steps", "3", "--warmup", "1",
             "--dump-outputs", str(tmp_path / name),
             "--nmf-cols", "512", "--nmf-rows-per-batch", "64",
             "--nmf-nnz-per-row", "8", "--mlr-features", "64",
             "--mlr-batch", "64", "--lda-vocab", "500",
             "--lda-docs-per-batch", "32", "--lda-tokens-per-doc", "8"]
            + extra, capture_output=True, text=True, timeout=300, cwd=REPO)
        assert out.returncode == 0, out.stderr[-2000:]
        d = json.loads(out.stdout.strip().splitlines()[-1])
        assert d["metric"] == "aggregate_examples_per_sec_3job"
        assert d["steps"] == 3 and d["ms_per_step"] > 0
        assert abs(d["ms_per_step"] * d["steps"]
                   - d["makespan_sec"] * 1e3) < 1e-6 * d["makespan_sec"] * 1e3
        files = sorted(p.name for p in (tmp_path / name).iterdir())
        assert files == ["lda_assignments.npy", "lda_doc_topic.npy",
                         "lda_model.npy", "mlr_grad.npy", "mlr_model.npy",
                         "nmf_L.npy", "nmf_model.npy", "nmf_rgrad.npy"]
        dumps.append({f: np.load(tmp_path / name / f) for f in files})
    a, b = dumps
    assert sum(x.nbytes for x in a.values()) <= 64e6
    for f, x in a.items():
        assert x.dtype == np.float32 and x.size > 0, f
        assert np.isfinite(x).all(), f
        assert np.array_equal(x, b[f]), f
    assert a["mlr_model.npy"].shape == (10 * 8, 64 // 8)
    assert np.abs(a["mlr_grad.npy"]).max() > 0


def test_bench_dump_samples_large_arrays(tmp_path):
    """An array over the per-array cap keeps a fixed sample of its rows."""
    import importlib.util

    import numpy as np
    import torch

    spec = importlib.util.spec_from_file_location("bench", REPO + "/bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rows = bench.DUMP_ARRAY_BYTES // 4 // 8 + 1000   # 8 floats a row: over
    big = torch.arange(rows * 8, dtype=torch.float64).view(rows, 8) % 1000
    bench.dump_outputs(str(tmp_path), {"big": big.to(torch.int32),
                                       "small": big[:3]})
    got = np.load(tmp_path / "big.npy")
    small = np.load(tmp_path / "small.npy")
    assert got.dtype == np.float32 and got.nbytes <= bench.DUMP_ARRAY_BYTES
    assert got.shape == (bench.DUMP_ARRAY_BYTES // 32, 8)
    idx = np.sort(np.random.default_rng(0).choice(
        rows, size=got.shape[0], replace=False))
    assert np.array_equal(got, big.numpy()[idx].astype(np.float32))
    assert small.dtype == np.float64 and small.shape == (3, 8)


def test_bench_runtime_mode_contract():
    """--mode runtime drives the same jobs through run_job/WorkerTasklet
    (benchmark through the real runtime)."""
    out = subprocess.run(
        [sys.executable, "bench.py", "--mode", "runtime", "--steps", "2",
         "--nmf-cols", "512", "--nmf-rows-per-batch", "64",
         "--nmf-nnz-per-row", "8", "--mlr-features", "64",
         "--mlr-batch", "64", "--lda-vocab", "500",
         "--lda-docs-per-batch", "32", "--lda-tokens-per-doc", "8"],
        capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.strip().splitlines()[-1]
    d = json.loads(line)
    assert d["metric"] == "aggregate_examples_per_sec_3job_runtime"
    assert d["value"] > 0
    for job in ("nmf", "mlr", "lda"):
        pj = d["per_job"][job]
        assert pj["examples_per_sec"] > 0 and pj["timed_epochs"] >= 1


def test_bench_elastic_contract():
    """--mode runtime --elastic at world 2: the timeline shows the
    stopped rank's zero-example window and recovery (BASELINE config #5
    through the bench contract)."""
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29734", "bench.py", "--mode", "runtime",
         "--elastic", "--gpus", "2", "--steps", "40", "--device", "cpu",
         "--apps", "nmf,mlr", "--nmf-cols", "2048",
         "--nmf-rows-per-batch", "256", "--nmf-nnz-per-row", "8",
         "--mlr-features", "512", "--mlr-batch", "256"],
        capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if '"metric"' in l][-1]
    d = json.loads(line)
    tl = d["elastic_timeline"]
    assert tl is not None and len(tl) == 2
    ex1 = [row[3] for row in tl[1]]
    assert 0 in ex1, ex1[:8]            # rank 1 truly stopped mid-run
    assert ex1[0] > 0 and ex1[-1] > 0   # worked at both ends (restarted)


def test_bench_direct_world2_torchrun():
    """The driver's SCALE invocation shape: direct mode under torchrun at
    world 2 (tickets + collectives + clock-warm loop all engaged)."""
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29734", "bench.py", "--gpus", "2",
         "--device", "cpu", "--steps", "3", "--warmup", "1",
         "--nmf-rows-per-batch", "64", "--nmf-cols", "256",
         "--mlr-batch", "64", "--mlr-features", "64",
         "--lda-docs-per-batch", "32", "--lda-vocab", "500",
         "--lda-tokens-per-doc", "8"],
        capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["metric"] == "aggregate_examples_per_sec_3job"
    assert d["n_gpus"] == 2 and d["value"] > 0
