"""bench.py end to end on a small graph: the JSON line carries the driver's contract (metric, value, n_gpus, roofline with
algorithmic bytes / HIP-event durations, cpu_baseline from the oracle), plain and under torch.distributed.run."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=dict(os.environ, MASTER_ADDR="127.0.0.1"))
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_bench_contract_small_graph():
    d = _run([sys.executable, "bench.py", "--graph", "small", "--queries", "64", "--steps", "2", "--warmup", "1", "--cpu-seconds", "2",
              "--full"])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["value"] > 0 and d["vs_baseline"] is None
    assert "workload" in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert r["algorithmic_counts"].startswith("sequential FIFO oracle")
    assert r["fifo_relaxations_per_query"] <= r["gpu_relaxations_per_query"]   # the schedule's extra work is not credited
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and "sample" in c
    assert d["accuracy"]["holds"] and d["accuracy"]["cpu_vs_gpu_exact_linf"] < 1e-9


def test_bench_topk_and_torchrun_rank():
    d = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
              "--master-port", "29633", "bench.py", "--gpus", "1", "--graph", "small", "--queries", "32", "--topk", "50", "--with-idx",
              "--steps", "1", "--warmup", "1", "--scaling", "strong", "--full"])
    assert d["n_gpus"] == 1 and d["scaling"] == "strong" and d["config"]["k"] == 50 and d["value"] > 0
    assert d["config"]["gather_bytes_per_step"] == 32 * 50 * 12
    # the top-k line carries a roofline of its pushes on FIFO top-k push counts (oracle: orc_topk_push_counts with the GPU run's rounds)
    r = d["roofline"]
    assert r is not None and r["bound"] == "hbm" and 0 < r["frac"] < 1 and "FIFO top-k pushes" in r["algorithmic_counts"]


def test_bench_plain_line_and_dump_outputs(tmp_path):
    """Without --full the line carries the headline and nothing that needs runs of its own; --dump-outputs writes what the
    last timed step computed, the same from run to run."""
    import numpy as np
    args = ["bench.py", "--graph", "small", "--queries", "64", "--steps", "3", "--warmup", "1"]
    d = _run([sys.executable, *args, "--dump-outputs", str(tmp_path / "a")])
    assert d["steps"] == 3 and d["value"] > 0 and abs(d["ms_per_step"] - 1e3 * 64 / d["value"]) < 1e-6 * d["ms_per_step"]
    for k in ("cpu_baseline", "cpu_baseline_all_cores", "accuracy", "variants", "configs"):
        assert k not in d, k
    _run([sys.executable, *args, "--dump-outputs", str(tmp_path / "b")])
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "b").iterdir())
    out = {n: np.load(tmp_path / "a" / n) for n in names}
    for n, a in out.items():
        assert a.dtype == np.float64 and np.array_equal(a, np.load(tmp_path / "b" / n)), n
    assert out["stats_n_walks.npy"].shape == (64,) and (out["stats_ppr_sum_fix.npy"] == 2.0 ** 62).all()
    assert out["ppr.npy"].shape == (8, 32_000) and np.allclose(out["ppr.npy"].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    t = tmp_path / "topk"
    _run([sys.executable, "bench.py", "--graph", "small", "--queries", "16", "--topk", "20", "--with-idx", "--steps", "1", "--warmup", "1",
          "--dump-outputs", str(t)])
    ids, sc = np.load(t / "topk_ids.npy"), np.load(t / "topk_scores.npy")
    assert ids.shape == sc.shape == (16, 20) and (np.diff(sc, axis=1) <= 0).all() and np.load(t / "topk_rounds.npy").shape == (16,)


def test_bench_line_names_the_walk_bound_and_its_sources():
    d = _run([sys.executable, "bench.py", "--graph", "small", "--queries", "64", "--steps", "2", "--warmup", "1", "--no-cpu", "--no-accuracy", "--no-variants"])
    w = d["walk_bound"]  # the dominant kernel of the headline step: gathers per second, not an HBM fraction
    assert w["gathers_per_s"] > 0 and w["steps"] > 0 and "k_walk_dg" in w["kernel"]
