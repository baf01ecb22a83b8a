"""bench.py's one-line JSON contract (task statement, "Measurement"), exercised end to end on the tiny config so that a
change to the engine cannot silently break the line the driver parses; and __graft_entry__.smoke()."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(*flags):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "tiny", "--steps", "6", "--warmup", "2", *flags],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_line_contract():
    d = _run_bench("--full")
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["unit"] == "tokens/s" and d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "bf16"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - 8 * 6 / (d["ms_per_step"] * 6e-3)) <= 0.02 * d["value"]        # value == tokens / timed seconds
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in r, key
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert "t2i" in d and d["t2i"]["images_per_s"] > 0


def test_bench_plain_run_is_headline_only():
    """Without --full the run measures the headline decode and nothing else: the same headline keys, the step-level roofline
    (arithmetic on the timed step) and no kernel replays or extra legs."""
    d = _run_bench()
    assert d["unit"] == "tokens/s" and d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "bf16"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - 8 * 6 / (d["ms_per_step"] * 6e-3)) <= 0.02 * d["value"]
    assert set(d) == {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                      "dtype", "data", "config", "roofline"}, sorted(d)
    r = d["roofline"]
    assert set(r) == {"bound", "peak", "unit", "step_algorithmic_GBps", "step_frac_of_peak", "step_mfma_frac_of_2500"}, sorted(r)
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and r["step_algorithmic_GBps"] > 0
    assert abs(r["step_frac_of_peak"] - r["step_algorithmic_GBps"] / r["peak"]) < 1e-3


def test_bench_no_graph_and_flags():
    d = _run_bench("--no-graph", "--no-t2i", "--batch", "3")
    assert d["config"]["decode"] == "eager" and d["config"]["batch_per_gpu"] == 3 and "t2i" not in d
    assert d["value"] > 0


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs DIR: the headline decode's timed outputs - every timed step's ids and the last step's logits - as float .npy;
    the last row of ids picks a maximum of the dumped logits (greedy)."""
    import numpy as np
    d = _run_bench("--no-t2i", "--dump-outputs", str(tmp_path))
    ids, logits = np.load(tmp_path / "ids.npy"), np.load(tmp_path / "logits.npy")
    assert ids.dtype == np.float64 and ids.shape == (d["steps"], d["config"]["batch_per_gpu"]) and np.all(ids == np.round(ids))
    assert logits.dtype == np.float32 and logits.shape == (d["config"]["batch_per_gpu"], 320) and np.isfinite(logits).all()
    assert np.array_equal(logits[np.arange(len(logits)), ids[-1].astype(np.int64)], logits.max(-1))    # a maximum (bf16 ties)


def test_graft_entry_smoke():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.smoke()


@pytest.mark.parametrize("gather", ["ids", "logits"])
def test_bench_self_launches_two_ranks(gather):
    """`python bench.py --gpus 2` without torchrun: bench.py spawns its own ranks (unimedvl_amd.launch), they rendezvous on
    127.0.0.1, decode, gather (C1: ids or every step's logits), barrier, take the slowest rank's time and rank 0 prints ONE line
    with n_gpus 2 and twice one rank's tokens.  On the 1-GPU test box both ranks share cuda:0 and the collectives stage through
    host memory over gloo (RCCL needs one device per rank); everything else is the production flow."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(PYTHONDONTWRITEBYTECODE="1", UMV_BENCH_BACKEND="gloo", UMV_BENCH_SHARE_GPU="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "tiny", "--steps", "6", "--warmup", "2",
                        "--gather", gather, "--full"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2" and d["config"]["c1_gather"] == gather
    assert abs(d["value"] - 2 * 8 * 6 / (d["ms_per_step"] * 6e-3)) <= 0.02 * d["value"]    # whole-job tokens / slowest rank's seconds
    assert "cpu_baseline" not in d and d["t2i"]["images_per_s"] > 0


def test_bench_configs3_workload_two_ranks():
    """`python bench.py --workload configs3 --gpus 2`: BASELINE.json configs[3] (32 samples per GPU) through the N-rank flow -
    per-rank CPU binding, rendezvous on 127.0.0.1, 32 samples per rank, ids all-gather, one line with whole-job tokens/s."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(PYTHONDONTWRITEBYTECODE="1", UMV_BENCH_BACKEND="gloo", UMV_BENCH_SHARE_GPU="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "tiny", "--workload", "configs3",
                        "--steps", "8", "--warmup", "2", "--no-t2i"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["batch_per_gpu"] == 32 and d["config"]["parallelism"] == "dp2"
    assert abs(d["value"] - 2 * 32 * 8 / (d["ms_per_step"] * 8e-3)) <= 0.02 * d["value"]
    b = d["config"]["cpu_binding"]
    assert b is not None and ("bound" in b)


def _need_gpus(n):
    """One GPU per rank: oversubscribing a single device with this many GPU-holding processes is not supported."""
    found = torch.cuda.device_count()
    if found < n:
        pytest.skip(f"needs {n} GPUs, found {found}")


def _dry_run_env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(PYTHONDONTWRITEBYTECODE="1", UMV_BENCH_BACKEND="gloo", UMV_BENCH_SHARE_GPU="1")
    return env


def _one_line(p):
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"rank 0 must print exactly ONE line, got {len(lines)}:\n{p.stdout[-2000:]}"
    return json.loads(lines[0])


@pytest.mark.parametrize("flags", [("--gather", "ids"), ("--gather", "logits"), ("--workload", "configs3", "--no-t2i")])
def test_bench_eight_rank_dry_run(flags):
    """The driver's scaling run is `bench.py --gpus 8` on an 8-GPU node, which no lease here has ever had (VERDICT r05 "missing" #2).  This is
    that run at the SAME world size, one GPU per rank (skipped on a node with fewer than 8 GPUs), collectives over gloo - rendezvous on 127.0.0.1,
    bind_rank_to_gpu_socket for 8 ranks over the host's sockets, the (ragged, for configs3) all-gather of ids / of every step's logits at
    world size 8, barrier + max over ranks, ONE line from rank 0 with whole-job tokens.  What stays unexercised is the `nccl` backend itself."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    _need_gpus(8)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--config", "tiny", "--steps", "6", "--warmup", "2", *flags],
                       cwd=ROOT, env=_dry_run_env(), capture_output=True, text=True, timeout=1200)
    d = _one_line(p)
    per_gpu = 32 if "configs3" in flags else 8
    assert d["n_gpus"] == 8 and d["config"]["parallelism"] == "dp8" and d["config"]["batch_per_gpu"] == per_gpu and d["scaling"] == "weak"
    assert abs(d["value"] - 8 * per_gpu * 6 / (d["ms_per_step"] * 6e-3)) <= 0.02 * d["value"]
    assert "cpu_baseline" not in d
    if "--gather" in flags:
        assert d["config"]["c1_gather"] == flags[1]
    b = d["config"].get("cpu_binding")
    assert b is not None and "bound" in b


def test_bench_eight_ranks_under_torch_distributed_run():
    """... and launched the way the driver launches it: `python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1
    --master-port P bench.py --gpus 8 ...` (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment)."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    _need_gpus(8)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
                        "--master-port", "29533", os.path.join(ROOT, "bench.py"), "--gpus", "8", "--config", "tiny", "--steps", "6", "--warmup", "2",
                        "--no-t2i"], cwd=ROOT, env=_dry_run_env(), capture_output=True, text=True, timeout=1200)
    d = _one_line(p)
    assert d["n_gpus"] == 8 and d["config"]["parallelism"] == "dp8"
    assert abs(d["value"] - 8 * 8 * 6 / (d["ms_per_step"] * 6e-3)) <= 0.02 * d["value"]
