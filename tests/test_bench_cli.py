"""bench.py's rank contract (the driver's launch line): `--gpus N` is the number of ranks.  On a box without
N GPUs it must refuse with a message — never print an n_gpus = 1 line for a request of N — and under a launcher whose
WORLD_SIZE disagrees with N it must refuse as well."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def _run(extra_env, *argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(extra_env)
    return subprocess.run([sys.executable, str(ROOT / "bench.py"), *argv], env=env, capture_output=True, text=True, timeout=300)


def test_bare_multi_gpu_request_without_gpus_refuses():
    # one GPU more than this node shows (at least 2: --gpus 1 starts no ranks), counted in a child as bench.py counts them
    c = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count() if torch.cuda.is_available() else 0)"],
                       capture_output=True, text=True, timeout=300)
    have = int(c.stdout.strip().splitlines()[-1])
    want = max(2, have + 1)
    r = _run({}, "--gpus", str(want), "--steps", "1", "--warmup", "0")
    assert r.returncode != 0
    assert f"--gpus {want} needs {want} MI355X" in r.stderr and f"found {have}" in r.stderr
    assert '"n_gpus"' not in r.stdout


def test_world_size_mismatch_refuses():
    r = _run({"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"}, "--gpus", "2")
    assert r.returncode != 0 and "WORLD_SIZE=4" in r.stderr
    assert '"n_gpus"' not in r.stdout


def test_launcher_command_line(monkeypatch):
    """With enough devices the bare process starts torch.distributed.run with one rank per GPU on 127.0.0.1 as a fresh child
    process and exits with its status."""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 8)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    seen = {}

    def fake_call(argv, env):
        seen["argv"], seen["env"] = argv, env
        return 3

    monkeypatch.setattr(bench.subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7"])
    with pytest.raises(SystemExit) as e:
        bench.launch_ranks_if_needed(types.SimpleNamespace(gpus=4))
    assert e.value.code == 3          # the child's exit status is this process's
    a = seen["argv"]
    assert a[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in a and "--nnodes=1" in a
    assert a[a.index("--master-addr") + 1] == "127.0.0.1"
    assert a[-4:] == ["--gpus", "4", "--steps", "7"] and a[-5].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_multi_gpu_default_is_the_north_star_metric_strong_scaling_of_the_4096_batch():
    """`bench.py --gpus N` (the driver's line) measures "a batch of 4096 instances at 1 / 2 / 4 / 8 MI355X": the 4096 are SPLIT over
    the ranks (512 per GPU at 8, contiguous shards that cover the batch exactly once), the metric string states the total; --weak
    keeps 4096 per GPU and says so."""
    import types
    bench = _bench_module()
    args = types.SimpleNamespace(batch=4096, total_batch=0, weak=False)
    for world in (1, 2, 4, 8):
        covered = []
        for rank in range(world):
            strong, total, B, first = bench.plan_batch(args, world, rank)
            assert strong and total == 4096 and B == 4096 // world
            covered += list(range(first, first + B))
        assert covered == list(range(4096))
        assert bench.metric_string(True, total, B, world, 100) == "MPC+WBC updates/sec (batch=4096, N=100, 12-DoF)"
    strong, total, B, first = bench.plan_batch(types.SimpleNamespace(batch=4096, total_batch=0, weak=True), 8, 3)
    assert (strong, total, B, first) == (False, 32768, 4096, 3 * 4096)
    assert "4096 per GPU x 8 GPUs = 32768" in bench.metric_string(False, total, B, 8, 100)
    strong, total, B, first = bench.plan_batch(types.SimpleNamespace(batch=4096, total_batch=1000, weak=False), 8, 7)
    assert strong and total == 1000 and first + B == 1000   # uneven split: the last shard ends the batch
    with pytest.raises(SystemExit):
        bench.plan_batch(types.SimpleNamespace(batch=4096, total_batch=96, weak=True), 2, 0)


def test_counter_file_is_tied_to_the_kernel_sources():
    """roofline.traffic comes from profiles/pmc_latest.json, collected in a separate rocprofv3 run: the file carries the sha256 of the
    kernel sources it was collected on (+ the commit), and bench.py drops the figure when the running tree's sources differ."""
    import json
    bench = _bench_module()
    fp = bench.source_fingerprint()
    assert len(fp) == 64 and fp == bench.source_fingerprint()
    pj = json.loads((ROOT / "profiles" / "pmc_latest.json").read_text())
    assert "source_sha256" in pj and "git_head" in pj and "tag" in pj


@pytest.mark.gpu
def test_bench_under_the_launcher_goes_through_rccl_even_with_one_rank():
    """The driver's multi-GPU launch line with ONE rank on the one GPU of this box: process group on the nccl (= RCCL) backend,
    barrier, MAX / SUM all-reduces of the timing and the status histograms on device tensors, and the optional all-gather of the
    outputs — the code the 2 / 4 / 8-rank runs execute, minus the peers."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", "29533", str(ROOT / "bench.py"), "--gpus", "1", "--total-batch", "96", "--nodes", "24", "--steps", "4",
                        "--warmup", "1", "--random-cmd", "--gather", "--full", "--no-cpu-baseline", "--no-extras"], env=env, capture_output=True, text=True,
                       timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-2000:]
    j = json.loads(lines[-1])
    assert j["n_gpus"] == 1 and j["scaling"] == "strong" and j["config"]["total_instances"] == 96 and j["config"]["batch_per_gpu"] == 96
    # the line says who took part: one rank in the RCCL all-reduce, one distinct device (N of each on N GPUs — what a SCALE run is audited on)
    assert j["rccl_ranks"] == 1 and isinstance(j["devices"], list) and len(j["devices"]) == 1 and j["devices"][0]
    assert j["metric"] == "MPC+WBC updates/sec (batch=96, N=24, 12-DoF)" and j["value_per_gpu"] == j["value"]
    assert j["gather"]["bytes_per_rank"] > 0 and j["gather"]["ms_per_step"] > 0
    assert j["roofline"]["frac"] > 0 and j["roofline"]["traffic"] is None   # (counter traffic belongs to the 4096 x 100 headline only)
    assert sum(j["solver_state"]["mpc_status_histogram_all_ranks"]) == 96


@pytest.mark.gpu
def test_bench_line_under_the_launcher_keeps_roofline_and_cpu_baseline():
    """With --full, rank 0 prints `roofline` and `cpu_baseline` at ANY world size (the CPU leg runs after the final barrier)."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", "29534", str(ROOT / "bench.py"), "--gpus", "1", "--batch", "64", "--nodes", "24", "--steps", "3",
                        "--warmup", "1", "--full", "--no-extras"], env=env, capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-2000:]
    j = json.loads(lines[-1])
    assert j["scaling"] == "strong" and j["config"]["total_instances"] == 64
    assert j["cpu_baseline"]["value"] > 0 and j["cpu_baseline"]["kind"] == "port" and j["roofline"]["kernel"] in ("k_lq", "k_ric_bwd", "k_ric_fwd")
    assert sum(j["solver_state"]["mpc_status_histogram_all_ranks"]) == 64


def test_dumped_outputs_are_float64_within_budget_on_a_fixed_sample(tmp_path):
    """--dump-outputs: every array of the timed path as <name>.npy in float64, under 64 MiB in all; a batch too large for the budget
    is cut to the same seeded sample of instances in every array and in every run, and `instances` names the rows kept."""
    import numpy as np
    bench = _bench_module()
    rng = np.random.default_rng(0)
    B, N = 4096, 100
    outputs = {"mpc_x": rng.standard_normal((B, N + 1, 22)), "mpc_u": rng.standard_normal((B, N, 22)),
               "wbc_solution": rng.standard_normal((B, 38)), "wbc_status": np.zeros(B, dtype=np.int32),
               "mpc_status": rng.integers(0, 4, B).astype(np.int32), "mpc_performance": rng.standard_normal((B, 4))}
    shapes = bench.dump_outputs(outputs, tmp_path / "a")
    bench.dump_outputs(outputs, tmp_path / "b")
    files = sorted((tmp_path / "a").glob("*.npy"))
    assert sorted(f.stem for f in files) == sorted(list(outputs) + ["instances"]) == sorted(shapes)
    assert sum(f.stat().st_size for f in files) <= 64 << 20
    idx = np.load(tmp_path / "a" / "instances.npy")
    assert idx.dtype == np.float64 and 0 < len(idx) < B and np.all(np.diff(idx) > 0) and idx[-1] < B
    for f in files:
        a = np.load(f)
        assert a.dtype == np.float64 and np.array_equal(a, np.load(tmp_path / "b" / f.name))
        if f.stem != "instances":
            assert np.array_equal(a, outputs[f.stem][idx.astype(np.int64)].astype(np.float64))
    # a batch within the budget is written whole, in instance order; several ranks write side by side
    small = {k: v[:8] for k, v in outputs.items()}
    bench.dump_outputs(small, tmp_path / "c", "_rank1")
    assert np.array_equal(np.load(tmp_path / "c" / "instances_rank1.npy"), np.arange(8))
    assert np.array_equal(np.load(tmp_path / "c" / "mpc_u_rank1.npy"), small["mpc_u"])


@pytest.mark.gpu
def test_plain_bench_line_is_the_headline_and_dumps_the_same_outputs_every_run(tmp_path):
    """A plain run prints the headline line only (the rest is behind --full), takes --steps timed steps, and --dump-outputs writes
    what the timed path computed in its last step: the same arrays, bit for bit, in two runs with the same arguments."""
    import json
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--batch", "256", "--nodes", "24", "--steps", "5",
                            "--warmup", "2", "--dump-outputs", str(tmp_path / d)], env=env, capture_output=True, text=True, timeout=600)
        out = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert r.returncode == 0 and out, r.stdout[-2000:] + r.stderr[-2000:]
        lines.append(json.loads(out[-1]))
    j = lines[0]
    assert j["unit"] == "updates/s" and j["higher_is_better"] is True and j["dtype"] == "f64" and j["steps"] == 5
    assert j["metric"] == "MPC+WBC updates/sec (batch=256, N=24, 12-DoF)" and j["ms_per_step"] > 0
    assert abs(j["value"] - 256 / (j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]
    assert not {"roofline", "phase_ms", "halves", "solver_state", "cpu_baseline", "config1_latency_ms"} & set(j)
    names = sorted(f.name for f in (tmp_path / "a").glob("*.npy"))
    assert names == sorted(f"{k}.npy" for k in ("mpc_x", "mpc_u", "wbc_solution", "wbc_status", "mpc_status", "mpc_performance", "instances"))
    assert sorted(j["dumped_outputs"]["arrays"]) == sorted(n[:-4] for n in names)
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float64 and a.shape[0] == 256 and np.array_equal(a, b), n
    assert np.isfinite(np.load(tmp_path / "a" / "mpc_x.npy")).all() and np.load(tmp_path / "a" / "wbc_status.npy").max() == 0
