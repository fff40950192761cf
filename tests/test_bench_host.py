"""Host-side pieces of bench.py that need no GPU: the algorithmic byte count, the rule that a PMC
summary of an older kernel source is never reported as this kernel's traffic, and the CPU leg's thread count."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_algorithmic_bytes_follow_the_survey_formula():
    # 36 B read + 64 B matrix + 1 visibility bit + 20 B per emitted command
    assert bench.algorithmic_bytes_per_instance(0.0) == pytest.approx(100.125)
    assert bench.algorithmic_bytes_per_instance(1.0) == pytest.approx(120.125)
    assert bench.algorithmic_bytes_per_instance(0.268553) == pytest.approx(100.125 + 20 * 0.268553)


def test_committed_pmc_summary_belongs_to_the_committed_kernel():
    """profiles/r02_cfg3_pmc_summary.json must have been collected from the kernel sources in this tree; otherwise
    bench.py would print traffic = null ("stale") on the driver's run."""
    row, stale = bench.pmc_traffic(3, 1_000_000)
    if row is None:  # mid-development state: visible, not fatal (bench.py then says "stale", never a wrong number)
        pytest.skip(f"no PMC summary matches the kernel source hash {bench.kernel_source_sha()} (stale: {stale}): "
                    "re-run tools/r02_profiles.sh on the GPU box and copy the summary into profiles/")
    assert 0.98 < row["hbm_bytes_per_launch"] / (1_000_000 * bench.algorithmic_bytes_per_instance(0.268553)) < 1.10


def test_a_summary_of_another_kernel_is_reported_stale_not_as_traffic(monkeypatch):
    monkeypatch.setattr(bench, "kernel_source_sha", lambda: "0" * 16)
    row, stale = bench.pmc_traffic(3, 1_000_000)
    assert row is None and stale and stale.endswith("pmc_summary.json")


def test_cpu_leg_thread_count_is_bounded(monkeypatch):
    monkeypatch.setenv("MIP_BENCH_MAX_THREADS", "3")
    assert 1 <= bench.host_cores() <= 3


def test_committed_bench_line_carries_the_contract_fields():
    line = json.load(open(os.path.join(ROOT, "profiles", "r03_bench_default.json")))
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline", "parity"):
        assert key in line, key
    assert line["config"]["workload"].startswith("mixed 64-mesh scene, 1 M instances") and line["vs_baseline"] is None
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert line["cpu_baseline"]["kind"] == "port" and "unpinned" in line["parity"]


def test_steps_sets_the_number_of_timed_steps():
    for steps in (1, 5, 19, 20, 39, 40, 41, 999, 1000, 1001, 20_000):
        batches = bench.split_steps(steps, 50)
        assert sum(batches) == steps and 1 <= len(batches) <= 50
        assert min(batches) >= min(steps, bench.STEPS_PER_SAMPLE) and max(batches) - min(batches) <= 1
    assert bench.split_steps(1000, 50) == [20] * 50  # the batches the headline was always timed in


def test_a_plain_run_measures_the_headline_only(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "10", "--warmup", "2"])
    args = bench.parse_args()
    assert not args.full and args.dump_outputs is None and args.steps == 10


def test_dumped_outputs_are_exact_bounded_and_repeatable(tmp_path):
    """--dump-outputs at the headline's size: float32 / float64 files only, integers exact, under 64 MB, and the model
    rows sampled the same way on every run."""
    n, count = 1_000_000, 268_553
    rng = np.random.default_rng(1)
    cmds = rng.integers(0, 2**32, size=(count, 5), dtype=np.uint32)
    outs = {"model": rng.standard_normal((n, 16)).astype(np.float32), "visible_bitmap": rng.integers(0, 2**32, (n + 31) // 32, dtype=np.uint32),
            "draw_cmds": cmds, "draw_count": np.array([count], np.uint32), "draw_index_total": np.array([2**32 - 1], np.uint32)}
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), outs)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.OUTPUT_BYTES_MAX
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    for f in files:
        assert np.array_equal(got[f[:-4]], np.load(tmp_path / "b" / f))
        assert got[f[:-4]].dtype in (np.float32, np.float64), f
    assert np.array_equal(got["draw_cmds"], cmds.astype(np.float64)) and got["draw_index_total"][0] == 2**32 - 1
    rows = got["model_rows"].astype(np.int64)
    assert len(rows) == bench.OUTPUT_ROW_LIMITS["model"] and np.all(np.diff(rows) > 0)
    assert np.array_equal(got["model"], outs["model"][rows])


def _run_bench(argv, env_extra, drop=("WORLD_SIZE", "RANK", "LOCAL_RANK", "MIP_BENCH_FORCE_DIST")):
    import subprocess

    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True, text=True, timeout=300)


def test_gpus_n_without_a_launcher_never_prints_a_single_gpu_line():
    """VERDICT r02 'missing 4': `python bench.py --gpus 8` started plainly used to run the 1-GPU leg and print
    n_gpus = 1. Now it launches N child ranks itself — and on a node with fewer GPUs it exits non-zero with
    nothing on stdout."""
    import torch

    if torch.cuda.device_count() >= 2:
        pytest.skip("this node has the GPUs: the call would run the real bench")
    r = _run_bench(["--gpus", "2", "--steps", "1"], {})
    assert r.returncode != 0 and r.stdout.strip() == "" and "no line printed" in r.stderr


def test_world_size_that_disagrees_with_gpus_prints_no_line():
    r = _run_bench(["--gpus", "2"], {"WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode != 0 and r.stdout.strip() == "" and "WORLD_SIZE 1" in r.stderr
    r = _run_bench(["--gpus", "1"], {"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode != 0 and r.stdout.strip() == "" and "WORLD_SIZE 2" in r.stderr


def test_spawned_ranks_get_the_callers_arguments(monkeypatch):
    """The launcher is a child process (no exec from this one) and carries the caller's arguments through."""
    import subprocess

    import torch

    seen = {}
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 4)
    monkeypatch.setattr(subprocess, "call", lambda cmd, env=None: seen.update(cmd=cmd, env=env) or 7)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "2"])
    args = bench.parse_args()
    assert bench.spawn_ranks(args) == 7  # the launcher's exit code is passed on
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "2"] and cmd[-7].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
