"""bench.py's rank launcher on CPU: `--gpus N` must itself start N ranks (VERDICT r01 / ADVICE r01: it used to parse
--gpus and ignore it), and a torchrun environment whose WORLD_SIZE differs from --gpus must fail loudly.  The ranks run
bench.py's DPF_BENCH_SELFTEST path over gloo: no GPU work, only the rendezvous and the two reductions the timed path uses."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, extra_env):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(extra_env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=300)


def test_gpus_flag_launches_that_many_ranks():
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "1"], {"DPF_BENCH_SELFTEST": "1", "DPF_BENCH_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout                      # rank 0 prints ONE line
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["max_rank_plus_1"] == 2.0 and out["flat_sum_ok"]


def test_world_size_mismatch_is_an_error():
    r = _run(["--gpus", "4"], {"DPF_BENCH_SELFTEST": "1", "DPF_BENCH_BACKEND": "gloo", "WORLD_SIZE": "2", "RANK": "0",
                               "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29999"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout)


def test_a_stalled_rank_ends_the_job_with_a_diagnosis():
    """rank 1 never reaches the first all-reduce; its watchdog prints where it stands and ends it (status 86),
    the launcher tears the job down and exits non-zero -- in seconds, not after the process group's timeout."""
    import time
    t0 = time.time()
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "1"], {"DPF_BENCH_SELFTEST": "1", "DPF_BENCH_BACKEND": "gloo",
                                                               "DPF_BENCH_SELFTEST_STALL_RANK": "1", "DPF_BENCH_WATCHDOG_S": "4"})
    assert r.returncode != 0
    dumps = [json.loads(ln) for ln in r.stderr.splitlines() if ln.startswith("{") and "watchdog" in ln]
    assert dumps and any(d["rank"] == 1 and "before the first all-reduce" in d["last_stage"] for d in dumps), r.stderr[-1500:]
    assert time.time() - t0 < 120


def test_the_launcher_bounds_the_whole_job():
    r = _run(["--gpus", "2"], {"DPF_BENCH_SELFTEST": "1", "DPF_BENCH_BACKEND": "gloo", "DPF_BENCH_SELFTEST_STALL_RANK": "0",
                               "DPF_BENCH_WATCHDOG_S": "0", "DPF_BENCH_LAUNCH_TIMEOUT_S": "20"})
    assert r.returncode == 124 and '"launcher": "timeout"' in r.stderr


def test_single_process_needs_no_launcher():
    r = _run(["--gpus", "1"], {"DPF_BENCH_SELFTEST": "1", "DPF_BENCH_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])["n_gpus"] == 1


def test_config_defaults():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse([])
    assert (a.config, a.layers, a.points, a.latent, a.steps, a.warmup) == ("cfg2", 14, 2048, 128, 1000, 300)
    a = bench.parse(["--config", "cfg3", "--layers", "63"])
    assert (a.latent, a.layers) == (512, 63)
    a = bench.parse(["--config", "cfg4"])
    assert (a.latent, a.points, a.layers) == (512, 2048, 14)
    a = bench.parse(["--config", "cfg5"])
    assert (a.points, a.steps) == (8192, 10)
    a = bench.parse(["--leg", "train"])
    assert a.layers == 63


def test_a_stall_behind_the_measured_line_does_not_lose_it():
    """The headline is measured before the extra legs: a rank 0 that stalls in one of them still prints its line (marked, with
    the watchdog's dump inside) and the job still ends with the watchdog's status."""
    r = _run(["--gpus", "1"], {"DPF_BENCH_SELFTEST": "1", "DPF_BENCH_BACKEND": "gloo", "DPF_BENCH_SELFTEST_STALL_AFTER_LINE": "1",
                               "DPF_BENCH_WATCHDOG_S": "3"})
    assert r.returncode == 86, (r.returncode, r.stderr[-1500:])
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and lines[0]["selftest"] and lines[0]["n_gpus"] == 1
    wd = lines[0]["extra"]["watchdog"]
    assert wd["rank"] == 0 and "behind the measured line" in wd["last_stage"] and "stalled" in lines[0]["extra"]["note"]


def test_plain_run_is_lean_and_full_is_opt_in():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path):
    """float32 stays float32, integer indices become exact float64, and an array over its share of the 64 MB budget is
    written as the same seeded sample every time."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    pts = torch.randn(2, 3, 5)
    idx = torch.tensor([[0, 7, 2**24 + 1]], dtype=torch.int32)
    big = torch.arange(bench.DUMP_BUDGET_BYTES // 8 + 100, dtype=torch.float64)      # element i holds i: positions stay readable
    arrays = {"points": pts, "idx": idx, "big": big}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    p = np.load(tmp_path / "a" / "points.npy")
    assert p.dtype == np.float32 and np.array_equal(p, pts.numpy())
    i = np.load(tmp_path / "a" / "idx.npy")
    assert i.dtype == np.float64 and np.array_equal(i, idx.numpy().astype(np.float64))
    total = sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in arrays)
    assert total <= bench.DUMP_BUDGET_BYTES + 3 * 128
    s1, s2 = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert s1.dtype == np.float64 and s1.size < big.numel() and np.array_equal(s1, s2)
    assert np.all(np.diff(s1) > 0) and s1[0] >= 0 and s1[-1] < big.numel()
