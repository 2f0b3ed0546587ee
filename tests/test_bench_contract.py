"""bench.py's launch contract (round-1 verdict, item 1a): `--gpus N` never reports a job smaller than the one asked
for — it starts N ranks itself or exits non-zero — and the JSON line carries the agreed blocks."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra=None, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=env, timeout=timeout)


def test_more_gpus_than_devices_is_refused_not_downgraded():
    """Asking for more GPUs than the box has must fail loudly (here: 0 or 1 device), never run one rank and print a line."""
    sys.path.insert(0, ROOT)
    import bench
    have = bench.visible_gpu_count()   # counted from the KFD topology: the launcher never loads the HIP runtime
    r = _run(["--gpus", str(have + 2), "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert "n_gpus" not in r.stdout
    assert "refusing" in r.stderr


def test_world_size_mismatch_is_refused():
    r = _run(["--gpus", "4", "--steps", "1"], env_extra={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "n_gpus" not in r.stdout
    assert "WORLD_SIZE=2" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_bench_line_has_the_agreed_blocks():
    """A small run of the real thing (20k points, RCCL initialised with one rank): one JSON line with the median-of-
    windows value, roofline + traffic source, both CPU baselines, cold-start times, the converged-inner block and parity."""
    r = _run(["--full", "--n", "20000", "--steps", "4", "--warmup", "2", "--windows", "3", "--force-dist", "--cpu-iters", "3"])
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1
    out = json.loads(line[0])
    assert out["n_gpus"] == 1 and out["steps"] == 4 and out["warmup"] == 2 and out["scaling"] == "weak"
    assert out["windows"]["count"] == 3 and len(out["windows"]["it_per_s"]) == 3
    assert out["windows"]["min_it_per_s"] <= out["value"] <= out["windows"]["max_it_per_s"]
    assert abs(out["ms_per_step"] * out["steps"] - out["windows"]["window_ms"]) < 1e-9
    assert out["roofline"]["bound"] == "hbm" and 0 < out["roofline"]["frac"] < 1 and "traffic_source" in out["roofline"]
    assert out["cpu_baseline"]["kind"] == "port" and out["cpu_baseline"]["value"] > 0
    assert out["cpu_baseline_refshape"]["cores"] == 1 and out["cpu_baseline_refshape"]["value"] > 0
    assert len(out["cold_ms_per_iteration"]) == 5
    assert out["converged_inner"]["mean_inner_steps"] >= 1 and out["converged_inner"]["it_per_s"] > 0
    assert out["parity"]["rot_err_rad"] < 1e-5 and out["parity"]["trans_err_m"] < 1e-5
    assert out["gathered_transforms"] == 1
    # round 3: the timed instantiation is the roofline's kernel (stand-alone figure beside it), set-up cost per pair,
    # window spread, and the C++ classes timed in a child process on both inner schedules
    assert "folded in" in out["roofline"]["kernel"] and out["roofline"]["standalone"]["avg_kernel_ms"] > 0
    assert out["setup_ms"]["total"] > 0 and out["setup_ms"]["grid_and_source_sort_kernels"] > 0
    assert out["windows"]["spread"] >= 0 and "settle" in out["windows"]
    for key in ("inner_steps_1", "default_inner_to_f_tol"):
        assert out["cpp_api"][key]["steady_it_per_s"] > 0, out["cpp_api"]


def test_launcher_counts_devices_without_the_hip_runtime():
    """spawn_ranks' device count must not load libamdhip64 (the parent of the ranks stays GPU-clean)."""
    code = ("import sys; sys.path.insert(0, %r); import bench; n = bench.visible_gpu_count(); "
            "import os; maps = open('/proc/self/maps').read(); "
            "assert 'libamdhip64' not in maps and 'libhsa-runtime' not in maps, 'HIP/HSA runtime loaded'; print(n)") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert int(r.stdout.strip()) >= 0


def test_dump_outputs_writes_the_last_windows_arrays(tmp_path):
    """--dump-outputs on the rank logic's CPU stand-in: float64 arrays of the last timed call, shaped by --steps, equal
    from run to run; a plain line carries the headline fields and none of the --full blocks."""
    import numpy as np
    dumps = []
    for d in ("a", "b"):
        r = _run(["--gpus", "1", "--points", "300", "--steps", "3", "--warmup", "1", "--windows", "2", "--backend", "gloo",
                  "--fake-register", "--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stdout + r.stderr
        out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in out
        assert out["steps"] == 3 and abs(out["ms_per_step"] * 3 - out["windows"]["window_ms"]) < 1e-9
        for key in ("cpu_baseline", "parity", "converged_inner", "setup_ms", "cpp_api", "cli_default_shapes"):
            assert key not in out
        dumps.append({f: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    assert sorted(dumps[0]) == ["costs.npy", "history.npy", "inner_steps.npy", "transforms.npy"]
    assert dumps[0]["transforms.npy"].shape == (1, 3, 4) and dumps[0]["history.npy"].shape == (1, 3, 3, 4)
    assert np.array_equal(dumps[0]["history.npy"][0, -1], dumps[0]["transforms.npy"][0])
    for f, arr in dumps[0].items():
        assert arr.dtype == np.float64 and np.array_equal(arr, dumps[1][f])


@pytest.mark.gpu
def test_gpu_dump_outputs_of_a_plain_run(tmp_path):
    """The real thing at 20k points: a plain run writes the last window's transforms and per-iteration history."""
    import numpy as np
    r = _run(["--n", "20000", "--steps", "4", "--warmup", "2", "--windows", "2", "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 4 and out["ms_per_step"] > 0 and "cpu_baseline" not in out and "parity" not in out
    T, hist = np.load(tmp_path / "transforms.npy"), np.load(tmp_path / "history.npy")
    assert T.shape == (1, 3, 4) and hist.shape == (1, 4, 3, 4) and T.dtype == hist.dtype == np.float64
    assert np.array_equal(hist[0, -1], T[0]) and np.isfinite(hist).all()
    assert np.load(tmp_path / "costs.npy").shape == (1, 4, 2) and np.load(tmp_path / "inner_steps.npy").shape == (1, 4)
    # a rigid transform came out: R^T R = 1 to rounding
    assert np.abs(T[0][:, :3].T @ T[0][:, :3] - np.eye(3)).max() < 1e-12


@pytest.mark.gpu
def test_steps_past_convergence_are_all_timed(tmp_path):
    """--steps sets the number of timed iterations also where the pair converges long before the window ends (with a
    stopping threshold of 0 the rule ended such a window after some 400 iterations): 1500 steps, 1500 rows of history."""
    import numpy as np
    r = _run(["--n", "20000", "--steps", "1500", "--warmup", "2", "--windows", "2", "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 1500 and abs(out["ms_per_step"] * 1500 - out["windows"]["window_ms"]) < 1e-9
    hist = np.load(tmp_path / "history.npy")
    assert hist.shape == (1, 1500, 3, 4) and np.isfinite(hist).all()


@pytest.mark.gpu
def test_config5_batch_line_small():
    """--config 5 shape at a reduced size: 64 pairs on the one GPU of the test box, every gathered transform verified
    against its single-rank run inside bench.py itself."""
    r = _run(["--full", "--config", "5", "--n", "6000", "--steps", "3", "--warmup", "1", "--windows", "2", "--no-cpu-baseline",
              "--no-extras"])
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert out["config"]["pairs"] == 64 and out["config"]["pairs_per_gpu"] == 64 and out["scaling"] == "strong"
    assert out["gathered_transforms"] == 64
    assert out["batch_verification"]["pairs_checked"] == 64
    assert out["batch_verification"]["max_abs_diff_vs_single_rank_run"] < 1e-9
