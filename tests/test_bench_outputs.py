"""bench.py --dump-outputs: the result planes of the last timed step as .npy files, within 64 MB, the same cells
from run to run; --steps as the number of timed steps; and a plain run as the headline alone, the rest behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _result(h, w, seed):
    return np.random.default_rng(seed).standard_normal((4, h, w))


def test_small_results_are_written_whole(tmp_path):
    r = _result(30, 20, 1)
    arrays, manifest = bench.result_sample([("", r)])
    assert sorted(arrays) == sorted(bench.RESULT_PLANES) and manifest["sample"] is None
    for k, name in enumerate(bench.RESULT_PLANES):
        assert arrays[name].dtype == np.float64 and np.array_equal(arrays[name], r[k])
    line = bench.write_outputs(str(tmp_path), (arrays, manifest))
    assert not line["sampled"] and line["files"] == sorted(bench.RESULT_PLANES)
    for k, name in enumerate(bench.RESULT_PLANES):
        assert np.array_equal(np.load(tmp_path / (name + ".npy")), r[k])
    assert json.load(open(tmp_path / "outputs.json"))["files"]["amp"]["cells"] == "all"


def test_large_results_are_sampled_within_the_budget(tmp_path):
    budget = 1 << 20
    results = [("scale%g_" % s, _result(300, 400, s)) for s in (5, 10)]
    arrays, manifest = bench.result_sample(results, max_bytes=budget)
    assert manifest["sample"] is not None and len(arrays) == 8
    line = bench.write_outputs(str(tmp_path), (arrays, manifest))
    assert line["sampled"] and line["bytes"] <= budget
    assert sum(os.path.getsize(tmp_path / (n + ".npy")) for n in arrays) <= budget
    # the same cells of every plane, drawn by the documented rule
    k = int(manifest["sample"].split("k = ")[1])
    cells = np.unique(np.random.default_rng(bench.DUMP_SEED).integers(0, 300 * 400, size=k))
    for prefix, r in results:
        for j, name in enumerate(bench.RESULT_PLANES):
            assert np.array_equal(arrays[prefix + name], r[j].reshape(-1)[cells])
    # ... and the same ones on every call
    again, _ = bench.result_sample([(p, r.copy()) for p, r in results], max_bytes=budget)
    assert all(np.array_equal(arrays[n], again[n]) for n in arrays)


def test_the_benchmark_result_fits_64_mb(tmp_path):
    """The headline's result (4 x 10000 x 10000 float64, 3.2 GB; here a broadcast view, no memory) within 64 MB."""
    assert bench.DUMP_MAX_BYTES <= 64 * 10 ** 6
    r = np.broadcast_to(np.arange(4.0)[:, None, None], (4, 10000, 10000))
    line = bench.write_outputs(str(tmp_path), bench.result_sample([("", r)]))
    assert line["sampled"] and line["bytes"] <= bench.DUMP_MAX_BYTES
    assert np.all(np.load(tmp_path / "snr.npy") == 3.0) and np.load(tmp_path / "snr.npy").size > 10 ** 6


def _bench(args, timeout=120):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env,
                          capture_output=True, text=True, timeout=timeout)


def test_steps_below_one_and_emulated_dumps_are_refused():
    """(refused by the argument parser: before any import of the package, no GPU needed)"""
    r = _bench(["--gpus", "1", "--steps", "0"])
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr and "n_gpus" not in r.stdout
    r = _bench(["--gpus", "1", "--emulate-ranks", "2", "--dump-outputs", "x"])
    assert r.returncode != 0 and "--dump-outputs" in r.stderr and "n_gpus" not in r.stdout


@pytest.mark.gpu
def test_dump_outputs_of_a_small_config_repeat(tmp_path):
    """C1 twice with the same arguments: the line counts the steps asked for, and both runs write the same planes
    (whole: 900 x 505 cells), every file float64."""
    lines = []
    for run in ("a", "b"):
        r = _bench(["--gpus", "1", "--config", "C1", "--steps", "3", "--warmup", "1", "--no-verify", "--no-cpu-baseline",
                    "--no-e2e", "--dump-outputs", str(tmp_path / run)], timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    for ln in lines:
        assert ln["steps"] == 3 and ln["outputs"]["files"] == sorted(bench.RESULT_PLANES) and not ln["outputs"]["sampled"]
    for name in bench.RESULT_PLANES:
        a_, b_ = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a_.dtype == np.float64 and a_.shape == (900, 505)
        assert np.array_equal(a_, b_, equal_nan=True), name


def test_a_plain_run_leaves_every_leg_after_the_timed_loop_to_full():
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not a.full and a.no_cpu_baseline and a.no_verify and a.no_e2e and a.no_other_configs
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1", "--full"])
    assert a.full and not (a.no_cpu_baseline or a.no_verify or a.no_e2e or a.no_other_configs)
    a = bench.parse(["--full", "--no-cpu-baseline", "--no-other-configs"])
    assert a.no_cpu_baseline and a.no_other_configs and not (a.no_verify or a.no_e2e)


@pytest.mark.gpu
def test_full_adds_the_checks_to_the_plain_line():
    """C1 plain: the contract's fields and nothing from after the timed loop; C1 --full (CPU baseline left out): the
    same fields, plus the end-to-end call and the oracle's check of the result, which passes."""
    lines = {}
    for run, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline"])):
        r = _bench(["--gpus", "1", "--config", "C1", "--steps", "3", "--warmup", "1"] + extra, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines[run] = json.loads(r.stdout.strip().splitlines()[-1])
    for ln in lines.values():
        assert ln["n_gpus"] == 1 and ln["steps"] == 3 and ln["warmup"] == 1 and ln["dtype"] == "f32"
        assert ln["higher_is_better"] is True and ln["value"] > 0 and ln["ms_per_step"] > 0
        assert ln["config"]["mode"] == "exact" and "settle" in ln and "roofline" in ln
    assert not {"verified", "verification", "end_to_end", "cpu_baseline", "float32_mode", "other_configs"} & set(lines["plain"])
    assert lines["full"]["verified"] is True and lines["full"]["verification"]["cells_off_the_oracle_argmax"] == 0
    assert "end_to_end" in lines["full"] and "cpu_baseline" not in lines["full"]
