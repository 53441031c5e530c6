"""The bench line's contract (task statement): one JSON line with the metric and the roofline of the timed steps; with --full also
the CPU baseline and the records that take runs of their own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_line_contract_on_a_small_run():
    d = _run("--config", "B", "--steps", "6", "--warmup", "2", "--no-extra", "--cpu-sample", "65536", "--full")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["unit"] == "candidates/s" and d["dtype"] == "f64" and d["data"] == "synthetic" and "workload" in d["config"]
    assert abs(d["value"] - 2048 * 2048 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-9
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel_ms", "device_ms_per_step", "set_phase_ms", "set_phase_hbm_frac", "store_roofline_frac"):
        assert k in r, k
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and 0.0 < r["kernel_ms"] < r["device_ms_per_step"] <= d["ms_per_step"]
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "sample" in c and c["unit"] == "candidates/s"
    assert d["config"]["guard_audit_violations"] == 0


def test_plain_run_measures_the_headline_alone():
    """Without --full the default config's run times its steps and reports them, and nothing that takes runs of its own."""
    d = _run("--gpus", "1", "--steps", "4", "--warmup", "2")
    assert d["steps"] == 4 and d["warmup"] == 2 and d["higher_is_better"] is True and d["unit"] == "candidates/s" and d["dtype"] == "f64"
    assert abs(d["value"] - 4096 * 4096 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-9
    for k in ("cpu_baseline", "iteration", "table_kernel", "extra", "comm"):
        assert k not in d, k
    for k in ("full_posterior", "lean_1", "lean_2", "iteration_ms", "iteration_value"):
        assert k not in d["config"], k
    r = d["roofline"]
    for k in ("store_roofline_frac_written", "objective_tiles_with_a_safe_candidate", "table_kernel_frac"):
        assert k not in r, k
    assert "one_stream" not in r["hbm"] and "exposed" not in r["hbm"]
    assert 0.0 < r["kernel_ms"] < r["device_ms_per_step"] <= d["ms_per_step"] and r["set_phase_ms"] == r["set_phase_exposed_ms"]
    assert d["config"]["lean"] == 2 and d["config"]["guard_audit_violations"] == 0 and d["config"]["result"]["guard_band"] == 0


def test_dump_outputs_hold_the_last_timed_result_and_repeat(tmp_path):
    """--dump-outputs: every entry of the last timed sweep's result as float64 .npy, the same files from two runs with the same
    arguments (seeded inputs), and the counts / indices the bench line reports."""
    runs = [_run("--config", "B", "--steps", "3", "--warmup", "1", "--no-extra", "--cpu-sample", "0", "--dump-outputs", str(tmp_path / r))
            for r in ("a", "b")]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "minimizer_index.npy" in names and "u_star.npy" in names
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b), f
    r = runs[1]["config"]["result"]
    assert runs[1]["steps"] == 3
    for k in ("count_S", "count_M", "count_G", "minimizer_index", "expander_index", "expander_index_c"):
        assert np.array_equal(np.load(tmp_path / "b" / f"{k}.npy"), np.asarray(r[k], dtype=np.float64)), k
