"""CPU tests of bench.py's command line: arguments it cannot honour are refused before any device is touched."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("args", [["--steps", "0"], ["--steps", "-3"], ["--warmup", "-1"], ["--full", "--steps", "0"]])
def test_bench_refuses_step_counts_it_cannot_time(args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 2 and "--steps must be >= 1" in out.stderr, out.stderr[-2000:]
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]
