"""Writes record_before_one_front.npz: what the cases of tests/test_gpu_recheck_pins.py return on an MI355X at the commit that is
checked out.  Run at the commit to pin, with that module and this file in place:

    python tests/golden/recheck/record.py tests/golden/recheck/record_before_one_front.npz [--commit <sha>]

(the commit is read from ``git rev-parse HEAD``; ``--commit`` names it where the tree travels without its history, and is refused
where it contradicts the history).  Every single-process case runs twice on one engine, in two orders, and the two runs must agree: a
value that depended on what the engine did before could not be pinned."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [ROOT, TESTS]

import test_gpu_recheck_pins as pins  # noqa: E402


def single_process(eng, order):
    flat, checks = {}, []
    cases = [(n, pins.run_f32, n, pins.check_f32) for n in pins.F32_CASES] + [(pins._f64_id(c), pins.run_f64, c, pins.check_f64) for c in pins.F64_CASES]
    for name, run, arg, check in cases[::order]:
        got = run(eng, arg)
        flat.update(pins.arrays(name, got))
        checks.append((name, check, got))
    return flat, checks


def main():
    import safebo_amd
    ap = argparse.ArgumentParser()
    ap.add_argument("record", metavar="PATH")
    ap.add_argument("--commit", help="the commit of the tree, where git cannot tell")
    a = ap.parse_args()
    try:
        git = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        head = git.stdout.strip() if git.returncode == 0 else None
    except OSError:
        head = None
    if head is None and not a.commit:
        ap.error("no git history here: name the commit with --commit")
    if head is not None and a.commit and a.commit != head:
        ap.error(f"--commit {a.commit} is not HEAD ({head})")
    with safebo_amd.SweepEngine(0) as eng:
        eng.set_option("guard_audit_every", 1)             # (as the suite's engine: tests/conftest.py)
        flat, checks = single_process(eng, 1)
        again, _ = single_process(eng, -1)
    differ = sorted(k for k in flat if flat[k].shape != again[k].shape or not np.array_equal(flat[k], again[k]))
    with tempfile.TemporaryDirectory() as tmp:
        flat.update(pins.arrays("ranks2_B128_f32", pins.run_ranks(tmp)))
    os.makedirs(os.path.dirname(os.path.abspath(a.record)), exist_ok=True)
    np.savez_compressed(a.record, commit=np.array([head or a.commit]), **pins.pack(flat))
    print(f"{a.record}: {len(flat)} entries, {os.path.getsize(a.record)} bytes")
    for name, check, got in checks:
        print(name, {step: (v["profile_posterior_kernel"], v["profile_fp64_rechecks"], v["guard_rechecks"], v["guard_passes"],
                            v["profile_posterior_launches"], v["profile_host_syncs"]) for step, v in got.items()})
    assert not differ, f"entries that depend on the engine's history: {differ}"
    for name, check, got in checks:
        check(got)


if __name__ == "__main__":
    main()
