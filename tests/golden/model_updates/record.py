"""Writes record_before_one_driver.npz: what the cases of tests/test_gpu_model_update_pins.py give on an MI355X at the commit that is
checked out.  Run at the commit to pin, with that module and this file in place:

    python tests/golden/model_updates/record.py tests/golden/model_updates/record_before_one_driver.npz [--commit <sha>]

(the commit is read from ``git rev-parse HEAD``; ``--commit`` names it where the tree travels without its history, and is refused where
it contradicts the history).  Every case runs twice on one engine, in two orders, and the two runs must agree: a value that depended
on what the engine did before could not be pinned.

    python tests/golden/model_updates/record.py --host tests/golden/model_updates/host_classes_before_helpers.npz

writes, without a GPU, what the cases of tests/test_host_classes.py::test_host_updates_leave_what_they_left_before_the_helpers leave on
the host."""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [ROOT, TESTS]

import test_gpu_model_update_pins as pins  # noqa: E402
from test_gpu_recheck_pins import pack  # noqa: E402


def one_pass(eng, order):
    flat, checks = {}, []
    for name in list(pins.CASES)[::order]:
        got = pins.CASES[name](eng)
        flat.update(pins.arrays(name, got))
        checks.append((name, got))
    return flat, checks


def main():
    import safebo_amd
    ap = argparse.ArgumentParser()
    ap.add_argument("record", metavar="PATH")
    ap.add_argument("--host", action="store_true", help="the host-class states (no GPU), not the device record")
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
    if a.host:
        import test_host_classes as host
        flat = {f"{name}/{k}": v for name in host.HOST_UPDATES for k, v in host.host_update_state(name).items()}
        np.savez_compressed(a.record, commit=np.array([head or a.commit]), **flat)
        print(f"{a.record}: {len(flat)} entries, {os.path.getsize(a.record)} bytes")
        return
    with safebo_amd.SweepEngine(0) as eng:
        eng.set_option("guard_audit_every", 1)             # (as the suite's engine: tests/conftest.py)
        flat, checks = one_pass(eng, 1)
        again, _ = one_pass(eng, -1)
        assert eng.profile()["guard_audit_violations"] == 0
    differ = sorted(k for k in flat if flat[k].shape != again[k].shape or not np.array_equal(flat[k], again[k]))
    for name, got in checks:
        print(name, {step: {k: (np.asarray(v[k]).tolist() if k != "error" else bytes(v[k]).decode()) for k in
                            ("n", "status", "error", "grid_default_kernel", "list_kernel", "sweep_empty", "sweep_count_S", "profile_host_syncs")
                            if k in v} for step, v in got.items()}, flush=True)
    assert not differ, f"entries that depend on the engine's history: {differ}"
    for name, got in checks:
        pins.check_case(name, got)
    os.makedirs(os.path.dirname(os.path.abspath(a.record)), exist_ok=True)
    np.savez_compressed(a.record, commit=np.array([head or a.commit]), **pack(flat))
    print(f"{a.record}: {len(flat)} entries, {os.path.getsize(a.record)} bytes")


if __name__ == "__main__":
    main()
