"""Writes record_before_steps.npz: what the cases of tests/test_gpu_colpath_pins.py return on an MI355X at the commit that is checked
out.  Run at the commit to pin, with that module and this file in place:

    python tests/golden/colpath_steps/record.py tests/golden/colpath_steps/record_before_steps.npz [--commit <sha>] [--marks PATH]

(the commit is read from ``git rev-parse HEAD``; ``--commit`` names it where the tree travels without its history, and is refused where
it contradicts the history).  Every case runs twice on one engine, in two orders, and the two runs must agree: a value that depended on
what the engine did before could not be pinned.

``--marks PATH``: for a run under a kernel trace.  One pass over the cases, no file written; in front of every sweep a small torch fill
kernel is launched (no sweep launches one) and the sweep's name is appended to PATH, so that the trace can be cut into sweeps: the k-th
fill kernel stands in front of the k-th name."""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [ROOT, TESTS]

import test_gpu_colpath_pins as pins  # noqa: E402
from test_gpu_recheck_pins import pack  # noqa: E402


def one_pass(eng, order):
    flat, checks = {}, []
    for name in list(pins.CASES)[::order]:
        got, kernels = pins.run_case(eng, name)
        flat.update(pins.rpins.arrays(name, got))
        checks.append((name, got, kernels))
    return flat, checks


def marked(path):
    import torch
    buf = torch.zeros(256, device="cuda")
    names = open(path, "w")

    def mark(name):
        torch.cuda.synchronize()
        buf.fill_(1.0)
        torch.cuda.synchronize()
        names.write(name + "\n")
        names.flush()
    return mark


def main():
    import safebo_amd
    ap = argparse.ArgumentParser()
    ap.add_argument("record", metavar="PATH")
    ap.add_argument("--commit", help="the commit of the tree, where git cannot tell")
    ap.add_argument("--marks", metavar="PATH", help="one marked pass for a kernel trace; writes the sweeps' names, not the record")
    a = ap.parse_args()
    if a.marks:
        pins.MARK = marked(a.marks)
        with safebo_amd.SweepEngine(0) as eng:
            eng.set_option("guard_audit_every", 1)
            one_pass(eng, 1)
        return
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
        flat, checks = one_pass(eng, 1)
        again, _ = one_pass(eng, -1)
    differ = sorted(k for k in flat if flat[k].shape != again[k].shape or not np.array_equal(flat[k], again[k]))
    for name, got, _ in checks:
        print(name, {step: ({k: (v[k].tolist() if isinstance(v[k], np.ndarray) else v[k]) for k in
                             ("count_S", "count_U", "count_M", "count_G", "n_exact_rechecks", "guard_passes", "profile_host_syncs",
                              "profile_posterior_kernel", "profile_k1_tiles_skipped", "profile_k1_tiles_skipped_safe") if k in v}
                            if "empty" not in v else bytes(v["empty"]).decode()) for step, v in got.items()})
    assert not differ, f"entries that depend on the engine's history: {differ}"
    for name, got, kernels in checks:
        pins.check_case(name, got, kernels)
    os.makedirs(os.path.dirname(os.path.abspath(a.record)), exist_ok=True)
    np.savez_compressed(a.record, commit=np.array([head or a.commit]), **pack(flat))
    print(f"{a.record}: {len(flat)} entries, {os.path.getsize(a.record)} bytes")


if __name__ == "__main__":
    main()
