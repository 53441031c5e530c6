"""sbo_posterior_joint returns the bits it returned before its tile steps were written once beside those of sbo_expander_gain and
sbo_sample_paths (the residual kernel, the stage-1 body, the 64 x 64 row-product step, the 128 x Spad tile with its arg-best epilogue,
the partials merge): tests/golden/joint/bits_before_shared_tiles.npz holds what the commit named in its ``commit`` entry returned on
an MI355X for the cases listed here.

The fixture is the output of one command at that commit, with this module in place:

    python tests/test_gpu_joint_bits.py --record tests/golden/joint/bits_before_shared_tiles.npz [--commit <sha>]

(the commit is read from ``git rev-parse HEAD``; ``--commit`` names it where the tree travels without its history, and is refused
where it contradicts the history).

The cases are every entry of joint_oracle.CASES, which stand at every edge of the code that moved (only ``make_case`` is needed, not
the NumPy references): m in {1, 2, 63, 64, 65, 129, 257, 513, 2048} around the 64- and 128-tiles; n in {1, 31, 32, 33, 300, 1025, 2048}
around the slab and the three tiers of whiten_tile; S in {0, 1, 16, 17, 64} over the three instantiations of the draw kernel; dpad 2,
4 and 8.  Each case runs twice: ``full`` with every array requested (mean, cov, chol, draws, index, value, pivot_min, pivot_row) and
``lean`` without cov, chol and draws -- the cov-null and draws-null branches are other stores in the same kernels.

An array of more than 1100 values is recorded as its SHA-256, under ``<name>.sha256``: the comparison is as exact, and the fixture
stays small.  Nothing is compared at a tolerance: contraction is off and the operation order is kept, so every value is equal.
"""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import joint_oracle as jo  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "joint", "bits_before_shared_tiles.npz")
DIGEST_ABOVE = 1100


def _joint(engine):
    out = {}
    for c in jo.CASES:
        ds, pts, z = jo.make_case(c)
        engine.set_model(ds, use_invK=c["use_invK"])
        kw = dict(output=c["output"], z=z, noise=bool(c["noise"]), jitter=c["jitter"], maximize=bool(c["maximize"]))
        for run, want in (("full", True), ("lean", False)):
            r = engine.posterior_joint(pts, return_cov=want, return_chol=want, return_draws=want, **kw)
            r.pop("x", None)                                  # (gathered on the host from index)
            r["pivot_min"], r["pivot_row"] = np.array([r["pivot_min"]], dtype=np.float64), np.array([r["pivot_row"]], dtype=np.int64)
            out[f"joint_{run}_" + jo.case_id(c)] = r
    return out


def _arrays(results):
    """{"case/key": array} of every entry; floats as their uint64 bit patterns, long arrays as their SHA-256."""
    flat = {}
    for case, res in results.items():
        for k, v in res.items():
            a = np.ascontiguousarray(v)
            a = a.view(np.uint64) if a.dtype == np.float64 else a.astype(np.int64)
            if a.size > DIGEST_ABOVE:
                flat[f"{case}/{k}.sha256"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy()
            else:
                flat[f"{case}/{k}"] = a
    return flat


def test_posterior_joint_returns_the_bits_it_returned_before_the_shared_tiles(engine):
    z = np.load(FIXTURE)
    got = _arrays(_joint(engine))
    assert got
    differ = 0
    for name, a in got.items():
        want = z[name]
        bad = int(np.sum(a != want)) if a.shape == want.shape else "shape"
        differ += bad != 0
        print(f"{name}: {a.size} values, {bad} differ")
        assert a.dtype == want.dtype and np.array_equal(a, want), name
    recorded = {k for k in z.files if k != "commit"}
    assert recorded == set(got), recorded ^ set(got)
    print(f"posterior_joint: {len(got)} entries, {differ} differ")


def main():
    import argparse
    import subprocess
    import safebo_amd
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, metavar="PATH")
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
        flat = _arrays(_joint(eng))
    n = len(flat)
    flat["commit"] = np.array([head or a.commit])
    os.makedirs(os.path.dirname(os.path.abspath(a.record)), exist_ok=True)
    np.savez_compressed(a.record, **flat)
    print(f"{a.record}: {n} arrays, {os.path.getsize(a.record)} bytes")


if __name__ == "__main__":
    main()
