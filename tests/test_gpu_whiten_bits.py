"""sbo_batch_select, sbo_expander_gain and sbo_sample_paths return the bits they returned before the arithmetic they share on the
resident factor moved into one header (csrc/whiten.hpp: rbf_scale / rbf_k, the prep kernel, whiten_tile, factor_lower_mv /
factor_upper_mv, the slab image helpers): tests/golden/whiten/bits_before_shared_core.npz holds what the commit named in its
``commit`` entry returned on an MI355X for the cases listed here.

The fixture is the output of one command at that commit, with this module in place:

    python tests/test_gpu_whiten_bits.py --record tests/golden/whiten/bits_before_shared_core.npz [--commit <sha>]

(the commit is read from ``git rev-parse HEAD``; ``--commit`` names it where the tree travels without its history, and is refused
where it contradicts the history).

The cases are the committed lists, which stand at every edge of the shared code; only ``make_case`` is needed, not the NumPy
references:

batch_select (index, std, n_selected, var): batch_oracle.CASES[FIRST_LARGE:] -- the first eight are pinned by
  tests/golden/point_calls/bits_before_shared_plumbing.npz.  These add whiten_tile's tiers P = 16 and 8 (n = 505 .. 2048) and the two
  mat-vecs of k_batch_u beyond one stride of 1024 threads (n = 1020 with 3 pending and k = 8 up to n = 2048 with k = 59).
expander_gain (count, margin, witness): every entry of expander_oracle.CASES -- n = 1, 2 the first row block; n = 32 | 33, 64 | 65
  the zero-filled rows of w and T; d = 1, 3, 6 the padded lanes; q = 3, 4 several slots of the prep kernel; all three tiers.
sample_paths (index, value, values): every entry of paths_oracle.CASES -- n = 1024 | 1025 | 2048 the two mat-vecs of k_path_solve;
  d = 8 the full dpad; S = 1 .. 64 the three instantiations of the slab multiply step.

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

import batch_oracle as bo  # noqa: E402
import expander_oracle as eo  # noqa: E402
import paths_oracle as po  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "whiten", "bits_before_shared_core.npz")
DIGEST_ABOVE = 1100


def _batch(engine):
    out = {}
    for c in bo.CASES[bo.FIRST_LARGE:]:
        ds, pool, pending = bo.make_case(c)
        engine.set_model(ds, use_invK=c["use_invK"])
        r = engine.batch_select(pool, c["k"], c["output"], pending, return_var=True)
        out["batch_" + bo.case_id(c)] = {"index": r["index"], "std": r["std"], "n_selected": np.array([len(r["index"])], dtype=np.int64),
                                         "var": r["var"]}
    return out


def _expander(engine):
    out = {}
    for c in eo.CASES:
        ds, S, T = eo.make_case(c)
        engine.set_model(ds, use_invK=c["use_invK"])
        cons = None if c["mask"] == 0 else eo.constraints_of(c["q"], c["mask"])
        r = engine.expander_gain(S, T, c["b"], cons, return_margin=True)
        out["expander_" + eo.case_id(c)] = {k: r[k] for k in ("count", "margin", "witness")}
    return out


def _paths(engine):
    out = {}
    for c in po.CASES:
        ds, pts, draws = po.make_case(c)
        engine.set_model(ds, use_invK=c["use_invK"])
        r = engine.sample_paths(pts, c["S"], c["output"], draws=draws, maximize=bool(c["maximize"]), return_values=True)
        out["paths_" + po.case_id(c)] = {k: r[k] for k in ("index", "value", "values")}
    return out


GROUPS = {"batch_select": _batch, "expander_gain": _expander, "sample_paths": _paths}


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


@pytest.mark.parametrize("group", list(GROUPS))
def test_factor_point_calls_return_the_bits_they_returned_before_the_shared_core(engine, group):
    z = np.load(FIXTURE)
    got = _arrays(GROUPS[group](engine))
    assert got
    differ = 0
    for name, a in got.items():
        want = z[name]
        bad = int(np.sum(a != want)) if a.shape == want.shape else "shape"
        differ += bad != 0
        print(f"{name}: {a.size} values, {bad} differ")
        assert a.dtype == want.dtype and np.array_equal(a, want), name
    prefix = next(iter(got)).split("_")[0] + "_"
    recorded = {k for k in z.files if k.startswith(prefix)}
    assert recorded == set(got), recorded ^ set(got)
    print(f"{group}: {len(got)} entries, {differ} differ")


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
    flat = {"commit": np.array([head or a.commit])}
    with safebo_amd.SweepEngine(0) as eng:
        for fn in GROUPS.values():
            flat.update(_arrays(fn(eng)))
    os.makedirs(os.path.dirname(os.path.abspath(a.record)), exist_ok=True)
    np.savez_compressed(a.record, **flat)
    print(f"{a.record}: {len(flat) - 1} arrays, {os.path.getsize(a.record)} bytes")


if __name__ == "__main__":
    main()
