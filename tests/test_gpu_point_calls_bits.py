"""sbo_mean_grad, sbo_lipschitz and sbo_batch_select return the bits they returned before their scratch layouts, arg-best reductions,
workgroup sums and dpad dispatch moved into shared code (csrc/internal.hpp, csrc/device_common.hpp):
tests/golden/point_calls/bits_before_shared_plumbing.npz holds what the commit named in its ``commit`` entry returned on an MI355X
for the cases listed here.  (The refine calls have their own pins: test_gpu_solver_bits.py, test_gpu_robust_refine_bits.py and the
bits_before_sets.npz test of test_gpu_refine_sets.py.)

The fixture is the output of one command at that commit, with this module in place:

    python tests/test_gpu_point_calls_bits.py --record tests/golden/point_calls/bits_before_shared_plumbing.npz [--commit <sha>]

(the commit is read from ``git rev-parse HEAD``; ``--commit`` names it where the tree travels without its history, and is refused
where it contradicts the history).

Why each case is here:

mean_grad (gradient and inf-norm; the dpad dispatch of k_mean_grad and the layout of its scratch), each model with a list of one
point and a list of 257 (two workgroups of 256):
  n = 513, d = 2    config B as test_gpu_lipschitz.py builds it: one observation past the 512-row LDS chunk, dpad 2;
  n = 65, d = 3     dpad 4, a d that is not dpad;
  n = 65, d = 5     dpad 8, likewise.
  The d = 3 and d = 5 data are test_mean_grad_over_d's (uniform rows, two smooth outputs) at n = 65.

lipschitz (every field of the result; k_lip_top's two scans, lip_argmax in k_lip_seedmax and k_lip_final, the workgroup sums of
k_lipschitz, the scratch layout):
  B64 top = 2       lipschitz_oracle.case("B64"), default seeds, d = 2: two rounds of k_lip_top ("open behind the last pick");
  B64 streamed      the same call with lipschitz_lds = 0: k_lipschitz<false>;
  D128              the one further dpad lipschitz_oracle.CASES offers (d = 4, dpad 4: three axes more in the key of lip_argmax);
  B64 seed list     a box with a degenerate axis (lo == hi on axis 1), twelve seeds on that line, one seed outside the box, then
                    the twelve again -- every usable seed has an exact duplicate, so each round of k_lip_top and the final
                    arg-max over seeds and iterates meet equal values and must take the lowest entry --, output 1 only.

batch_select (index, std, n_selected and var_out; the block arg-max over one and over several workgroups, the scratch layout,
the dpad dispatch):
  the first eight entries of batch_oracle.CASES, which are the ones that commit had (n in 1 .. 300, m in 1 .. 5000, dpad 2, 4 and
  8, pending points, k > m; the later entries, n = 505 and up, are compared with the oracle in tests/test_gpu_batch_select.py);
  the duplicated pool of test_ties_permutations_embeddings_and_repeated_calls (every row twice: each pick is a tie between two
  workgroups' candidates).

An array of more than 1100 values (the gradients of the 257-point lists at d = 3 and 5, var_out at m = 5000) is recorded as its
SHA-256, under ``<name>.sha256``: the comparison is as exact, and the fixture stays at a few tens of KB.
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
import lipschitz_oracle as lo_  # noqa: E402
from safebo_amd import synthetic  # noqa: E402
from test_gpu_batch_select import _config_b as batch_config_b, _pool  # noqa: E402
from test_gpu_lipschitz import B_HI, B_LO, _box_points, _config_b  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_calls", "bits_before_shared_plumbing.npz")
DIGEST_ABOVE = 1100


def _model_d(d, n=65):
    """test_mean_grad_over_d's data at n rows: -> (ds, lo, hi)."""
    rng = np.random.default_rng(200 + d)
    X = rng.uniform(-1.0, 1.0, size=(n, d))
    Y = np.column_stack([np.sum(np.sin(2.0 * X), axis=1), np.sum(X * X, axis=1) - 0.5 * X[:, 0]])
    return synthetic.make_dataset(X, Y, synthetic.default_hypopt(d, 2)), -np.ones(d), np.ones(d)


def _mean_grad(engine):
    out = {}
    ds, use_invK = _config_b(513)
    models = [("n513_d2", use_invK, ds, B_LO, B_HI)] + [(f"n65_d{d}", True, *_model_d(d)) for d in (3, 5)]
    for tag, use_invK, ds, lo, hi in models:
        engine.set_model(ds, use_invK=use_invK)
        assert engine.n == int(tag[1:].split("_")[0])
        for count in (1, 257):
            grad, inf = engine.mean_grad(_box_points(lo, hi, count, 900 + count), infnorm=True)
            out[f"grad_{tag}_N{count}"] = {"grad": grad, "inf": inf}
    return out


def _duplicate_seeds(lo, hi):
    """Twelve seeds on the line x_1 = 0.3 of the box, one seed outside it, the twelve again."""
    line = np.stack([np.linspace(lo[0], hi[0], 12), np.full(12, 0.3)], axis=1)
    return np.vstack([line, [[hi[0] + 0.1, 0.3]], line])


def _lipschitz(engine):
    out = {}
    c = lo_.case("B64")
    engine.set_model(c["ds"])
    out["lip_B64_top2"] = engine.lipschitz(c["lo"], c["hi"], top=2)
    engine.set_option("lipschitz_lds", 0)
    try:
        out["lip_B64_streamed"] = engine.lipschitz(c["lo"], c["hi"], top=2)
    finally:
        engine.set_option("lipschitz_lds", 1)
    lo, hi = np.array([c["lo"][0], 0.3]), np.array([c["hi"][0], 0.3])
    r = engine.lipschitz(lo, hi, seeds=_duplicate_seeds(lo, hi), outputs=[1])
    assert r["seeds_used"] == 24 and r["problems"] == 1 * 1 * 2 * 4
    out["lip_B64_seed_list"] = r
    c = lo_.case("D128")
    engine.set_model(c["ds"])
    assert engine.d == 4
    out["lip_D128"] = engine.lipschitz(c["lo"], c["hi"])
    return out


def _batch(engine):
    out = {}
    for c in bo.CASES[:bo.FIRST_LARGE]:                     # (the cases that existed when the fixture was recorded)
        ds, pool, pending = bo.make_case(c)
        engine.set_model(ds, use_invK=c["use_invK"])
        out["batch_" + bo.case_id(c)] = _batch_call(engine, pool, c["k"], c["output"], pending)
    ds, bound, _ = batch_config_b(40)
    P = _pool(bound, 257, 301)
    engine.set_model(ds)
    out["batch_duplicated_pool"] = _batch_call(engine, np.vstack([P, P]), 8, 0, None)
    return out


def _batch_call(engine, pool, k, output, pending):
    r = engine.batch_select(pool, k, output, pending, return_var=True)
    return {"index": r["index"], "std": r["std"], "n_selected": np.array([len(r["index"])], dtype=np.int64), "var": r["var"]}


GROUPS = {"mean_grad": _mean_grad, "lipschitz": _lipschitz, "batch_select": _batch}


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
def test_point_calls_return_the_bits_they_returned_before_the_shared_plumbing(engine, group):
    z = np.load(FIXTURE)
    got = _arrays(GROUPS[group](engine))
    assert got
    for name, a in got.items():
        want = z[name]
        print(f"{name}: {a.size} values, {int(np.sum(a != want)) if a.shape == want.shape else 'shape'} differ")
        assert a.dtype == want.dtype and np.array_equal(a, want), name
    recorded = {k for k in z.files if k.split("/")[0] in {n.split("/")[0] for n in got}}
    assert recorded == set(got), recorded ^ set(got)


def main():
    import argparse
    import safebo_amd
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, metavar="PATH")
    ap.add_argument("--commit", help="the commit of the tree, where git cannot tell")
    a = ap.parse_args()
    import subprocess
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
