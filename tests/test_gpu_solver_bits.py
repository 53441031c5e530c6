"""The projected-BFGS solver behind sbo_refine_sets, sbo_fit_local and sbo_model_fit's polish returns the bits it returned before
k_fit_local and k_refine came to share one core (csrc/pbfgs.hpp): tests/golden/solver/bits_before_shared_core.npz holds what the
commit named in its ``commit`` entry returned on an MI355X for the cases listed here, all built by the existing tests' own input
builders.  (sbo_refine has its own pin, tests/golden/refine/bits_before_sets.npz, in test_gpu_refine_sets.py.)

The fixture is the output of one command at that commit, with this module and the builders it imports in place:

    python tests/test_gpu_solver_bits.py --record tests/golden/solver/bits_before_shared_core.npz [--commit <sha>]

(the commit is read from ``git rev-parse HEAD``; ``--commit`` names it where the tree travels without its history, and is refused
where it contradicts the history).

Of the nine (n, d) of test_fit_local_many_outputs_across_the_workgroup_switch (264 workgroups each) two are recorded, (97, 1) and
(96, 5): all nine would take the fixture past 150 KB, against the few tens of KB it may have.  The three shapes of
test_fit_local_reaches_slsqp_at_new_shapes cover d + 2 = 3, 7 and 10 (the core's full dimension) on both sides of the
workgroup-size switch and run to convergence.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import refine_sets_oracle as rs  # noqa: E402
from test_gpu_fit_local import wo_data  # noqa: E402
from test_gpu_fit_shapes import many_outputs_problem, slsqp_problem  # noqa: E402
from test_gpu_model_fit import SAFE_BOX, _lhs, _norm_ds  # noqa: E402
from test_gpu_refine_sets import _cases, _run, appended_pair_problem  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver", "bits_before_shared_core.npz")
REFINE_KEYS = ("x", "xp", "value", "status", "evaluations", "best")
FIT_KEYS = ("x", "nll", "iters", "evals", "pgnorm", "status")
MODEL_KEYS = ("hypopt", "nll", "polish_status", "polish_evals")


def _refine_grid(engine):
    """The M, G, T and E problems of grid_case("benoit_n20_50x50") from the host classes' seeds (LDS tier)."""
    case, problems = _cases("benoit_n20_50x50")
    assert {label[0] for label, _, _ in problems} == set("MGTE")
    engine.set_model(case["ds"])
    return {f"sets_{label}": (_run(engine, P, seed), REFINE_KEYS) for label, P, seed in problems}


def _refine_appended(engine):
    """The pair problem of test_refine_sets_follows_appended_samples at n0 = 300 on the appended model (streamed tier)."""
    n0 = 300
    ds0, _, Xn, Yn, P, seed, _ = appended_pair_problem(n0)
    engine.set_model(ds0)
    for i in range(n0, len(Xn)):
        engine.append_sample(Xn[i], Yn[i])
    return {"sets_appended_n300": (_run(engine, P, seed), REFINE_KEYS)}


def _fit_local(engine):
    out = {}
    for n, d in ((97, 1), (96, 5)):
        X, Y, B, starts, maxiter = many_outputs_problem(n, d)
        out[f"fit_many_n{n}_d{d}"] = (engine.fit_local(X, Y, B, starts, maxiter=maxiter), FIT_KEYS)
    for n, d in ((97, 1), (96, 5), (95, 8)):
        X, y, B, starts = slsqp_problem(n, d)
        out[f"fit_slsqp_n{n}_d{d}"] = (engine.fit_local(X, y[:, None], B, starts), FIT_KEYS)
    # a start on two faces of the box: the first start of the (96, 5) problem moved to lo on axis 0 and to hi on the noise axis
    X, y, B, starts = slsqp_problem(96, 5)
    face = starts[:1].copy()
    face[0, 0], face[0, -1] = B[0, 0], B[-1, 1]
    out["fit_face_n96_d5"] = (engine.fit_local(X, y[:, None], B, face), FIT_KEYS)
    return out


def _model_fit(engine):
    """test_polish_contract_and_host_lbfgsb's ("wo", 64) call with the polish on."""
    Xn, Yn = wo_data(engine, 64)
    r = engine.model_fit(_norm_ds(Xn, Yn), SAFE_BOX, _lhs(SAFE_BOX, 60, 11), seed=11, maxiter=48, tol=0.01, polish=True)
    return {"model_fit_wo_n64": (r, MODEL_KEYS)}


GROUPS = {"refine_grid": _refine_grid, "refine_appended": _refine_appended, "fit_local": _fit_local, "model_fit": _model_fit}


def _arrays(results):
    """{"case/key": array} of the compared entries; floats as their uint64 bit patterns."""
    flat = {}
    for case, (res, keys) in results.items():
        for k in keys:
            if k not in res:
                assert k == "xp", (case, k)             # (single mode returns no x')
                continue
            a = np.ascontiguousarray(res[k])
            flat[f"{case}/{k}"] = a.view(np.uint64) if a.dtype == np.float64 else a
    return flat


@pytest.mark.parametrize("group", list(GROUPS))
def test_solver_returns_the_bits_it_returned_before_the_shared_core(engine, group):
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
