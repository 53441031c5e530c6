"""sbo_refine_robust returns the bits it returned before k_refine and k_refine_robust came to share one barrier step (ref_step) and
one scenario pass (csrc/refine.hip): tests/golden/refine/bits_before_shared_step.npz holds what the commit named in its ``commit``
entry returned on an MI355X for the calls listed here, all built by robust_refine_oracle.py's builders.  (k_refine through
ref_advance is pinned by test_gpu_solver_bits.py and by bits_before_sets.npz in test_gpu_refine_sets.py.)

The fixture is the output of one command at that commit, with this module in place:

    python tests/test_gpu_robust_refine_bits.py --record tests/golden/refine/bits_before_shared_step.npz [--commit <sha>]

(the commit is read from ``git rev-parse HEAD``; ``--commit`` names it where the tree travels without its history, and is refused
where it contradicts the history).  Recording prints status, rounds, scenarios and evaluations of every call:
profiles/robust_step_core_checks.md has that table, and so which paths of the step the pin covers.

MAX_EVALS were chosen against that commit so that a d3_q3 call ends SBO_REFINE_MAX_EVAL after at least one round.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import robust_refine_oracle as R  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(HERE, "golden", "refine", "bits_before_shared_step.npz")
KEYS = ("status", "xc", "value", "seed_value", "worst_d", "g_min", "scenarios", "rounds", "evaluations", "gap")
B = R.B
MAX_EVALS = (2, 700)


def _start(engine, name):
    """The model of a case on the engine and the coarse robust sweep's winner, the seed."""
    case = R.build_case(name)
    engine.set_model(case["ds0"], mean_prior=case["mp"])
    if case["rows"] is not None:
        for xn, yn in zip(*case["rows"]):
            engine.append_sample(xn, yn)
    engine.set_grid(case["lo"], case["hi"], case["count"])
    res = engine.sweep_robust(B, case["nxc"], "ucb")
    assert res["index"] >= 0
    return case, res["xc"]


def _call(engine, name, kind="ucb", lds=1, fed_back=False, **kw):
    case, xc = _start(engine, name)
    engine.set_option("refine_lds", lds)
    try:
        if fed_back:
            xc = engine.refine_robust(B, xc, case["nxc"], case["lo"], case["hi"], case["count_d"], kind)["xc"]
        return engine.refine_robust(B, xc, case["nxc"], case["lo"], case["hi"], case["count_d"], kind, **kw)
    finally:
        engine.set_option("refine_lds", 1)


def _no_safe_control(engine, xc):
    """test_a_model_without_a_robust_safe_control_is_an_infeasible_seed's model and call."""
    ds, lo, hi = R.make_model(2, 2, 25, 6, shift=(0.0, -5.0))
    engine.set_model(ds, mean_prior=np.zeros(2))
    return engine.refine_robust(B, xc, 1, lo, hi, [7], "lcb")


CALLS = {name: (lambda e, name=name: _call(e, name)) for name in R.CASES}
CALLS.update({
    "d2_q2_streamed": lambda e: _call(e, "d2_q2", lds=0),
    "d3_q3_streamed": lambda e: _call(e, "d3_q3", lds=0),
    "d2_q2_scen1": lambda e: _call(e, "d2_q2", max_scenarios=1),
    "d2_q2_scen2": lambda e: _call(e, "d2_q2", max_scenarios=2),
    "d2_q2_mean": lambda e: _call(e, "d2_q2", kind="mean"),
    "d2_q2_lcb": lambda e: _call(e, "d2_q2", kind="lcb"),
    f"d3_q3_eval{MAX_EVALS[0]}": lambda e: _call(e, "d3_q3", max_eval=MAX_EVALS[0]),
    f"d3_q3_eval{MAX_EVALS[1]}": lambda e: _call(e, "d3_q3", max_eval=MAX_EVALS[1]),
    "d2_q2_fed_back": lambda e: _call(e, "d2_q2", fed_back=True),
    "no_safe_control_a": lambda e: _no_safe_control(e, [0.125]),
    "no_safe_control_b": lambda e: _no_safe_control(e, [1.7]),
})


def _arrays(label, res):
    """{"label/key": array} of the compared entries; floats as their uint64 bit patterns."""
    flat = {}
    for k in KEYS:
        a = np.ascontiguousarray(res[k])
        flat[f"{label}/{k}"] = a.view(np.uint64) if a.dtype == np.float64 else a
    return flat


@pytest.mark.parametrize("label", list(CALLS))
def test_robust_refine_returns_the_bits_it_returned_before_the_shared_step(engine, label):
    z = np.load(FIXTURE)
    res = CALLS[label](engine)
    print(f"{label}: status {res['status']} rounds {res['rounds']} scenarios {len(res['scenarios'])} evaluations {res['evaluations']}")
    got = _arrays(label, res)
    for name, a in got.items():
        want = z[name]
        print(f"{name}: {a.size} values, {int(np.sum(a != want)) if a.shape == want.shape else 'shape'} differ")
        assert a.dtype == want.dtype and np.array_equal(a, want), name
    assert {k for k in z.files if k.split("/")[0] == label} == set(got)


def test_the_fixture_records_exactly_these_calls():
    z = np.load(FIXTURE)
    assert {k.split("/")[0] for k in z.files} == set(CALLS) | {"commit"}


def main():
    import argparse
    import subprocess
    import safebo_amd
    from safebo_amd import _lib
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
    hit_max_eval = False
    with safebo_amd.SweepEngine(0) as eng:
        print("| call | status | rounds | scenarios | evaluations |\n|---|---|---|---|---|")
        for label, fn in CALLS.items():
            res = fn(eng)
            print(f"| `{label}` | {res['status']} | {res['rounds']} | {len(res['scenarios'])} | {res['evaluations']} |", flush=True)
            hit_max_eval = hit_max_eval or (label.startswith("d3_q3_eval") and res["status"] == _lib.SBO_REFINE_MAX_EVAL and res["rounds"] >= 1)
            flat.update(_arrays(label, res))
    if not hit_max_eval:
        sys.exit("no d3_q3 call with a max_eval of MAX_EVALS ends SBO_REFINE_MAX_EVAL after a round: choose others")
    os.makedirs(os.path.dirname(os.path.abspath(a.record)), exist_ok=True)
    np.savez_compressed(a.record, **flat)
    print(f"{a.record}: {len(flat) - 1} arrays, {os.path.getsize(a.record)} bytes")


if __name__ == "__main__":
    main()
