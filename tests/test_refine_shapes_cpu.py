"""The reference alone on every case of tests/refine_shapes.py (no GPU): the preconditions that make
tests/test_gpu_refine_shapes.py meaningful.  A device result must never pass because the reference problem behind it was slack: the
seed is strictly feasible, the SLSQP yardstick is itself stationary to a tenth of the bar the device is held to, it really moves off
the seed, and both halves of the posterior gradient carry weight where it ends."""
import os

import numpy as np
import pytest

import refine_sets_oracle as rs
import refine_shapes as S
import refine_solver_twin as twin
import robust_refine_oracle as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(S.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_the_reference_problem_of_every_case_is_sharp(name):
    case = S.CASES[name]
    P, seeds, yard = S.problem(case), S.seeds(case), S.yardstick(case)
    ds = S.dataset(case)
    assert ds["X_norm"].shape == (case["n"], case["d"]) and ds["Y_norm"].shape[1] == case["q"]
    assert 1 <= len(seeds) <= 4 and seeds.shape[1] == (2 if P["pair"] else 1) * case["d"]
    assert case["max_eval"] is None or case["max_eval"] <= S.eval_cap(case["n"])
    sg = -1.0 if P["maximize"] else 1.0
    for seed, y in zip(seeds, yard):
        ok, slack = rs.feasible(P, seed)
        assert ok and slack > 1e-6, (name, slack)                       # not on a boundary
        assert rs.feasible(P, y["z"])[0], name
        print(f"{name}: reference kkt {y['kkt']:.3e} after {y['nit']} iterations, seed {y['seed_value']!r} -> {y['value']!r}")
        assert y["kkt"] <= 0.1 * S.kkt_bar(case), (name, y["kkt"])
        assert y["nit"] < 100, (name, y["nit"])
        assert sg * (y["seed_value"] - y["value"]) > 1e-3 * (1.0 + abs(y["seed_value"])), (name, y["seed_value"], y["value"])
        g_mean, g_var, g_obj, var_rel = S.gradient_shares(P, y["z"])
        if case["kind"] == "var":
            assert var_rel > 1e-2, (name, var_rel)
        else:
            assert min(g_mean, g_var) >= 1e-2 * (g_obj + 1.0), (name, g_mean, g_var, g_obj)


@pytest.mark.parametrize("name", [n for n in NAMES if S.CASES[n]["cls"] == "slots" and S.CASES[n]["n"] > 256])
def test_the_solver_twin_converges_on_exact_gradients_within_the_budget(name):
    """The slots cases above 256 rows, whose data seeds the twin chose (tests/refine_shapes.py): the same algorithm on the reference gradients must reach the last barrier stage
    within the budget, at the yardstick's value.  (How many evaluations the last stage's line searches take hangs on the rounding
    of the sums, which the twin does not share with the device: its own end there is not held to the budget.)"""
    case = S.CASES[name]
    P = S.problem(case)
    sg = -1.0 if P["maximize"] else 1.0
    for seed, y in zip(S.seeds(case), S.yardstick(case)):
        status, nev, mu, x, v = twin.run(P, seed, case["max_eval"] or twin.DEFAULT_EVAL)
        print(f"{name}: twin {status} after {nev} evaluations, value {v!r} against {y['value']!r}")
        assert mu <= 1.001 * twin.MUFLOOR, (name, status, nev, mu)
        assert sg * v <= sg * y["value"] + 1e-8 * (1.0 + abs(y["value"])), (name, v, y["value"])


def test_the_solver_twin_stalls_with_a_free_direction_along_an_active_constraint():
    """The finding that shaped the slots cases: fan_model(5, d=3, n=257, seed 0), lcb -- SLSQP needs 7 iterations, the twin on exact
    gradients is short of the optimum by 2e-6 after 4000 evaluations, at barrier weight 1e-5 (the device: 1.5e-6 after 20000)."""
    import many_constraints as mc
    ds = mc.fan_model(5, 3, 257, 0)
    lo, hi = mc.box(3)
    P = rs.problem(ds, mc.B, lo, hi, "lcb")
    seed = np.array([-1.2, -0.96, -1.2 + 2.4 * 1 / 9])
    assert rs.feasible(P, seed)[0]
    z, res = rs.slsqp(P, seed)
    status, nev, mu, x, v = twin.run(P, seed, 4000)
    assert res.nit < 20 and status == "MAX_EVAL" and mu >= 1e-6
    assert 1e-7 < (v - rs.value(P, rs.make_feasible(P, z, seed))) / (1.0 + abs(v)) < 1e-4


def test_tier_switch_points_follow_the_rule_of_refine_lds_bytes():
    """144 KiB for the staged triangles beside 16 n bytes per further point: a change of either fails here."""
    assert S.LDS_M == 144 * 1024 and S.POINT_BYTES == 16
    src = open(os.path.join(ROOT, "safe-bayesian-optimization_amd", "csrc", "refine.hip")).read()
    assert "kRefLdsM = 144 * 1024" in src and "kvuv = sizeof(double) * 2 * (size_t)n" in src
    assert (S.N1, S.N2, S.N3, S.N8, S.NP2) == (191, 135, 110, 67, 134)
    for slots, points, n in ((1, 1, 191), (2, 1, 135), (3, 1, 110), (8, 1, 67), (2, 2, 134)):
        assert S.staged(n, slots, points) and not S.staged(n + 1, slots, points)
    assert (S.threads(256), S.threads(257)) == (256, 1024)
    assert (S.eval_cap(512), S.eval_cap(1025), S.eval_cap(2048)) == (15258, 3807, 953)


def test_the_table_covers_the_shape_range():
    by = {}
    for c in S.CASES.values():
        by.setdefault(c["cls"], []).append(c)
    assert {c["n"] for c in by["launch"]} == {63, 64, 65, 255, 256, 257, 1023, 1025, 2048}
    assert {c["kind"] for c in by["launch"]} == {"lcb", "ucb", "var"} and all(S.slots(c) == 2 and c["b"] == 2.0 for c in by["launch"])
    assert all(c["d"] >= 4 for c in by["launch"] if c["kind"] == "var")
    tiers = {(S.slots(c), S.problem(c)["pair"], c["n"]) for c in by["tier"]}
    assert tiers == {(1, False, 191), (1, False, 192), (2, False, 135), (2, False, 136), (3, False, 110), (3, False, 111),
                     (8, False, 67), (8, False, 68), (2, True, 134), (2, True, 135)}
    assert all(c["tiers"] for c in by["tier"])
    for q in (4, 5, 8):
        ns = sorted({c["n"] for c in by["slots"] if c["q"] == q})
        assert ns[0] == 40 and ns[-1] > 256, (q, ns)
        assert {c["kind"] for c in by["slots"] if c["q"] == q} == {"lcb", "var"}
    assert all(S.slots(c) == c["q"] and S.problem(c)["safe"] == list(range(1, c["q"])) for c in by["slots"])
    assert {c["d"] for c in by["dim"] if not S.problem(c)["pair"]} == {1, 8}
    pairs = [c for c in by["dim"] if S.problem(c)["pair"]]
    assert all(c["d"] == 4 and S.problem(c)["link"] is not None and S.problem(c)["unsafe"] == [1] for c in pairs)
    assert {S.staged(c["n"], 2, 2) for c in pairs} == {True, False} and max(c["n"] for c in pairs) > 256


@pytest.mark.parametrize("n0", S.REMOVALS)
def test_removal_cases_start_feasible_and_move(n0):
    order = S.removal_order(n0, S.REMOVE_K)
    assert order[:3] == [0, (n0 - 1) // 2, n0 - 3] and len(order) == S.REMOVE_K
    ds = S.after_removals(S._synthetic(n0, 2, 5), order)
    assert ds["X_norm"].shape[0] == n0 - S.REMOVE_K
    for label, P, seed in S.removal_problems(ds, n0):
        ok, slack = rs.feasible(P, seed)
        v_seed, v_yard, _ = rs.yardstick(P, seed)
        assert ok and slack > 1e-6 and (v_yard > v_seed if P["maximize"] else v_yard < v_seed), (label, slack, v_seed, v_yard)
    c = S.robust_case(n0)
    win = rr.grid_winner(dict(c, ds=S.after_removals(c["ds0"], order)))
    assert win["index"] >= 0 and c["lo"][0] < win["xc"][0] < c["hi"][0]


def test_one_removal_case_crosses_the_tier_switch_downwards():
    n0 = 140
    assert n0 in S.REMOVALS and not S.staged(n0, 2) and not S.staged(n0, 2, 2)
    assert S.staged(n0 - S.REMOVE_K, 2) and S.staged(n0 - S.REMOVE_K, 2, 2)


@pytest.mark.parametrize("n0", S.WINDOW)
def test_window_cases_start_feasible(n0):
    ds0, Xn, Yn, ds = S.window_model(n0)
    assert ds0["X_norm"].shape[0] == n0 == ds["X_norm"].shape[0] and len(Xn) == S.WINDOW_STEPS
    assert np.array_equal(ds["X_norm"][-1], Xn[-1]) and np.array_equal(ds["X_norm"][0], ds0["X_norm"][S.WINDOW_STEPS])
    for label, P, seed in S.removal_problems(ds, n0):
        ok, slack = rs.feasible(P, seed)
        assert ok and slack > 1e-6, (label, slack)


def test_tiny_models_have_a_feasible_and_an_infeasible_seed_off_the_boundary():
    ds0, order, ds, seeds = S.tiny_model(2)
    assert ds0["X_norm"].shape[0] == 4 and ds["X_norm"].shape[0] == 2 and S.tiny_model(1)[2]["X_norm"].shape[0] == 1
    P = rs.problem(ds, 2.0, -np.ones(2), np.ones(2), "lcb")
    slack = [rs.feasible(P, s)[1] for s in seeds]
    assert min(abs(s) for s in slack) > 1e-6 and max(slack) > 0 > min(slack), slack
