"""CPU tests of sbo_refine_sets' pieces that need no GPU: the SLSQP yardstick of M_t and G_t on the committed
fixtures, the analytic Jacobians of the reference terms, and the binding -- the export and the ctypes mirrors against a C
compiler's layout of include/safebo.h."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from safebo_amd import _lib

import refine_sets_oracle as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# fixture -> (std at the grid seed, std of the feasible SLSQP answer), M_t and G_t alike, rounded to five figures
YARDSTICK = {"benoit_n20_50x50": (0.35377, 0.37170), "benoit_n128_64x48": (0.27065, 0.27335), "wo3_n64_48x40": (9.2613, 9.6568)}


@pytest.mark.parametrize("name", sorted(YARDSTICK))
def test_grid_seeds_are_strictly_feasible_and_the_slsqp_yardstick_beats_them(name):
    case = rs.grid_case(name)
    seed_std, slsqp_std = YARDSTICK[name]
    digits = 5 if seed_std < 1.0 else 4
    best_g = -np.inf
    for key, (P, seed) in [("M", case["M"])] + [("G", pg) for pg in case["G"]]:
        ok, slack = rs.feasible(P, seed)
        assert ok and slack > 0.0, (key, slack)
        v_seed, v_yard, z = rs.yardstick(P, seed)
        assert rs.feasible(P, z)[0]
        assert v_yard > v_seed
        assert round(float(np.sqrt(v_seed)), digits) == seed_std, (key, np.sqrt(v_seed))
        if key == "M":
            assert round(float(np.sqrt(v_yard)), digits) == slsqp_std, np.sqrt(v_yard)
        else:
            best_g = max(best_g, float(np.sqrt(v_yard)))           # (Expander keeps the largest over the constraints)
    assert round(best_g, digits) == slsqp_std, best_g
    assert len(case["G"]) == case["ds"]["Y_norm"].shape[1] - 1


def test_smallest_seed_slack_per_fixture():
    """The log-barrier method starts from these seeds: 1.1e-4 on wo3, 9e-3 on benoit_n128 and 4e-2 on benoit_n20."""
    got = {}
    for name in YARDSTICK:
        case = rs.grid_case(name)
        got[name] = min(rs.feasible(P, seed)[1] for P, seed in [case["M"]] + case["G"])
    assert 1.0e-4 < got["wo3_n64_48x40"] < 1.3e-4
    assert 8e-3 < got["benoit_n128_64x48"] < 1e-2
    assert 3.5e-2 < got["benoit_n20_50x50"] < 4.5e-2


@pytest.mark.parametrize("name", ["benoit_n20_50x50", "wo3_n64_48x40"])
def test_term_and_objective_jacobians_match_central_differences(name):
    case = rs.grid_case(name)
    rng = np.random.default_rng(11)
    for P, seed in [case["M"], case["G"][0], case["T"][0], case["E"]]:
        lo, hi = rs.box(P)
        z = seed + 1e-3 * rng.uniform(-1, 1, seed.shape) * (hi - lo)
        h = 1e-6 * (hi - lo)
        fd = []
        for a in range(len(z)):
            e = np.zeros(len(z))
            e[a] = h[a]
            up, dn = rs.terms(P, z + e), rs.terms(P, z - e)
            fd.append([(u[1] - w[1]) / (2 * h[a]) for u, w in zip(up, dn)] + [(rs.objective(P, z + e)[0] - rs.objective(P, z - e)[0]) / (2 * h[a])])
        fd = np.array(fd).T                                          # [terms + objective, nz]
        an = np.array([t[2] for t in rs.terms(P, z)] + [rs.objective(P, z)[1]])
        np.testing.assert_allclose(an, fd, rtol=2e-5, atol=2e-5 * (1.0 + np.max(np.abs(fd))))


def test_refine_sets_is_exported_and_bound_with_its_declared_signature():
    lib = _lib.load()
    assert ("sbo_refine_sets" in [s[0] for s in _lib.SYMBOLS])
    assert lib.sbo_refine_sets.restype is C.c_int
    assert len(lib.sbo_refine_sets.argtypes) == 10
    res = _lib.RefineSetsResult()
    assert lib.sbo_refine_sets(None, None, 1, None, None, None, None, None, None, C.byref(res)) == _lib.SBO_E_INVALID
    assert lib.sbo_version() == 3


def test_refine_sets_struct_layout_matches_the_header(tmp_path):
    fields_o = ["pair", "kind", "safe_mask", "unsafe_mask", "level_output", "link_output", "max_eval", "level", "L", "lo", "hi", "x_0", "r",
                "target", "tol"]
    fields_r = ["best_x", "best_xp", "best_value", "evaluations", "converged"]
    exprs = (["sizeof(sbo_refine_sets_opts)", "sizeof(sbo_refine_sets_result)", "(size_t)SBO_REFINE_DIST"]
             + [f"offsetof(sbo_refine_sets_opts, {f})" for f in fields_o] + [f"offsetof(sbo_refine_sets_result, {f})" for f in fields_r])
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safebo.h"\nint main(void) { printf("' + "%zu " * len(exprs) + '\\n", '
                   + ", ".join(exprs) + "); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    O, R = _lib.RefineSetsOpts, _lib.RefineSetsResult
    assert got == ([C.sizeof(O), C.sizeof(R), _lib.SBO_REFINE_DIST] + [getattr(O, f).offset for f in fields_o]
                   + [getattr(R, f).offset for f in fields_r])


@pytest.mark.parametrize("r", [0.3, 0.002])
def test_ball_term_of_the_trust_region_problem(r):
    """sbo_refine's trust-region case (test_benoit_trust_region_refines_and_unsticks_small_radii: x_0 = point 44786 of the 400 x 400
    grid) through the shared functions: the ball's Jacobian against central differences (a quadratic: exact up to rounding), the
    feasible yardstick from SLSQP's answer and from a point outside the ball, and stationarity of that answer -- with the ball's
    multiplier where the ball binds, which at r = 0.002 it must (the unconstrained step from x_0 is longer than 0.0015)."""
    import oracle
    ds, b, lo, hi = rs.load("benoit_n20_50x50")
    x0 = oracle.grid_points(lo, hi, [400, 400], first=44786, n=1)[0]
    P = rs.problem(ds, b, lo, hi, "lcb", safe=[1], ball=(x0, r))
    assert [t[0] for t in rs.terms(P, x0)] == ["safe1", "ball"] and rs.terms(P, x0)[1][1] == r * r
    z = x0 + np.array([0.3, -0.4]) * r
    h = 1e-3 * r
    for a in range(2):
        e = np.zeros(2)
        e[a] = h
        fd = (rs.terms(P, z + e)[1][1] - rs.terms(P, z - e)[1][1]) / (2 * h)
        assert abs(fd - rs.terms(P, z)[1][2][a]) <= 1e-6 * r
    far = x0 + np.array([0.8, -0.5]) * 2 * r
    assert not rs.feasible(P, far)[0]
    back = rs.make_feasible(P, far, x0)
    assert rs.feasible(P, back)[0] and np.linalg.norm(back - x0) <= r
    xs, _ = rs.slsqp(P, x0)
    xs = rs.make_feasible(P, xs, x0)
    assert rs.feasible(P, xs)[0] and rs.value(P, xs) < rs.value(P, x0)
    print(f"r {r}: |xs - x0| {np.linalg.norm(xs - x0):.6g}, ball slack / r^2 {rs.terms(P, xs)[1][1] / r ** 2:.3g}, kkt {rs.kkt_residual(P, xs):.3g}")
    assert rs.kkt_residual(P, xs) <= 1e-6
    if r == 0.002:
        assert np.linalg.norm(xs - x0) > 0.0015
        assert 0.0 <= rs.terms(P, xs)[1][1] <= 1e-6 * r * r       # (inside kkt_residual's active band: its gradient is a column)
