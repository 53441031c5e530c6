"""CPU side of sbo_refine_paths: the oracle's path gradient against central differences and against the
posterior mean's gradient; the solver's twin on every committed problem the device test holds to the KKT bar; the two teeth of that
bar; the case list against the kernels' constants, read from the source; the symbol and its structures against include/safebo.h;
the host's argument checks; SafeOpt.BO.ThompsonRefined with the C calls stubbed (the device call itself is checked under the
gpu marker, tests/test_gpu_refine_paths.py).

Measured (profiles/refine_paths_checks.md): the analytic gradient agrees with central differences (h = 1e-5) within 9.3e-10 relative
over the committed cases -- the assertion is ten times that, 1e-8; the twin converges on every held problem but 3 of the 64 starts of
the K = 64 case (MAX_EVAL; the share allowed is one in eight); without the last feature in the gradient the twin's KKT residual is
4.8e-1 on the F = 1 case (bar 1e-6), without the last observation 5.6e-1 on the n = 20 case (bar 1e-4)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from safebo_amd import SafeOpt, SweepEngine, _lib

import model_remove as mr
import refine_oracle as ro
import refine_paths_oracle as rp
import refine_shapes as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "safe-bayesian-optimization_amd", "csrc")
IDS = [rp.case_id(c) for c in rp.CASES]
GRAD_BAR = 1e-8                     # ten times the worst measured agreement (9.3e-10)


# ------------------------------------------------------------------------------------------ the oracle's gradient
@pytest.mark.parametrize("i", range(len(rp.CASES)), ids=IDS)
def test_path_grad_agrees_with_central_differences(i):
    c, case = rp.CASES[i], rp.make_case(i)
    co, d, h, worst = case["co"], c["d"], 1e-5, 0.0
    for s in sorted({0, c["S"] - 1}):
        for k in sorted({0, c["K"] - 1}):
            x = np.clip(case["seeds"][s, k], case["lo"], case["hi"])
            g = rp.path_grad(co, s, x)
            num = np.array([(rp.path_value(co, s, x + h * e) - rp.path_value(co, s, x - h * e)) / (2 * h) for e in np.eye(d)])
            worst = max(worst, float(np.max(np.abs(g - num)) / (1.0 + np.max(np.abs(g)))))
    print(rp.case_id(c), "gradient against central differences", worst)
    assert worst < GRAD_BAR, worst


@pytest.mark.parametrize("i", [2, 4, 16], ids=[IDS[i] for i in (2, 4, 16)])
def test_a_path_with_zero_draws_is_the_posterior_mean_with_its_gradient(i):
    """(On the caller's inverse: refine_oracle reads invKopt, the path solves K + sn2 I -- the two agree to rounding.)"""
    c, case = rp.CASES[i], rp.make_case(i)
    omega, phase, weights, noise = case["draws"]
    co = rp.coeffs(case["ds"], c["output"], (omega, phase, np.zeros_like(weights), np.zeros_like(noise)))
    for x in case["seeds"][0]:
        m, _, gm, _ = ro.posterior_grad(x, case["ds"])
        ys = case["ds"]["Y_std"][c["output"]]
        assert abs(rp.path_value(co, 0, x) - m[c["output"]]) < 1e-9 * ys
        assert float(np.max(np.abs(rp.path_grad(co, 0, x) - gm[c["output"]]))) < 1e-8 * ys


# ------------------------------------------------------------------------------------------ the solver's twin
@pytest.mark.parametrize("i", [i for i, c in enumerate(rp.CASES) if rp.held(c)], ids=[IDS[i] for i, c in enumerate(rp.CASES) if rp.held(c)])
def test_the_twin_converges_on_the_held_problems_and_meets_the_bar(i):
    c, case = rp.CASES[i], rp.make_case(i)
    other, worst, n_held = [], 0.0, 0
    for s, k in rp.held(c):
        P, seed = case["problems"][s], case["seeds"][s, k]
        if not rp.feasible(P, seed):
            continue
        n_held += 1
        status, nev, mu, x = rp.run(P, seed, c.get("max_eval") or 400)
        if status != "CONVERGED":
            other.append((s, k, status))
            continue
        assert rp.feasible(P, x)
        worst = max(worst, rp.kkt_residual(P, x))
    print(rp.case_id(c), "twin: held", n_held, "not converged", other, "kkt", worst)
    assert n_held > 0 and 8 * len(other) <= n_held, other
    assert worst <= rp.kkt_bar(c), worst
    if c.get("bad"):
        assert not rp.feasible(case["problems"][-1], case["seeds"][-1, -1])


@pytest.mark.parametrize("drop, i", [("feature", 0), ("observation", 2)])
def test_the_kkt_bar_tells_a_gradient_without_its_last_term(drop, i):
    c, case = rp.CASES[i], rp.make_case(i)
    worst = 0.0
    for s, k in rp.held(c):
        P, seed = case["problems"][s], case["seeds"][s, k]
        if rp.feasible(P, seed):
            worst = max(worst, rp.kkt_residual(P, rp.run(P, seed, 400, drop=drop)[3]))
    print(rp.case_id(c), "without the last", drop, "kkt", worst)
    assert worst > rp.kkt_bar(c), worst


def test_slsqp_agrees_with_the_twin_where_both_end_at_the_same_optimum():
    c, case = rp.CASES[2], rp.make_case(2)
    P, seed = case["problems"][0], case["seeds"][0, 0]
    z = rp.slsqp(P, seed)
    x = rp.run(P, seed)[3]
    assert rp.feasible(P, z) and rp.value(P, z) <= rp.value(P, seed)
    assert abs(rp.value(P, z) - rp.value(P, x)) < 1e-5 * case["ds"]["Y_std"][0] or rp.value(P, x) < rp.value(P, z)


# ------------------------------------------------------------------------------------------ the case list
def _const(text, pattern):
    hit = re.search(pattern, text)
    assert hit, f"csrc/refine.hip no longer states {pattern!r} in the form this test reads: revisit refine_paths_oracle.CASES"
    return hit


def test_the_case_list_covers_every_edge():
    text = open(os.path.join(CSRC, "refine.hip")).read()
    header = open(os.path.join(ROOT, "include", "safebo.h")).read()
    lds_m = _const(text, r"constexpr\s+size_t\s+kRefLdsM\s*=\s*(\d+)\s*\*\s*1024\s*;")
    assert int(lds_m.group(1)) * 1024 == sh.LDS_M
    _const(text, r"static int refine_threads\(int n\) \{ return n > 256 \? 1024 : 256; \}")
    assert "for (int f = tid; f < F; f += bd)" in text and "for (int j = tid; j < n; j += bd)" in text      # ref_path_eval's strides
    assert "refine_lds_bytes(c, A.nu, 1, 0, lds_tier)" in text and "p / PA.K" in text
    assert int(_const(header, r"#define\s+SBO_REFINE_PATHS_MAX_STARTS\s+(\d+)").group(1)) == _lib.SBO_REFINE_PATHS_MAX_STARTS == 64
    assert (rp.N1, rp.N2) == (191, 135) and sh.staged(rp.N1, 1) and not sh.staged(rp.N1 + 1, 1) and sh.staged(rp.N2, 2) and not sh.staged(rp.N2 + 1, 2)
    col = lambda key, cases=rp.CASES: {c[key] for c in cases}
    small, large = [c for c in rp.CASES if c["n"] <= 256], [c for c in rp.CASES if c["n"] > 256]
    assert col("F", small) >= {1, 255, 256, 257} and col("F", large) >= {1023, 1025} and _lib.SBO_MAX_FEATURES in col("F")
    assert col("n") >= {1, 2, 20, 256, 257, 512, rp.N1, rp.N1 + 1, rp.N2, rp.N2 + 1, _lib.SBO_MAX_N}
    for n, slots in ((rp.N1, 1), (rp.N1 + 1, 1), (rp.N2, 2), (rp.N2 + 1, 2)):
        assert any(c["n"] == n and len(c["safe"]) == slots for c in rp.CASES), (n, slots)
    big = [c for c in rp.CASES if c["n"] == _lib.SBO_MAX_N]
    assert len(big) == 1 and big[0]["max_eval"] == 60
    assert col("S") >= {1, 17, _lib.SBO_MAX_PATHS} and col("K") >= {1, 3, _lib.SBO_REFINE_PATHS_MAX_STARTS}
    assert any(c["S"] * c["K"] == 4096 and c["n"] == 20 for c in rp.CASES)
    assert col("d") == {1, 2, 3, 4, 6, 8} and col("q") == {1, 2, 4}
    assert any(c["q"] == 1 and not c["safe"] for c in rp.CASES)
    assert any(c["q"] == 4 and c["output"] == 0 for c in rp.CASES) and any(c["q"] == 4 and c["output"] == 3 for c in rp.CASES)
    assert any(c["output"] in c["safe"] for c in rp.CASES)                                  # the path's output is also a constraint
    assert col("maximize") == {0, 1} and col("use_invK") == {True, False} and len(col("seed")) == len(rp.CASES)
    assert sum(1 for c in rp.CASES if c.get("bad")) == 2


# ------------------------------------------------------------------------------------------ the ABI
def test_symbol_and_structures_match_the_header(tmp_path):
    text = open(os.path.join(ROOT, "include", "safebo.h")).read()
    assert re.search(r"\bint\s+sbo_refine_paths\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "sbo_refine_paths" in {n for n, _, _ in _lib.SYMBOLS}
    fields_o = ["b", "output", "n_paths", "n_features", "n_starts", "maximize", "constraint_mask", "max_eval", "reserved", "lo", "hi", "tol"]
    fields_r = ["best", "best_x", "best_value", "evaluations", "converged", "reserved"]
    items = (["sizeof(sbo_refine_paths_opts)"] + [f"offsetof(sbo_refine_paths_opts, {f})" for f in fields_o] +
             ["sizeof(sbo_refine_paths_result)"] + [f"offsetof(sbo_refine_paths_result, {f})" for f in fields_r])
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safebo.h"\nint main(void) { printf("' + "%zu " * len(items) +
                   '%d\\n", ' + ", ".join(items) + ", SBO_ABI_VERSION); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    O, R = _lib.RefinePathsOpts, _lib.RefinePathsResult
    assert got == ([C.sizeof(O)] + [getattr(O, f).offset for f in fields_o] + [C.sizeof(R)] + [getattr(R, f).offset for f in fields_r] + [3])
    lib = _lib.load()
    assert hasattr(C.CDLL(_lib.library_path()), "sbo_refine_paths")
    assert lib.sbo_refine_paths(None, None, None, None, None, None, None, None, None, None, None) == _lib.SBO_E_INVALID
    res = R()
    for s in range(_lib.SBO_MAX_PATHS):
        res.best[s], res.best_value[s], res.best_x[s][1] = 5, 2.0, 3.0
    res.evaluations = res.converged = 4
    assert lib.sbo_refine_paths(None, None, None, None, None, None, None, None, None, None, C.byref(res)) == _lib.SBO_E_INVALID
    assert list(res.best) == [-1] * _lib.SBO_MAX_PATHS and np.isnan(np.array(res.best_value)).all()
    assert not np.array([list(r) for r in res.best_x]).any() and res.evaluations == 0 and res.converged == 0


# ------------------------------------------------------------------------------------------ the host's checks
def _bare_engine(d=2, q=3, n=4):
    eng = SweepEngine.__new__(SweepEngine)
    eng._ctx, eng._lib, eng.d, eng.q, eng.n = None, None, d, q, n
    return eng


SD = np.zeros((2, 3, 2))
BOX = dict(lo=[-1.0, -1.0], hi=[1.0, 1.0])


@pytest.mark.parametrize("kwargs", [
    dict(seeds=np.zeros((2, 3, 3))), dict(seeds=np.zeros(2)), dict(seeds=np.zeros((0, 2))), dict(seeds=np.zeros((2, 65, 2))),
    dict(seeds=np.zeros((65, 1, 2))), dict(seeds=np.zeros((1, 2, 3, 2))), dict(seeds=SD, b=-1.0), dict(seeds=SD, b=np.nan),
    dict(seeds=SD, b="3"), dict(seeds=SD, output=3), dict(seeds=SD, output=-1), dict(seeds=SD, features=0), dict(seeds=SD, features=8193),
    dict(seeds=SD, seed=-1), dict(seeds=SD, maximize=2), dict(seeds=SD, constraints=[0]), dict(seeds=SD, constraints=[3]),
    dict(seeds=SD, constraints=[1.0]), dict(seeds=SD, lo=[-1.0], hi=[1.0]), dict(seeds=SD, lo=[1.0, 1.0], hi=[-1.0, -1.0]),
    dict(seeds=SD, lo=[-np.inf, -1.0], hi=[1.0, 1.0]), dict(seeds=SD, max_eval=1.5), dict(seeds=SD, tol=np.nan),
    dict(seeds=SD, draws=SweepEngine.path_draws(2, 4, 3, 8, 0)), dict(seeds=SD, draws=SweepEngine.path_draws(3, 4, 2, 8, 0)),
    dict(seeds=SD, draws=SweepEngine.path_draws(2, 5, 2, 8, 0)),
])
def test_refine_paths_checks_its_arguments_on_the_host(kwargs):
    args = dict(b=2.0, **BOX)
    args.update(kwargs)
    with pytest.raises(ValueError):
        _bare_engine().refine_paths(**args)
    with pytest.raises(ValueError):
        SweepEngine.refine_paths_arguments(2, 3, 4, **args)
    with pytest.raises((ValueError, TypeError)):
        SweepEngine.refine_paths_arguments(2, 3, 4, 2.0, SD)                                # (the box is required)


def test_accepted_arguments_come_back_in_library_form():
    out = SweepEngine.refine_paths_arguments(2, 3, 4, 2, np.zeros((5, 2), dtype=np.float32), 1, 64, 7, None, True, None, **BOX)
    sd, b, o, F, seed, mx, draws, mask, lo, hi, max_eval, tol = out
    assert sd.shape == (5, 1, 2) and sd.dtype == np.float64 and sd.flags["C_CONTIGUOUS"]
    assert (b, o, F, seed, mx, draws, mask, max_eval, tol) == (2.0, 1, 64, 7, 1, None, 0b110, 0, 0.0)
    nan_seed = np.full((1, 2, 2), np.nan)                                                    # (the library reports it infeasible)
    assert SweepEngine.refine_paths_arguments(2, 3, 4, 0.0, nan_seed, constraints=[], **BOX)[7] == 0
    got = SweepEngine.refine_paths_arguments(2, 3, 4, 0.0, nan_seed, constraints=[2], max_eval=9, tol=1e-6, **BOX)
    assert (got[7], got[10], got[11]) == (0b100, 9, 1e-6)
    given = SweepEngine.path_draws(2, 4, 5, 9, 0)
    assert SweepEngine.refine_paths_arguments(2, 3, 4, 1.0, np.zeros((5, 2)), draws=given, **BOX)[3] == 9


# ------------------------------------------------------------------------------------------ the host class
class _FakeEngine:
    n = 7

    def __init__(self, S):
        self.S, self.calls, self.refined = S, [], []

    def mask(self, which, c=0):
        return self.S

    def sample_paths(self, points, n_paths, output=0, features=1024, seed=0, **kw):
        self.calls.append(dict(points=np.array(points), n_paths=n_paths, output=output, features=features, seed=seed, **kw))
        idx = (3 * np.arange(n_paths)) % len(points)
        return {"index": idx, "x": np.asarray(points)[idx], "value": np.arange(n_paths, dtype=np.float64)}

    def refine_paths(self, b, seeds, output=0, features=1024, seed=0, draws=None, maximize=False, constraints=None, *, lo, hi, **kw):
        self.refined.append(dict(b=b, seeds=np.array(seeds), output=output, features=features, seed=seed, draws=draws, maximize=maximize,
                                 constraints=constraints, lo=np.array(lo), hi=np.array(hi), **kw))
        S = len(seeds)
        return {"best_x": np.asarray(seeds)[:, 0] + 0.5, "best_value": -np.arange(S, dtype=np.float64)}


def _model(monkeypatch):
    m = SafeOpt.BO([mr.benoit_f, mr.benoit_g], mr.BOUND, 3.0, grid=(6, 5))
    S = np.zeros(30, dtype=bool)
    S[[28, 3, 17, 4, 9]] = True
    fake = _FakeEngine(S)
    monkeypatch.setattr(m, "_engine", fake)
    monkeypatch.setattr(m, "sweep", lambda want_masks=False: None)
    return m, fake


def test_thompson_itself_is_the_present_call(monkeypatch):
    """ThompsonRefined is a method of its own: Thompson keeps its signature, its single sample_paths call and its answer."""
    import inspect
    m, fake = _model(monkeypatch)
    assert [p.name for p in inspect.signature(SafeOpt.BO.Thompson).parameters.values()] == ["self", "k", "seed", "features", "exact"]
    X, v = m.Thompson(4, seed=11, features=256)
    pool = m._all_points()[[3, 4, 9, 17, 28]]
    assert np.array_equal(X, pool[(3 * np.arange(4)) % 5]) and v.tolist() == [0.0, 1.0, 2.0, 3.0]
    assert len(fake.calls) == 1 and np.array_equal(fake.calls[0]["points"], pool) and not fake.refined


@pytest.mark.parametrize("starts", [1, 3])
def test_thompson_refined_seeds_every_path_with_its_own_and_its_neighbours_arg_mins(monkeypatch, starts):
    m, fake = _model(monkeypatch)
    k = 4
    X, v = m.ThompsonRefined(k, seed=11, features=256, starts=starts)
    assert len(fake.calls) == 1 and len(fake.refined) == 1
    pool = m._all_points()[[3, 4, 9, 17, 28]]
    grid_x = pool[(3 * np.arange(k)) % 5]
    assert np.array_equal(fake.calls[0]["points"], pool) and (fake.calls[0]["features"], fake.calls[0]["seed"]) == (256, 11)
    call = fake.refined[0]
    want = np.stack([[grid_x[(s + j) % k] for j in range(starts)] for s in range(k)])
    assert call["seeds"].shape == (k, starts, 2) and np.array_equal(call["seeds"], want)
    assert (call["b"], call["output"], call["features"], call["seed"], call["constraints"], call["maximize"]) == (3.0, 0, 256, 11, None, False)
    assert call["draws"] is None and np.array_equal(call["lo"], mr.BOUND[:, 0]) and np.array_equal(call["hi"], mr.BOUND[:, 1])
    assert np.array_equal(X, grid_x + 0.5) and v.tolist() == [0.0, -1.0, -2.0, -3.0]


def test_thompson_refined_refuses_bad_starts_and_has_no_exact_form(monkeypatch):
    import inspect
    m, fake = _model(monkeypatch)
    assert "exact" not in inspect.signature(SafeOpt.BO.ThompsonRefined).parameters       # (an exact draw is a vector, not a function)
    with pytest.raises(TypeError):
        m.ThompsonRefined(4, exact=True)
    for bad in (0, 1.5, True):
        with pytest.raises(ValueError):
            m.ThompsonRefined(4, starts=bad)
    assert not fake.calls and not fake.refined
    fake.S = np.zeros(30, dtype=bool)
    X0, v0 = m.ThompsonRefined(2)
    assert X0.shape == (0, 2) and v0.shape == (0,) and not fake.refined
