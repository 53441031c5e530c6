"""sbo_refine_paths on the device against tests/refine_paths_oracle.py: every committed case -- feasibility
under ``bounds``, the value bit for bit ``sample_paths``' at the returned point and within TOL64 of the oracle's, no worse than at the
seed, the statuses of infeasible seeds, the result block, local optimality (the KKT bars of tests/test_gpu_refine.py) and real progress
--, then bits (tiers, repeat calls, permuted starts, K = 1 inside K = 3), the model's history, untouched residents, refusals, and the
host class."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
from safebo_amd import SafeOpt, SweepEngine, _lib, synthetic

import model_remove as mr
import refine_paths_oracle as rp
import refine_sets_oracle as rs

pytestmark = pytest.mark.gpu

IDS = [rp.case_id(c) for c in rp.CASES]
INFEASIBLE, CONVERGED = _lib.SBO_REFINE_INFEASIBLE_SEED, _lib.SBO_REFINE_CONVERGED


def _call(eng, c, case, seeds=None, **kw):
    args = rp.engine_args(c, case)
    args.update(kw)
    return eng.refine_paths(rp.B, case["seeds"] if seeds is None else seeds, **args)


def _values_at(eng, c, case, x):
    """sample_paths' values [S, K] at the points x [S, K, d]: column s of the row of (s, k)."""
    S, K, d = x.shape
    v = eng.sample_paths(x.reshape(-1, d), S, c["output"], draws=case["draws"], return_values=True)["values"]
    return v.reshape(S, K, S)[np.arange(S), :, np.arange(S)]


def _bits(out):
    return tuple(out[k].tobytes() for k in ("x", "value", "status", "best", "best_x", "best_value")) + (out["evaluations"], out["converged"])


# ------------------------------------------------------------------------------------------ 1. every committed case
@pytest.mark.parametrize("i", range(len(rp.CASES)), ids=IDS)
def test_every_committed_case_against_the_oracle(engine, i):
    c, case = rp.CASES[i], rp.make_case(i)
    ds, seeds, S, K, d, o = case["ds"], case["seeds"], c["S"], c["K"], c["d"], c["output"]
    engine.set_model(ds, use_invK=c["use_invK"])
    out = _call(engine, c, case)
    x, val, st = out["x"], out["value"], out["status"]
    assert x.shape == (S, K, d) and val.shape == st.shape == (S, K) and st.dtype == np.int32
    sg = -1.0 if c["maximize"] else 1.0
    # the seeds' statuses: infeasible exactly where the oracle says so, and those rows come back unchanged
    bad = np.array([[not rp.feasible(case["problems"][s], seeds[s, k]) for k in range(K)] for s in range(S)])
    assert np.array_equal(st == INFEASIBLE, bad), (st, bad)
    assert np.array_equal(x[bad], seeds[bad]) and bad.sum() == (1 if c.get("bad") else 0)
    # feasible under the values bounds() gives at the returned points
    flat = x.reshape(-1, d)
    assert np.all((flat >= case["lo"]) & (flat <= case["hi"]) | bad.reshape(-1, 1))
    if c["safe"]:
        engine.set_points(flat)
        for cc in c["safe"]:
            lcb = engine.bounds(rp.B, cc, "lcb").reshape(S, K)
            assert np.all(lcb[~bad] >= 0.0), (cc, lcb)
    # the value: sample_paths' bits at the returned point, the oracle's within TOL64, no worse than sample_paths' at the seed
    at_x, at_seed = _values_at(engine, c, case, x), _values_at(engine, c, case, seeds)
    assert val.tobytes() == at_x.tobytes()
    ref = rp.path_values(ds, o, case["draws"], flat).reshape(S, K, S)[np.arange(S), :, np.arange(S)]
    err = float(np.max(np.abs(val - ref)) / ds["Y_std"][o])
    print(rp.case_id(c), "value against paths_solve", err)
    assert err < rp.TOL64, err
    assert np.all(sg * val <= sg * at_seed), (val, at_seed)
    # the result block
    for s in range(S):
        key = np.where(bad[s] | np.isnan(val[s]), np.inf, sg * val[s])
        want = int(np.argmin(key)) if np.isfinite(key).any() else -1
        assert out["best"][s] == want, (s, out["best"][s], want)
        if want >= 0:
            assert np.array_equal(out["best_x"][s], x[s, want]) and out["best_value"][s] == val[s, want]
    assert out["converged"] == int(np.sum(st == CONVERGED)) and out["evaluations"] >= int(np.sum(~bad))
    # local optimality where the device converged; at most one feasible problem in eight may end otherwise
    held = [(s, k) for s, k in rp.held(c) if not bad[s, k]]
    if held:
        other = [(s, k, int(st[s, k])) for s, k in held if st[s, k] != CONVERGED]
        worst = max([rp.kkt_residual(case["problems"][s], x[s, k]) for s, k in held if st[s, k] == CONVERGED], default=0.0)
        print(rp.case_id(c), "kkt", worst, "not converged", other)
        assert worst <= rp.kkt_bar(c), worst
        assert 8 * len(other) <= len(held), other
    # real progress (tests/test_gpu_refine.py): a feasible seed off its optimum improves by more than 1e-6
    if c["n"] >= 20:
        for s, k in held:
            if rp.kkt_residual(case["problems"][s], seeds[s, k]) > 1e-3:
                assert sg * (at_seed[s, k] - val[s, k]) > rp.PROGRESS * ds["Y_std"][o], (s, k, at_seed[s, k], val[s, k])


# ------------------------------------------------------------------------------------------ 2. bits
TIER_CASES = [i for i, c in enumerate(rp.CASES) if c["n"] in (rp.N1, rp.N1 + 1, rp.N2, rp.N2 + 1)] + [2]


@pytest.mark.parametrize("i", TIER_CASES, ids=[IDS[i] for i in TIER_CASES])
def test_lds_and_streamed_tiers_and_two_calls_give_identical_bits(engine, i):
    c, case = rp.CASES[i], rp.make_case(i)
    engine.set_model(case["ds"], use_invK=c["use_invK"])
    a, again = _call(engine, c, case), _call(engine, c, case)
    engine.set_option("refine_lds", 0)
    try:
        b = _call(engine, c, case)
    finally:
        engine.set_option("refine_lds", 1)
    assert _bits(a) == _bits(again) == _bits(b)
    assert a["converged"] > 0


def test_permuted_starts_permute_the_results_and_one_start_is_the_first_of_three(engine):
    i = 2
    c, case = rp.CASES[i], rp.make_case(i)
    assert c["K"] == 3
    engine.set_model(case["ds"], use_invK=c["use_invK"])
    a = _call(engine, c, case)
    perm = [2, 0, 1]
    b = _call(engine, c, case, seeds=np.ascontiguousarray(case["seeds"][:, perm]))
    for k in ("x", "value", "status"):
        assert np.ascontiguousarray(a[k][:, perm]).tobytes() == b[k].tobytes(), k
    one = _call(engine, c, case, seeds=np.ascontiguousarray(case["seeds"][:, :1]))
    for k in ("x", "value", "status"):
        assert np.ascontiguousarray(a[k][:, :1]).tobytes() == one[k].tobytes(), k
    flat = _call(engine, c, case, seeds=np.ascontiguousarray(case["seeds"][:, 0]))      # ([S, d] is K = 1)
    assert _bits(flat) == _bits(one)


# ------------------------------------------------------------------------------------------ 3. the model's history
def test_the_call_follows_appends_and_removals(engine):
    """After append_sample and after remove_sample the call is held to the oracle on the changed data (values within TOL64, feasible,
    no worse than the seed); an append followed by the removal of that row gives the first call's bits back."""
    i = 2
    c, case = rp.CASES[i], rp.make_case(i)
    ds = case["ds"]
    n, d, S = c["n"], c["d"], c["S"]
    rng = np.random.default_rng(3)
    xn, yn = rng.uniform(-0.5, 0.5, d), np.array([0.1, 0.4])
    grown = mr.with_rows(ds, np.vstack([ds["X_norm"], xn]), np.vstack([ds["Y_norm"], yn]))
    shrunk = mr.without(ds, 3)
    seeds = np.ascontiguousarray(case["seeds"][:, :1])

    def check(data, n_rows):
        draws = SweepEngine.path_draws(d, n_rows, S, c["F"], c["seed"])
        out = engine.refine_paths(rp.B, seeds, c["output"], draws=draws, constraints=c["safe"], lo=case["lo"], hi=case["hi"])
        ref = rp.path_values(data, c["output"], draws, out["x"].reshape(-1, d)).reshape(S, 1, S)[np.arange(S), :, np.arange(S)]
        assert float(np.max(np.abs(out["value"] - ref)) / data["Y_std"][c["output"]]) < rp.TOL64
        at_seed = rp.path_values(data, c["output"], draws, seeds.reshape(-1, d)).reshape(S, 1, S)[np.arange(S), :, np.arange(S)]
        ok = out["status"] != INFEASIBLE
        assert ok.any() and np.all(out["value"][ok] <= at_seed[ok] + rp.TOL64 * data["Y_std"][c["output"]])
        m, v = oracle.gp_inference(out["x"].reshape(-1, d), data)
        lcb = (m[:, 1] - rp.B * np.sqrt(v[:, 1])).reshape(S, 1)
        assert np.all(lcb[ok] >= -rp.TOL64 * data["Y_std"][1])
        return out

    engine.set_model(ds, use_invK=c["use_invK"])
    first = check(ds, n)
    engine.append_sample(xn, yn)
    check(grown, n + 1)
    engine.remove_sample(n)
    assert _bits(check(ds, n)) == _bits(first)
    engine.remove_sample(3)
    check(shrunk, n - 1)


# ------------------------------------------------------------------------------------------ 4. residents
def test_the_call_does_not_touch_sweeps_masks_or_audit(engine):
    ds, b, lo, hi = rs.load("benoit_n20_50x50")
    engine.set_model(ds)
    engine.set_grid(lo, hi, [50, 50])
    first = engine.sweep_safeopt(b, want_masks=True)
    masks = {k: engine.mask(k) for k in ("S", "U", "M")}
    prof = engine.profile()
    out = engine.refine_paths(b, np.tile(first["minimizer_x"], (4, 1)), features=64, seed=1, lo=lo, hi=hi)
    assert out["x"].shape == (4, 1, 2)
    after = engine.profile()
    for k in ("guard_audit_samples", "guard_audit_violations", "guard_audit_skipped"):
        assert after[k] == prof[k], k
    again = engine.sweep_safeopt(b, want_masks=True, posterior_ready=True)
    for k in ("minimizer_index", "expander_index", "count_S", "count_U", "count_M", "u_star"):
        assert again[k] == first[k], k
    for k in masks:
        assert np.array_equal(engine.mask(k), masks[k]), k
    fresh = engine.sweep_safeopt(b, want_masks=True)
    assert fresh["minimizer_index"] == first["minimizer_index"] and fresh["count_S"] == first["count_S"]


# ------------------------------------------------------------------------------------------ 5. refusals
STALE = 7.5


def _raw(eng, draws, seeds, S, F, K, lo, hi, null=(), ctx=True, result=True, **fields):
    """The C call itself with stale outputs: (status, result, x, value, status array)."""
    arrays = dict(zip(("omega", "phase", "weights", "noise"), (np.ascontiguousarray(a, dtype=np.float64) for a in draws)))
    arrays["seeds"] = np.ascontiguousarray(seeds, dtype=np.float64)
    ptr = lambda name: None if name in null else arrays[name].ctypes.data_as(C.c_void_p)
    d = len(lo)
    o = _lib.RefinePathsOpts()
    o.b, o.n_paths, o.n_features, o.n_starts, o.constraint_mask = rp.B, S, F, K, 2
    for a in range(d):
        o.lo[a], o.hi[a] = lo[a], hi[a]
    for k, v in fields.items():
        setattr(o, k, v)
    res = _lib.RefinePathsResult()
    for s in range(_lib.SBO_MAX_PATHS):
        res.best[s], res.best_value[s], res.best_x[s][0] = 5, STALE, STALE
    res.evaluations, res.converged = 9, 9
    x, val, st = np.full((S, K, d), STALE), np.full((S, K), STALE), np.full((S, K), 9, dtype=np.int32)
    rc = eng._lib.sbo_refine_paths(eng._ctx if ctx else None, C.byref(o), ptr("omega"), ptr("phase"), ptr("weights"), ptr("noise"),
                                   ptr("seeds"), x.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p),
                                   st.ctypes.data_as(C.c_void_p), C.byref(res) if result else None)
    return rc, res, x, val, st


def _cleared(res):
    return (list(res.best) == [-1] * _lib.SBO_MAX_PATHS and np.isnan(np.array(res.best_value)).all() and
            not np.array([list(r) for r in res.best_x]).any() and res.evaluations == 0 and res.converged == 0)


def test_every_refusal_clears_the_result_writes_nothing_and_leaves_the_next_call_intact(engine):
    i = 2
    c, case = rp.CASES[i], rp.make_case(i)
    S, K, F, lo, hi = c["S"], c["K"], c["F"], case["lo"], case["hi"]
    engine.set_model(case["ds"], use_invK=c["use_invK"])
    want = _call(engine, c, case)
    dr, sd = case["draws"], case["seeds"]
    nan_w = np.array(dr[2]); nan_w[0, 0] = np.nan
    refusals = [dict(null=("omega",)), dict(null=("phase",)), dict(null=("weights",)), dict(null=("noise",)), dict(null=("seeds",)),
                dict(ctx=False), dict(n_paths=0), dict(n_paths=65), dict(n_features=0), dict(n_features=8193), dict(n_starts=0),
                dict(n_starts=65), dict(output=2), dict(output=-1), dict(maximize=2), dict(constraint_mask=1), dict(constraint_mask=4),
                dict(b=-1.0), dict(b=np.nan), dict(tol=np.nan), dict(draws=(dr[0], dr[1], nan_w, dr[3]))]
    for kw in refusals:
        draws = kw.pop("draws", dr)
        rc, res, x, val, st = _raw(engine, draws, sd, S, F, K, lo, hi, **kw)
        assert rc == _lib.SBO_E_INVALID, kw
        assert _cleared(res) and np.all(x == STALE) and np.all(val == STALE) and np.all(st == 9), kw
    rc, res, x, val, st = _raw(engine, dr, sd, S, F, K, hi, lo)                               # a bad box
    assert rc == _lib.SBO_E_INVALID and _cleared(res) and np.all(x == STALE)
    assert engine._lib.sbo_refine_paths(engine._ctx, None, None, None, None, None, None, None, None, None, None) == _lib.SBO_E_INVALID
    rc, res, x, val, st = _raw(engine, dr, sd, S, F, K, lo, hi)                               # the same arguments, accepted
    assert rc == _lib.SBO_OK and x.tobytes() == want["x"].tobytes() and val.tobytes() == want["value"].tobytes()
    assert st.tobytes() == want["status"].tobytes() and list(res.best[:S]) == want["best"].tolist() and list(res.best[S:]) == [-1] * (64 - S)
    engine.set_model(case["ds"], dtype="f32")
    try:
        rc, res, x, val, st = _raw(engine, dr, sd, S, F, K, lo, hi)
        assert rc == _lib.SBO_E_UNSUPPORTED and _cleared(res) and np.all(x == STALE)
    finally:
        engine.set_model(case["ds"], use_invK=c["use_invK"])
    assert _bits(_call(engine, c, case)) == _bits(want)
    # a non-finite seed is infeasible with value NaN; the other problems are what they were
    sd2 = np.array(sd); sd2[0, 0, 0] = np.nan
    out = _call(engine, c, case, seeds=sd2)
    assert out["status"][0, 0] == INFEASIBLE and np.isnan(out["value"][0, 0]) and np.isnan(out["x"][0, 0, 0])
    keep = np.ones((S, K), dtype=bool); keep[0, 0] = False
    assert out["value"][keep].tobytes() == want["value"][keep].tobytes() and out["x"][keep].tobytes() == want["x"][keep].tobytes()


def test_without_a_model_the_call_is_no_model():
    import safebo_amd
    with safebo_amd.SweepEngine(0) as eng:
        rc, res, x, val, st = _raw(eng, SweepEngine.path_draws(2, 4, 1, 8, 0), np.zeros((1, 1, 2)), 1, 8, 1, -np.ones(2), np.ones(2))
        assert rc == _lib.SBO_E_NO_MODEL and _cleared(res) and np.all(x == STALE)


# ------------------------------------------------------------------------------------------ 6. host class
def test_thompson_refined_on_benoit():
    """Benoit, fixture benoit_n20_50x50 (its data, hyper-parameters and b) on the 50 x 50 grid, k = 16, seed 5."""
    z = np.load(os.path.join(rs.GOLDEN, "benoit_n20_50x50.npz"))
    m = SafeOpt.BO([mr.benoit_f, mr.benoit_g], z["bound"], float(z["b"]), grid=(50, 50))
    m.fixed_hyper = z["hypopt"]
    m.GP_initialization(z["X"], z["Y"], "RBF", multi_hyper=5, var_out=True)
    Xg, vg = m.Thompson(16, seed=5)
    X1, v1 = m.ThompsonRefined(16, seed=5)
    X3, v3 = m.ThompsonRefined(16, seed=5, starts=3)
    again = m.Thompson(16, seed=5)
    assert Xg.tobytes() == again[0].tobytes() and vg.tobytes() == again[1].tobytes()
    assert X1.shape == X3.shape == (16, 2)
    m.engine.set_points(np.vstack([X1, X3]))
    assert np.all(m.engine.bounds(m.b, 1, "lcb") >= 0.0)
    ys = m.inference_datasets["Y_std"][0]
    gain = (vg - v1) / ys
    print("ThompsonRefined: gain per path (normalised)", np.sort(gain))
    assert np.all(v1 <= vg) and np.all(v3 <= v1)
    assert int(np.sum(gain > 1e-6)) >= 12, gain
