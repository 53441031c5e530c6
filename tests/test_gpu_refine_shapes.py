"""The refine solver's posterior gradient (csrc/refine.hip: ref_eval) over its shape range, on the device.

The exact check behind the solver launders a gradient that is subtly wrong: a descent method with an Armijo test still "moves and
improves".  What notices is the KKT residual of the returned point under the NumPy gradients and "no worse than SLSQP", here at
the shapes where ref_eval's loops change path (tests/refine_shapes.py: launch shape, the LDS tier's boundary, up to eight slots,
d = 1 and 8, a pair at d = 4), and the same call after sbo_model_remove against the dataset set afresh -- a removal leaves f_cap and
a_ld where they were while n shrinks.  tests/test_refine_shapes_cpu.py checks every case against the reference alone; the measured
figures are in profiles/refine_shape_checks.md."""
import numpy as np
import pytest

import oracle
from safebo_amd import _lib

import refine_sets_oracle as rs
import refine_shapes as S
import robust_refine_oracle as rr

pytestmark = pytest.mark.gpu

MOVED = (_lib.SBO_REFINE_CONVERGED, _lib.SBO_REFINE_MAX_EVAL)
KEYS = ("x", "xp", "value", "status")


def _call(engine, P, seeds, max_eval=None):
    """sbo_refine for a point with safe terms only, sbo_refine_sets for a pair."""
    seeds = np.atleast_2d(seeds)
    d = P["d"]
    if P["pair"]:
        return engine.refine_sets(P["b"], seeds[:, :d], seeds[:, d:], max_eval=max_eval, **rs.engine_args(P))
    return engine.refine(P["b"], seeds, P["objective"], P["kind"], P["maximize"], constraints=P["safe"], lo=P["lo"], hi=P["hi"],
                         max_eval=max_eval)


def _both_tiers(engine, P, seeds, max_eval=None):
    """The same call with M staged in LDS (where it fits) and streamed (option refine_lds = 0); the two must agree bit for bit."""
    try:
        a = _call(engine, P, seeds, max_eval)
        engine.set_option("refine_lds", 0)
        b = _call(engine, P, seeds, max_eval)
    finally:
        engine.set_option("refine_lds", 1)
    for k in KEYS:
        if k in a:
            assert np.array_equal(a[k], b[k]), k
    assert a["evaluations"] == b["evaluations"] and a["best"] == b["best"]
    return a


def _z(P, out, s):
    return np.concatenate([out["x"][s], out["xp"][s]]) if P["pair"] else out["x"][s].copy()


def _exact(engine, P, z):
    """Every term and the reported figure at z from ``engine.bounds`` on the point list (x, x'): ({term: g >= 0}, value)."""
    d, b = P["d"], P["b"]
    pts = np.asarray(z).reshape(-1, d)
    engine.set_points(pts)
    lcb = {c: engine.bounds(b, c, "lcb") for c in set(P["safe"]) | set(P["unsafe"])}
    g = {f"safe{c}": lcb[c][0] for c in P["safe"]}
    for c in P["unsafe"]:
        g[f"unsafe{c}"] = -lcb[c][1]
    if P["link"] is not None:
        c, L = P["link"]
        g["link"] = engine.bounds(b, c, "ucb")[0] - L * oracle.shifted_norm(pts[0], pts[1])
    lo, hi = rs.box(P)
    g["box"] = 0.0 if (np.all(z >= lo) and np.all(z <= hi)) else -1.0
    return g, float(engine.bounds(b, P["objective"], P["kind"])[1 if P["at"] == "xp" else 0])


def measure(engine, case):
    """One call (two where the case asks for both tiers) on the case's model: per seed the figures the record lists."""
    P, seeds, yard = S.problem(case), S.seeds(case), S.yardstick(case)
    engine.set_model(S.dataset(case))
    out = (_both_tiers if case["tiers"] else _call)(engine, P, seeds, case["max_eval"])
    sg = -1.0 if P["maximize"] else 1.0
    rows = []
    for s, (seed, y) in enumerate(zip(seeds, yard)):
        z, v = _z(P, out, s), float(out["value"][s])
        g, v_exact = _exact(engine, P, z)
        _, v_seed = _exact(engine, P, seed)
        rows.append({"case": case["name"], "seed": s, "status": int(out["status"][s]), "evaluations": out["evaluations"], "value": v,
                     "exact": v_exact, "seed_value": v_seed, "slack": min(g.values()), "kkt": rs.kkt_residual(P, z),
                     "gap": sg * (v - y["value"]) / (1.0 + abs(y["value"])), "yardstick": y["value"], "ref_kkt": y["kkt"], "sg": sg,
                     "bar": S.kkt_bar(case), "z": z.tolist()})
    return rows


def check(rows):
    for r in rows:
        print("refine shapes {case} seed {seed}: status {status} evaluations {evaluations} value {value!r} yardstick {yardstick!r} "
              "gap {gap:.3e} kkt {kkt:.3e} (reference {ref_kkt:.3e}) slack {slack:.3g} at {z}".format(**r))
    for r in rows:
        assert r["status"] in MOVED, r
        assert r["value"] == r["exact"], r                                     # the figure of sbo_bounds at the returned point
        assert r["slack"] >= 0.0, r                                            # every enforced term under the closed predicates
        assert r["sg"] * r["value"] <= r["sg"] * r["seed_value"], r
        assert r["gap"] <= 1e-8, r                                             # no worse than the SLSQP yardstick
        assert r["status"] == _lib.SBO_REFINE_CONVERGED, r
        assert r["kkt"] <= r["bar"], r


@pytest.mark.parametrize("name", list(S.CASES))
def test_returned_points_are_stationary_and_no_worse_than_slsqp(engine, name):
    check(measure(engine, S.CASES[name]))


# ---- after sbo_model_remove ---------------------------------------------------------------------------------------------------------
def _against_fresh(label, P, seed, out, fresh):
    z, zf = _z(P, out, 0), _z(P, fresh, 0)
    v, vf, vo = float(out["value"][0]), float(fresh["value"][0]), rs.value(P, z)
    d = P["d"]
    print(f"refine shapes {label}: status {out['status'][0]} evaluations {out['evaluations']} dx {np.max(np.abs(z[:d] - zf[:d])):.3e} "
          f"dxp {np.max(np.abs(z[d:] - zf[d:]), initial=0.0):.3e} "
          f"dvalue {abs(v - vf):.3e} against the oracle {abs(v - vo):.3e} value {v!r}")
    sg = -1.0 if P["maximize"] else 1.0
    assert out["status"][0] in MOVED and sg * v < sg * rs.value(P, seed), label
    # x' of a pair is held to the bar where a term pins it: with its terms slack at the solution (lcb_c(x') <= 0 and the link) the
    # objective, at x, does not depend on it, and it ends wherever the barrier's last stages left it
    free = P["pair"] and all(g > 1e-3 for name, g, _ in rs.terms(P, zf) if name.startswith(("unsafe", "link")))
    assert np.max(np.abs(z[:d] - zf[:d] if free else z - zf)) <= 1e-5, label
    assert abs(v - vf) <= 1e-9 * max(1.0, abs(vf)), label
    assert abs(v - vo) <= 1e-10 * max(1.0, abs(vo)), label


@pytest.mark.parametrize("n0", S.REMOVALS)
def test_refine_and_refine_sets_follow_removed_samples(engine, n0):
    """f_cap and a_ld stay at the parent's while n shrinks: both entry points, in both tiers, land where the same dataset set afresh
    lands (n0 = 140 crosses the tier switch of two slots, and of a pair, downwards)."""
    ds0, order = S._synthetic(n0, 2, 5), S.removal_order(n0, S.REMOVE_K)
    ds = S.after_removals(ds0, order)
    problems = S.removal_problems(ds, n0)
    engine.set_model(ds)
    fresh = [_call(engine, P, seed) for _, P, seed in problems]
    engine.set_model(ds0)
    for j in order:
        engine.remove_sample(j)
    assert engine.n == n0 - S.REMOVE_K
    for (label, P, seed), f in zip(problems, fresh):
        out = _both_tiers(engine, P, seed)
        _against_fresh(f"{label} after removals n0 {n0}", P, seed, out, f)
        g, v = _exact(engine, P, _z(P, out, 0))
        assert min(g.values()) >= 0.0 and v == out["value"][0], label


def _robust(engine, c, xc):
    return engine.refine_robust(rr.B, xc, c["nxc"], c["lo"], c["hi"], c["count_d"], "ucb")


@pytest.mark.parametrize("n0", S.REMOVALS)
def test_refine_robust_follows_removed_samples(engine, n0):
    c, order = S.robust_case(n0), S.removal_order(n0, S.REMOVE_K)
    ds = S.after_removals(c["ds0"], order)
    xc0 = rr.grid_winner(dict(c, ds=ds))["xc"]
    engine.set_model(ds, mean_prior=c["mp"])
    fresh = _robust(engine, c, xc0)
    engine.set_model(c["ds0"], mean_prior=c["mp"])
    for j in order:
        engine.remove_sample(j)
    try:
        out = _robust(engine, c, xc0)
        engine.set_option("refine_lds", 0)
        streamed = _robust(engine, c, xc0)
    finally:
        engine.set_option("refine_lds", 1)
    assert out.keys() == streamed.keys()
    for k in out:
        assert np.array_equal(np.asarray(out[k]), np.asarray(streamed[k])), k
    Cset = np.vstack((rr.check_grid(c["lo"], c["hi"], c["nxc"], c["count_d"]), out["scenarios"]))
    f, l = rr.exact_on(out["xc"], Cset, ds, c["mp"], rr.B, "ucb")
    print(f"refine shapes robust after removals n0 {n0}: status {out['status']} rounds {out['rounds']} evaluations {out['evaluations']} "
          f"dxc {np.max(np.abs(out['xc'] - fresh['xc'])):.3e} dvalue {abs(out['value'] - fresh['value']):.3e} against the oracle "
          f"{abs(out['value'] - f.max()):.3e} seed {out['seed_value']!r} value {out['value']!r}")
    assert out["status"] in MOVED and out["value"] < out["seed_value"]
    assert np.max(np.abs(out["xc"] - fresh["xc"])) <= 1e-5
    assert abs(out["value"] - fresh["value"]) <= 1e-9 * max(1.0, abs(fresh["value"]))
    assert abs(out["value"] - f.max()) <= 1e-10 * max(1.0, abs(f.max()))
    assert np.all(out["g_min"] >= 0.0) and np.all(l[:, 1:].min(axis=0) >= -1e-10 * np.maximum(1.0, ds["Y_std"][1:]))


@pytest.mark.parametrize("n0", S.WINDOW)
def test_refine_follows_a_sliding_window(engine, n0):
    ds0, Xn, Yn, ds = S.window_model(n0)
    problems = S.removal_problems(ds, n0)
    engine.set_model(ds)
    fresh = [_call(engine, P, seed) for _, P, seed in problems]
    engine.set_model(ds0)
    for xn, yn in zip(Xn, Yn):
        engine.remove_sample(0)
        engine.append_sample(xn, yn)
    assert engine.n == n0
    for (label, P, seed), f in zip(problems, fresh):
        _against_fresh(f"{label} after a window n0 {n0}", P, seed, _both_tiers(engine, P, seed), f)


@pytest.mark.parametrize("n", [2, 1])
def test_models_of_two_rows_and_of_one(engine, n):
    """Reachable by removals only.  Two rows: the values against the oracle and the feasibility contract.  One row: the call
    returns, its value is sbo_bounds' at the returned point and both tiers agree (the optimum sits on the box)."""
    ds0, order, ds, seeds = S.tiny_model(n)
    engine.set_model(ds0)
    for j in order:
        engine.remove_sample(j)
    assert engine.n == n
    P = rs.problem(ds, 2.0, -np.ones(2), np.ones(2), "lcb")
    out = _both_tiers(engine, P, seeds)
    for s, seed in enumerate(seeds):
        x, v = out["x"][s], float(out["value"][s])
        g, v_exact = _exact(engine, P, x)
        print(f"refine shapes n {n} seed {s}: status {out['status'][s]} x {x} value {v!r} lcb_1 {g['safe1']!r}")
        assert v == v_exact
        if n == 1:
            continue
        ok, slack = rs.feasible(P, seed)
        assert (out["status"][s] == _lib.SBO_REFINE_INFEASIBLE_SEED) == (not ok), (s, slack)
        assert abs(v - rs.value(P, x)) <= 1e-10 * max(1.0, abs(rs.value(P, x)))
        if ok:
            assert g["safe1"] >= 0.0 and g["box"] == 0.0 and v <= rs.value(P, seed) + 1e-12 * (1.0 + abs(v))
        else:
            assert np.array_equal(x, seed)
    if n == 2:
        assert out["best"] >= 0 and np.any(np.isin(out["status"], MOVED))
