"""sbo_refine on the device: refined acquisition optima against SciPy SLSQP and the NumPy oracle, the exact
check, statuses and determinism of seed batches, box handling, the LDS and streamed tiers, appended models, no interference with
the sweeps, argument errors and the host classes' opt-in ``refine``."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
from safebo_amd import BayesRTOjax, GoOSE, GP_TR, SafeOpt, _lib, synthetic
from safebo_amd.BayesRTOjax import DataStorage

import refine_oracle as ro
import refine_sets_oracle as rs
from refine_shapes import _synthetic

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
X0_BENOIT = np.array([1.43157895, -0.44360902])        # ~ 400 x 400 grid point 44786: the r = 0.3 trust-region winner from there


def _fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return synthetic.make_dataset(z["X"], z["Y"], z["hypopt"]), float(z["b"]), z["bound"][:, 0].copy(), z["bound"][:, 1].copy()


def _bounds_at(engine, x, b):
    engine.set_points(np.atleast_2d(x))
    return {(o, k): engine.bounds(b, o, k) for o in range(engine.q) for k in ("mean", "ucb", "lcb", "var")}


def _masked_argmin(engine, b, lo, hi, count, kind="lcb", maximize=False):
    engine.set_grid(lo, hi, count)
    f = engine.bounds(b, 0, kind)
    ok = engine.bounds(b, 1, "lcb") >= 0
    g = int(np.argmin(np.where(ok, -f if maximize else f, np.inf)))
    return oracle.grid_points(lo, hi, count, first=g, n=1)[0]


def test_rosen4_refines_the_32_grid_winner_to_the_continuous_optimum(engine):
    ds, b, lo, hi = _fixture("rosen4_n128_9x8x7x6")
    engine.set_model(ds)
    seed = _masked_argmin(engine, b, lo, hi, [32] * 4)
    out = engine.refine(b, seed[None, :], 0, "lcb", lo=lo, hi=hi)
    x, v = out["x"][0], out["value"][0]
    assert out["status"][0] in (_lib.SBO_REFINE_CONVERGED, _lib.SBO_REFINE_MAX_EVAL)
    assert v <= -373.60, v                                  # SLSQP: -373.6037 (infeasible by 5e-8); the grid: -345.23
    bnd = _bounds_at(engine, x, b)
    assert bnd[(1, "lcb")][0] >= 0.0
    assert bnd[(0, "lcb")][0] == v
    assert out["best"] == 0 and np.array_equal(out["best_x"], x) and out["best_value"] == v
    assert rs.kkt_residual(rs.problem(ds, b, lo, hi, "lcb", safe=[1]), x) <= 1e-5


def test_benoit_trust_region_refines_and_unsticks_small_radii(engine):
    ds, b, lo, hi = _fixture("benoit_n20_50x50")
    engine.set_model(ds)
    x0 = oracle.grid_points(lo, hi, [400, 400], first=44786, n=1)[0]
    assert np.allclose(x0, X0_BENOIT, atol=1e-8)
    engine.set_grid(lo, hi, [400, 400])
    tr = engine.sweep_tr(b, x0, 0.3)
    assert tr["index"] == 44786
    out = engine.refine(b, np.stack([tr["x"], x0]), lo=lo, hi=hi, x_0=x0, r=0.3)
    assert out["best_value"] <= 0.37312 and np.linalg.norm(out["best_x"] - x0) <= 0.3
    # below the grid spacing the ball holds x_0 only: the sweep stays, the refine moves
    engine.set_grid(lo, hi, [400, 400])
    tr = engine.sweep_tr(b, x0, 0.002)
    assert tr["count_T"] == 1 and np.array_equal(tr["x"], x0)
    out = engine.refine(b, x0[None, :], lo=lo, hi=hi, x_0=x0, r=0.002)
    step = np.linalg.norm(out["best_x"] - x0)
    assert 0.0015 < step <= 0.002
    assert tr["lcb"] - out["best_value"] >= 2.9e-4
    assert _bounds_at(engine, out["best_x"], b)[(1, "lcb")][0] >= 0.0


@pytest.mark.parametrize("name,count", [("benoit_n20_50x50", [50, 50]), ("rosen4_n128_9x8x7x6", [9, 8, 7, 6])])
@pytest.mark.parametrize("kind,maximize", [("mean", False), ("ucb", False), ("lcb", False), ("var", True)])
def test_each_kind_is_feasible_no_worse_than_its_seed_and_than_slsqp(engine, name, count, kind, maximize):
    ds, b, lo, hi = _fixture(name)
    engine.set_model(ds)
    seed = _masked_argmin(engine, b, lo, hi, count, kind, maximize)
    out = engine.refine(b, seed[None, :], 0, kind, maximize, lo=lo, hi=hi)
    x, v = out["x"][0], out["value"][0]
    sg = -1.0 if maximize else 1.0
    bnd = _bounds_at(engine, seed, b)
    assert sg * v <= sg * bnd[(0, kind)][0]
    bnd = _bounds_at(engine, x, b)
    assert bnd[(1, "lcb")][0] >= 0.0 and bnd[(0, kind)][0] == v
    P = rs.problem(ds, b, lo, hi, kind, maximize=maximize, safe=[1])
    xs, _ = rs.slsqp(P, seed)
    xs = rs.make_feasible(P, xs, seed)                     # (SLSQP ends a hair outside the safe set on boundary optima)
    fs = ro.bound_grad(xs, ds, b, 0, kind)[0]
    assert sg * v <= sg * fs + 1e-8 * (1.0 + abs(fs)), (v, fs)
    assert rs.kkt_residual(P, x) <= 1e-4


def test_seed_batch_statuses_best_and_determinism(engine):
    ds, b, lo, hi = _fixture("benoit_n20_50x50")
    engine.set_model(ds)
    rng = np.random.default_rng(3)
    pts = oracle.grid_points(lo, hi, [50, 50])
    pm, pv = oracle.gp_inference(pts, ds)
    safe = np.flatnonzero(pm[:, 1] - b * np.sqrt(pv[:, 1]) >= 0)
    seeds = np.concatenate([pts[rng.choice(safe, min(40, safe.size), replace=False)], lo + rng.uniform(size=(24, 2)) * (hi - lo)])
    seeds[5] = [np.nan, 0.0]
    seeds[6] = [np.inf, 0.0]
    seeds[7] = hi + 0.1                                     # outside the box: infeasible, not clipped
    seeds[8] = lo - 0.01
    seeds[9] = seeds[10]                                    # a tie: the lower index is best if it wins
    m, v = oracle.gp_inference(seeds, ds)
    lcb1 = m[:, 1] - b * np.sqrt(v[:, 1])
    inbox = np.all(np.isfinite(seeds), axis=1) & np.all(seeds >= lo, axis=1) & np.all(seeds <= hi, axis=1)
    feasible = inbox & (lcb1 >= 0)
    assert feasible.sum() >= 4 and (~feasible).sum() >= 8
    out = engine.refine(b, seeds, lo=lo, hi=hi)
    st = out["status"]
    assert np.array_equal(st == _lib.SBO_REFINE_INFEASIBLE_SEED, ~feasible)
    bad = ~feasible
    assert np.array_equal(out["x"][bad], seeds[bad], equal_nan=True)
    ok = out["value"][feasible]
    best = int(np.flatnonzero(feasible)[np.argmin(ok)])
    assert out["best"] == best and out["best_value"] == out["value"][best]
    seed_vals = m[:, 0] - b * np.sqrt(v[:, 0])
    assert np.all(out["value"][feasible] <= seed_vals[feasible] + 1e-12 * (1 + np.abs(seed_vals[feasible])))
    again = engine.refine(b, seeds, lo=lo, hi=hi)
    for k in ("x", "value", "status"):
        assert np.array_equal(out[k], again[k], equal_nan=True), k
    assert again["best"] == out["best"] and again["evaluations"] == out["evaluations"]


def test_box_only_and_held_faces(engine):
    ds, b, lo, hi = _fixture("benoit_n20_50x50")
    engine.set_model(ds)
    rng = np.random.default_rng(11)
    seeds = lo + rng.uniform(0.2, 0.8, size=(6, 2)) * (hi - lo)
    out = engine.refine(b, seeds, 0, "mean", constraints=[], lo=lo, hi=hi, max_eval=2000)
    for x in out["x"]:
        assert rs.kkt_residual(rs.problem(ds, b, lo, hi, "mean", safe=[]), x) <= 1e-6
    # a seed on a box face where the function keeps improving outward keeps that coordinate exactly (maximised mean: the faces
    # stay active) -- and no returned point leaves a face whose gradient still points out of the box
    held = 0
    for a in range(2):
        for face, sign in ((lo[a], 1.0), (hi[a], -1.0)):
            for t in np.linspace(0.1, 0.9, 9):
                s = lo + t * (hi - lo)
                s[a] = face
                _, g = ro.bound_grad(s, ds, b, 0, "mean")
                if sign * -g[a] > 0:
                    o = engine.refine(b, s[None, :], 0, "mean", True, constraints=[], lo=lo, hi=hi)
                    x = o["x"][0]
                    _, gx = ro.bound_grad(x, ds, b, 0, "mean")
                    if x[a] == face:
                        held += 1
                    else:
                        assert not (sign * -gx[a] > 1e-9 * (1 + np.abs(gx).max())), (a, face, x, gx)
    assert held > 0


@pytest.mark.parametrize("n,d", [(4, 2), (20, 2), (128, 2), (128, 4), (512, 2), (2048, 4)])
def test_size_range_agrees_with_the_oracle(engine, n, d):
    ds = _synthetic(n, d, n + d)
    engine.set_model(ds)
    lo, hi = -np.ones(d), np.ones(d)
    b = 2.0
    seeds = np.zeros((2, d))
    seeds[1] = 0.1
    out = engine.refine(b, seeds, lo=lo, hi=hi, max_eval=None if n <= 512 else 60)
    moved = (_lib.SBO_REFINE_CONVERGED, _lib.SBO_REFINE_MAX_EVAL)
    m0, v0 = oracle.gp_inference(seeds, ds)
    m, v = oracle.gp_inference(out["x"], ds)
    lcb = m - b * np.sqrt(v)
    seed_ok = m0[:, 1] - b * np.sqrt(v0[:, 1]) >= 0
    assert np.array_equal(out["status"] == _lib.SBO_REFINE_INFEASIBLE_SEED, ~seed_ok)
    for s in range(2):
        if not seed_ok[s]:
            continue
        assert abs(out["value"][s] - lcb[s, 0]) <= 1e-12 * max(1.0, abs(lcb[s, 0]))
        assert lcb[s, 1] >= -1e-12
        # real progress, not the seed handed back by the exact check (the streamed tier from n = 512 on)
        assert out["status"][s] in moved, out["status"][s]
        assert out["value"][s] < m0[s, 0] - b * np.sqrt(v0[s, 0]) - 1e-6
    assert (out["best"] >= 0) == bool(seed_ok.any())
    if n >= 20:
        assert seed_ok.any()


def _both_tiers(engine, *args, **kw):
    """The same refine with M staged in LDS (where it fits) and streamed from L2 (option refine_lds = 0)."""
    a = engine.refine(*args, **kw)
    engine.set_option("refine_lds", 0)
    try:
        b = engine.refine(*args, **kw)
    finally:
        engine.set_option("refine_lds", 1)
    return a, b


@pytest.mark.parametrize("n,d", [(20, 2), (128, 2), (100, 4)])
def test_lds_and_streamed_tiers_give_identical_results(engine, n, d):
    ds = _synthetic(n, d, 7 * n + d)
    engine.set_model(ds)
    seeds = np.array([np.zeros(d), np.full(d, 0.1), np.full(d, -0.2)])
    a, b = _both_tiers(engine, 2.0, seeds, lo=-np.ones(d), hi=np.ones(d))
    for k in ("x", "value", "status"):
        assert np.array_equal(a[k], b[k]), k
    assert a["evaluations"] == b["evaluations"] and a["best"] >= 0
    assert np.all(np.isin(a["status"], (_lib.SBO_REFINE_CONVERGED, _lib.SBO_REFINE_MAX_EVAL)))


@pytest.mark.parametrize("n0", [16, 300])
def test_refine_follows_appended_samples(engine, n0):
    """After appends the factor's leading dimension f_cap and alpha's stride a_ld are no longer n / npad: the refine must read
    both with their strides -- in both tiers -- and land where a refine of the same dataset set afresh lands."""
    d, k = 2, 5
    full = _synthetic(n0 + k, d, 5)
    X = full["X_norm"] * full["X_std"] + full["X_mean"]
    Y = full["Y_norm"] * full["Y_std"] + full["Y_mean"]
    ds0 = synthetic.make_dataset(X[:n0], Y[:n0], full["hypopt"])
    Xn = (X - ds0["X_mean"]) / ds0["X_std"]
    Yn = (Y - ds0["Y_mean"]) / ds0["Y_std"]
    app = dict(ds0, X_norm=Xn, Y_norm=Yn, invKopt=oracle.build_invK(Xn, full["hypopt"]))
    lo, hi = -np.ones(d), np.ones(d)
    seed = np.array([[0.05, -0.1]])
    engine.set_model(app)                                   # the appended dataset set afresh: f_cap = n, a_ld = npad
    fresh = engine.refine(2.0, seed, lo=lo, hi=hi)
    engine.set_model(ds0)
    for i in range(n0, n0 + k):
        engine.append_sample(Xn[i], Yn[i])
    out, streamed = _both_tiers(engine, 2.0, seed, lo=lo, hi=hi)
    for key in ("x", "value", "status"):
        assert np.array_equal(out[key], streamed[key]), key
    m0, v0 = oracle.gp_inference(seed, app)
    assert out["status"][0] in (_lib.SBO_REFINE_CONVERGED, _lib.SBO_REFINE_MAX_EVAL)
    assert out["value"][0] < m0[0, 0] - 2.0 * np.sqrt(v0[0, 0]) - 1e-6
    m, v = oracle.gp_inference(out["x"], app)
    assert abs(out["value"][0] - (m[0, 0] - 2.0 * np.sqrt(v[0, 0]))) <= 1e-10 * max(1.0, abs(m[0, 0]))
    assert np.max(np.abs(out["x"][0] - fresh["x"][0])) <= 1e-5
    assert abs(out["value"][0] - fresh["value"][0]) <= 1e-9 * max(1.0, abs(fresh["value"][0]))


def test_seed_on_the_ball_sphere_is_on_boundary(engine):
    ds, b, lo, hi = _fixture("benoit_n20_50x50")
    engine.set_model(ds)
    # dyadic points: x - x_0 = (1/16, 0) exactly, so ||x - x_0|| == r in floating point
    pts = np.array([[i / 16.0, j / 16.0] for i in range(-9, 24) for j in range(-16, 16)])
    m, v = oracle.gp_inference(pts, ds)
    s = pts[int(np.argmax(m[:, 1] - b * np.sqrt(v[:, 1])))]
    x0 = s + np.array([1.0 / 16.0, 0.0])
    out = engine.refine(b, s[None, :], lo=lo, hi=hi, x_0=x0, r=1.0 / 16.0)
    assert out["status"][0] == _lib.SBO_REFINE_ON_BOUNDARY
    assert np.array_equal(out["x"][0], s) and out["best"] == 0
    inner = engine.refine(b, s[None, :], lo=lo, hi=hi, x_0=x0, r=1.0 / 8.0)
    assert inner["status"][0] in (_lib.SBO_REFINE_CONVERGED, _lib.SBO_REFINE_MAX_EVAL)


def test_refine_does_not_touch_sweeps_masks_or_audit(engine):
    ds, b, lo, hi = _fixture("benoit_n20_50x50")
    engine.set_model(ds)
    engine.set_grid(lo, hi, [50, 50])
    first = engine.sweep_safeopt(b, want_masks=True)
    masks = {k: engine.mask(k) for k in ("S", "U", "M")}
    prof = engine.profile()
    engine.refine(b, np.array([first["minimizer_x"]]), 0, "ucb", lo=lo, hi=hi)
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


def test_errors_change_nothing(engine):
    ds, b, lo, hi = _fixture("benoit_n20_50x50")
    engine.set_model(ds)
    engine.set_grid(lo, hi, [50, 50])
    ref = engine.sweep_safeopt(b, want_masks=True)
    seed = np.array([[1.4, -0.6]])
    bad_kwargs = [dict(objective=2), dict(constraints=[0]), dict(constraints=[2]), dict(x_0=[1.4, -0.6], r=0.0),
                  dict(x_0=[1.4, -0.6], r=np.nan), dict(x_0=[np.nan, -0.6], r=0.1), dict(lo=hi, hi=lo)]
    for kw in bad_kwargs:
        args = dict(lo=lo, hi=hi)
        args.update(kw)
        with pytest.raises(ValueError):
            engine.refine(b, seed, **args)
    lib = _lib.load()
    opts = _lib.RefineOpts()
    opts.b, opts.kind, opts.constraint_mask = b, _lib.SBO_LCB, 2
    for a in range(2):
        opts.lo[a], opts.hi[a] = lo[a], hi[a]
    res = _lib.RefineResult()
    s = np.ascontiguousarray(seed)
    assert lib.sbo_refine(engine._ctx, C.byref(opts), 0, s.ctypes.data_as(C.c_void_p), None, None, None, C.byref(res)) == _lib.SBO_E_INVALID
    opts.kind = 7
    assert lib.sbo_refine(engine._ctx, C.byref(opts), 1, s.ctypes.data_as(C.c_void_p), None, None, None, C.byref(res)) == _lib.SBO_E_INVALID
    assert lib.sbo_refine(engine._ctx, None, 1, s.ctypes.data_as(C.c_void_p), None, None, None, C.byref(res)) == _lib.SBO_E_INVALID
    again = engine.sweep_safeopt(b, want_masks=True, posterior_ready=True)
    assert again["minimizer_index"] == ref["minimizer_index"] and again["count_S"] == ref["count_S"]
    engine.set_model(ds, dtype="f32")
    with pytest.raises(_lib.SafeBOError) as e:
        engine.refine(b, seed, lo=lo, hi=hi)
    assert e.value.code == _lib.SBO_E_UNSUPPORTED
    engine.set_model(ds)


def test_refine_before_a_model_is_no_model():
    import safebo_amd
    with safebo_amd.SweepEngine(0) as eng:
        opts = _lib.RefineOpts()
        res = _lib.RefineResult()
        s = np.zeros(2)
        assert eng._lib.sbo_refine(eng._ctx, C.byref(opts), 1, s.ctypes.data_as(C.c_void_p), None, None, None,
                                   C.byref(res)) == _lib.SBO_E_NO_MODEL


# ---- host classes ---------------------------------------------------------------------------------------------------------
BOUND = np.array([[-.6, 1.5], [-1., 1.]])
TR_PARAMS = {"radius": 0.3, "radius_max": 1, "radius_red": 0.8, "radius_inc": 1.1, "rho_lb": 0.2, "rho_ub": 0.8}


def benoit_f(u, noise=0):
    return u[0] ** 2 + u[1] ** 2 + u[0] * u[1]


def benoit_g(u, noise=0):
    return -(1. - u[0] + u[1] ** 2 + 2. * u[1])


def _init(cls, n=12, grid=(50, 50), **kw):
    if "TR_parameters" in kw:
        m = cls([benoit_f, benoit_g], BOUND, 3.0, kw.pop("TR_parameters"), grid=grid, **kw)
    else:
        m = cls([benoit_f, benoit_g], BOUND, 3.0, grid=grid, **kw)
    X, Y = m.Data_sampling(n, np.array([1.4, -.8]), 0.3)
    m.fixed_hyper = synthetic.default_hypopt(2, 2)
    m.GP_initialization(X, Y, "RBF", multi_hyper=5, var_out=True)
    return m


def test_host_classes_refine_is_feasible_and_no_worse_than_the_grid():
    m = _init(GP_TR.BO, n=20, TR_parameters=dict(TR_PARAMS))
    x_0 = np.array([1.4, -0.8])
    xg, vg = m.minimize_obj_lcb(0.3, x_0)
    assert [np.array_equal(a, b) for a, b in zip(m.minimize_obj_lcb(0.3, x_0, refine=False), (xg, vg))] == [True, True]
    xr, vr = m.minimize_obj_lcb(0.3, x_0, refine=True)
    assert vr <= vg and m.lcb(xr, 1) >= 0 and np.linalg.norm(xr - x_0) <= 0.3 and m.lcb(xr, 0) == vr
    s = _init(SafeOpt.BO, n=12)
    xg, vg = s.minimize_obj_ucb()
    xr, vr = s.minimize_obj_ucb(refine=True)
    assert vr <= vg and s.lcb(xr, 1) >= 0 and s.ucb(xr, 0) == vr
    g = _init(GoOSE.BO, n=12, refine=True)
    xr, vr = g.minimize_obj_lcb()
    xg, vg = g.minimize_obj_lcb(refine=False)
    assert vr <= vg and g.lcb(xr, 1) >= 0


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_host_classes_refine_false_is_bit_identical_to_omitting_it():
    s = _init(SafeOpt.BO, n=12)
    assert _same(s.minimize_obj_ucb(refine=False), s.minimize_obj_ucb())
    g = _init(GoOSE.BO, n=12)
    assert _same(g.minimize_obj_lcb(refine=False), g.minimize_obj_lcb())
    t = _init(GP_TR.BO, n=20, grid=(400, 400), TR_parameters=dict(TR_PARAMS))
    xg, vg = t.minimize_obj_lcb(0.3, np.array([1.4, -0.8]))
    # below the grid spacing (about 0.005) the ball around a grid point holds that point only: refine=False stays there
    x2, v2 = t.minimize_obj_lcb(0.002, xg, refine=False)
    assert np.array_equal(x2, xg) and _same((x2, v2), t.minimize_obj_lcb(0.002, xg))
    xr, vr = t.minimize_obj_lcb(0.002, xg, refine=True)
    assert vr <= v2 and t.lcb(xr, 1) >= 0 and np.linalg.norm(xr - xg) <= 0.002
    m = BayesRTOjax.BayesianOpt([lambda u: benoit_f(u), lambda u: benoit_g(u)], grid=(41, 41))
    m.fixed_hyper = synthetic.default_hypopt(2, 2)
    X, Y = m.Data_sampling(6, np.array([1.1, -0.8]), 0.5)
    m.GP_initialization(X, Y, "RBF", multi_hyper=10, var_out=True)
    store = DataStorage(["plant_temporary"])
    store.data["plant_temporary"].append([1e9, 0.0])
    x_0 = np.array([1.1, -0.8])
    assert _same(m.minimize_acquisition(0.4, x_0, store, b=3.0, refine=False), m.minimize_acquisition(0.4, x_0, store, b=3.0))


def test_gp_tr_campaign_with_refine_keeps_every_step_safe_under_the_model():
    m = _init(GP_TR.BO, n=12, TR_parameters=dict(TR_PARAMS), refine=True)
    x_0, r = np.array([1.4, -0.8]), 0.3
    for _ in range(4):
        x_new, val = m.minimize_obj_lcb(r, x_0)
        assert np.isfinite(val) and m.lcb(x_new, 1) >= 0.0 and np.linalg.norm(x_new - x_0) <= r
        plant_old, plant_new = m.calculate_plant_outputs(x_0), m.calculate_plant_outputs(x_new)
        x_c, r = m.update_TR(x_0, x_new, r, plant_old, plant_new)
        m.add_sample(x_new, plant_new)
        x_0 = np.asarray(x_c, dtype=np.float64)


def test_bayesrto_refine_is_no_worse_than_the_grid():
    m = BayesRTOjax.BayesianOpt([lambda u: benoit_f(u), lambda u: benoit_g(u)], grid=(41, 41), refine=False)
    m.fixed_hyper = synthetic.default_hypopt(2, 2)
    X, Y = m.Data_sampling(6, np.array([1.1, -0.8]), 0.5)
    m.GP_initialization(X, Y, "RBF", multi_hyper=10, var_out=True)
    store = DataStorage(["plant_temporary"])
    store.data["plant_temporary"].append([1e9, 0.0])      # (a stay value every safe point beats)
    x_0 = np.array([1.1, -0.8])
    dg, vg = m.minimize_acquisition(0.4, x_0, store, b=3.0)
    dr, vr = m.minimize_acquisition(0.4, x_0, store, b=3.0, refine=True)
    assert vr <= vg and np.linalg.norm(dr) <= 0.4 and m.constraint(x_0 + dr, 3.0, 1) >= 0.0   # (the point the caller applies)
