"""sbo_refine_sets on the device: SafeOpt's M_t / G_t and GoOSE's target / explore_safeset refined off the
grid -- the exact check of every term, the SLSQP yardstick, degenerate seeds and argument errors, the invariants carried over
from sbo_refine (tiers, determinism, no interference, appended models, sbo_refine's own bits) and the host classes' ``refine``."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
from safebo_amd import GoOSE, SafeOpt, _lib, synthetic

import refine_sets_oracle as rs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
YARDSTICK = ["benoit_n20_50x50", "benoit_n128_64x48", "wo3_n64_48x40"]
MOVED = (_lib.SBO_REFINE_CONVERGED, _lib.SBO_REFINE_MAX_EVAL)
MAX_EVAL = 4000


def _cases(name):
    """[(label, problem, seed z)]: the four steps with the host classes' seeds; on rosen4 (no G_c / O_c on its grid) the pair
    problems take a caller's L that leaves the link a quarter of ucb_1 at the seed, and the distance a caller's target."""
    case = rs.grid_case(name)
    out = [("M", ) + case["M"]] + [(f"G{P['link'][0]}", P, s) for P, s in case["G"]] + [(f"T{P['link'][0]}", P, s) for P, s in case["T"]]
    if "E" in case:
        out.append(("E", ) + case["E"])
    if name == "rosen4_n128_9x8x7x6":
        ds, b, lo, hi, pts, so = (case[k] for k in ("ds", "b", "lo", "hi", "pts", "safeopt"))
        assert not case["G"] and not case["T"]
        g = int(np.argmax(np.where(so["S"], so["var"][:, 0], -np.inf)))
        Uidx = np.nonzero(so["U"])[0]
        h = int(Uidx[np.argmin(oracle.shifted_norm(pts[g][None, :], pts[Uidx]))])
        L = 0.75 * so["ucb"][g, 1] / oracle.shifted_norm(pts[g], pts[h])
        seed = np.concatenate([pts[g], pts[h]])
        out.append(("G1", rs.problem(ds, b, lo, hi, "var", maximize=True, link=(1, L), pair=True), seed))
        out.append(("T1", rs.problem(ds, b, lo, hi, "lcb", at="xp", link=(1, L), pair=True), seed))
        out.append(("E", rs.problem(ds, b, lo, hi, "dist", target=pts[h]), pts[g].copy()))
    return case, out


def _run(engine, P, seeds, **kw):
    seeds = np.atleast_2d(seeds)
    d = P["d"]
    kw.setdefault("max_eval", MAX_EVAL)
    return engine.refine_sets(P["b"], seeds[:, :d], seeds[:, d:] if P["pair"] else None, **rs.engine_args(P), **kw)


def _z(P, out, s=0):
    return np.concatenate([out["x"][s], out["xp"][s]]) if P["pair"] else out["x"][s].copy()


def _exact(engine, P, z):
    """Every term and the reported figure at z from ``engine.bounds`` on the point list (x, x'): ({term: g}, value); g >= 0 is
    the sweeps' closed predicate (lcb_c >= 0, lcb_o <= level, lcb_c(x') <= 0, link >= 0)."""
    d, b = P["d"], P["b"]
    pts = z.reshape(-1, d)
    engine.set_points(pts)
    bnd = {(o, k): engine.bounds(b, o, k) for o in range(engine.q) for k in ("mean", "ucb", "lcb", "var")}
    g = {f"safe{c}": bnd[(c, "lcb")][0] for c in P["safe"]}
    if P["level"] is not None:
        g["level"] = P["level"][1] - bnd[(P["level"][0], "lcb")][0]
    for c in P["unsafe"]:
        g[f"unsafe{c}"] = -bnd[(c, "lcb")][1]
    if P["link"] is not None:
        c, L = P["link"]
        g["link"] = bnd[(c, "ucb")][0] - L * oracle.shifted_norm(pts[0], pts[1])
    lo, hi = rs.box(P)
    g["box"] = 0.0 if (np.all(z >= lo) and np.all(z <= hi)) else -1.0
    if P["kind"] == "dist":
        val = float(np.sqrt(np.sum((pts[0] - P["target"]) ** 2)))
    else:
        val = float(bnd[(P["objective"], P["kind"])][1 if P["at"] == "xp" else 0])
    return g, val


# ---- 1. conditions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", YARDSTICK + ["benoit_n4_40x40", "rosen4_n128_9x8x7x6"])
def test_every_returned_point_meets_every_term_and_is_no_worse_than_its_seed(engine, name):
    case, problems = _cases(name)
    engine.set_model(case["ds"])
    labels = [p[0][0] for p in problems]
    assert all(k in labels for k in "MGTE"), labels
    for label, P, seed in problems:
        out = _run(engine, P, seed)
        z, v, st = _z(P, out), out["value"][0], int(out["status"][0])
        g_seed, v_seed = _exact(engine, P, seed)
        g, v_exact = _exact(engine, P, z)
        print(f"{name} {label}: status {st} evaluations {out['evaluations']} seed {v_seed!r} value {v!r} min slack {min(g.values()):.3g}")
        assert min(g_seed.values()) >= 0.0, (label, g_seed)         # (checked strictly on the CPU for the yardstick fixtures)
        assert st != _lib.SBO_REFINE_INFEASIBLE_SEED, label
        assert all(val >= 0.0 for val in g.values()), (label, g)
        assert abs(v - v_exact) <= 1e-12 * max(1.0, abs(v_exact)), (label, v, v_exact)
        sg = -1.0 if P["maximize"] else 1.0
        assert sg * v <= sg * v_seed, (label, v, v_seed)
        if st in MOVED:
            assert out["best"] == 0 and out["best_value"] == v and np.array_equal(out["best_x"], out["x"][0])
            if P["pair"]:
                assert np.array_equal(out["best_xp"], out["xp"][0])
        else:                                                       # the seed came back: unchanged, with its own value
            assert st in (_lib.SBO_REFINE_NO_PROGRESS, _lib.SBO_REFINE_ON_BOUNDARY), (label, st)
            assert np.array_equal(z, seed) and v == v_seed
        if name in YARDSTICK:
            assert st in MOVED, (label, st)
        assert out["evaluations"] <= MAX_EVAL + 1 and out["evaluations"] % (2 if P["pair"] else 1) == 0


# ---- 2. against the yardstick -----------------------------------------------------------------------------------------------
# Measured on one MI355X, gap = (yardstick - device) / (yardstick - seed) in var_0 and the KKT residual at the device's answer:
#   benoit_n20  M 7.0e-10 / 4.0e-8    G1 8.1e-10 / 9.2e-10
#   benoit_n128 M 5.2e-9 / 7.7e-18    G1 4.6e-9 / 6.1e-17 (MAX_EVAL at 4000 evaluations)
#   wo3_n64     M -2.1e-7 / 1.1e-16   G1 -3.2e-7 / 3.0e-18   G2 -3.8e-7 / 1.5e-18   (negative: the device is ahead of the yardstick)
# The thresholds are twice the largest figure, rounded up to one digit.  The allowance is for the barrier floor (mu = 1e-11,
# tol 1e-9) and SLSQP's ftol stopping at different points.
GAP_MAX = 2e-8
KKT_MAX = 8e-8


@pytest.mark.parametrize("name", YARDSTICK)
def test_m_t_and_g_t_close_the_gap_to_the_slsqp_yardstick(engine, name):
    case, problems = _cases(name)
    engine.set_model(case["ds"])
    for label, P, seed in problems:
        if label[0] not in "MG":
            continue
        v_seed, v_yard, _ = rs.yardstick(P, seed)
        out = _run(engine, P, seed)
        v = out["value"][0]
        gap = (v_yard - v) / (v_yard - v_seed)
        kkt = rs.kkt_residual(P, _z(P, out))
        print(f"{name} {label}: seed std {np.sqrt(v_seed):.6f} device std {np.sqrt(v):.6f} yardstick std {np.sqrt(v_yard):.6f} "
              f"gap {gap:.3e} kkt {kkt:.3e} status {out['status'][0]} evaluations {out['evaluations']}")
        assert v > v_seed, (label, v, v_seed)
        assert gap <= GAP_MAX, (label, gap)
        assert kkt <= KKT_MAX, (label, kkt)


# ---- 3. degenerate seeds and errors -------------------------------------------------------------------------------------------
def test_degenerate_seeds_come_back_unchanged_with_their_status(engine):
    case, problems = _cases("benoit_n128_64x48")
    engine.set_model(case["ds"])
    by = {label[0]: (P, seed) for label, P, seed in problems}
    # the link violated: a hundred times the sweep's L
    P, seed = by["G"]
    bad = dict(P, link=(P["link"][0], 100.0 * P["link"][1]))
    assert _exact(engine, bad, seed)[0]["link"] < 0.0
    out = _run(engine, bad, seed)
    assert out["status"][0] == _lib.SBO_REFINE_INFEASIBLE_SEED and np.array_equal(_z(bad, out), seed) and out["best"] == -1
    # x' inside S
    inside = np.concatenate([seed[:2], seed[:2]])
    out = _run(engine, P, inside)
    assert out["status"][0] == _lib.SBO_REFINE_INFEASIBLE_SEED and np.array_equal(_z(P, out), inside)
    # the level violated, and met exactly
    P, seed = by["M"]
    engine.set_points(seed[None, :])
    lcb0 = float(engine.bounds(P["b"], 0, "lcb")[0])
    out = _run(engine, dict(P, level=(0, lcb0 - 0.1)), seed)
    assert out["status"][0] == _lib.SBO_REFINE_INFEASIBLE_SEED and np.array_equal(out["x"][0], seed)
    out = _run(engine, dict(P, level=(0, lcb0)), seed)
    assert out["status"][0] == _lib.SBO_REFINE_ON_BOUNDARY and np.array_equal(out["x"][0], seed) and out["best"] == 0
    # a batch keeps the usable seed apart from the unusable ones
    out = _run(engine, P, np.stack([seed, case["hi"] + 1.0, seed]))
    assert list(out["status"][[1]]) == [_lib.SBO_REFINE_INFEASIBLE_SEED] and out["best"] == 0
    assert np.array_equal(out["x"][0], out["x"][2]) and out["value"][0] == out["value"][2]


def _synthetic(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, size=(n, d))
    Y = np.stack([np.sum(X ** 2, axis=1) + 0.3 * np.sin(3 * X[:, 0]), 0.8 - np.sum(np.abs(X), axis=1) / d], axis=1)
    return synthetic.make_dataset(X, Y, synthetic.default_hypopt(d, 2))


def _sweep_state(engine, b, **kw):
    res = engine.sweep_safeopt(b, want_masks=True, **kw)
    return res, {k: engine.mask(k) for k in ("S", "U", "M")}, engine.mask("G", 1)


def test_errors_change_nothing(engine):
    case, problems = _cases("benoit_n20_50x50")
    ds, b, lo, hi = (case[k] for k in ("ds", "b", "lo", "hi"))
    engine.set_model(ds)
    engine.set_grid(lo, hi, [50, 50])
    ref, masks, G = _sweep_state(engine, b)
    P, seed = next((P, s) for label, P, s in problems if label[0] == "G")
    x, xp = seed[None, :2], seed[None, 2:]
    base = dict(rs.engine_args(P))
    bad = [dict(safe=[0]), dict(unsafe=[2]), dict(link=(0, 1.0)), dict(link=(1, -1.0)), dict(link=(1, np.nan)), dict(level=(2, 0.0)),
           dict(level=(0, np.inf)), dict(objective=2), dict(lo=hi, hi=lo), dict(x_0=[1.4, -0.6], r=0.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            engine.refine_sets(b, x, xp, **dict(base, **kw))
    single = dict(base, link=None, unsafe=[])
    for kw in (dict(link=(1, 1.0)), dict(unsafe=[1]), dict(at="xp")):           # terms on x' without a pair
        with pytest.raises(ValueError):
            engine.refine_sets(b, x, None, **dict(single, **kw))
    with pytest.raises(ValueError):                                             # the distance is minimised only
        engine.refine_sets(b, x, None, **dict(single, kind="dist", target=[0.0, 0.0], maximize=True))
    lib = _lib.load()
    opts, res = _lib.RefineSetsOpts(), _lib.RefineSetsResult()
    opts.b, opts.kind, opts.pair = b, _lib.SBO_LCB, 1
    for a in range(2):
        opts.lo[a], opts.hi[a] = lo[a], hi[a]
    sp = np.ascontiguousarray(x).ctypes.data_as(C.c_void_p)
    assert lib.sbo_refine_sets(engine._ctx, C.byref(opts), 1, sp, None, None, None, None, None, C.byref(res)) == _lib.SBO_E_INVALID   # no seeds_p
    assert lib.sbo_refine_sets(engine._ctx, C.byref(opts), 0, sp, sp, None, None, None, None, C.byref(res)) == _lib.SBO_E_INVALID
    opts.kind = 7
    assert lib.sbo_refine_sets(engine._ctx, C.byref(opts), 1, sp, sp, None, None, None, None, C.byref(res)) == _lib.SBO_E_INVALID
    again, masks2, G2 = _sweep_state(engine, b, posterior_ready=True)
    for k in ("minimizer_index", "expander_index", "count_S", "count_U", "count_M", "u_star", "minimizer_std", "expander_std"):
        assert again[k] == ref[k], k
    assert all(np.array_equal(masks[k], masks2[k]) for k in masks) and np.array_equal(G, G2)
    # fp32 models are not served
    engine.set_model(ds, dtype="f32")
    with pytest.raises(_lib.SafeBOError) as e:
        engine.refine_sets(b, x, xp, **base)
    assert e.value.code == _lib.SBO_E_UNSUPPORTED
    # pair mode ends at d = 4: 2 d = 10 variables do not fit the solver's state
    engine.set_model(_synthetic(20, 5, 3))
    with pytest.raises(_lib.SafeBOError) as e:
        engine.refine_sets(2.0, np.zeros((1, 5)), np.full((1, 5), 0.9), objective=0, kind="var", maximize=True, link=(1, 0.01),
                           lo=-np.ones(5), hi=np.ones(5))
    assert e.value.code == _lib.SBO_E_UNSUPPORTED and "d <= 4" in str(e.value)
    one = engine.refine_sets(2.0, np.zeros((1, 5)), objective=0, kind="var", maximize=True, safe=[], lo=-np.ones(5), hi=np.ones(5))
    assert one["status"][0] in MOVED                                            # (single mode is served at d = 5)
    engine.set_model(ds)
    engine.set_grid(lo, hi, [50, 50])
    fresh, masks3, G3 = _sweep_state(engine, b)
    assert fresh["minimizer_index"] == ref["minimizer_index"] and fresh["count_S"] == ref["count_S"] and fresh["u_star"] == ref["u_star"]
    assert all(np.array_equal(masks[k], masks3[k]) for k in masks) and np.array_equal(G, G3)


def test_refine_sets_before_a_model_is_no_model():
    import safebo_amd
    with safebo_amd.SweepEngine(0) as eng:
        opts, res = _lib.RefineSetsOpts(), _lib.RefineSetsResult()
        s = np.zeros(2)
        assert eng._lib.sbo_refine_sets(eng._ctx, C.byref(opts), 1, s.ctypes.data_as(C.c_void_p), None, None, None, None, None,
                                        C.byref(res)) == _lib.SBO_E_NO_MODEL


# ---- 4. invariants ----------------------------------------------------------------------------------------------------------
KEYS = ("x", "xp", "value", "status")


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS if k in a) and a["evaluations"] == b["evaluations"] and a["best"] == b["best"]


@pytest.mark.parametrize("name", ["benoit_n20_50x50", "benoit_n128_64x48", "wo3_n64_48x40", "rosen4_n128_9x8x7x6"])
def test_tiers_and_repeated_calls_give_identical_bits(engine, name):
    """n = 128 with two outputs fits the LDS tier in both modes (2 x 66 KiB of triangles + 4 KiB of vectors); wo3 has three."""
    case, problems = _cases(name)
    engine.set_model(case["ds"])
    for label, P, seed in problems:
        a = _run(engine, P, seed)
        again = _run(engine, P, seed)
        engine.set_option("refine_lds", 0)
        try:
            streamed = _run(engine, P, seed)
        finally:
            engine.set_option("refine_lds", 1)
        assert _same(a, again), label
        assert _same(a, streamed), label


def test_a_call_between_two_sweeps_leaves_masks_results_and_audit_alone(engine):
    case, problems = _cases("wo3_n64_48x40")
    ds, b, lo, hi = (case[k] for k in ("ds", "b", "lo", "hi"))
    engine.set_model(ds)
    engine.set_grid(lo, hi, [48, 40])
    first, masks, G = _sweep_state(engine, b)
    prof = engine.profile()
    for label, P, seed in problems:
        d = P["d"]
        engine.refine_sets(b, seed[None, :d], seed[None, d:] if P["pair"] else None, **rs.engine_args(P))
    after = engine.profile()
    for k in ("guard_audit_samples", "guard_audit_violations", "guard_audit_skipped"):
        assert after[k] == prof[k], k
    again, masks2, G2 = _sweep_state(engine, b, posterior_ready=True)
    for k in ("minimizer_index", "expander_index", "count_S", "count_U", "count_M", "u_star", "minimizer_std", "expander_std"):
        assert again[k] == first[k], k
    assert np.array_equal(again["count_G"], first["count_G"]) and np.array_equal(again["expander_index_c"], first["expander_index_c"])
    assert all(np.array_equal(masks[k], masks2[k]) for k in masks) and np.array_equal(G, G2)


def appended_pair_problem(n0):
    """test_refine_sets_follows_appended_samples' inputs: the first n0 rows as a dataset, the whole (n0 + 5 rows in its
    normalisation), those rows normalised, the pair problem on the whole, its seed and the posterior variance at the seed."""
    d, k, b = 2, 5, 2.0
    full = _synthetic(n0 + k, d, 5)
    X = full["X_norm"] * full["X_std"] + full["X_mean"]
    Y = full["Y_norm"] * full["Y_std"] + full["Y_mean"]
    ds0 = synthetic.make_dataset(X[:n0], Y[:n0], full["hypopt"])
    Xn = (X - ds0["X_mean"]) / ds0["X_std"]
    Yn = (Y - ds0["Y_mean"]) / ds0["Y_std"]
    app = dict(ds0, X_norm=Xn, Y_norm=Yn, invKopt=oracle.build_invK(Xn, full["hypopt"]))
    lo, hi = -np.ones(d), np.ones(d)
    x, xp = np.array([0.05, -0.1]), np.array([0.95, 0.9])
    m, v = oracle.gp_inference(np.stack([x, xp]), app)
    assert m[0, 1] - b * np.sqrt(v[0, 1]) > 0 and m[1, 1] - b * np.sqrt(v[1, 1]) < 0
    L = 0.5 * (m[0, 1] + b * np.sqrt(v[0, 1])) / oracle.shifted_norm(x, xp)
    P = rs.problem(app, b, lo, hi, "var", maximize=True, link=(1, L), pair=True)
    return ds0, app, Xn, Yn, P, np.concatenate([x, xp]), v


@pytest.mark.parametrize("n0", [16, 300])
def test_refine_sets_follows_appended_samples(engine, n0):
    """test_refine_follows_appended_samples for a pair: f_cap / a_ld strides in both tiers, against the same dataset set afresh."""
    ds0, app, Xn, Yn, P, seed, v = appended_pair_problem(n0)
    k = len(Xn) - n0
    engine.set_model(app)
    fresh = _run(engine, P, seed)
    engine.set_model(ds0)
    for i in range(n0, n0 + k):
        engine.append_sample(Xn[i], Yn[i])
    out = _run(engine, P, seed)
    engine.set_option("refine_lds", 0)
    try:
        streamed = _run(engine, P, seed)
    finally:
        engine.set_option("refine_lds", 1)
    assert _same(out, streamed)
    assert out["status"][0] in MOVED and out["value"][0] > v[0, 0] + 1e-6
    assert rs.feasible(P, _z(P, out))[1] >= -1e-9
    assert abs(out["value"][0] - rs.value(P, _z(P, out))) <= 1e-10 * max(1.0, abs(out["value"][0]))
    print(f"n0 {n0}: |dz| {np.max(np.abs(_z(P, out) - _z(P, fresh))):.3e} dv {abs(out['value'][0] - fresh['value'][0]):.3e}")
    assert np.max(np.abs(_z(P, out) - _z(P, fresh))) <= 1e-5
    assert abs(out["value"][0] - fresh["value"][0]) <= 1e-9 * max(1.0, abs(fresh["value"][0]))


@pytest.mark.parametrize("n,d", [(4, 2), (20, 2), (128, 2), (128, 4), (512, 2), (2048, 4)])
def test_sbo_refine_returns_the_bits_it_returned_before(engine, n, d):
    """The cases of test_size_range_agrees_with_the_oracle against tests/golden/refine/bits_before_sets.npz: what sbo_refine
    returned on an MI355X before its internals were generalised for sbo_refine_sets."""
    z = np.load(os.path.join(GOLDEN, "refine", "bits_before_sets.npz"))
    engine.set_model(_synthetic(n, d, n + d))
    seeds = np.zeros((2, d))
    seeds[1] = 0.1
    out = engine.refine(2.0, seeds, lo=-np.ones(d), hi=np.ones(d), max_eval=None if n <= 512 else 60)
    tag = f"n{n}_d{d}_"
    for k in ("x", "value", "status"):
        assert np.array_equal(out[k], z[tag + k]), k
    assert out["evaluations"] == int(z[tag + "evaluations"]) and out["best"] == int(z[tag + "best"])
    assert np.array_equal(out["best_value"], z[tag + "best_value"], equal_nan=True) and out["converged"] == int(z[tag + "converged"])
    assert np.array_equal(out["best_x"], z[tag + "best_x"])


# ---- 5. host classes ----------------------------------------------------------------------------------------------------------
BOUND = np.array([[-.6, 1.5], [-1., 1.]])


def benoit_f(u, noise=0):
    return u[0] ** 2 + u[1] ** 2 + u[0] * u[1]


def benoit_g(u, noise=0):
    return -(1. - u[0] + u[1] ** 2 + 2. * u[1])


def _init(cls, n=12, grid=(50, 50), **kw):
    m = cls([benoit_f, benoit_g], BOUND, 3.0, grid=grid, **kw)
    X, Y = m.Data_sampling(n, np.array([1.4, -.8]), 0.3)
    m.fixed_hyper = synthetic.default_hypopt(2, 2)
    m.GP_initialization(X, Y, "RBF", multi_hyper=5, var_out=True)
    return m


def _init_fixture(cls, name="benoit_n20_50x50", **kw):
    """The host class on a committed fixture's data and hyper-parameters: S, G_1 and O_1 are non-empty on its 50 x 50 grid."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    m = cls([benoit_f, benoit_g], z["bound"], float(z["b"]), grid=tuple(rs.GRIDS[name]), **kw)
    m.fixed_hyper = z["hypopt"]
    m.GP_initialization(z["X"], z["Y"], "RBF", multi_hyper=5, var_out=True)
    return m


def _pair_same(a, b):
    return np.array_equal(np.asarray(a[0]), np.asarray(b[0]), equal_nan=True) and a[1] == b[1]


def test_host_classes_refine_false_is_bit_identical_to_omitting_it():
    s = _init_fixture(SafeOpt.BO)
    assert _pair_same(s.Minimizer(refine=False), s.Minimizer()) and _pair_same(s.Expander(refine=False), s.Expander())
    grid = s.sweep()
    assert _pair_same(s.Minimizer(), (grid["minimizer_x"], grid["minimizer_std"]))
    assert _pair_same(s.Expander(), (grid["expander_x"], grid["expander_std"]))
    s.Minimizer(refine=True)
    s.Expander(refine=True)                                   # (a refine changes no later grid answer)
    assert _pair_same(s.Minimizer(), (grid["minimizer_x"], grid["minimizer_std"]))
    assert _pair_same(s.Expander(), (grid["expander_x"], grid["expander_std"]))
    g = _init_fixture(GoOSE.BO)
    t = g.Target()
    assert np.all(np.isfinite(t[0])) and _pair_same(g.Target(refine=False), t)
    assert np.array_equal(g.explore_safeset(t[0], refine=False), g.explore_safeset(t[0]))
    other = np.array([0.2, 0.3])
    assert np.array_equal(g.explore_safeset(other, refine=False), g.explore_safeset(other))
    g.Target(refine=True)
    g.explore_safeset(t[0], refine=True)
    assert _pair_same(g.Target(), t)
    empty = _init(GoOSE.BO)                                   # no optimistic point on this model's grid: nothing to refine
    assert np.isinf(empty.Target(refine=True)[1]) and np.isinf(empty.Target()[1])


def test_safeopt_refined_minimizer_and_expander_meet_their_definitions():
    s = _init_fixture(SafeOpt.BO)
    grid = dict(s.sweep())
    assert grid["expander_index"] >= 0
    x, std = s.Minimizer(refine=True)
    _, u_star = s.minimize_obj_ucb(refine=True)
    assert s.lcb(x, 1) >= 0.0 and s.lcb(x, 0) <= u_star
    assert std >= grid["minimizer_std"] or u_star < grid["u_star"]         # (a lower level can only shrink M_t)
    sd = (s.ucb(x, 0) - s.lcb(x, 0)) / (2.0 * s.b)
    assert abs(std - sd) <= 1e-9 * max(1.0, sd), (std, sd)
    x, std = s.Expander(refine=True)
    assert s.lcb(x, 1) >= 0.0 and std >= grid["expander_std"]
    sd = (s.ucb(x, 0) - s.lcb(x, 0)) / (2.0 * s.b)
    assert abs(std - sd) <= 1e-9 * max(1.0, sd), (std, sd)
    if s.expander_witness is None:                            # (the grid value was kept: the grid point itself)
        assert std == grid["expander_std"] and np.array_equal(x, grid["expander_x"])
    else:
        xp, c, L = s.expander_witness
        assert s.lcb_constraint_min(xp) <= 0.0
        assert s.Lipschitz_continuity_constraint(np.concatenate([x, xp]), c, L) >= 0.0
        assert L == s.maximize_infnorm_mean_grad(s.n_fun - 1)


def test_goose_refined_target_and_explore_meet_their_definitions():
    g = _init_fixture(GoOSE.BO)
    tx, tl = g.Target()
    assert np.all(np.isfinite(tx))
    ex = g.explore_safeset(tx)
    x, lcb = g.Target(refine=True)
    assert lcb <= tl
    found = []
    for target in (tx, x, np.array([0.2, 0.3])):              # (the bound calls below replace the resident grid: explore first)
        found.append((target, g.explore_safeset(target, refine=False), g.explore_safeset(target, refine=True)))
    assert np.array_equal(g.explore_safeset(tx), ex)
    assert g.lcb_constraint_min(x) <= 0.0
    assert abs(lcb - g.lcb(x, 0)) <= 1e-12 * max(1.0, abs(lcb))
    if g.target_witness is not None:
        xs, c, L = g.target_witness
        assert g.lcb(xs, 1) >= 0.0 and g.Lipschitz_continuity_constraint(np.concatenate([xs, x]), c, L) >= 0.0
    for target, near_grid, near in found:
        assert g.lcb(near, 1) >= 0.0
        assert np.linalg.norm(near - target) <= np.linalg.norm(near_grid - target)


def test_safeopt_campaign_with_refine_keeps_every_step_safe_under_the_model():
    m = _init_fixture(SafeOpt.BO, refine=True)
    for _ in range(4):
        x_min, std_min = m.Minimizer()
        x_exp, std_exp = m.Expander()
        x = np.asarray(x_min if std_min > std_exp else x_exp, dtype=np.float64)      # test/test_SafeOpt.py:153-158
        assert np.all(x >= BOUND[:, 0]) and np.all(x <= BOUND[:, 1])
        assert m.lcb(x, 1) >= 0.0
        m.add_sample(x, m.calculate_plant_outputs(x))
