"""History independence of a SweepEngine: whatever the context did before, a sweep returns what a fresh context returns for the same
model, candidates and options.  Seeded walks (tests/history_walk.py) check every step against NumPy references; directed sequences
cover what walks rarely reach -- K1t plans decided by a lean sweep, a lean K1i sweep outside the column path, one K1t box shared by two
models, a column-path sweep that skipped tiles, and back-to-back sweeps under the standing audit.  On K1t-sized grids the reference is
a second, fresh context on the exact kernel (K1g)."""
import numpy as np
import pytest

import history_cases as hc
import history_walk as hw
import model_append_batch as mb
import model_remove as mr
import oracle
import skip_safe_cases as cases
from safebo_amd import synthetic

pytestmark = pytest.mark.gpu

KERNELS = {}          # seed -> [(step, kind, posterior_kernel, set_path)] of the walks run so far
APPENDS = {}          # seed -> posterior kernels resident at each append
REMOVES, BLOCKS = {}, {}      # ... at each removal, at each block append
ROBUST_REFUSALS = {}          # seed -> model-changing steps behind which robust_arrays() was asserted refused
CALLS, DIRECT, DEVS = {}, {}, {}      # seed -> the new calls as run, {read-only call: change labels directly in front}, largest deviations
DIRECT_ROBUST = {}            # seed -> direct read-only calls around which robust_arrays() was asserted refused


@pytest.fixture(scope="module")
def fresh():
    """A second context for the reference on grids NumPy cannot afford: exact kernel (tensor_cheb 0: K1g), every sweep audited."""
    import safebo_amd
    eng = safebo_amd.SweepEngine(0)
    eng.set_option("tensor_cheb", 0)
    eng.set_option("guard_audit_every", 1)
    yield eng
    eng.synchronize()
    prof = eng.profile()
    eng.close()
    assert prof["guard_audit_violations"] == 0, prof["guard_audit_violations"]


def _run_walk(engine, seed):
    w = hw.Walk(engine, seed, hw.make_walk(seed))
    try:
        KERNELS[seed] = w.run()
        APPENDS[seed], REMOVES[seed], BLOCKS[seed] = w.append_kernels, w.remove_kernels, w.block_kernels
        ROBUST_REFUSALS[seed] = w.robust_refusals
        CALLS[seed], DIRECT[seed], DEVS[seed], DIRECT_ROBUST[seed] = w.calls, w.direct, w.devs, w.direct_robust
        if w.devs:
            print("seed", seed, "largest deviation per new step kind:", w.devs)
    finally:
        for k, v in hw.DEFAULTS.items():
            engine.set_option(k, v)


@pytest.mark.parametrize("seed", hw.SEEDS)
def test_history_walk(engine, seed):
    _run_walk(engine, seed)


def test_history_walks_took_every_kernel_path(engine):
    """Over all walks, every posterior kernel a 2-D problem or a list can take ran and was checked -- generic (1 / 2), K1g (3), K1b (4),
    K1i (6) --, both set paths (byte masks, column words), and an append, a removal and a block append each found each of K1i, K1b and
    K1g resident; a removal, a block append and a fit each stood directly behind a robust sweep, whose arrays were then refused.
    expander_gain and sample_paths each ran with each of K1i, K1b and K1g resident, on a list, on an fp32 model, and directly behind
    each model-changing step (where mask("S") was refused before the call and after it); each of the ten read-only calls ran directly
    behind some model change, each of the four dtype-free ones directly behind an fp32 update."""
    for seed in hw.SEEDS:
        if seed not in KERNELS:
            _run_walk(engine, seed)
    sweeps = [r for rec in KERNELS.values() for r in rec if r[1] in hw.SWEEPS]
    kernels = {r[2] for r in sweeps}
    paths = {r[3] for r in sweeps if r[1] == "safeopt"}
    assert kernels & {1, 2} and {3, 4, 6} <= kernels, sorted(kernels)
    assert paths == {0, 1}, paths
    assert {3, 4, 6} <= set().union(*APPENDS.values()), APPENDS
    assert {3, 4, 6} <= set().union(*REMOVES.values()) and {3, 4, 6} <= set().union(*BLOCKS.values()), (REMOVES, BLOCKS)
    assert sum(ROBUST_REFUSALS.values()) >= 3 and all(ROBUST_REFUSALS[seed] >= 1 for seed in (9, 12, 15)), ROBUST_REFUSALS
    calls = [c for rec in CALLS.values() for c in rec]
    direct = {k: set().union(*(d.get(k, set()) for d in DIRECT.values())) for k in hw.READ_ONLY3}
    for kind in hw.NEW_CALLS:
        mine = [c for c in calls if c["kind"] == kind]
        resident = {c["kernel"] for c in mine if c["direct"] is None and not c["on_list"] and c["dtype"] == "f64"}
        assert {3, 4, 6} <= resident, (kind, sorted(resident))
        assert any(c["on_list"] for c in mine) and any(c["dtype"] == "f32" for c in mine), kind
        assert set(hw.CHANGES) <= direct[kind], (kind, sorted(direct[kind]))
    assert all(direct[k] for k in hw.READ_ONLY3), direct
    assert all({d for d in direct[k] if d.startswith("f32:")} for k in hw.F32_READS), direct
    assert sum(DIRECT_ROBUST.values()) >= 2, DIRECT_ROBUST
    print("largest deviation per new step kind over all walks:", {k: max(d.get(k, 0.0) for d in DEVS.values()) for k in hw.NEW_CALLS})


# ---- directed sequences ----------------------------------------------------------------------------------------------------------
def _tensor_ds(d, seed=3, log_ell=-0.5):
    rng = np.random.default_rng(seed)
    n = 96
    X = rng.uniform(-2.0, 2.0, size=(n, d))
    Y = np.stack([np.sum(X ** 2, axis=1) + np.sin(2.0 * X[:, 0]), 3.0 - 0.5 * np.sum(X ** 2, axis=1) + X[:, 1]], axis=1)
    return synthetic.make_dataset(X, Y, synthetic.default_hypopt(d, 2, log_ell=log_ell))


def _fresh_ref(fresh, lo, hi, count, ds, kind, b):
    """One full sweep of a fresh model on the reference context: (result, masks)."""
    fresh.set_grid(lo, hi, count)
    fresh.set_model(ds)
    if kind == "safeopt":
        res = fresh.sweep_safeopt(b, want_masks=True)
        return res, {"S": fresh.mask("S"), "U": fresh.mask("U"), "M": fresh.mask("M"), "G": fresh.mask("G", 1)}
    res = fresh.sweep_goose(b, want_masks=True)
    return res, {"S": fresh.mask("S"), "U": fresh.mask("U"), "O": fresh.mask("O", 1)}


def _masks(eng, kind):
    if kind == "safeopt":
        return {"S": eng.mask("S"), "U": eng.mask("U"), "M": eng.mask("M"), "G": eng.mask("G", 1)}
    return {"S": eng.mask("S"), "U": eng.mask("U"), "O": eng.mask("O", 1)}


def _same_as_fresh(eng, kind, res, ref, ys, label):
    """Decisions identical to the fresh context's; L within the relative band the plan claims for its Lipschitz keys (guard_rl)."""
    rres, rmasks = ref
    masks = _masks(eng, kind)
    for k in rmasks:
        assert np.array_equal(masks[k], rmasks[k]), (label, k)
    if kind == "safeopt":
        keys = ("minimizer_index", "expander_index", "count_S", "count_U", "count_M", "choose_minimizer")
        assert abs(res["u_star"] - rres["u_star"]) < 1e-9 * ys, (label, res["u_star"], rres["u_star"])
    else:
        keys = ("safe_min_index", "target_index", "explore_index", "count_S", "count_U", "choose_safe_min")
    for k in keys:
        assert res[k] == rres[k], (label, k, res[k], rres[k])
    rl = np.array(eng.profile()["guard_rl"][:2])
    for o in range(2):
        assert abs(res["L"][o] - rres["L"][o]) <= max(1e-9, rl[o]) * rres["L"][o], (label, o, res["L"], rres["L"], rl)


@pytest.mark.parametrize("d,count", [(3, [160, 168, 160]), (4, [64, 64, 64, 64])])
def test_k1t_lean_sweep_then_full_reuse_reports_the_objectives_key(engine, fresh, d, count):
    """K1t, a plan decided by a lean sweep: a following full SafeOpt and GoOSE sweep on posterior_ready must report L[0] (the lean
    launch left it out), and the full sweep's band on L[0] (guard_rl) must be measured, as on a plan a full sweep decided."""
    ds, b = _tensor_ds(d), 2.0
    lo, hi = np.full(d, -2.0), np.full(d, 2.0)
    ys = max(1.0, float(np.max(ds["Y_std"])))
    ref_s = _fresh_ref(fresh, lo, hi, count, ds, "safeopt", b)
    ref_g = _fresh_ref(fresh, lo, hi, count, ds, "goose", b)
    assert fresh.profile()["posterior_kernel"] == 3
    engine.set_grid(lo, hi, count)
    # the plan decided by a full sweep: its band on L[0].  (Twice: a first plan that needed its second attempt starts the next model
    # on this box one step up the ladder -- the second decision is the one the lean-decided plan below repeats)
    for _ in range(2):
        engine.set_model(ds)
        res = engine.sweep_safeopt(b, want_masks=True)
    assert engine.profile()["posterior_kernel"] == 5
    _same_as_fresh(engine, "safeopt", res, ref_s, ys, "full first")
    rl_full = engine.profile()["guard_rl"][0]
    assert rl_full > 1e-13
    # the same model again (a new plan), decided by a lean sweep
    engine.set_model(ds)
    lean = engine.sweep_safeopt(b, want_masks=True, lean=1)
    assert engine.profile()["posterior_kernel"] == 5 and lean["L"][0] == 0.0
    res = engine.sweep_safeopt(b, want_masks=True, posterior_ready=True)
    assert res["L"][0] > 0.0, ("a full sweep behind a lean one reports the objective's key", res["L"])
    _same_as_fresh(engine, "safeopt", res, ref_s, ys, "lean, then full on posterior_ready")
    # (the measured part of the band -- 16 x the probes' largest gradient deviation / L -- sits at the rounding level and moves a little
    # from one decision to the next; a plan that never probed output 0 reports the bare 1e-13 floor)
    rl_lean = engine.profile()["guard_rl"][0]
    assert rl_lean > 1e-13 and 0.25 < (rl_lean - 1e-13) / (rl_full - 1e-13) < 4.0, (rl_lean, rl_full)
    engine.sweep_safeopt(b, want_masks=True, lean=1)
    res = engine.sweep_goose(b, want_masks=True, posterior_ready=True)
    assert res["L"][0] > 0.0, ("GoOSE behind a lean sweep reports the objective's key", res["L"])
    _same_as_fresh(engine, "goose", res, ref_g, ys, "lean, then GoOSE on posterior_ready")


def test_k1t_box_shared_by_two_models_back_and_forth(engine, fresh):
    """One K1t box, two models in turn (the second needs finer nodes: the per-box ladder bump carries over): every sweep is the fresh
    context's."""
    d, count, b = 3, [160, 168, 160], 2.0
    lo, hi = np.full(d, -2.0), np.full(d, 2.0)
    models = (_tensor_ds(d, 3, -0.5), _tensor_ds(d, 4, -0.8))
    refs = [_fresh_ref(fresh, lo, hi, count, ds, "safeopt", b) for ds in models]
    engine.set_grid(lo, hi, count)
    for i in (0, 1, 0, 1):
        ds = models[i]
        engine.set_model(ds)
        lean = 1 if i == 1 else 0
        res = engine.sweep_safeopt(b, want_masks=True, lean=lean)
        assert engine.profile()["posterior_kernel"] == 5
        if lean:
            res = engine.sweep_safeopt(b, want_masks=True, posterior_ready=True)
        _same_as_fresh(engine, "safeopt", res, refs[i], max(1.0, float(np.max(ds["Y_std"]))), f"model {i}")


def _walk(engine, problem, steps):
    w = hw.Walk(engine, -1, [], problem=problem)
    return w, lambda *more: (w.steps.extend(more), w.run(len(w.steps) - len(more)))


def test_k1i_lean_sweep_outside_the_column_path_then_full_reuse(engine):
    """Config C (q = 3: no column path): the model's first sweep -- K1i -- is lean, the next full sweep on posterior_ready must report
    the oracle's L[0]; so must GoOSE."""
    w, do = _walk(engine, "C", [])
    b = 2.0
    do(("set_grid", "t256x128"), ("set_model", "C", "f64"), ("safeopt", b, 1, False, True))
    assert engine.profile()["posterior_kernel"] == 6
    do(("safeopt", b, 0, True, True))
    do(("safeopt", b, 1, False, True), ("goose", b, True), ("posterior",))


def test_column_path_lean2_skip_then_refusal_then_reuse(engine):
    """A column-path lean-2 sweep that skipped constraint tiles, a refused sweep (b = NaN), then SafeOpt / GoOSE / TR / robust sweeps on
    posterior_ready and the posterior: all the oracle's."""
    engine.set_option("fuse_classify", 1)
    engine.set_option("col_path", 2)
    try:
        w, do = _walk(engine, "H", [])
        b = 3.0
        do(("set_grid", "t256x128"), ("set_model", "H", "f64"), ("safeopt", b, 0, False, True), ("safeopt", b, 0, False, True))
        assert engine.profile()["posterior_kernel"] == 4
        do(("safeopt", b, 2, False, True))
        prof = engine.profile()
        assert prof["set_path"] == 1 and prof["k1_tiles_skipped"] > 0, prof["k1_tiles_skipped"]
        do(("refuse", "b_nan"), ("safeopt", b, 0, True, True), ("goose", b, True), ("tr", b, 0.5, True), ("robust", b, "ucb", True),
           ("posterior",))
    finally:
        engine.set_option("fuse_classify", -1)
        engine.set_option("col_path", 1)


def test_back_to_back_sweeps_under_the_standing_audit(engine):
    """K1i -> K1b (the plan is built: the band is rewritten) -> K1b with every sweep audited and no host work between the sweeps: the
    audit of one sweep must compare against that sweep's band, not the next plan's.  Results are the oracle's afterwards."""
    cfg = synthetic.make_config("B", n=64)
    lo, hi, count = cfg["bound"][:, 0], cfg["bound"][:, 1], [256, 128]
    pts = oracle.grid_points(lo, hi, count)
    ref = oracle.safeopt_sweep(pts, cfg["ds"], cfg["b"])
    engine.synchronize()
    before = engine.profile()["guard_audit_samples"]
    for _ in range(2):
        engine.set_grid(lo, hi, count)
        engine.set_model(cfg["ds"], dtype="f64")
        kernels = []
        for _ in range(3):
            res = engine.sweep_safeopt(cfg["b"])
            kernels.append(engine.profile_struct().posterior_kernel)
        assert kernels == [6, 4, 4], kernels
        assert res["minimizer_index"] == ref["minimizer_index"] and list(res["expander_index_c"]) == list(ref["expander_index"])
        assert (res["count_S"], res["count_U"], res["count_M"]) == (ref["S"].sum(), ref["U"].sum(), ref["M"].sum())
    engine.synchronize()
    prof = engine.profile()
    assert prof["guard_audit_samples"] > before and prof["guard_audit_violations"] == 0


# ---- what has joined the ABI since the walks were written: the fp64 twin's owner, read-only calls, model updates under recorded tiles --
def _sweeps3(eng, b, x0, r):
    """A SafeOpt, a GoOSE and a trust-region sweep with everything they leave: results, masks, the rechecked count of each."""
    out = []
    for kind in ("safeopt", "goose", "tr"):
        if kind == "safeopt":
            res, names = eng.sweep_safeopt(b, want_masks=True), (("S", 0), ("U", 0), ("M", 0), ("G", 1))
        elif kind == "goose":
            res, names = eng.sweep_goose(b, want_masks=True), (("S", 0), ("U", 0), ("O", 1))
        else:
            res, names = eng.sweep_tr(b, x0, r), (("S", 0), ("M", 0))
        out.append((kind, res, {k: eng.mask(k, c) for k, c in names}, int(eng.profile()["fp64_rechecks"])))
    return out


def test_a_stale_twin_takes_no_part_in_a_single_append(engine):
    """An fp32 model leaves its fp64 twin in the context; the fp64 model set next is not that twin's.  The append that the twin of
    the inconsistent model refuses (tests/test_gpu_append.py::test_refused_append_on_an_fp32_model_with_its_fp64_twin: x_iso again, pivot
    far below zero on output 1) is accepted by the consistent fp64 model -- both of its pivots are positive -- and gives the rebuilt
    model's posterior."""
    ds = mb.refusal_model()
    ds_ok = mb.with_rows(ds, ds["X_norm"], ds["Y_norm"])
    x, y = ds["X_norm"][-1], np.array([0.1, 0.2])
    pivots = [float(mb.block_pivots(ds_ok, x[None], y[None], o)[0]) for o in range(2)]
    assert min(pivots) >= 0.02 and mb.block_pivots(ds, x[None], y[None], 1)[0] < -2.0, pivots
    lo, hi, count = np.array([-2.0, -2.0]), np.array([2.0, 2.0]), [64, 66]
    engine.set_model(ds, dtype="f32")
    engine.set_model(ds_ok)
    engine.append_sample(x, y)
    assert engine.n == 65
    engine.set_grid(lo, hi, count)
    mb.check_post(engine, mb.extended(ds_ok, x, y), oracle.grid_points(lo, hi, count), mb.TOL64, "stale twin, single append")


def test_fp64_recheck_toggled_across_a_model(engine):
    """fp32 model A (its twin is built), fp64_recheck 0, fp32 model B of the same shape (no twin is built: A's stays), fp64_recheck 1.
    The option takes effect at the next set_model, and A's twin is not B's: B's sweeps are the plain fp32 sweeps of a context that
    never had a twin, bit for bit, with nothing rechecked; B's appends and its removal do not reach A's twin; and the next
    set_model(B) builds B's twin, whose rechecked masks are B's fp64 oracle's.  tests/history_cases.py builds A and B so that the twins
    can be told apart: 16 candidates that B's fp64 posterior decides by 1e-8 (its fp32 posterior by its rounding) and A's fp64
    posterior by 2e-2, on the side B's fp64 posterior has them.  Both premises are asserted below; the fp32-only masks in them are
    those of the device's own fp32 sweep on the context without a twin (a float32 NumPy posterior would not reproduce the kernels'
    rounding, which is what decides these candidates), the fp64 decisions of A and B are NumPy's."""
    import safebo_amd
    m = hc.twin_models()
    A, B, pts, picked = m["A"], m["B"], m["pts"], m["picked"]
    b, lo, hi, count = hc.B_CONF, hc.LO, hc.HI, hc.COUNT
    ref64, refA = oracle.safeopt_sweep(pts, B, b), oracle.safeopt_sweep(pts, A, b)
    gref = oracle.goose_sweep(pts, B, b, mean_var=(ref64["mean"], ref64["var"]))
    x0, r = pts[gref["safe_min_index"]], 1.0
    with safebo_amd.SweepEngine(0) as plain:             # never had a twin: the option is off from the start
        plain.set_option("fp64_recheck", 0)
        plain.set_option("guard_audit_every", 1)
        plain.set_model(B, dtype="f32")
        plain.set_grid(lo, hi, count)
        want = _sweeps3(plain, b, x0, r)
        assert plain.profile()["guard_audit_violations"] == 0
    # the premises: B's fp32-only masks differ from its fp64 masks, and where they do A's fp64 posterior contradicts the fp32 one
    S32 = want[0][2]["S"]
    differ = np.nonzero(S32 != ref64["S"])[0]
    told = [int(j) for j in differ if refA["S"][j] != S32[j]]
    print("fp32-only S differs from the fp64 oracle's at", differ.tolist(), "of them decided otherwise by A's fp64 posterior:", told)
    assert np.array_equal(refA["S"][picked], ref64["S"][picked]) and np.array_equal(refA["U"][picked], ref64["U"][picked])
    assert len(differ) >= 1 and len(told) >= 1, (differ, told)
    try:
        engine.set_model(A, dtype="f32")
        engine.set_grid(lo, hi, count)
        engine.sweep_safeopt(b, want_masks=True)
        assert engine.profile()["fp64_rechecks"] > 0     # (A's twin is there and at work)
        engine.set_option("fp64_recheck", 0)
        engine.set_model(B, dtype="f32")
        engine.set_option("fp64_recheck", 1)
        engine.set_grid(lo, hi, count)
        got = _sweeps3(engine, b, x0, r)
        for (kind, res, masks, rechecks), (_, wres, wmasks, _) in zip(got, want):
            assert rechecks == 0, (kind, rechecks)
            for k in wres:
                assert np.array_equal(np.asarray(res[k]), np.asarray(wres[k])), (kind, k, res[k], wres[k])
            for k in wmasks:
                assert np.array_equal(masks[k], wmasks[k]), (kind, k, int((masks[k] != wmasks[k]).sum()))
        # B's updates: accepted, and B's posterior is the rebuilt model's
        rng = np.random.default_rng(21)
        xn = (rng.uniform(-1.8, 1.8, size=(4, 2)) - B["X_mean"]) / B["X_std"]
        yn = rng.uniform(-0.5, 0.5, size=(4, 2))
        engine.append_sample(xn[0], yn[0])
        engine.append_samples(xn[1:], yn[1:])
        engine.remove_sample(5)
        assert engine.n == 67
        ref = mr.without(mb.extended(B, xn, yn), 5)
        engine.set_grid(lo, hi, count)
        mb.check_post(engine, ref, pts, mb.TOL32, "B after an append, a block and a removal")
        assert engine.sweep_safeopt(b)["count_S"] > 0 and engine.profile()["fp64_rechecks"] == 0
        # the next set_model builds B's own twin
        engine.set_model(B, dtype="f32")
        engine.set_grid(lo, hi, count)
        res = engine.sweep_safeopt(b, want_masks=True)
        assert engine.profile()["fp64_rechecks"] > 0
        for k in ("S", "U", "M"):
            got_k = engine.mask(k)
            assert np.array_equal(got_k, ref64[k]), (k, np.nonzero(got_k != ref64[k])[0].tolist())
        assert res["minimizer_index"] == ref64["minimizer_index"]
    finally:
        engine.set_option("fp64_recheck", 1)


@pytest.fixture
def colpath(engine):
    """The column-path options of tests/test_gpu_skip_safe.py on the shared engine, and the defaults back afterwards."""
    cases.colpath_options(engine)
    yield engine
    engine.set_option("fuse_classify", -1)
    engine.set_option("col_path", 1)


def _h_box():
    lo, hi, _ = cases.grid(cases.WHOLE)
    return lo, hi


def _ro_loo(eng, ds, res):
    eng.model_loo(3.0, ds["Y_norm"])


def _ro_mean_grad(eng, ds, res):
    lo, hi = _h_box()
    eng.mean_grad(np.random.default_rng(31).uniform(lo, hi, size=(257, 2)), infnorm=True)


def _ro_lipschitz(eng, ds, res):
    assert np.all(eng.lipschitz(*_h_box())["L"] > 0)


def _ro_batch_select(eng, ds, res):
    lo, hi = _h_box()
    assert len(eng.batch_select(np.random.default_rng(32).uniform(lo, hi, size=(500, 2)), 4)["index"]) == 4


def _ro_refine(eng, ds, res):
    lo, hi = _h_box()
    assert eng.refine(1.0, res["minimizer_x"], 0, "lcb", lo=lo, hi=hi)["best"] == 0


def _ro_refine_sets(eng, ds, res):
    lo, hi = _h_box()
    assert eng.refine_sets(1.0, res["minimizer_x"], objective=0, kind="var", maximize=True, level=(0, res["u_star"] + 0.1), lo=lo, hi=hi)["best"] == 0


def _ro_nll(eng, ds, res):
    H = np.random.default_rng(33).uniform(-1.0, 0.5, size=(8, 4))
    assert np.isfinite(eng.nll_batch(ds["X_norm"], ds["Y_norm"][:, 0], H)).all()


def _ro_expander_gain(eng, ds, res):
    lo, hi = _h_box()
    rng = np.random.default_rng(34)
    assert eng.expander_gain(rng.uniform(lo, hi, size=(9, 2)), rng.uniform(lo, hi, size=(257, 2)), 1.0)["count"].shape == (9,)


def _ro_sample_paths(eng, ds, res):
    lo, hi = _h_box()
    out = eng.sample_paths(np.random.default_rng(35).uniform(lo, hi, size=(257, 2)), 17, 1, features=257, seed=36)
    assert np.all(out["index"] >= 0) and np.isfinite(out["value"]).all()


READ_ONLY = [_ro_loo, _ro_mean_grad, _ro_lipschitz, _ro_batch_select, _ro_refine, _ro_refine_sets, _ro_nll, _ro_expander_gain,
             _ro_sample_paths]


def test_read_only_calls_are_no_writers_of_the_resident_posterior(colpath):
    """Behind a lean-2 column-path sweep that skipped the tiles the plan's enclosures prove safe (the set phase reads what the
    recording sweep stored there): model_loo, mean_grad, lipschitz, batch_select, refine, refine_sets, nll_batch, expander_gain and
    sample_paths leave the stored posterior, the plan and its record alone -- the next lean-2 sweep skips exactly the census's tiles again and equals the fresh
    engine's lean-0 sweep and the oracle, bit for bit."""
    eng, name, b = colpath, cases.WHOLE, 1.0
    ds = cases.config()["ds"]
    census = cases.census_safe(name, b)
    assert census > 0
    cases.start(eng, name, b)
    out = cases.sweep(eng, b, 2)
    assert cases.skips(eng)[0] == census
    unsafe = cases.skips(eng)[1]
    for call in READ_ONLY:
        call(eng, ds, out[0])
        out = cases.sweep(eng, b, 2)
        prof = eng.profile()
        assert prof["posterior_kernel"] == 4 and prof["set_path"] == 1, call.__name__
        assert cases.skips(eng) == (census, unsafe), (call.__name__, cases.skips(eng), census, unsafe)
        cases.same(out, cases.fresh(name, b))
        cases.check_oracle(*out, cases.reference(name, b))


def _updated(kind, ds):
    """(the update as a call on an engine, the rebuilt NumPy model) of sequence d: a removal, or a block of three rows."""
    if kind == "remove":
        return (lambda e: e.remove_sample(40)), mr.without(ds, 40)
    cfg = cases.config()
    x = np.random.default_rng(41).uniform(cfg["bound"][:, 0], cfg["bound"][:, 1], size=(3, 2))
    xn, yn = (x - ds["X_mean"]) / ds["X_std"], (synthetic.benoit(x) - ds["Y_mean"]) / ds["Y_std"]
    return (lambda e: e.append_samples(xn, yn)), mb.extended(ds, xn, yn)


@pytest.mark.parametrize("kind", ["remove", "append_block"])
def test_model_updates_under_recorded_tiles(colpath, kind):
    """A removal, or a block append, behind lean-2 sweeps that skipped proved-safe tiles: the updated model's first K1b sweep skips
    nothing of either kind (it evaluates, stores and records again), the one after skips again, and every sweep equals, bit for bit,
    that of a fresh engine given the model, the same update and no sweep before it -- whose S, U and M are the NumPy oracle's of the
    model rebuilt from the rows (no candidate of it within 1e-9 of a threshold: asserted)."""
    import safebo_amd
    eng, name, b = colpath, cases.WHOLE, 1.0
    ds = cases.config()["ds"]
    lo, hi, count = cases.grid(name)
    update, rebuilt = _updated(kind, ds)
    with safebo_amd.SweepEngine(0) as f:
        cases.colpath_options(f)
        f.set_option("guard_audit_every", 1)
        f.set_grid(lo, hi, list(count))
        f.set_model(ds, dtype="f64")
        update(f)
        want, fresh_kernels = [], []
        for lean in (2, 0, 0):                   # (the first is the plan's recording sweep: the same call as below)
            want.append(cases.sweep(f, b, lean))
            fresh_kernels.append(f.profile()["posterior_kernel"])
        f.synchronize()
        assert f.profile()["set_path"] == 1 and f.profile()["guard_audit_violations"] == 0
    # the fresh engine's masks against NumPy (S, U, M and the minimiser: the oracle's expander set of this grid takes a minute)
    mean, var = oracle.gp_inference(oracle.grid_points(lo, hi, list(count)), rebuilt)
    lcb, ucb = oracle.bounds(mean, var, b)
    S, U = lcb[:, 1] >= 0, lcb[:, 1] <= 0
    u_star = np.min(ucb[S, 0])
    M = S & (lcb[:, 0] <= u_star)
    margin = min(np.min(np.abs(lcb[:, 1])) / max(1.0, rebuilt["Y_std"][1]), np.min(np.abs(lcb[S, 0] - u_star)) / max(1.0, rebuilt["Y_std"][0]))
    print(kind, "smallest decision margin", margin)
    assert margin > 1e-9, margin
    for res, masks in want:
        assert np.array_equal(masks["S"], S) and np.array_equal(masks["U"], U) and np.array_equal(masks["M"], M)
        assert res["minimizer_index"] == int(np.argmax(np.where(M, var[:, 0], -np.inf))) and abs(res["u_star"] - u_star) < 1e-10
    cases.start(eng, name, b)
    cases.sweep(eng, b, 2)
    assert cases.skips(eng)[0] == cases.census_safe(name, b) > 0
    update(eng)
    with pytest.raises(Exception):
        eng.mask("S")
    kernels, skips = [], []
    for w in want + want[-1:]:
        cases.same(cases.sweep(eng, b, 2), w)
        kernels.append(eng.profile()["posterior_kernel"])
        skips.append(cases.skips(eng))
    # (an update keeps the grid's plan box: the updated model's first sweep is already K1b's, and it is the recording one)
    assert kernels == [4, 4, 4, 4] and fresh_kernels == [4, 4, 4], (kernels, fresh_kernels)
    assert skips[0] == (0, 0) and skips[1][0] > 0 and skips[1][1] > 0 and skips[2] == skips[1] and skips[3] == skips[1], skips
