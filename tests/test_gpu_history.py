"""History independence of a SweepEngine: whatever the context did before, a sweep returns what a fresh context returns for the same
model, candidates and options.  Seeded walks (tests/history_walk.py) check every step against NumPy references; directed sequences
cover what walks rarely reach -- K1t plans decided by a lean sweep, a lean K1i sweep outside the column path, one K1t box shared by two
models, a column-path sweep that skipped tiles, and back-to-back sweeps under the standing audit.  On K1t-sized grids the reference is
a second, fresh context on the exact kernel (K1g)."""
import numpy as np
import pytest

import history_walk as hw
import oracle
from safebo_amd import synthetic

pytestmark = pytest.mark.gpu

KERNELS = {}          # seed -> [(step, kind, posterior_kernel, set_path)] of the walks run so far
APPENDS = {}          # seed -> posterior kernels resident at each append


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
        APPENDS[seed] = w.append_kernels
    finally:
        for k, v in hw.DEFAULTS.items():
            engine.set_option(k, v)


@pytest.mark.parametrize("seed", hw.SEEDS)
def test_history_walk(engine, seed):
    _run_walk(engine, seed)


def test_history_walks_took_every_kernel_path(engine):
    """Over all walks, every posterior kernel a 2-D problem or a list can take ran and was checked -- generic (1 / 2), K1g (3), K1b (4),
    K1i (6) --, both set paths (byte masks, column words), and an append found each of K1i, K1b and K1g resident."""
    for seed in hw.SEEDS:
        if seed not in KERNELS:
            _run_walk(engine, seed)
    sweeps = [r for rec in KERNELS.values() for r in rec if r[1] in hw.SWEEPS]
    kernels = {r[2] for r in sweeps}
    paths = {r[3] for r in sweeps if r[1] == "safeopt"}
    assert kernels & {1, 2} and {3, 4, 6} <= kernels, sorted(kernels)
    assert paths == {0, 1}, paths
    assert {3, 4, 6} <= set().union(*APPENDS.values()), APPENDS


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
