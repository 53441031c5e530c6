"""sbo_model_remove over its range: every position and 16-row padding crossing down to one row, every model source and dtype,
several column strips of the kernel, a long sliding window of remove-oldest + append, the model at SBO_MAX_N, refusals -- which
must leave the model exactly as it was -- and the host classes.

The reference for every posterior is the model rebuilt in NumPy from the remaining rows with the frozen normalisation and
hyper-parameters (oracle.build_invK + oracle.gp_inference), in the normalised error and with the tolerances of
tests/test_gpu_append.py."""
import numpy as np
import pytest

import oracle
import safebo_amd
from safebo_amd import GoOSE, SafeOpt, _lib, synthetic

import model_remove as mr
from model_remove import KERNEL, TOL32, TOL64

pytestmark = pytest.mark.gpu


def _grid_check(eng, ds, lo, hi, count, pts, tol, label):
    eng.set_grid(lo, hi, count)
    mr.check_post(eng, ds, pts, tol, label)


# ------------------------------------------------------------------------------------------ 1. positions and paddings
@pytest.mark.parametrize("grown", [False, True])
def test_removals_at_every_position_down_to_one_row(engine, grown):
    """Config B (q = 2, fp64) from n = 90 down to n = 1 at random indices (the first removal takes index 0, the second the last
    index): at every crossing of a 16-row padding boundary, at n = 1 and at the end the posterior on K1b, K1g and the generic
    kernels equals the oracle of the remaining rows.  Once from a freshly built model (tight factor, leading dimension n), once
    from one whose factor an append has grown first."""
    cfg = synthetic.make_config("B", n=90)
    ds0 = cfg["ds"]
    lo, hi, count = cfg["bound"][:, 0], cfg["bound"][:, 1], [64, 72]
    grid_pts = oracle.grid_points(lo, hi, count)
    rng = np.random.default_rng(41 + grown)
    list_pts = rng.uniform(lo, hi, size=(1500, 2))
    if grown:
        engine.set_model(mr.with_rows(ds0, ds0["X_norm"][:89], ds0["Y_norm"][:89]))
        engine.append_sample(ds0["X_norm"][89], ds0["Y_norm"][89])
    else:
        engine.set_model(ds0)
    Xn, Yn = ds0["X_norm"].copy(), ds0["Y_norm"].copy()
    seen, checked = set(), []
    while Xn.shape[0] > 1:
        n = Xn.shape[0]
        j = 0 if n == 90 else (n - 1 if n == 89 else int(rng.integers(0, n)))
        seen |= {"first"} if j == 0 else ({"last"} if j == n - 1 else set())
        engine.remove_sample(j)
        Xn, Yn = np.delete(Xn, j, axis=0), np.delete(Yn, j, axis=0)
        assert engine.n == n - 1
        if (n - 1) % 16 == 0 or n - 1 == 1:
            mr.check_paths(engine, mr.with_rows(ds0, Xn, Yn), lo, hi, count, grid_pts, list_pts, "f64", (grown, n - 1))
            checked.append(n - 1)
    assert checked == [80, 64, 48, 32, 16, 1] and seen == {"first", "last"}


# ------------------------------------------------------------------------------------------ 2. model sources
def _fit_box():
    return np.array([[-1.5, 1.5]] * 3 + [[-2.5, -1.5]])


@pytest.mark.parametrize("source", ["invK", "hyper", "fit"])
def test_one_removal_on_every_model_source(engine, source):
    """n = 40, j = 13 on a model built from the caller's invK, from the hyper-parameters, and by sbo_model_fit (a tiny DE; noise
    box [-2.5, -1.5] so that the oracle stays sharp): every path equals the oracle of the 39 remaining rows."""
    from scipy.stats import qmc
    cfg = synthetic.make_config("B", n=90)
    ds0 = cfg["ds"]
    ds = mr.with_rows(ds0, ds0["X_norm"][:40], ds0["Y_norm"][:40])
    if source == "fit":
        box = _fit_box()
        pop = qmc.scale(qmc.LatinHypercube(4, seed=7).random(20), box[:, 0], box[:, 1])
        data = {k: ds[k] for k in ("X_mean", "X_std", "Y_mean", "Y_std", "X_norm", "Y_norm")}
        rep = engine.model_fit(data, box, pop, seed=7, maxiter=8, tol=0.01)
        ds = dict(ds)
        ds["hypopt"] = rep["hypopt"]
        ds["invKopt"] = oracle.build_invK(ds["X_norm"], ds["hypopt"])
    else:
        engine.set_model(ds, use_invK=source == "invK")
    lo, hi, count = cfg["bound"][:, 0], cfg["bound"][:, 1], [64, 72]
    list_pts = np.random.default_rng(5).uniform(lo, hi, size=(1500, 2))
    engine.remove_sample(13)
    assert engine.n == 39
    mr.check_paths(engine, mr.without(ds, 13), lo, hi, count, oracle.grid_points(lo, hi, count), list_pts, "f64", source)


@pytest.mark.parametrize("q", [1, 3])
def test_one_removal_with_other_output_counts(engine, q):
    """q = 1 and q = 3 with different hyper-parameters per output: the same removal (n = 40, j = 13), then the last and the first."""
    rng = np.random.default_rng(60 + q)
    lo, hi, count = np.array([-.6, -1.0]), np.array([1.5, 1.0]), [64, 72]
    X = rng.uniform(lo, hi, size=(40, 2))
    Y = np.column_stack([synthetic.benoit(X), np.sin(2.0 * X[:, 0]) - X[:, 1]])[:, :q]
    hyp = synthetic.default_hypopt(2, q)
    variants = [synthetic.default_hypopt(2, 1, log_ell=-0.3, log_sn=-1.5)[:, 0], synthetic.default_hypopt(2, 1, log_ell=-0.7, log_sf=0.2)[:, 0]]
    for o in range(1, q):
        hyp[:, o] = variants[o - 1]
    if q == 1:
        hyp[:, 0] = variants[0]
    ds = synthetic.make_dataset(X, Y, hyp)
    list_pts = rng.uniform(lo, hi, size=(1500, 2))
    engine.set_model(ds)
    ref = ds
    for j in (13, 38, 0):
        engine.remove_sample(j)
        ref = mr.without(ref, j)
    assert engine.n == 37 and engine.q == q
    mr.check_paths(engine, ref, lo, hi, count, oracle.grid_points(lo, hi, count), list_pts, "f64", q)


# ------------------------------------------------------------------------------------------ 3. several column strips
@pytest.mark.parametrize("n", [300, 1040])
def test_removals_across_several_column_strips(engine, n):
    """k_model_remove walks strips of 64 new columns (model_remove.STRIP): n - 1 = 299 = 4 x 64 + 43 and 1039 = 16 x 64 + 15
    leave a partial last strip, and the removed column lies in the first strip, in a middle one and in the last.  log_sn = -1.0
    keeps the oracle sharp; the posterior on a 40 x 36 grid after the removal of index 0, n / 2 and n - 2, each from a fresh model."""
    assert mr.STRIP == 64 and (n - 1) % mr.STRIP != 0 and (n - 1) // mr.STRIP >= 4
    cfg = synthetic.make_config("B", n=n, seed=5)
    ds = synthetic.make_dataset(cfg["X"], cfg["Y"], synthetic.default_hypopt(2, 2, log_sn=-1.0))
    lo, hi, count = cfg["bound"][:, 0], cfg["bound"][:, 1], [40, 36]
    pts = oracle.grid_points(lo, hi, count)
    for j in (0, n // 2, n - 2):
        engine.set_model(ds, use_invK=False)
        engine.remove_sample(j)
        assert engine.n == n - 1
        _grid_check(engine, mr.without(ds, j), lo, hi, count, pts, TOL64, (n, j))


# ------------------------------------------------------------------------------------------ 4. sliding window
@pytest.mark.parametrize("seed", [201, 202])
def test_a_long_sliding_window_stays_on_the_rebuilt_model(engine, seed):
    """n = 90, 300 steps of remove(0) + append of a Benoit sample drawn uniformly in the box: every 50 steps and at the end the
    posterior on all four paths equals the oracle of the current window, and at the end a SafeOpt and a GoOSE sweep equal the
    oracle's -- S, U, M, G_1 / O_1, indices and counts -- once the oracle's own margins show that no decision is a tie."""
    cfg = synthetic.make_config("B", n=90)
    ds0 = cfg["ds"]
    lo, hi, count, b = cfg["bound"][:, 0], cfg["bound"][:, 1], [64, 72], cfg["b"]
    grid_pts = oracle.grid_points(lo, hi, count)
    rng = np.random.default_rng(seed)
    Xnew = rng.uniform(lo, hi, size=(300, 2))
    list_pts = rng.uniform(lo, hi, size=(1500, 2))
    xn = (Xnew - ds0["X_mean"]) / ds0["X_std"]
    yn = (synthetic.benoit(Xnew) - ds0["Y_mean"]) / ds0["Y_std"]
    engine.set_model(ds0)
    Xw, Yw = np.vstack([ds0["X_norm"], xn]), np.vstack([ds0["Y_norm"], yn])
    for t in range(300):
        engine.remove_sample(0)
        engine.append_sample(xn[t], yn[t])
        assert engine.n == 90
        if (t + 1) % 50 == 0:
            ref = mr.with_rows(ds0, Xw[t + 1:t + 91], Yw[t + 1:t + 91])
            mr.check_paths(engine, ref, lo, hi, count, grid_pts, list_pts, "f64", (seed, t + 1))
    sref = oracle.safeopt_sweep(grid_pts, ref, b)
    mr.assert_sharp(sref)
    engine.set_grid(lo, hi, count)
    res = engine.sweep_safeopt(b, want_masks=True)
    mr.assert_safeopt_equal(engine, res, sref)
    g = engine.sweep_goose(b, want_masks=True)
    mr.assert_goose_equal(engine, g, oracle.goose_sweep(grid_pts, ref, b))


# ------------------------------------------------------------------------------------------ 5. capacity
def test_a_model_at_capacity_goes_on_after_a_removal(engine):
    """The n = SBO_MAX_N model of the append test (log_sn = -1.0): an append is refused, remove_sample(0) followed by the same
    append succeeds, and the posterior on a 40 x 36 grid equals the oracle of rows 1 .. 2047 plus the new one."""
    N = _lib.SBO_MAX_N
    cfg = synthetic.make_config("B", n=N, seed=5)
    hyp = synthetic.default_hypopt(2, 2, log_sn=-1.0)
    full = synthetic.make_dataset(cfg["X"], cfg["Y"], hyp)
    engine.set_model(full, use_invK=False)
    x_new, y_new = full["X_norm"][0] * 0.5, full["Y_norm"][0]
    with pytest.raises(safebo_amd.SafeBOError) as ei:
        engine.append_sample(x_new, y_new)
    assert ei.value.code == _lib.SBO_E_UNSUPPORTED and engine.n == N
    engine.remove_sample(0)
    engine.append_sample(x_new, y_new)
    assert engine.n == N
    ref = mr.extended(mr.without(full, 0), x_new, y_new)
    lo, hi, count = cfg["bound"][:, 0], cfg["bound"][:, 1], [40, 36]
    _grid_check(engine, ref, lo, hi, count, oracle.grid_points(lo, hi, count), TOL64, "capacity")


# ------------------------------------------------------------------------------------------ 6. fp32
def test_removals_on_an_fp32_model_take_its_fp64_twin_along(engine):
    """fp32 model, n = 90: the first, the middle and the last row leave, then one slide (remove-oldest + append).  The fp32 posterior
    stays within TOL32 and the rechecked SafeOpt sweep's masks equal the fp64 oracle's: the fp64 twin of the recheck followed."""
    cfg = synthetic.make_config("B", n=90)
    ds0 = cfg["ds"]
    lo, hi, count, b = cfg["bound"][:, 0], cfg["bound"][:, 1], [64, 72], cfg["b"]
    grid_pts = oracle.grid_points(lo, hi, count)
    rng = np.random.default_rng(17)
    list_pts = rng.uniform(lo, hi, size=(1500, 2))
    engine.set_model(ds0, dtype="f32")
    ref = ds0
    for j in (0, 44, 87):
        engine.remove_sample(j)
        ref = mr.without(ref, j)
    x = rng.uniform(lo, hi, size=(1, 2))
    xn, yn = ((x - ds0["X_mean"]) / ds0["X_std"])[0], ((synthetic.benoit(x) - ds0["Y_mean"]) / ds0["Y_std"])[0]
    engine.remove_sample(0)
    engine.append_sample(xn, yn)
    ref = mr.extended(mr.without(ref, 0), xn, yn)
    assert engine.n == 87
    mr.check_paths(engine, ref, lo, hi, count, grid_pts, list_pts, "f32", "f32")
    sref = oracle.safeopt_sweep(grid_pts, ref, b)
    mr.assert_sharp(sref)
    engine.set_grid(lo, hi, count)
    res = engine.sweep_safeopt(b, want_masks=True)
    mr.assert_safeopt_equal(engine, res, sref)


# ------------------------------------------------------------------------------------------ 7. three dimensions
def test_removals_from_a_three_dimensional_model_on_the_tensor_path(engine):
    """The d = 3 model of the append test at n = 130: five rows leave across the 129 -> 128 padding crossing; K1t on a sample of
    the 160 x 160 x 168 grid against the oracle of the remaining rows after the crossing and at the end."""
    d, n0, n = 3, 60, 130
    rng = np.random.default_rng(7)
    Xall = rng.uniform(-2.0, 2.0, size=(n, d))
    Yall = np.stack([np.sum(Xall ** 2, axis=1) + np.sin(2.0 * Xall[:, 0]), 3.0 - 0.5 * np.sum(Xall ** 2, axis=1) + Xall[:, 1]], axis=1)
    base = synthetic.make_dataset(Xall[:n0], Yall[:n0], synthetic.default_hypopt(d, 2, log_ell=-0.5))
    ref = mr.with_rows(base, (Xall - base["X_mean"]) / base["X_std"], (Yall - base["Y_mean"]) / base["Y_std"])
    lo, hi, count = np.full(d, -2.0), np.full(d, 2.0), [160, 160, 168]
    total = int(np.prod(count))
    idx = np.unique(np.concatenate([rng.integers(0, total, size=3000), [0, total - 1, count[0] - 1, total - count[0]]]))
    axes = oracle.grid_axes(lo, hi, count)
    sub = np.empty((idx.size, d))
    f = idx.copy()
    for a in range(d):
        sub[:, a] = axes[a][f % count[a]]
        f //= count[a]
    engine.set_model(ref)
    for step, j in enumerate((0, 128, 64, 126, 3)):
        engine.remove_sample(j)
        ref = mr.without(ref, j)
        if step in (1, 4):
            assert engine.n == (128 if step == 1 else 125)
            engine.set_grid(lo, hi, count)
            mean, var = engine.posterior()
            assert engine.profile()["posterior_kernel"] == KERNEL["K1t"], step
            om, ov = oracle.gp_inference(sub, ref)
            em, ev = mr.nerr(mean[idx], om, ref["Y_std"], 1), mr.nerr(var[idx], ov, ref["Y_std"], 2)
            assert em < TOL64 and ev < TOL64, (step, em, ev)


# ------------------------------------------------------------------------------------------ 8. refusals
def _snapshot(eng, lo, hi, count, b):
    """What the resident model gives, bit for bit (tests/test_gpu_append.py): n, the posterior on a fresh grid on K1b and on K1g, a
    full SafeOpt sweep and its masks."""
    out = {"n": eng.n}
    try:
        for name, bl in (("K1b", 2), ("K1g", 0)):
            eng.set_option("bilinear", bl)
            eng.set_grid(lo, hi, count)
            eng.posterior_run()
            kernel = eng.profile()["posterior_kernel"]          # (n <= 16: K1b's plan hands the model to K1g, model_remove.check_paths)
            assert kernel == KERNEL[name] or (eng.n <= 16 and kernel == KERNEL["K1g"]), (name, kernel)
            out[name] = eng.posterior()
    finally:
        eng.set_option("bilinear", 1)
    eng.set_grid(lo, hi, count)
    eng.sweep_safeopt(b)
    out["sweep"] = eng.sweep_safeopt(b, want_masks=True)
    out["masks"] = [eng.mask(k) for k in ("S", "U", "M")] + [eng.mask("G", 1)]
    return out


def _assert_same(a, b):
    assert a["n"] == b["n"]
    for name in ("K1b", "K1g"):
        for x, y in zip(a[name], b[name]):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), name
    for k, v in a["sweep"].items():
        assert np.array_equal(np.asarray(v), np.asarray(b["sweep"][k])), k
    for x, y in zip(a["masks"], b["masks"]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("rows", [40, 1])
def test_a_refused_removal_changes_nothing(engine, rows):
    """index = -1 and index = n are SBO_E_INVALID, and so is any index at n == 1; the snapshot around each refused call -- n, the
    K1b and K1g posteriors bit for bit, a full sweep result and the masks -- is the same."""
    cfg = synthetic.make_config("B", n=90)
    ds0 = cfg["ds"]
    sel = slice(0, rows) if rows > 1 else slice(45, 46)    # (row 45 has the largest constraint value: alone it still has a safe set)
    ds = mr.with_rows(ds0, ds0["X_norm"][sel], ds0["Y_norm"][sel])
    lo, hi, count, b = cfg["bound"][:, 0], cfg["bound"][:, 1], [64, 72], cfg["b"]
    engine.set_model(ds)
    before = _snapshot(engine, lo, hi, count, b)
    for bad in ((-1, rows) if rows > 1 else (-1, 1, 0)):
        assert engine._lib.sbo_model_remove(engine._ctx, bad) == _lib.SBO_E_INVALID, bad
        with pytest.raises(ValueError):
            engine.remove_sample(bad)
        assert engine.n == rows
        _assert_same(before, _snapshot(engine, lo, hi, count, b))
    assert engine._lib.sbo_model_remove(None, 0) == _lib.SBO_E_INVALID
    for bad in (1.0, None, True):
        with pytest.raises(ValueError):
            engine.remove_sample(bad)
    _assert_same(before, _snapshot(engine, lo, hi, count, b))


def test_a_removal_without_a_model_is_refused():
    with safebo_amd.SweepEngine(0) as eng:
        assert eng._lib.sbo_model_remove(eng._ctx, 0) == _lib.SBO_E_NO_MODEL
        with pytest.raises(safebo_amd.SafeBOError) as ei:
            eng.remove_sample(0)
        assert ei.value.code == _lib.SBO_E_NO_MODEL and eng.n == 0


# ------------------------------------------------------------------------------------------ 9. round trip
def test_an_append_taken_back_gives_the_original_model(engine):
    """Append x, then remove the last index: posterior within TOL64 of the original model's on every path, sweep masks exactly
    the original model's (not required to be bitwise equal in the posterior)."""
    cfg = synthetic.make_config("B", n=90)
    ds = cfg["ds"]
    lo, hi, count, b = cfg["bound"][:, 0], cfg["bound"][:, 1], [64, 72], cfg["b"]
    grid_pts = oracle.grid_points(lo, hi, count)
    rng = np.random.default_rng(23)
    list_pts = rng.uniform(lo, hi, size=(1500, 2))
    sref = oracle.safeopt_sweep(grid_pts, ds, b)
    mr.assert_sharp(sref)
    engine.set_model(ds)
    engine.set_grid(lo, hi, count)
    m0, v0 = engine.posterior()
    r0 = engine.sweep_safeopt(b, want_masks=True)
    k0 = [engine.mask(k) for k in ("S", "U", "M")] + [engine.mask("G", 1)]
    x = rng.uniform(lo, hi, size=(1, 2))
    engine.append_sample(((x - ds["X_mean"]) / ds["X_std"])[0], ((synthetic.benoit(x) - ds["Y_mean"]) / ds["Y_std"])[0])
    engine.remove_sample(90)
    assert engine.n == 90
    mr.check_paths(engine, ds, lo, hi, count, grid_pts, list_pts, "f64", "round trip")
    engine.set_grid(lo, hi, count)
    m1, v1 = engine.posterior()
    assert mr.nerr(m1, m0, ds["Y_std"], 1) < TOL64 and mr.nerr(v1, v0, ds["Y_std"], 2) < TOL64
    r1 = engine.sweep_safeopt(b, want_masks=True)
    for a, c in zip(k0, [engine.mask(k) for k in ("S", "U", "M")] + [engine.mask("G", 1)]):
        assert np.array_equal(a, c)
    for k in ("minimizer_index", "count_S", "count_U", "count_M"):
        assert r0[k] == r1[k], k
    mr.assert_safeopt_equal(engine, r1, sref)


# ------------------------------------------------------------------------------------------ 10. host classes
@pytest.mark.parametrize("cls", [SafeOpt.BO, GoOSE.BO])
def test_remove_sample_invalidates_the_cached_sweep(cls):
    """sweep -> remove_sample(3) -> sweep must be the sweep of the (n - 1)-point model: a new result that equals the oracle's on the
    host copy of the model (Schur complement of the old inverse), which stays a complete, uploadable state."""
    m = mr.init_bo(cls, n=14, grid=(60, 50))
    first = m.sweep()
    m.remove_sample(3)
    assert m.n_point == 13 and m.inference_datasets["X_norm"].shape == (13, 2) and m.inference_datasets["invKopt"][0].shape == (13, 13)
    second = m.sweep()
    assert second is not first
    pts = oracle.grid_points(mr.BOUND[:, 0], mr.BOUND[:, 1], [60, 50])
    ref = oracle.safeopt_sweep(pts, m.inference_datasets, 3.0)
    assert second["minimizer_index"] == ref["minimizer_index"] and second["count_S"] == int(ref["S"].sum())
    assert second["count_M"] == int(ref["M"].sum())
    assert second["minimizer_std"] == pytest.approx(ref["minimizer_std"], rel=1e-7)
    if cls is GoOSE.BO:
        g = m.goose_sweep()
        gref = oracle.goose_sweep(pts, m.inference_datasets, 3.0)
        assert g["safe_min_index"] == gref["safe_min_index"] and g["target_index"] == gref["target_index"]
    mean, var = m.GP_inference(pts[::37], None)
    om, ov = oracle.gp_inference(pts[::37], m.inference_datasets)
    assert np.max(np.abs(mean - om)) < 1e-8 and np.max(np.abs(var - ov)) < 1e-8


def test_a_windowed_campaign_keeps_its_size_and_matches_the_oracle():
    """20 steps of sweep -> sample the minimiser -> add_sample(incremental=True, window=14) from n = 14: n_point stays 14 and every
    step's sweep is the oracle's sweep of the current window."""
    m = mr.init_bo(SafeOpt.BO, n=14, grid=(60, 50))
    pts = oracle.grid_points(mr.BOUND[:, 0], mr.BOUND[:, 1], [60, 50])
    for step in range(20):
        res = m.sweep()
        ref = oracle.safeopt_sweep(pts, m.inference_datasets, 3.0)
        assert res["minimizer_index"] == ref["minimizer_index"] and res["count_S"] == int(ref["S"].sum()), step
        assert res["count_M"] == int(ref["M"].sum()), step
        assert res["minimizer_std"] == pytest.approx(ref["minimizer_std"], rel=1e-7), step
        x_new = np.asarray(res["minimizer_x"])
        oldest = m.X[1].copy()
        m.add_sample(x_new, m.calculate_plant_outputs(x_new), incremental=True, window=14)
        assert m.n_point == 14 and m.engine.n == 14 and m.inference_datasets["X_norm"].shape == (14, 2), step
        assert np.array_equal(m.X[0], oldest) and np.array_equal(m.X[-1], x_new)
