"""sbo_model_append_batch on the device: k observations in one block update against the model rebuilt in NumPy
from all rows (oracle.build_invK + oracle.gp_inference, frozen normalisation and hyper-parameters), against k single appends, and
next to its neighbours.  Every shape comes from tests/model_append_batch.py, where the CPU tests show it sharp."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import safebo_amd
from safebo_amd import SafeOpt, _lib, synthetic

import model_append_batch as mb
import model_loo as ml
from model_append_batch import TOL32, TOL64
from model_remove import init_bo

pytestmark = pytest.mark.gpu


def _set(eng, ds, source="invK", dtype="f64"):
    eng.set_model(ds, dtype=dtype, use_invK=source == "invK")


def _raw(eng, k, X, Y):
    """The C call itself, past the host checks of SweepEngine.append_samples."""
    X, Y = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(Y, dtype=np.float64)
    return eng._lib.sbo_model_append_batch(eng._ctx, int(k), X.ctypes.data_as(C.c_void_p), Y.ctypes.data_as(C.c_void_p))


def _config_b(n0, total, log_sn, seed=5):
    """Config B's Benoit rows: ds of the first n0 of `total` rows (normalised over all of them), and the ds of all rows."""
    cfg = synthetic.make_config("B", n=total, seed=seed)
    full = synthetic.make_dataset(cfg["X"], cfg["Y"], synthetic.default_hypopt(2, 2, log_sn=log_sn))
    return mb.with_rows(full, full["X_norm"][:n0], full["Y_norm"][:n0]), full, cfg


# ------------------------------------------------------------------------------------------ 1. equals a rebuild
@pytest.mark.parametrize("case", mb.CASES, ids=mb.case_id)
def test_a_block_equals_a_rebuild(engine, case):
    """Every committed case: after append_samples the posterior equals the oracle of the model rebuilt from all rows within TOL64 --
    d = 2 on K1b and K1g on a 64 x 72 grid, every d on the generic kernels (posterior_path 1 and 2) on a 1500-point list; on
    (250, 64) a SafeOpt and a GoOSE sweep have the oracle's masks, indices and counts."""
    n0, k, d, q, _, source = case
    ds, xn, yn, full = mb.case_data(case)
    _set(engine, ds, source)
    engine.append_samples(xn, yn)
    assert (engine.n, engine.d, engine.q) == (n0 + k, d, q)
    b = mb.box(d)
    list_pts = np.random.default_rng(7).uniform(b[:, 0], b[:, 1], size=(1500, d))
    if d != 2:
        mb.check_list_paths(engine, full, list_pts, TOL64, mb.case_id(case))
        return
    lo, hi, count = b[:, 0], b[:, 1], [64, 72]
    grid_pts = oracle.grid_points(lo, hi, count)
    mb.check_paths(engine, full, lo, hi, count, grid_pts, list_pts, "f64", mb.case_id(case))
    if (n0, k) != (250, 64):
        return
    sref = oracle.safeopt_sweep(grid_pts, full, 3.0)
    mb.assert_sharp(sref)
    engine.set_grid(lo, hi, count)
    mb.assert_safeopt_equal(engine, engine.sweep_safeopt(3.0, want_masks=True), sref)
    mb.assert_goose_equal(engine, engine.sweep_goose(3.0, want_masks=True), oracle.goose_sweep(grid_pts, full, 3.0))


def test_a_block_on_a_three_dimensional_model_on_the_tensor_path(engine):
    """d = 3, n0 = 60 + a block of 21 (crosses npad = 64 -> 96): K1t on a sample of a 160 x 160 x 168 grid against the oracle."""
    d, n0, k = 3, 60, 21
    rng = np.random.default_rng(7)
    X = rng.uniform(-2.0, 2.0, size=(n0 + k, d))
    full = synthetic.make_dataset(X, mb.plant(X, 2), synthetic.default_hypopt(d, 2, log_ell=-0.5))
    engine.set_model(mb.with_rows(full, full["X_norm"][:n0], full["Y_norm"][:n0]))
    engine.append_samples(full["X_norm"][n0:], full["Y_norm"][n0:])
    lo, hi, count = np.full(d, -2.0), np.full(d, 2.0), [160, 160, 168]
    total = int(np.prod(count))
    idx = np.unique(np.concatenate([rng.integers(0, total, size=3000), [0, total - 1, count[0] - 1, total - count[0]]]))
    axes = oracle.grid_axes(lo, hi, count)
    sub, f = np.empty((idx.size, d)), idx.copy()
    for a in range(d):
        sub[:, a] = axes[a][f % count[a]]
        f //= count[a]
    engine.set_grid(lo, hi, count)
    mean, var = engine.posterior()
    assert engine.profile()["posterior_kernel"] == mb.KERNEL["K1t"]
    om, ov = oracle.gp_inference(sub, full)
    assert mb.nerr(mean[idx], om, full["Y_std"], 1) < TOL64 and mb.nerr(var[idx], ov, full["Y_std"], 2) < TOL64


# ------------------------------------------------------------------------------------------ 2. growth
def test_blocks_that_grow_the_factor(engine):
    """From n0 = 90 (first capacity 384) blocks of 64 with log_sn = -1: the fifth, 346 -> 410, crosses the capacity; the posterior
    is checked after every block.  Then a model grown by single appends from 90 to 380 takes a block of 8 across the same capacity."""
    ds, full, cfg = _config_b(90, 410, -1.0)
    lo, hi, count = cfg["bound"][:, 0], cfg["bound"][:, 1], [64, 72]
    grid_pts = oracle.grid_points(lo, hi, count)
    list_pts = np.random.default_rng(3).uniform(lo, hi, size=(1500, 2))
    Xn, Yn = full["X_norm"], full["Y_norm"]
    _set(engine, ds)
    for n in range(90, 410, 64):
        engine.append_samples(Xn[n:n + 64], Yn[n:n + 64])
        assert engine.n == n + 64
        mb.check_paths(engine, mb.with_rows(full, Xn[:n + 64], Yn[:n + 64]), lo, hi, count, grid_pts, list_pts, "f64", n + 64)
    _set(engine, ds)
    for j in range(90, 380):
        engine.append_sample(Xn[j], Yn[j])
    engine.append_samples(Xn[380:388], Yn[380:388])
    assert engine.n == 388
    mb.check_paths(engine, mb.with_rows(full, Xn[:388], Yn[:388]), lo, hi, count, grid_pts, list_pts, "f64", "singles then a block")


# ------------------------------------------------------------------------------------------ 3. capacity
@functools.lru_cache(maxsize=1)
def _capacity_model():
    N = _lib.SBO_MAX_N
    cfg = synthetic.make_config("B", n=N, seed=5)
    full = synthetic.make_dataset(cfg["X"], cfg["Y"], synthetic.default_hypopt(2, 2, log_sn=-1.0))
    lo, hi, count = cfg["bound"][:, 0], cfg["bound"][:, 1], [40, 36]
    pts = oracle.grid_points(lo, hi, count)
    return full, lo, hi, count, pts, oracle.gp_inference(pts, full)


def _short(full, n0):
    ds = dict(full)
    ds["X_norm"], ds["Y_norm"], ds["invKopt"] = full["X_norm"][:n0], full["Y_norm"][:n0], None   # (use_invK=False: never read)
    return ds


def test_a_block_that_reaches_capacity(engine):
    """n0 = 1984, k = 64 reaches SBO_MAX_N: the posterior equals the n = 2048 oracle; one more row is SBO_E_UNSUPPORTED."""
    full, lo, hi, count, pts, (om, ov) = _capacity_model()
    N = _lib.SBO_MAX_N
    engine.set_model(_short(full, 1984), use_invK=False)
    engine.append_samples(full["X_norm"][1984:], full["Y_norm"][1984:])
    assert engine.n == N
    engine.set_grid(lo, hi, count)
    mean, var = engine.posterior()
    assert mb.nerr(mean, om, full["Y_std"], 1) < TOL64 and mb.nerr(var, ov, full["Y_std"], 2) < TOL64
    with pytest.raises(safebo_amd.SafeBOError) as ei:
        engine.append_samples(full["X_norm"][:1] * 0.5, full["Y_norm"][:1])
    assert ei.value.code == _lib.SBO_E_UNSUPPORTED and engine.n == N
    engine.set_grid(lo, hi, count)
    again = engine.posterior()
    assert np.array_equal(mean, again[0]) and np.array_equal(var, again[1])


def test_a_block_that_does_not_fit_appends_no_prefix(engine):
    """From n0 = 2040 a block of 9 is SBO_E_UNSUPPORTED with n still 2040 and the posterior bit for bit as before; a block of 8 is
    then accepted and gives the n = 2048 oracle."""
    full, lo, hi, count, pts, (om, ov) = _capacity_model()
    engine.set_model(_short(full, 2040), use_invK=False)
    engine.set_grid(lo, hi, count)
    before = engine.posterior()
    nine = np.vstack([full["X_norm"][2040:], full["X_norm"][:1] * 0.5]), np.vstack([full["Y_norm"][2040:], full["Y_norm"][:1]])
    with pytest.raises(safebo_amd.SafeBOError) as ei:
        engine.append_samples(*nine)
    assert ei.value.code == _lib.SBO_E_UNSUPPORTED and engine.n == 2040
    engine.set_grid(lo, hi, count)
    after = engine.posterior()
    for x, y in zip(before, after):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    engine.append_samples(full["X_norm"][2040:], full["Y_norm"][2040:])
    assert engine.n == _lib.SBO_MAX_N
    engine.set_grid(lo, hi, count)
    mean, var = engine.posterior()
    assert mb.nerr(mean, om, full["Y_std"], 1) < TOL64 and mb.nerr(var, ov, full["Y_std"], 2) < TOL64


# ------------------------------------------------------------------------------------------ 4. refusals
REFUSALS = ["pivot_k8_at0", "pivot_k8_at3", "pivot_k8_at7", "pivot_k64_at63", "x_nan_mid", "y_inf_mid", "k0", "k65"]


@pytest.mark.parametrize("trigger", REFUSALS)
def test_a_refused_block_changes_nothing(engine, trigger):
    """A refused block -- a Schur pivot that is not > 0 on output 1 at the first, a middle or the last row of the block (after the
    device computed every output's update), a non-finite value in a middle row, k = 0, k = 65 -- leaves n, the posterior on K1b and
    K1g and a full want-masks sweep bit for bit as they were.  A valid block afterwards equals the oracle of the block-bordered
    inverse of the caller's matrices."""
    ds = mb.refusal_model()
    lo, hi, count, b = np.array([-2.0, -2.0]), np.array([2.0, 2.0]), [64, 66], 2.0
    pts = oracle.grid_points(lo, hi, count)
    engine.set_model(ds)
    before = mb.snapshot(engine, lo, hi, count, b)
    n = ds["X_norm"].shape[0]
    if trigger.startswith("pivot"):
        k, pos = int(trigger.split("_")[1][1:]), int(trigger.split("at")[1])
        xn, yn = mb.refusal_block(ds, k, pos)
        # the margins of the trigger, in NumPy: output 0 accepts the block, output 1 refuses it at row pos and not before
        p0, p1 = mb.block_pivots(ds, xn, yn, 0), mb.block_pivots(ds, xn, yn, 1)
        assert p0.shape == (k,) and np.all(p0 >= 0.02) and p1.shape == (pos + 1,) and p1[pos] < -2.0 and np.all(p1[:pos] >= 0.02)
        with pytest.raises(ValueError, match=f"output 1, row {pos} "):
            engine.append_samples(xn, yn)
    else:
        xn, yn = mb.refusal_block(ds, 8, 0)
        xn[0] = [0.3, -0.2]
        k = 8
        if trigger == "x_nan_mid":
            xn[4, 1] = np.nan
        elif trigger == "y_inf_mid":
            yn[3, 0] = np.inf
        elif trigger == "k0":
            k = 0
        else:
            k, xn, yn = 65, np.tile(xn, (9, 1))[:65], np.tile(yn, (9, 1))[:65]
        assert _raw(engine, k, xn, yn) == _lib.SBO_E_INVALID
        with pytest.raises(ValueError):
            engine.append_samples(xn[:k] if k <= 8 else xn, yn[:k] if k <= 8 else yn)
    assert engine.n == n
    mb.assert_same(before, mb.snapshot(engine, lo, hi, count, b))
    xv, yv = mb.refusal_block(ds, 8, 0)
    xv[0] = [0.25, -0.4]
    engine.append_samples(xv, yv)
    assert engine.n == n + 8
    ref = mb.extended(ds, xv, yv, invK=[mb.bordered_invK(ds, xv, o) for o in range(2)])
    try:
        for bl in (2, 0):
            engine.set_option("bilinear", bl)
            engine.set_grid(lo, hi, count)
            engine.posterior_run()
            assert engine.profile()["posterior_kernel"] == mb.KERNEL["K1b" if bl else "K1g"]
            mb.check_post(engine, ref, pts, TOL64, (trigger, bl))
    finally:
        engine.set_option("bilinear", 1)


def test_a_block_without_a_model_is_no_model():
    with safebo_amd.SweepEngine(0) as eng:
        assert _raw(eng, 2, np.zeros((2, 2)), np.zeros((2, 2))) == _lib.SBO_E_NO_MODEL
        assert _raw(eng, 0, np.zeros((2, 2)), np.zeros((2, 2))) == _lib.SBO_E_INVALID


# ------------------------------------------------------------------------------------------ 5. fp32 with its fp64 twin
def test_an_fp32_model_with_its_fp64_twin(engine):
    """fp32 model (the fp64 twin of the recheck follows the block): a refused block leaves the posterior, the rechecked sweep and
    its masks as they were; after a valid block the fp32 posterior is within TOL32 and the rechecked SafeOpt sweep has the fp64
    oracle's masks."""
    ds = mb.refusal_model()
    lo, hi, count, b = np.array([-2.0, -2.0]), np.array([2.0, 2.0]), [64, 66], 2.0
    pts = oracle.grid_points(lo, hi, count)
    engine.set_model(ds, dtype="f32")
    engine.set_grid(lo, hi, count)
    m0, v0 = engine.posterior()
    r0 = engine.sweep_safeopt(b, want_masks=True, posterior_ready=True)
    k0 = [engine.mask(k) for k in ("S", "U", "M")]
    with pytest.raises(ValueError):
        engine.append_samples(*mb.refusal_block(ds, 8, 3))
    assert engine.n == ds["X_norm"].shape[0]
    engine.set_grid(lo, hi, count)
    m1, v1 = engine.posterior()
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    r1 = engine.sweep_safeopt(b, want_masks=True, posterior_ready=True)
    for k in r0:
        assert np.array_equal(np.asarray(r0[k]), np.asarray(r1[k])), k
    for a, c in zip(k0, [engine.mask(k) for k in ("S", "U", "M")]):
        assert np.array_equal(a, c)
    # a consistent model for the valid block: output 1's matrix as the data give it
    ds_ok = mb.with_rows(ds, ds["X_norm"], ds["Y_norm"])
    engine.set_model(ds_ok, dtype="f32")
    xv, yv = mb.refusal_block(ds, 8, 0)
    xv[0] = [0.25, -0.4]
    engine.append_samples(xv, yv)
    ref = mb.extended(ds_ok, xv, yv)
    engine.set_grid(lo, hi, count)
    mb.check_post(engine, ref, pts, TOL32, "f32")
    res = engine.sweep_safeopt(b, want_masks=True)
    sref = oracle.safeopt_sweep(pts, ref, b)
    for k in ("S", "U", "M"):
        assert np.array_equal(engine.mask(k), sref[k]), k
    assert res["minimizer_index"] == sref["minimizer_index"]


def test_a_twin_left_behind_by_an_earlier_fp32_model_takes_no_part(engine):
    """An fp32 model leaves its fp64 twin in the context.  A later fp64 model is not that twin's: a block the fp64 model accepts
    (x_iso again, on consistent matrices: every pivot >= 0.02) is accepted although the stale twin -- which still holds the
    inconsistent output 1 -- would refuse it (pivot -2.91)."""
    ds = mb.refusal_model()
    ds_ok = mb.with_rows(ds, ds["X_norm"], ds["Y_norm"])
    xn, yn = mb.refusal_block(ds, 8, 3)
    assert all(mb.block_pivots(ds_ok, xn, yn, o).min() >= 0.02 for o in range(2)) and mb.block_pivots(ds, xn, yn, 1)[-1] < -2.0
    engine.set_model(ds, dtype="f32")
    engine.set_model(ds_ok)
    engine.append_samples(xn, yn)
    assert engine.n == 72
    lo, hi, count = np.array([-2.0, -2.0]), np.array([2.0, 2.0]), [64, 66]
    engine.set_grid(lo, hi, count)
    mb.check_post(engine, mb.extended(ds_ok, xn, yn), oracle.grid_points(lo, hi, count), TOL64, "stale twin")


# ------------------------------------------------------------------------------------------ 6. against the single append
@pytest.mark.parametrize("case", [c for c in mb.CASES if (c[0], c[1]) in ((16, 17), (250, 64))], ids=mb.case_id)
def test_a_block_against_single_appends(engine, case):
    """The same rows by append_samples on one engine and by k append_sample calls on another: the posteriors agree within the
    project's bar (both are within it of the rebuilt oracle) and, the case being sharp, the sweep's masks and indices are identical."""
    n0, k, d, q, _, source = case
    ds, xn, yn, full = mb.case_data(case)
    b = mb.box(d)
    lo, hi, count = b[:, 0], b[:, 1], [64, 72]
    mb.assert_sharp(oracle.safeopt_sweep(oracle.grid_points(lo, hi, count), full, 3.0))
    _set(engine, ds, source)
    engine.append_samples(xn, yn)
    engine.set_grid(lo, hi, count)
    mean, var = engine.posterior()
    res = engine.sweep_safeopt(3.0, want_masks=True)
    masks = [engine.mask(m) for m in ("S", "U", "M")] + [engine.mask("G", 1)]
    with safebo_amd.SweepEngine(0) as other:
        _set(other, ds, source)
        for r in range(k):
            other.append_sample(xn[r], yn[r])
        other.set_grid(lo, hi, count)
        m2, v2 = other.posterior()
        res2 = other.sweep_safeopt(3.0, want_masks=True)
        masks2 = [other.mask(m) for m in ("S", "U", "M")] + [other.mask("G", 1)]
    em, ev = mb.nerr(mean, m2, full["Y_std"], 1), mb.nerr(var, v2, full["Y_std"], 2)
    print("block vs singles", mb.case_id(case), em, ev)
    assert em < TOL64 and ev < TOL64, (em, ev)
    for x, y in zip(masks, masks2):
        assert np.array_equal(x, y)
    for key in ("minimizer_index", "expander_index", "count_S", "count_U", "count_M"):
        assert np.array_equal(np.asarray(res[key]), np.asarray(res2[key])), key


# ------------------------------------------------------------------------------------------ 7. determinism and history
def test_same_block_same_bits_whatever_came_before():
    """Two fresh engines with the same block give a bit-identical posterior; an engine that swept before the block (its plans were
    built and dropped) sweeps afterwards bit for bit like a fresh engine given the same final calls."""
    case = (250, 64, 2, 2, -1.0, "invK")
    ds, xn, yn, full = mb.case_data(case)
    b = mb.box(2)
    lo, hi, count = b[:, 0], b[:, 1], [64, 72]
    out = []
    for swept in (False, False, True):
        with safebo_amd.SweepEngine(0) as eng:
            _set(eng, ds)
            if swept:
                eng.set_grid(lo, hi, count)
                eng.sweep_safeopt(3.0)
                eng.sweep_safeopt(3.0, want_masks=True)
            eng.append_samples(xn, yn)
            eng.set_grid(lo, hi, count)
            post = eng.posterior()
            eng.sweep_safeopt(3.0)
            res = eng.sweep_safeopt(3.0, want_masks=True)
            out.append((post, res, [eng.mask(m) for m in ("S", "U", "M")]))
    for other in out[1:]:
        for x, y in zip(out[0][0], other[0]):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        for key, v in out[0][1].items():
            assert np.array_equal(np.asarray(v), np.asarray(other[1][key])), key
        for x, y in zip(out[0][2], other[2]):
            assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------ 8. neighbours
def test_remove_eight_append_eight_cycles_stay_on_the_rebuilt_window(engine):
    """20 cycles of (remove index 0 eight times, block of 8) at n = 90 stay within the bar of the window rebuilt from its rows."""
    ds, full, cfg = _config_b(90, 250, -2.0)
    lo, hi, count = cfg["bound"][:, 0], cfg["bound"][:, 1], [64, 72]
    Xn, Yn = full["X_norm"], full["Y_norm"]
    _set(engine, ds)
    for c in range(20):
        for _ in range(8):
            engine.remove_sample(0)
        engine.append_samples(Xn[90 + 8 * c:98 + 8 * c], Yn[90 + 8 * c:98 + 8 * c])
    assert engine.n == 90
    ref = mb.with_rows(full, Xn[160:250], Yn[160:250])
    engine.set_grid(lo, hi, count)
    mb.check_post(engine, ref, oracle.grid_points(lo, hi, count), TOL64, "window")


def test_model_loo_after_a_block(engine):
    case = (64, 64, 2, 3, -2.0, "invK")
    ds, xn, yn, full = mb.case_data(case)
    _set(engine, ds)
    engine.append_samples(xn, yn)
    ml.check_loo(engine, full, ml.TOL64, "after a block")


def test_batch_select_then_a_block_of_its_picks(engine):
    """batch_select(k = 4, one pending point) followed by append_samples of those five points: posterior() has, at the pool, the
    variance var_out announced (TOL64 normalised, as for the single-append twin in tests/test_gpu_batch_select.py)."""
    ds, full, cfg = _config_b(40, 90, -2.0)
    bound = cfg["bound"]
    pool = np.random.default_rng(201).uniform(bound[:, 0], bound[:, 1], size=(257, 2))
    pending = np.random.default_rng(202).uniform(bound[:, 0], bound[:, 1], size=(1, 2))
    for o in (0, 1):
        _set(engine, ds)
        got = engine.batch_select(pool, 4, o, pending, return_var=True)
        assert len(got["index"]) == 4
        added = np.vstack([pending, got["x"]])
        engine.append_samples((added - ds["X_mean"]) / ds["X_std"], np.array([[0.3 * t - 0.5, 1.0 - 0.2 * t] for t in range(5)]))
        engine.set_points(pool)
        _, var = engine.posterior()
        err = float(np.max(np.abs(var[:, o] - got["var"]))) / float(ds["Y_std"][o]) ** 2
        print("batch_select", o, err)
        assert err < TOL64, err


def test_refine_and_mean_grad_after_a_block(engine):
    """A grown factor (leading dimension > n) under the refine and the mean gradient: both follow the block."""
    case = (16, 17, 2, 2, -2.0, "K")
    ds, xn, yn, full = mb.case_data(case)
    _set(engine, ds, "K")
    engine.append_samples(xn, yn)
    b = mb.box(2)
    lo, hi = b[:, 0], b[:, 1]
    pts = np.random.default_rng(4).uniform(lo, hi, size=(300, 2))
    got = engine.mean_grad(pts)
    got = got[0] if isinstance(got, tuple) else got
    want = oracle.mean_grad(pts, full)
    for o in range(2):
        scale = np.max(np.abs(want[:, o, :]))
        assert np.max(np.abs(got[:, o, :] - want[:, o, :])) <= 1e-9 * scale, o        # (tests/test_gpu_lipschitz.py: RTOL)
    seed = np.array([[0.4, 0.1]])
    out = engine.refine(2.0, seed, 0, "lcb", constraints=[], lo=lo, hi=hi)
    assert out["status"][0] in (_lib.SBO_REFINE_CONVERGED, _lib.SBO_REFINE_MAX_EVAL)
    m0, v0 = oracle.gp_inference(seed, full)
    m, v = oracle.gp_inference(out["x"], full)
    assert out["value"][0] <= m0[0, 0] - 2.0 * np.sqrt(v0[0, 0]) + 1e-12
    assert abs(out["value"][0] - (m[0, 0] - 2.0 * np.sqrt(v[0, 0]))) <= 1e-10 * max(1.0, abs(m[0, 0]))   # (tests/test_gpu_refine.py)
    engine.set_model(full)
    fresh = engine.refine(2.0, seed, 0, "lcb", constraints=[], lo=lo, hi=hi)
    assert np.max(np.abs(out["x"][0] - fresh["x"][0])) <= 1e-5 and abs(out["value"][0] - fresh["value"][0]) <= 1e-9 * max(1.0, abs(fresh["value"][0]))


# ------------------------------------------------------------------------------------------ 9. host classes
def test_batch_then_add_samples_of_a_host_class():
    """SafeOpt.BO: Batch(4) -> plant -> add_samples(incremental=True) -> sweep() equals the oracle's sweep of the host
    inference_datasets (which the block-bordered inverse keeps a complete, uploadable state)."""
    m = init_bo(SafeOpt.BO, n=14, grid=(60, 50))
    first = m.sweep()
    X, std = m.Batch(4)
    assert 1 <= len(X) <= 4
    Y = np.array([m.calculate_plant_outputs(x) for x in X])
    m.add_samples(X, Y, incremental=True)
    assert m.n_point == 14 + len(X) and m.inference_datasets["invKopt"][0].shape == (m.n_point, m.n_point)
    second = m.sweep()
    assert second is not first
    pts = oracle.grid_points(mb.box(2)[:, 0], mb.box(2)[:, 1], [60, 50])
    ref = oracle.safeopt_sweep(pts, m.inference_datasets, 3.0)
    assert second["minimizer_index"] == ref["minimizer_index"] and second["count_S"] == int(ref["S"].sum())
    assert second["minimizer_std"] == pytest.approx(ref["minimizer_std"], rel=1e-7)
    mean, var = m.GP_inference(pts[::37], None)
    om, ov = oracle.gp_inference(pts[::37], m.inference_datasets)
    assert np.max(np.abs(mean - om)) < 1e-8 and np.max(np.abs(var - ov)) < 1e-8


def test_a_window_over_blocks_of_three():
    """window = 14 over several blocks of 3 keeps n_point = 14, with sweeps equal to the oracle's on the host state."""
    m = init_bo(SafeOpt.BO, n=12, grid=(60, 50))
    pts = oracle.grid_points(mb.box(2)[:, 0], mb.box(2)[:, 1], [60, 50])
    rng = np.random.default_rng(6)
    for step in range(4):
        X = np.array([1.4, -0.8]) + 0.25 * rng.uniform(-1, 1, size=(3, 2))
        m.add_samples(X, np.array([m.calculate_plant_outputs(x) for x in X]), window=14)
        assert m.n_point == min(14, 12 + 3 * (step + 1)) and m.engine.n == m.n_point and np.array_equal(m.X[-3:], X)
        res = m.sweep()
        ref = oracle.safeopt_sweep(pts, m.inference_datasets, 3.0)
        assert res["minimizer_index"] == ref["minimizer_index"] and res["count_S"] == int(ref["S"].sum())
    assert m.n_point == 14
