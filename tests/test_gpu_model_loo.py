"""sbo_model_loo over its range: every size at which the column-sum kernel changes its shape (16-row padding, 64-column strips,
64-row chunks, SBO_MAX_N), every model source and output count, factors an append has grown or a removal has swapped, a true
leave-one-out on the device, read-only and bit-reproducible calls, a planted outlier, an fp32 model, refusals and the host classes.

The reference is the NumPy statement from the inverse (model_loo.loo_from_invK), normalised units; residuals are compared
absolutely, variances relatively, logdet / lpd / nll against max(1, |value|), all at TOL64 = 1e-10 (the NumPy routes among
themselves agree to 4e-13, tests/test_model_loo_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import oracle
import safebo_amd
from safebo_amd import SafeOpt, _lib, synthetic

import model_loo as ml
import model_remove as mr
from model_loo import TOL64

pytestmark = pytest.mark.gpu

KEYS = {"mean", "var", "z", "logdet", "lpd", "z_max", "z_argmax", "outside", "nll"}


def _config_b(n, log_sn=None):
    """Config B's data at n rows (seed 5); n < 3 takes the first rows of the 90-row dataset so that the constants stay finite."""
    if n < 3:
        ds0 = synthetic.make_config("B", n=90, seed=5)["ds"]
        return mr.with_rows(ds0, ds0["X_norm"][:n], ds0["Y_norm"][:n])
    cfg = synthetic.make_config("B", n=n, seed=5)
    if log_sn is None:
        return cfg["ds"]
    return synthetic.make_dataset(cfg["X"], cfg["Y"], synthetic.default_hypopt(2, 2, log_sn=log_sn))


def _bits(d):
    return {k: np.asarray(v).copy() for k, v in d.items()}


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


# ------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("n", [1, 2, 16, 17, 63, 64, 65, 127, 128, 129, 130, 300, 1040, 2048])
def test_every_shape_of_the_column_sums(engine, n):
    """q = 2, fp64: one row, the 16-row padding (16 | 17), the 64-column strip and 64-row chunk edges (63 | 64 | 65, 127 | 128 | 129),
    partial last strips (130, 300, 1040) and SBO_MAX_N.  log_sn = -1 from n = 300 up keeps the oracle sharp."""
    assert ml.STRIP == 64 and ml.ROWS == 64 and _lib.SBO_MAX_N == 2048
    ds = _config_b(n, log_sn=-1.0 if n >= 300 else None)
    engine.set_model(ds, use_invK=n < 300)
    assert engine.n == n
    ml.check_loo(engine, ds, TOL64, n)


@pytest.mark.parametrize("q", [1, 3])
def test_other_output_counts(engine, q):
    """q = 1 and q = 3 with different hyper-parameters per output (n = 40)."""
    rng = np.random.default_rng(60 + q)
    lo, hi = np.array([-.6, -1.0]), np.array([1.5, 1.0])
    X = rng.uniform(lo, hi, size=(40, 2))
    Y = np.column_stack([synthetic.benoit(X), np.sin(2.0 * X[:, 0]) - X[:, 1]])[:, :q]
    hyp = synthetic.default_hypopt(2, q)
    variants = [synthetic.default_hypopt(2, 1, log_ell=-0.3, log_sn=-1.5)[:, 0], synthetic.default_hypopt(2, 1, log_ell=-0.7, log_sf=0.2)[:, 0]]
    for o in range(1, q):
        hyp[:, o] = variants[o - 1]
    if q == 1:
        hyp[:, 0] = variants[0]
    ds = synthetic.make_dataset(X, Y, hyp)
    engine.set_model(ds)
    assert engine.q == q
    ml.check_loo(engine, ds, TOL64, q)


# ------------------------------------------------------------------------------------------ 2. model sources
@pytest.mark.parametrize("source", ["invK", "hyper", "fit"])
def test_every_model_source(engine, source):
    """n = 40 on a model built from the caller's invK, from the hyper-parameters, and by sbo_model_fit (the tiny DE of the removal
    tests; noise box [-2.5, -1.5] so that the oracle stays sharp)."""
    from scipy.stats import qmc
    cfg = synthetic.make_config("B", n=90)
    ds0 = cfg["ds"]
    ds = mr.with_rows(ds0, ds0["X_norm"][:40], ds0["Y_norm"][:40])
    engine.set_grid(cfg["bound"][:, 0], cfg["bound"][:, 1], [64, 72])
    if source == "fit":
        box = np.array([[-1.5, 1.5]] * 3 + [[-2.5, -1.5]])
        pop = qmc.scale(qmc.LatinHypercube(4, seed=7).random(20), box[:, 0], box[:, 1])
        data = {k: ds[k] for k in ("X_mean", "X_std", "Y_mean", "Y_std", "X_norm", "Y_norm")}
        rep = engine.model_fit(data, box, pop, seed=7, maxiter=8, tol=0.01)
        ds = dict(ds)
        ds["hypopt"] = rep["hypopt"]
        ds["invKopt"] = oracle.build_invK(ds["X_norm"], ds["hypopt"])
    else:
        engine.set_model(ds, use_invK=source == "invK")
    ml.check_loo(engine, ds, TOL64, source)


def test_a_deferred_factor_is_waited_for(engine):
    """A caller's invK at n = 300 on a K1b-capable grid leaves the factorisation to a side stream (option chol_async); the first
    consumer of the factor is this call."""
    cfg = synthetic.make_config("B", n=300, seed=5)
    ds = synthetic.make_dataset(cfg["X"], cfg["Y"], synthetic.default_hypopt(2, 2, log_sn=-1.0))
    engine.set_grid(cfg["bound"][:, 0], cfg["bound"][:, 1], [64, 72])
    engine.set_model(ds)
    ml.check_loo(engine, ds, TOL64, "deferred")


# ------------------------------------------------------------------------------------------ 3. changed factors
def test_after_an_append_a_removal_and_a_sliding_window(engine):
    """n = 90: after an append that grew the factor (leading dimension > n), after a removal (the spare buffers swapped in) and
    after 50 steps of remove-oldest + append the diagnostics equal the oracle's of the rows the model then holds."""
    cfg = synthetic.make_config("B", n=90)
    ds0 = cfg["ds"]
    lo, hi = cfg["bound"][:, 0], cfg["bound"][:, 1]
    engine.set_model(mr.with_rows(ds0, ds0["X_norm"][:89], ds0["Y_norm"][:89]))
    engine.append_sample(ds0["X_norm"][89], ds0["Y_norm"][89])
    ml.check_loo(engine, ds0, TOL64, "grown")
    engine.remove_sample(13)
    ml.check_loo(engine, mr.without(ds0, 13), TOL64, "removed")
    engine.set_model(ds0)
    rng = np.random.default_rng(301)
    Xnew = rng.uniform(lo, hi, size=(50, 2))
    xn = (Xnew - ds0["X_mean"]) / ds0["X_std"]
    yn = (synthetic.benoit(Xnew) - ds0["Y_mean"]) / ds0["Y_std"]
    for t in range(50):
        engine.remove_sample(0)
        engine.append_sample(xn[t], yn[t])
    Xw, Yw = np.vstack([ds0["X_norm"], xn]), np.vstack([ds0["Y_norm"], yn])
    assert engine.n == 90
    ml.check_loo(engine, mr.with_rows(ds0, Xw[50:], Yw[50:]), TOL64, "window")


# ------------------------------------------------------------------------------------------ 4. true leave-one-out on the device
@pytest.mark.parametrize("i", [0, 13, 39])
def test_against_a_removal_and_a_posterior_on_the_device(engine, i):
    """n = 40: resid[i] and var[i] equal what the device itself gives when the observation really leaves -- remove_sample(i) on a
    fresh copy of the model, the posterior at x_i, plus the noise the stored inverse carries -- in normalised units."""
    cfg = synthetic.make_config("B", n=90)
    ds0 = cfg["ds"]
    ds = mr.with_rows(ds0, ds0["X_norm"][:40], ds0["Y_norm"][:40])
    engine.set_model(ds)
    got = engine.model_loo(3.0)
    engine.set_model(ds)
    engine.remove_sample(i)
    engine.set_points(ds["X_norm"][i:i + 1] * ds["X_std"] + ds["X_mean"])
    mean, var = engine.posterior()
    e = ds["Y_norm"][i] - (mean[0] - ds["Y_mean"]) / ds["Y_std"]
    v = var[0] / ds["Y_std"] ** 2 + ml.noise(ds)
    err_e, err_v = float(np.max(np.abs(got["resid"][i] - e))), float(np.max(np.abs(got["var"][i] / v - 1.0)))
    print(i, err_e, err_v)
    assert err_e < TOL64 and err_v < TOL64, (i, err_e, err_v)


# ------------------------------------------------------------------------------------------ 5. read-only and reproducible
def _snapshot(eng, lo, hi, count, b):
    """What the resident model gives, bit for bit (tests/test_gpu_model_remove.py): the posterior on a fresh grid on K1b and on K1g, a
    full SafeOpt sweep and its masks."""
    out = {}
    try:
        for name, bl in (("K1b", 2), ("K1g", 0)):
            eng.set_option("bilinear", bl)
            eng.set_grid(lo, hi, count)
            eng.posterior_run()
            assert eng.profile()["posterior_kernel"] == mr.KERNEL[name], name
            out[name] = eng.posterior()
    finally:
        eng.set_option("bilinear", 1)
    eng.set_grid(lo, hi, count)
    eng.sweep_safeopt(b)
    out["sweep"] = eng.sweep_safeopt(b, want_masks=True)
    out["masks"] = [eng.mask(k) for k in ("S", "U", "M")] + [eng.mask("G", 1)]
    return out


def _assert_same(a, b):
    for name in ("K1b", "K1g"):
        for x, y in zip(a[name], b[name]):
            assert np.array_equal(x, y) and np.array_equal(x.view(np.uint64), y.view(np.uint64)), name
    for k, v in a["sweep"].items():
        assert np.array_equal(np.asarray(v), np.asarray(b["sweep"][k])), k
    for x, y in zip(a["masks"], b["masks"]):
        assert np.array_equal(x, y)


def test_the_call_changes_nothing_and_repeats_bit_for_bit(engine):
    """n = 90: the posterior on a 64 x 72 grid (K1b and K1g) and a SafeOpt sweep with its masks are identical before and after the
    call; two calls return identical bits; so does a call after an unrelated grid change and sweep."""
    cfg = synthetic.make_config("B", n=90)
    ds = cfg["ds"]
    lo, hi, count, b = cfg["bound"][:, 0], cfg["bound"][:, 1], [64, 72], cfg["b"]
    engine.set_model(ds)
    before = _snapshot(engine, lo, hi, count, b)
    first = _bits(engine.model_loo(b, ds["Y_norm"]))
    second = _bits(engine.model_loo(b, ds["Y_norm"]))
    _same_bits(first, second)
    _assert_same(before, _snapshot(engine, lo, hi, count, b))
    engine.set_grid(lo, hi, [33, 47])
    engine.sweep_goose(b)
    _same_bits(first, _bits(engine.model_loo(b, ds["Y_norm"])))
    err = ml.errors(first, ml.loo_from_invK(ds))
    assert all(v < TOL64 for v in err.values()), err


# ------------------------------------------------------------------------------------------ 6. planted outlier
def test_a_planted_outlier_is_found(engine):
    """n = 90 with Y[37, 1] += 6 Y_std[1] before normalisation.  Once the oracle itself shows the outlier as the arg-max of |z| of
    output 1 with a gap above 1e-6 to the runner-up, and no |z_i| within 1e-6 of b = 3, the device's z_argmax and outside equal the
    oracle's exactly and z_max within TOL64."""
    b, j = 3.0, 37
    cfg = synthetic.make_config("B", n=90, seed=5)
    Y = cfg["Y"].copy()
    Y[j, 1] += 6.0 * np.std(cfg["Y"][:, 1])
    ds = synthetic.make_dataset(cfg["X"], Y, synthetic.default_hypopt(2, 2))
    ref = ml.loo_from_invK(ds)
    az = np.abs(ref["z"])
    zmax, zarg, outside = ml.summaries_of(ref["z"], b)
    assert zarg[1] == j, zarg
    for o in range(2):
        top = np.sort(az[:, o])[-2:]
        assert top[1] - top[0] > 1e-6, (o, top)
    assert np.min(np.abs(az - b)) >= 1e-6
    engine.set_model(ds)
    got = engine.model_loo(b, ds["Y_norm"])
    assert np.array_equal(got["z_argmax"], zarg) and np.array_equal(got["outside"], outside), (got["z_argmax"], got["outside"])
    assert np.max(np.abs(got["z_max"] - zmax)) < TOL64
    err = ml.errors(got, ref)
    assert all(v < TOL64 for v in err.values()), err


# ------------------------------------------------------------------------------------------ 7. fp32
def test_an_fp32_model_keeps_fp64_diagnostics(engine):
    """Config B at n = 90 as an fp32 model: the factor and alpha the call reads are built in fp64 for every model dtype, so the
    results meet TOL64 (far inside the project's fp32 bar TOL32 = 1e-4)."""
    ds = synthetic.make_config("B", n=90)["ds"]
    engine.set_model(ds, dtype="f32")
    got, _ = ml.check_loo(engine, ds, TOL64, "f32")
    assert got["resid"].dtype == np.float64 and got["var"].dtype == np.float64
    assert TOL64 < ml.TOL32


# ------------------------------------------------------------------------------------------ 8. refusals
def test_a_call_without_a_model_is_refused():
    with safebo_amd.SweepEngine(0) as eng:
        res = _lib.ModelLooResult()
        assert eng._lib.sbo_model_loo(eng._ctx, 3.0, None, None, C.byref(res)) == _lib.SBO_E_NO_MODEL
        with pytest.raises(safebo_amd.SafeBOError) as ei:
            eng.model_loo(3.0)
        assert ei.value.code == _lib.SBO_E_NO_MODEL


def test_refused_calls_leave_the_next_one_intact(engine):
    """b = -1, NaN and inf are SBO_E_INVALID; all three output pointers NULL is accepted; after each the next valid call returns
    the expected values."""
    ds = _config_b(40)
    engine.set_model(ds)
    want, _ = ml.check_loo(engine, ds, TOL64, "first")
    want = _bits(want)
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        res = _lib.ModelLooResult()
        assert engine._lib.sbo_model_loo(engine._ctx, bad, None, None, C.byref(res)) == _lib.SBO_E_INVALID, bad
        with pytest.raises(ValueError):
            engine.model_loo(bad)
        _same_bits(want, _bits(engine.model_loo(3.0, ds["Y_norm"])))
    assert engine._lib.sbo_model_loo(engine._ctx, 3.0, None, None, None) == _lib.SBO_OK
    _same_bits(want, _bits(engine.model_loo(3.0, ds["Y_norm"])))
    # each output on its own
    res = _lib.ModelLooResult()
    var = np.empty((40, 2))
    assert engine._lib.sbo_model_loo(engine._ctx, 3.0, None, var.ctypes.data_as(C.c_void_p), C.byref(res)) == _lib.SBO_OK
    assert np.array_equal(var, want["var"]) and (res.n, res.q) == (40, 2) and res.z_argmax[0] == want["z_argmax"][0]
    with pytest.raises(ValueError):
        engine.model_loo(3.0, ds["Y_norm"][:-1])


# ------------------------------------------------------------------------------------------ 9. host classes
def _grid_posterior(m):
    pts = oracle.grid_points(mr.BOUND[:, 0], mr.BOUND[:, 1], [20, 18])
    return m.GP_inference(pts, None)


def test_loo_of_a_host_class_in_physical_units():
    m = mr.init_bo(SafeOpt.BO, n=12)
    got = m.loo()
    assert set(got) == KEYS
    ds = m.inference_datasets
    ref = ml.loo_from_invK(ds)
    assert np.max(np.abs(got["mean"] - (m.Y - ref["resid"] * m.Y_std)) / np.maximum(1.0, m.Y_std)) < TOL64
    assert np.max(np.abs(got["var"] / (ref["var"] * m.Y_std ** 2) - 1.0)) < TOL64
    assert np.max(np.abs(got["z"] - ref["z"])) < TOL64 * max(1.0, np.max(np.abs(ref["z"])))
    for k in ("logdet", "lpd", "nll"):
        assert np.max(np.abs(got[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k]))) < TOL64, k
    _, _, outside = ml.summaries_of(got["z"], 3.0)
    assert np.array_equal(got["outside"], outside)                       # (b defaults to the instance's b = 3)
    _, _, outside1 = ml.summaries_of(got["z"], 0.5)
    assert np.array_equal(m.loo(b=0.5)["outside"], outside1)


def test_refit_when_false_is_the_plain_incremental_path():
    a, c = mr.init_bo(SafeOpt.BO, n=12), mr.init_bo(SafeOpt.BO, n=12)
    x = np.array([1.35, -0.75])
    y = a.calculate_plant_outputs(x)
    seen = []
    a.add_sample(x, y, incremental=True, refit_when=lambda d: seen.append(d) or False)
    c.add_sample(x, y, incremental=True)
    assert len(seen) == 1 and set(seen[0]) == KEYS and seen[0]["z"].shape == (13, 2)
    assert np.array_equal(a.hypopt, c.hypopt) and np.array_equal(a.X_norm, c.X_norm) and a.n_point == c.n_point == 13
    for g, w in zip(_grid_posterior(a), _grid_posterior(c)):
        assert np.array_equal(g, w)


def test_refit_when_true_is_the_default_path():
    a, c = mr.init_bo(SafeOpt.BO, n=12), mr.init_bo(SafeOpt.BO, n=12)
    x = np.array([1.35, -0.75])
    y = a.calculate_plant_outputs(x)
    seen = []
    a.add_sample(x, y, incremental=True, refit_when=lambda d: seen.append(d) or True)
    c.add_sample(x, y)
    assert len(seen) == 1 and set(seen[0]) == KEYS
    assert np.array_equal(a.X_norm, c.X_norm) and np.array_equal(a.Y_norm, c.Y_norm) and np.array_equal(a.hypopt, c.hypopt)
    assert np.array_equal(a.X_mean, c.X_mean) and np.array_equal(a.Y_std, c.Y_std)
    (gm, gv), (wm, wv) = _grid_posterior(a), _grid_posterior(c)
    assert mr.nerr(gm, wm, a.Y_std, 1) < TOL64 and mr.nerr(gv, wv, a.Y_std, 2) < TOL64
    assert mr.nerr(a.loo()["mean"], c.loo()["mean"], a.Y_std, 1) < TOL64
