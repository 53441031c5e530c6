"""sbo_model_append over its whole range: long runs of appends that cross many 16-row padding boundaries and regrow the resident
factor, the model at SBO_MAX_N, and appends the library refuses -- which must leave the model exactly as it was.

The reference for every posterior is the model rebuilt in NumPy from all rows with the frozen normalisation and hyper-parameters
(oracle.build_invK + oracle.gp_inference)."""
import numpy as np
import pytest

import oracle
import safebo_amd
from safebo_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

TOL64, TOL32 = 1e-10, 1e-4
KERNEL = {"K1g": 3, "K1b": 4, "K1t": 5}


def _nerr(got, ref, ystd, power):
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, ystd) ** power))


def _extend(ds, xn, yn, invK=None):
    """ds with the normalised rows xn / yn appended (frozen constants) and the inverse recomputed (or given)."""
    out = dict(ds)
    out["X_norm"] = np.vstack([ds["X_norm"], np.atleast_2d(xn)])
    out["Y_norm"] = np.vstack([ds["Y_norm"], np.atleast_2d(yn)])
    out["invKopt"] = oracle.build_invK(out["X_norm"], ds["hypopt"]) if invK is None else invK
    return out


def _check_post(eng, ds, pts, tol, label):
    mean, var = eng.posterior()
    om, ov = oracle.gp_inference(pts, ds)
    em, ev = _nerr(mean, om, ds["Y_std"], 1), _nerr(var, ov, ds["Y_std"], 2)
    assert em < tol and ev < tol, (label, em, ev)


def _check_paths(eng, ds, lo, hi, count, grid_pts, list_pts, dtype, label):
    """The posterior of the resident model on every path a 2-D model can take: K1b (fp64 only) and K1g on the grid, the generic
    kernels (posterior_path 1 and 2) on a point list."""
    tol = TOL64 if dtype == "f64" else TOL32
    try:
        paths = (("K1b", 2), ("K1g", 0)) if dtype == "f64" else (("K1g", 1),)
        for name, bl in paths:
            eng.set_option("bilinear", bl)
            eng.set_grid(lo, hi, count)
            eng.posterior_run()
            assert eng.profile()["posterior_kernel"] == KERNEL[name], (label, name, eng.profile()["posterior_kernel"])
            _check_post(eng, ds, grid_pts, tol, (label, name))
    finally:
        eng.set_option("bilinear", 1)
    eng.set_points(list_pts)
    try:
        for path in (1, 2):
            eng.set_option("posterior_path", path)
            eng.posterior_run()
            # (posterior_path 1: the single-phase kernel while a 64-candidate tile of K* fits 64 KiB of LDS, the chunked one beyond)
            tile = (8 if dtype == "f64" else 4) * ((ds["X_norm"].shape[0] + 15) // 16 * 16) * 64
            assert eng.profile()["posterior_kernel"] == (2 if path == 2 or tile > 64 * 1024 else 1), (label, path)
            _check_post(eng, ds, list_pts, tol, (label, "generic", path))
    finally:
        eng.set_option("posterior_path", 0)


def _checkpoints(n0, appends, cap):
    """Append counts after which the posterior is checked: every 16th, each crossing of a 16-row padding boundary, the appends
    on either side of the factor's regrowth (n = cap -> cap + 1), and the last."""
    pts = {i for i in range(1, appends + 1) if i % 16 == 0 or (n0 + i) % 16 == 1}
    pts |= {i for i in (cap - n0, cap - n0 + 1) if 1 <= i <= appends}
    return sorted(pts | {appends})


def _first_capacity(n0):
    """model.hip: a built model's factor grows at the first append to min(SBO_MAX_N, (npad + 256 + 127) / 128 * 128) rows."""
    npad = (n0 + 15) // 16 * 16
    return min(_lib.SBO_MAX_N, (npad + 256 + 127) // 128 * 128)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n0,appends", [(1, 400), (90, 300)])
def test_long_append_runs_equal_a_rebuild(engine, n0, appends, dtype):
    """Rows appended one by one from n0 (Benoit, q = 2, frozen normalisation of config B): after every 16th append, at every
    padding boundary and around the factor's regrowth, the posterior on K1b / K1g / generic 1 / generic 2 equals the oracle of the
    model rebuilt from all rows; at the end a SafeOpt and a GoOSE sweep equal the oracle's (fp32: with the fp64 recheck)."""
    cfg = synthetic.make_config("B", n=90)
    ds0 = cfg["ds"]
    ds = dict(ds0)
    ds["X_norm"], ds["Y_norm"] = ds0["X_norm"][:n0].copy(), ds0["Y_norm"][:n0].copy()
    ds["invKopt"] = oracle.build_invK(ds["X_norm"], ds["hypopt"])
    lo, hi, count = cfg["bound"][:, 0], cfg["bound"][:, 1], [64, 72]
    grid_pts = oracle.grid_points(lo, hi, count)
    rng = np.random.default_rng(100 + n0)
    list_pts = rng.uniform(lo, hi, size=(1500, 2))
    Xnew = rng.uniform(lo, hi, size=(appends, 2))
    xn = (Xnew - ds["X_mean"]) / ds["X_std"]
    yn = (synthetic.benoit(Xnew) - ds["Y_mean"]) / ds["Y_std"]
    cap = _first_capacity(n0)
    checks = _checkpoints(n0, appends, cap)
    assert any((n0 + i) % 16 == 1 for i in checks) and (appends >= cap - n0 + 1) == (cap - n0 + 1 in checks)
    assert cap - n0 + 1 <= appends, "the run must regrow the factor once more"
    engine.set_model(ds, dtype=dtype)
    done = 0
    for i in checks:
        for j in range(done, i):
            engine.append_sample(xn[j], yn[j])
        done = i
        assert engine.n == n0 + i
        ref = _extend(ds, xn[:i], yn[:i])
        _check_paths(engine, ref, lo, hi, count, grid_pts, list_pts, dtype, (n0, i))
    # the sweeps of the final model against the oracle
    engine.set_grid(lo, hi, count)
    res = engine.sweep_safeopt(cfg["b"], want_masks=True)
    sref = oracle.safeopt_sweep(grid_pts, ref, cfg["b"])
    for k in ("S", "U", "M"):
        assert np.array_equal(engine.mask(k), sref[k]), k
    assert np.array_equal(engine.mask("G", 1), sref["G"][0])
    assert res["minimizer_index"] == sref["minimizer_index"]
    assert list(res["expander_index_c"]) == list(sref["expander_index"])
    assert (res["count_S"], res["count_U"], res["count_M"]) == (sref["S"].sum(), sref["U"].sum(), sref["M"].sum())
    assert res["count_G"][0] == sref["G"][0].sum() and sref["S"].any()
    if dtype == "f32":
        return
    g = engine.sweep_goose(cfg["b"], want_masks=True)
    gref = oracle.goose_sweep(grid_pts, ref, cfg["b"])
    assert np.array_equal(engine.mask("S"), gref["S"]) and np.array_equal(engine.mask("U"), gref["U"])
    assert np.array_equal(engine.mask("O", 1), gref["O"][0])
    assert g["safe_min_index"] == gref["safe_min_index"] and np.array_equal(g["target_index_c"], gref["target_index_c"])
    assert g["target_index"] == gref["target_index"] and g["explore_index"] == gref["explore_index"]
    assert np.array_equal(g["count_O"], gref["O"].sum(1)) and (g["count_S"], g["count_U"]) == (gref["S"].sum(), gref["U"].sum())


def test_appends_to_a_three_dimensional_model_on_the_tensor_path(engine):
    """A d = 3 model grown across padding boundaries: K1t (Chebyshev-node interpolation of 3-D grids) on a sample of the grid
    against the oracle of the rebuilt model after every crossing, and the K1t sweep's masks against K1g's."""
    d, n0, appends = 3, 60, 70
    rng = np.random.default_rng(7)
    Xall = rng.uniform(-2.0, 2.0, size=(n0 + appends, d))
    Yall = np.stack([np.sum(Xall ** 2, axis=1) + np.sin(2.0 * Xall[:, 0]), 3.0 - 0.5 * np.sum(Xall ** 2, axis=1) + Xall[:, 1]], axis=1)
    ds = synthetic.make_dataset(Xall[:n0], Yall[:n0], synthetic.default_hypopt(d, 2, log_ell=-0.5))
    xn = (Xall[n0:] - ds["X_mean"]) / ds["X_std"]
    yn = (Yall[n0:] - ds["Y_mean"]) / ds["Y_std"]
    lo, hi, count = np.full(d, -2.0), np.full(d, 2.0), [160, 160, 168]
    total = int(np.prod(count))
    idx = np.unique(np.concatenate([rng.integers(0, total, size=3000), [0, total - 1, count[0] - 1, total - count[0]]]))
    axes = oracle.grid_axes(lo, hi, count)
    sub = np.empty((idx.size, d))
    f = idx.copy()
    for a in range(d):
        sub[:, a] = axes[a][f % count[a]]
        f //= count[a]
    engine.set_model(ds)
    done = 0
    for i in [i for i in range(1, appends + 1) if (n0 + i) % 16 == 1] + [appends]:
        for j in range(done, i):
            engine.append_sample(xn[j], yn[j])
        done = i
        ref = _extend(ds, xn[:i], yn[:i])
        engine.set_grid(lo, hi, count)
        mean, var = engine.posterior()
        assert engine.profile()["posterior_kernel"] == KERNEL["K1t"], i
        om, ov = oracle.gp_inference(sub, ref)
        assert _nerr(mean[idx], om, ref["Y_std"], 1) < TOL64 and _nerr(var[idx], ov, ref["Y_std"], 2) < TOL64, i
    res_t = engine.sweep_safeopt(2.0, want_masks=True, posterior_ready=True)
    masks_t = [engine.mask(k) for k in ("S", "U", "M")]
    try:
        engine.set_option("tensor_cheb", 0)
        engine.set_grid(lo, hi, count)
        res_g = engine.sweep_safeopt(2.0, want_masks=True)
        assert engine.profile()["posterior_kernel"] == KERNEL["K1g"]
        masks_g = [engine.mask(k) for k in ("S", "U", "M")]
    finally:
        engine.set_option("tensor_cheb", 1)
    for a, b in zip(masks_t, masks_g):
        assert np.array_equal(a, b)
    for k in ("minimizer_index", "count_S", "count_U", "count_M"):
        assert res_t[k] == res_g[k], k


def test_append_up_to_capacity_then_refused(engine):
    """From n = 2040 (noise well above the floor: the n = 2048 oracle stays sharp) eight appends reach SBO_MAX_N; the ninth is
    refused with SBO_E_UNSUPPORTED and the model still equals the n = 2048 oracle, posterior and sweep."""
    n0, N = 2040, _lib.SBO_MAX_N
    cfg = synthetic.make_config("B", n=N, seed=5)
    hyp = synthetic.default_hypopt(2, 2, log_sn=-1.0)
    full = synthetic.make_dataset(cfg["X"], cfg["Y"], hyp)
    ds = dict(full)
    ds["X_norm"], ds["Y_norm"] = full["X_norm"][:n0], full["Y_norm"][:n0]
    ds["invKopt"] = oracle.build_invK(ds["X_norm"], hyp)
    engine.set_model(ds, use_invK=False)
    for j in range(n0, N):
        engine.append_sample(full["X_norm"][j], full["Y_norm"][j])
    assert engine.n == N
    lo, hi, count = cfg["bound"][:, 0], cfg["bound"][:, 1], [40, 36]
    pts = oracle.grid_points(lo, hi, count)
    engine.set_grid(lo, hi, count)
    before = engine.posterior()
    with pytest.raises(safebo_amd.SafeBOError) as ei:
        engine.append_sample(full["X_norm"][0] * 0.5, full["Y_norm"][0])
    assert ei.value.code == _lib.SBO_E_UNSUPPORTED
    assert engine.n == N
    engine.set_grid(lo, hi, count)
    mean, var = engine.posterior()
    assert np.array_equal(mean, before[0]) and np.array_equal(var, before[1])
    om, ov = oracle.gp_inference(pts, full)
    assert _nerr(mean, om, full["Y_std"], 1) < TOL64 and _nerr(var, ov, full["Y_std"], 2) < TOL64
    res = engine.sweep_safeopt(cfg["b"], want_masks=True, posterior_ready=True)
    sref = oracle.safeopt_sweep(pts, full, cfg["b"], mean_var=(om, ov))
    for k in ("S", "U", "M"):
        assert np.array_equal(engine.mask(k), sref[k]), k
    assert res["minimizer_index"] == sref["minimizer_index"]


# ---------------------------------------------------------------------------------------------- refused appends
def _refusal_model():
    """q = 2 on [-2, 2]^2 plus one isolated observation x_iso far outside the swept box.  Output 1 gets the caller's invK of
    D K D, where D scales x_iso's row by 1/2: a consistent model everywhere the grid looks (x_iso's covariance with any grid point
    is below 1e-9), but a new observation at x_iso has k^T invK k ~ 4 sf2 > kappa for output 1 (s <= 0) while output 0 accepts it."""
    rng = np.random.default_rng(11)
    X = np.vstack([rng.uniform(-2.0, 2.0, size=(63, 2)), [[6.0, 6.0]]])
    Y = synthetic.benoit(X)
    ds = synthetic.make_dataset(X, Y, synthetic.default_hypopt(2, 2))
    dvec = np.ones(X.shape[0])
    dvec[-1] = 0.5
    ds["invKopt"] = [ds["invKopt"][0], ds["invKopt"][1] / np.outer(dvec, dvec)]
    return ds


def _kvec(ds, xn, o):
    d = ds["X_norm"].shape[1]
    h = ds["hypopt"][:, o]
    return np.exp(2 * h[d]) * np.exp(-0.5 * np.sum((ds["X_norm"] - xn) ** 2 / np.exp(2 * h[:d]), axis=1))


def _kappa(ds, o):
    d = ds["X_norm"].shape[1]
    h = ds["hypopt"][:, o]
    return np.exp(2 * h[d]) + np.exp(2 * h[d + 1]) + float(np.finfo(np.float32).eps)


def _snapshot(eng, lo, hi, count, b):
    """What the resident model gives, bit for bit: n, the posterior on a fresh grid on K1b and on K1g, a full SafeOpt sweep."""
    out = {"n": eng.n}
    try:
        for name, bl in (("K1b", 2), ("K1g", 0)):
            eng.set_option("bilinear", bl)
            eng.set_grid(lo, hi, count)
            eng.posterior_run()
            assert eng.profile()["posterior_kernel"] == KERNEL[name]
            out[name] = eng.posterior()
    finally:
        eng.set_option("bilinear", 1)
    eng.set_grid(lo, hi, count)
    eng.sweep_safeopt(b)                                  # (the model's first sweep on this grid: K1i)
    out["sweep"] = eng.sweep_safeopt(b, want_masks=True)  # (the second: K1b's plan)
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


BAD_INPUTS = [("x", 0, np.nan), ("x", 1, np.inf), ("x", 0, -np.inf), ("y", 0, np.nan), ("y", 1, np.nan), ("y", 0, np.inf)]


@pytest.mark.parametrize("trigger", ["s_nonpositive"] + [f"{w}{i}_{v}" for w, i, v in BAD_INPUTS])
def test_a_refused_append_changes_nothing(engine, trigger):
    """A refused append (non-finite input: ValueError before anything is touched; s <= 0 on one output: ValueError after the
    device computed every output's update) leaves n, the posterior on K1b and K1g and a full sweep bit for bit as they were.
    A valid append afterwards equals the oracle of the model plus that one row."""
    ds = _refusal_model()
    lo, hi, count, b = np.array([-2.0, -2.0]), np.array([2.0, 2.0]), [64, 66], 2.0
    x_iso = ds["X_norm"][-1]
    # the margin of the trigger, in NumPy: output 0 accepts the new row at x_iso, output 1 refuses it
    s = [_kappa(ds, o) - _kvec(ds, x_iso, o) @ ds["invKopt"][o] @ _kvec(ds, x_iso, o) for o in range(2)]
    assert s[0] > 0.01 and s[1] < -0.5 * _kappa(ds, 1), s
    pts = oracle.grid_points(lo, hi, count)
    xg = (pts - ds["X_mean"]) / ds["X_std"]
    assert np.max(np.exp(-0.5 * np.sum((xg - x_iso) ** 2 / np.exp(2 * ds["hypopt"][:2, 1]), axis=1))) < 1e-9
    engine.set_model(ds)
    before = _snapshot(engine, lo, hi, count, b)
    _check_post_arrays(before["K1b"], ds, pts)
    y_ok = np.array([0.1, 0.2])
    if trigger == "s_nonpositive":
        x_bad, y_bad = x_iso.copy(), y_ok
    else:
        which, i, v = next((w, i, v) for w, i, v in BAD_INPUTS if f"{w}{i}_{v}" == trigger)
        x_bad, y_bad = np.array([0.3, -0.2]), y_ok.copy()
        (x_bad if which == "x" else y_bad)[i] = v
    with pytest.raises(ValueError):
        engine.append_sample(x_bad, y_bad)
    _assert_same(before, _snapshot(engine, lo, hi, count, b))
    # one valid append: the oracle is the bordered inverse of the caller's (inconsistent) matrices
    x_new = np.array([0.25, -0.4])
    engine.append_sample(x_new, y_ok)
    assert engine.n == ds["X_norm"].shape[0] + 1
    invK = []
    for o in range(2):
        k = _kvec(ds, x_new, o)
        Kimp = np.linalg.inv(ds["invKopt"][o])
        invK.append(np.linalg.inv(np.block([[Kimp, k[:, None]], [k[None, :], np.array([[_kappa(ds, o)]])]])))
    ref = _extend(ds, x_new, y_ok, invK=invK)
    try:
        engine.set_option("bilinear", 2)
        engine.set_grid(lo, hi, count)
        engine.posterior_run()
        assert engine.profile()["posterior_kernel"] == KERNEL["K1b"]
        _check_post_arrays(engine.posterior(), ref, pts)
        engine.set_option("bilinear", 0)
        engine.set_grid(lo, hi, count)
        _check_post_arrays(engine.posterior(), ref, pts)
    finally:
        engine.set_option("bilinear", 1)


def _check_post_arrays(mv, ds, pts):
    om, ov = oracle.gp_inference(pts, ds)
    em, ev = _nerr(mv[0], om, ds["Y_std"], 1), _nerr(mv[1], ov, ds["Y_std"], 2)
    assert em < TOL64 and ev < TOL64, (em, ev)


def test_refused_append_on_an_fp32_model_with_its_fp64_twin(engine):
    """fp32 model (with the fp64 twin of the recheck): a refused append leaves the fp32 posterior and the rechecked sweep as they
    were, and the next valid append still gives the sweep of the fp64 oracle."""
    ds = _refusal_model()
    lo, hi, count, b = np.array([-2.0, -2.0]), np.array([2.0, 2.0]), [64, 66], 2.0
    pts = oracle.grid_points(lo, hi, count)
    engine.set_model(ds, dtype="f32")
    engine.set_grid(lo, hi, count)
    m0, v0 = engine.posterior()
    r0 = engine.sweep_safeopt(b, want_masks=True, posterior_ready=True)
    k0 = [engine.mask(k) for k in ("S", "U", "M")]
    with pytest.raises(ValueError):
        engine.append_sample(ds["X_norm"][-1], np.array([0.1, 0.2]))
    assert engine.n == ds["X_norm"].shape[0]
    engine.set_grid(lo, hi, count)
    m1, v1 = engine.posterior()
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    r1 = engine.sweep_safeopt(b, want_masks=True, posterior_ready=True)
    for k in r0:
        assert np.array_equal(np.asarray(r0[k]), np.asarray(r1[k])), k
    for a, c in zip(k0, [engine.mask(k) for k in ("S", "U", "M")]):
        assert np.array_equal(a, c)
    # a consistent model for the valid append: output 1's matrix as the data give it
    ds_ok = dict(ds)
    ds_ok["invKopt"] = oracle.build_invK(ds["X_norm"], ds["hypopt"])
    engine.set_model(ds_ok, dtype="f32")
    x_new, y_new = np.array([0.25, -0.4]), np.array([0.1, 0.2])
    with pytest.raises(ValueError):
        engine.append_sample(np.array([np.nan, 0.0]), y_new)
    engine.append_sample(x_new, y_new)
    ref = _extend(ds_ok, x_new, y_new)
    engine.set_grid(lo, hi, count)
    res = engine.sweep_safeopt(b, want_masks=True)
    sref = oracle.safeopt_sweep(pts, ref, b)
    for k in ("S", "U", "M"):
        assert np.array_equal(engine.mask(k), sref[k]), k
    assert res["minimizer_index"] == sref["minimizer_index"]
