"""The robust (StableOpt) sweep on the device: sbo_model_set_prior, sbo_sweep_robust, sbo_robust_get and the StableOpt host class,
against NumPy reductions of the device's own posterior (bitwise), the exact kernel, and the zero-prior oracle of robust_oracle.py."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import oracle  # noqa: E402
import robust_oracle  # noqa: E402
import safebo_amd  # noqa: E402
from safebo_amd import StableOpt, _lib  # noqa: E402

pytestmark = pytest.mark.gpu

B = 2.0


def make_model(d, q, n, seed, shift=(0.0, 1.2, 0.9)):
    """A smooth d-input model of q outputs on [-1, 2] x [2, 4] (x more disturbance axes on [2, 4]): the objective is W-shaped in
    (xc, d), the constraints cross zero inside the box.  Fixed hyper-parameters, the caller's invK."""
    rng = np.random.default_rng(seed)
    lo = np.array([-1.0] + [-1.0] * (d - 2) + [2.0])
    hi = np.array([2.0] + [2.0] * (d - 2) + [4.0])
    X = lo + (hi - lo) * rng.uniform(size=(n, d))
    w = robust_oracle.w_shape(X[:, 0], X[:, -1]) + 0.3 * np.sum(X[:, 1:-1] ** 2, axis=1)
    outs = [w]
    for c in range(1, q):
        outs.append(shift[c] - 0.8 * X[:, 0] ** 2 + 0.2 * np.sin(2.0 * X[:, -1]) - 0.2 * c * np.sum(X[:, 1:-1], axis=1))
    Y = np.stack(outs, axis=1)
    hyp = np.zeros((d + 2, q))
    hyp[:d] = -0.2
    hyp[d] = 0.2
    hyp[d + 1] = -3.0
    return oracle.make_inference_dataset(X, Y, hyp), lo, hi


@pytest.fixture
def exact(engine):
    engine.set_option("bilinear", 0)
    engine.set_option("tensor_cheb", 0)
    yield engine
    engine.set_option("bilinear", 1)
    engine.set_option("tensor_cheb", 1)


def _tol(ds):
    return 1e-9 * max(1.0, float(np.max(np.abs(ds["Y_std"]))) ** 2)


# ---- 1. the prior ------------------------------------------------------------------------------------------------------
def test_set_prior_null_equals_set_list_and_priors_do_not_leak(engine):
    ds, lo, hi = make_model(2, 3, 40, 1)
    count = [96, 64]
    engine.set_grid(lo, hi, count)
    engine.set_model(ds)
    engine.sweep_safeopt(B)
    m_list, v_list = engine.posterior()
    engine.set_model(ds, mean_prior=None)
    engine.sweep_safeopt(B)
    assert np.array_equal(engine.posterior()[0], m_list)
    # sbo_model_set_prior(NULL) through the raw ABI: bitwise the same as sbo_model_set_list
    import ctypes as C
    lib = _lib.load()
    arrs = [np.ascontiguousarray(ds[k], dtype=np.float64) for k in ("X_mean", "X_std", "Y_mean", "Y_std", "X_norm", "Y_norm", "hypopt")]
    parts = [np.ascontiguousarray(a) for a in ds["invKopt"]]
    ptrs = (C.c_void_p * 3)(*[a.ctypes.data for a in parts])
    _lib.check(lib.sbo_model_set_prior(engine._ctx, 0, b"RBF", 40, 2, 3, *[a.ctypes.data for a in arrs], ptrs, None))
    engine.sweep_safeopt(B)
    m_raw, v_raw = engine.posterior()
    assert np.array_equal(m_raw, m_list) and np.array_equal(v_raw, v_list)
    pts = oracle.grid_points(lo, hi, count)
    ref_safe = oracle.gp_inference(pts, ds)
    ref_zero = robust_oracle.gp_inference_prior(pts, ds, np.zeros(3))
    tol = _tol(ds)
    # alternate the two priors on one context, two sweeps each (K1i, then the K1b plan): each must match its own oracle
    for mp, ref in ((np.zeros(3), ref_zero), (None, ref_safe), (np.zeros(3), ref_zero)):
        engine.set_model(ds, mean_prior=mp)
        for _ in range(2):
            engine.sweep_safeopt(B)
            m, v = engine.posterior()
            assert np.max(np.abs(m - ref[0])) < tol and np.max(np.abs(v - ref[1])) < tol
    assert np.max(np.abs(ref_zero[0][:, 1:] - ref_safe[0][:, 1:])) > 1e-3      # (the priors do differ)


# ---- 2. exact kernel: bitwise against NumPy reductions of the device posterior ---------------------------------------------------
@pytest.mark.parametrize("kind", ["mean", "ucb", "lcb"])
def test_robust_arrays_bitwise_on_exact_kernel(exact, kind):
    eng = exact
    ds, lo, hi = make_model(2, 3, 30, 2)
    count = [61, 41]
    eng.set_model(ds, mean_prior=np.zeros(3))
    eng.set_grid(lo, hi, count)
    res = eng.sweep_robust(B, 1, kind)
    assert eng.profile()["posterior_kernel"] in (1, 2, 3)
    f, g = eng.robust_arrays()
    mean, var = eng.posterior()
    r = robust_oracle.robust_from_posterior(mean, var, 61, B, kind)
    assert np.array_equal(f, r["f"]) and np.array_equal(g, r["g"])
    assert (res["index"], res["worst_d_index"], res["count_safe"]) == (r["index"], r["worst_d_index"], r["count_safe"])
    assert res["value"] == r["value"] and res["count_control"] == 61 and res["count_disturbance"] == 41
    assert res["candidate_index"] == r["candidate_index"] and res["guard_band"] == 0 and res["guard_passes"] == 0
    ref = robust_oracle.robust_sweep(lo, hi, count, 1, ds, B, kind)
    assert res["index"] == ref["index"] and res["worst_d_index"] == ref["worst_d_index"]
    assert np.max(np.abs(f - ref["f"])) < _tol(ds) and np.max(np.abs(g - ref["g"])) < _tol(ds)
    axes = oracle.grid_axes(lo, hi, count)
    assert res["xc"][0] == axes[0][res["index"]] and res["worst_d"][0] == axes[1][res["worst_d_index"]]


# ---- 3. approximating kernels against the exact one -------------------------------------------------------------------------
def _robust_exact(engine, ds, lo, hi, count, nca):
    engine.set_option("bilinear", 0)
    engine.set_option("tensor_cheb", 0)
    try:
        engine.set_model(ds, mean_prior=np.zeros(ds["Y_norm"].shape[1]))
        engine.set_grid(lo, hi, count)
        return engine.sweep_robust(B, nca, "ucb")
    finally:
        engine.set_option("bilinear", 1)
        engine.set_option("tensor_cheb", 1)


@pytest.mark.parametrize("case", ["3d", "2d"])
@pytest.mark.parametrize("guard", [1, 2])
def test_default_path_matches_exact_kernel(engine, case, guard):
    if case == "3d":
        ds, lo, hi = make_model(3, 3, 60, 3)
        count, nca, sweeps = [256, 128, 128], 2, 1         # (K1t: every axis >= 64 points, >= 2^22 candidates)
    else:
        ds, lo, hi = make_model(2, 2, 40, 4)
        count, nca, sweeps = [301, 201], 1, 2
    ref = _robust_exact(engine, ds, lo, hi, count, nca)
    engine.set_option("guard_band", guard)
    try:
        engine.set_model(ds, mean_prior=np.zeros(ds["Y_norm"].shape[1]))
        engine.set_grid(lo, hi, count)
        kernels = []
        for _ in range(sweeps):
            res = engine.sweep_robust(B, nca, "ucb")
            kernels.append(engine.profile()["posterior_kernel"])
            for k in ("index", "worst_d_index", "count_safe", "count_control", "count_disturbance", "candidate_index"):
                assert res[k] == ref[k], (k, res[k], ref[k], kernels)
            assert kernels[-1] in ((5,) if case == "3d" else (6, 4)), kernels
            if guard == 2:
                assert res["guard_passes"] == 1 and res["guard_rechecks"] == int(np.prod(count))
                assert res["value"] == ref["value"]
    finally:
        engine.set_option("guard_band", 1)
    print("robust", case, "guard", guard, "kernels", kernels)


# ---- 4. the W-shape campaign of the reference's StableOpt study --------------------------------------------------------------
def test_w_shape_campaign_matches_oracle():
    z = np.load(os.path.join(HERE, "golden", "stableopt", "w_shape.npz"))
    plants = [lambda x, noise=0: (float(robust_oracle.w_shape(x[0], x[1])), 0.0)]
    bo = StableOpt.BO(plants, np.array([[-1.0, 2.0]]), np.array([[2.0, 4.0]]), B, grid=(301,), grid_d=(201,))
    bo.de_options = {"seed": 0, "maxiter": 40}
    X = z["sampled_x"].astype(np.float64)
    Y = z["sampled_output"].astype(np.float64)
    bo.GP_initialization(X, Y, "RBF", multi_hyper=1)
    lo, hi, count = [-1.0, 2.0], [2.0, 4.0], [301, 201]
    D = bo.disturbance_points()
    try:
        for step in range(16):
            if step:
                bo.add_sample(z["observed_x"][step - 1].astype(np.float64), z["observed_output"][step - 1].astype(np.float64))
            ref = robust_oracle.robust_sweep(lo, hi, count, 1, bo.inference_datasets, B, "ucb")
            xc, value = bo.Minimize_Maximise(bo.ucb)
            res = bo.robust_sweep(bo.ucb)
            assert res["index"] == ref["index"], step
            assert xc[0] == bo.control_point(ref["index"])[0]
            # (values: the suite's parity bar is 1e-10 on mean and variance; near an observation the variance is ~0 (noise bound
            # exp(-8)) and b sqrt(var) carries a variance difference dv as up to b sqrt(dv) -- indices are compared exactly)
            vtol = 1e-9 + B * np.sqrt(1e-10) * float(bo.inference_datasets["Y_std"][0])
            assert abs(value - ref["value"]) < vtol, step
            assert res["worst_d_index"] == ref["worst_d_index"], step
            d_star, worst = bo.Maximise_d_with_constraints(bo.ucb, xc)
            m, v = robust_oracle.gp_inference_prior(np.hstack((np.repeat(xc[None, :], D.shape[0], 0), D)), bo.inference_datasets, [0.0])
            u = m[:, 0] + B * np.sqrt(v[:, 0])
            assert d_star[0] == D[int(np.argmax(u)), 0] and abs(worst - u.max()) < vtol
            assert bo.Maximise_d(bo.ucb, xc, 0) == worst
            assert abs(bo.Minimise_d(bo.lcb, xc, 0) - (m[:, 0] - B * np.sqrt(v[:, 0])).min()) < vtol
    finally:
        if bo._engine is not None:
            bo._engine.close()


# ---- 5. edge cases ------------------------------------------------------------------------------------------------------------
def test_no_constraints_every_control_is_safe(engine):
    ds, lo, hi = make_model(2, 1, 25, 5)
    engine.set_model(ds, mean_prior=np.zeros(1))
    engine.set_grid(lo, hi, [37, 23])                         # (Nc = 37: not a multiple of the block size)
    res = engine.sweep_robust(B, 1, "ucb")
    f, g = engine.robust_arrays()
    assert res["count_safe"] == 37 and g.shape == (0, 37)
    ref = robust_oracle.robust_sweep(lo, hi, [37, 23], 1, ds, B, "ucb")
    assert res["index"] == ref["index"] and res["worst_d_index"] == ref["worst_d_index"]


def test_no_robust_safe_control(engine):
    ds, lo, hi = make_model(2, 2, 25, 6, shift=(0.0, -5.0))
    engine.set_model(ds, mean_prior=np.zeros(2))
    engine.set_grid(lo, hi, [50, 30])
    res = engine.sweep_robust(B, 1, "lcb")
    assert res["index"] == -1 and res["value"] == float("inf") and res["count_safe"] == 0
    assert res["worst_d_index"] == -1 and res["candidate_index"] == -1


def test_uneven_controls_and_one_disturbance_plane(engine):
    ds, lo, hi = make_model(2, 3, 30, 7)
    engine.set_model(ds, mean_prior=np.zeros(3))
    for count in ([1003, 1], [333, 7]):
        lo1, hi1 = lo.copy(), hi.copy()
        if count[1] == 1:
            hi1[1] = lo1[1]
        engine.set_grid(lo1, hi1, count)
        res = engine.sweep_robust(B, 1, "ucb")
        f, g = engine.robust_arrays()
        mean, var = engine.posterior()
        r = robust_oracle.robust_from_posterior(mean, var, count[0], B, "ucb")
        assert np.array_equal(f, r["f"]) and np.array_equal(g, r["g"])
        assert (res["index"], res["worst_d_index"], res["count_safe"]) == (r["index"], r["worst_d_index"], r["count_safe"])


def test_invalid_arguments(engine):
    ds, lo, hi = make_model(3, 2, 20, 8)
    engine.set_model(ds, mean_prior=np.zeros(2))
    engine.set_grid(lo, hi, [10, 9, 8])
    for nca in (0, 3, -1):
        with pytest.raises(ValueError):
            engine.sweep_robust(B, nca, "ucb")
    with pytest.raises(ValueError):
        engine.sweep_robust(-1.0, 1, "ucb")
    with pytest.raises(ValueError):
        engine.sweep_robust(B, 1, "var")
    engine.set_points(oracle.grid_points(lo, hi, [4, 4, 4]))
    with pytest.raises(ValueError):
        engine.sweep_robust(B, 2, "ucb")
    engine.set_model(ds, dtype="f32", use_invK=False, mean_prior=np.zeros(2))
    engine.set_grid(lo, hi, [10, 9, 8])
    with pytest.raises(safebo_amd.SafeBOError) as e:
        engine.sweep_robust(B, 2, "ucb")
    assert e.value.code == _lib.SBO_E_UNSUPPORTED


def test_robust_sweep_between_safeopt_sweeps(engine):
    """Two SafeOpt sweeps of one model (K1i, then the K1b plan) give the same results with a robust sweep between them."""
    ds, lo, hi = make_model(2, 2, 40, 9)
    engine.set_grid(lo, hi, [128, 96])
    runs = []
    for robust in (False, True):
        engine.set_model(ds)
        a = engine.sweep_safeopt(B, want_masks=True)
        Sa = engine.mask("S")
        if robust:
            engine.sweep_robust(B, 1, "ucb")
        b = engine.sweep_safeopt(B, want_masks=True)
        c = engine.sweep_safeopt(B, want_masks=True, posterior_ready=True)
        runs.append((a, Sa, b, engine.mask("S"), c))
    (a0, S0, b0, T0, c0), (a1, S1, b1, T1, c1) = runs
    assert np.array_equal(S0, S1) and np.array_equal(T0, T1)
    for x, y in ((a0, a1), (b0, b1), (c0, c1)):
        for k in ("minimizer_index", "expander_index", "count_S", "count_M", "u_star", "minimizer_std"):
            assert x[k] == y[k], k


# ---- 6. two ranks on the one GPU ---------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def test_two_ranks_equal_one_rank(engine, tmp_path):
    spec = {"d": 3, "q": 3, "n": 40, "seed": 10, "count": [40, 30, 17], "nca": 2, "b": B, "kind": "ucb"}
    port, out = _free_port(), str(tmp_path / "res.npz")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_gpu_robust_rank_worker.py"), str(r), "2", port, out, json.dumps(spec)])
             for r in range(2)]
    try:
        ds, lo, hi = make_model(3, 3, 40, 10)
        engine.set_model(ds, mean_prior=np.zeros(3))
        engine.set_grid(lo, hi, spec["count"])
        one = engine.sweep_robust(B, 2, "ucb")
        f1, g1 = engine.robust_arrays()
        codes = [p.wait(timeout=600) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert codes == [0, 0]
    two = np.load(out)
    assert np.array_equal(two["f"], f1) and np.array_equal(two["g"], g1)
    for k in ("index", "value", "worst_d_index", "candidate_index", "count_safe", "count_control", "count_disturbance"):
        assert two[k] == one[k], k
