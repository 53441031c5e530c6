"""CPU tests of the robust (StableOpt) sweep's interface: the ABI mirror, argument checks that need no device, the host class, and
the NumPy oracle of tests/robust_oracle.py against brute force."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import robust_oracle  # noqa: E402
from safebo_amd import _lib, StableOpt, GP_Robust  # noqa: E402


def test_robust_result_size_matches_c(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "safebo.h"\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu\\n", sizeof(sbo_robust_result),'
                   ' offsetof(sbo_robust_result, value), offsetof(sbo_robust_result, guard_passes)); return 0;}\n')
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off_v, off_g = (int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(_lib.RobustResult)
    assert off_v == _lib.RobustResult.value.offset and off_g == _lib.RobustResult.guard_passes.offset


def test_null_arguments_are_invalid():
    lib = _lib.load()
    res = _lib.RobustResult()
    opts = _lib.SweepOpts(2.0, 1, 0, 0, 0)
    assert lib.sbo_sweep_robust(None, C.byref(opts), 1, _lib.SBO_UCB, C.byref(res)) == _lib.SBO_E_INVALID
    assert lib.sbo_robust_get(None, None, None) == _lib.SBO_E_INVALID
    one = (C.c_double * 8)()
    assert lib.sbo_model_set_prior(None, 0, b"RBF", 1, 1, 1, one, one, one, one, one, one, one, None, None) == _lib.SBO_E_INVALID


def _w_plants():
    return [lambda x, noise=0: (float(robust_oracle.w_shape(x[0], x[1])), 0.0)]


def test_stableopt_host_class_without_gpu():
    bo = StableOpt.BO(_w_plants(), np.array([[-1.0, 2.0]]), np.array([[2.0, 4.0]]), 2.0)
    assert bo.nxc_dim == 1 and bo.nd_dim == 1
    assert isinstance(bo, GP_Robust.GP) and bo.noise_lower_bound == -8.0 and bo.mean_prior_zero
    assert bo._engine is None                                   # nothing touched the device
    with pytest.raises(ValueError):
        bo.ucb(np.array([[0.0]]), np.array([2.0]), 0)            # xc not 1-D (and not a batch of equal length)
    with pytest.raises(ValueError):
        bo.lcb(np.array([0.0]), np.array([[2.0, 3.0]]), 0)
    with pytest.raises(ValueError):
        bo.Maximise_d(lambda xc, d, i: 0.0, np.array([0.0]), 0)  # a foreign fun
    with pytest.raises(ValueError):
        bo.Minimize_Maximise(np.sin)
    out, dist = bo.calculate_plant_outputs(np.array([0.5, 3.0]))
    assert out.shape == (1,) and out[0] == pytest.approx(robust_oracle.w_shape(0.5, 3.0))
    D = bo.disturbance_points()
    assert D.shape == (101, 1) and D[0, 0] == 2.0 and D[-1, 0] == 4.0
    assert np.array_equal(bo.control_point(0), [-1.0]) and np.array_equal(bo.control_point(200), [2.0])


def test_gp_robust_fit_uses_the_wider_noise_bound():
    seen = {}
    gp = GP_Robust.GP([lambda x, n=0: 0.0])
    import safebo_amd.GP_Safe as G
    orig = G.differential_evolution

    def spy(fun, bounds=None, **kw):
        seen["bounds"] = np.asarray(bounds)
        return type("R", (), {"x": np.asarray(bounds).mean(axis=1)})()
    G.differential_evolution = spy
    try:
        X = np.linspace(0, 1, 6).reshape(3, 2)
        gp.GP_initialization(X, np.array([[0.1], [0.4], [0.2]]), "RBF", multi_hyper=1)
    finally:
        G.differential_evolution = orig
    assert seen["bounds"][-1].tolist() == [-8.0, -2.0]


def test_oracle_equals_brute_force_loops():
    rng = np.random.default_rng(3)
    nc, nd, q, b = 7, 5, 3, 2.0
    mean = rng.normal(size=(nc * nd, q))
    mean[:, 1:] += 1.5
    var = rng.uniform(0.01, 0.5, size=(nc * nd, q))
    for kind in ("mean", "ucb", "lcb"):
        r = robust_oracle.robust_from_posterior(mean, var, nc, b, kind)
        sign = {"mean": 0.0, "ucb": 1.0, "lcb": -1.0}[kind]
        best, best_i, best_d = np.inf, -1, -1
        for x in range(nc):
            fx, ax = -np.inf, -1
            safe = True
            for dd in range(nd):
                g = dd * nc + x
                v = mean[g, 0] + sign * b * np.sqrt(var[g, 0])
                if v > fx:
                    fx, ax = v, dd
                for c in range(1, q):
                    safe = safe and mean[g, c] - b * np.sqrt(var[g, c]) >= 0
            assert r["f"][x] == fx
            if safe and fx < best:
                best, best_i, best_d = fx, x, ax
        assert (r["index"], r["value"], r["worst_d_index"]) == (best_i, best, best_d), kind


def test_oracle_zero_prior_differs_from_gp_safe_prior():
    import oracle
    rng = np.random.default_rng(0)
    X = rng.uniform(size=(8, 2))
    Y = np.stack([X.sum(1), 3.0 + X[:, 0]], axis=1)
    ds = oracle.make_inference_dataset(X, Y, np.array([[0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [-3.0, -3.0]]))
    pts = rng.uniform(size=(20, 2))
    m_safe, v_safe = oracle.gp_inference(pts, ds)
    m_same, v_same = robust_oracle.gp_inference_prior(pts, ds, oracle.mean_prior(ds))
    assert np.allclose(m_safe, m_same, rtol=0, atol=1e-12) and np.allclose(v_safe, v_same, rtol=0, atol=1e-12)
    m0, v0 = robust_oracle.gp_inference_prior(pts, ds, robust_oracle.zero_prior(ds))
    assert np.array_equal(m0[:, 0], m_safe[:, 0]) and not np.allclose(m0[:, 1], m_safe[:, 1])
    assert np.array_equal(v0, v_safe)


def test_w_shape_robust_optimum():
    """min_xc max_d of the true W-shape function: -0.2961 is the robust optimum the reference's study measures its regret against."""
    xc = np.linspace(-1.0, 2.0, 3001)
    d = np.linspace(2.0, 4.0, 2001)
    F = robust_oracle.w_shape(xc[None, :], d[:, None])
    f = F.max(axis=0)
    i = int(np.argmin(f))
    assert f[i] == pytest.approx(-0.29612, abs=5e-5)
    assert xc[i] == pytest.approx(-0.357, abs=2e-3)
