"""Shared helpers of the sbo_model_remove tests: the NumPy statement of the update the device performs,
the oracle datasets of a model that lost or gained rows under frozen constants, and the preconditions under which a sweep's
masks are compared exactly."""
import numpy as np

import oracle

TOL64, TOL32 = 1e-10, 1e-4           # tests/test_gpu_append.py: the project's bars for the append
KERNEL = {"K1g": 3, "K1b": 4, "K1t": 5}
STRIP = 64                            # csrc/model.hip: kRemoveStrip, the new columns one wave of k_model_remove walks


BOUND = np.array([[-.6, 1.5], [-1., 1.]])


def benoit_f(u, noise=0):
    return u[0] ** 2 + u[1] ** 2 + u[0] * u[1]


def benoit_g(u, noise=0):
    return -(1. - u[0] + u[1] ** 2 + 2. * u[1])


def init_bo(cls, n=12, grid=(50, 50), b=3.0):
    """A host class on the Benoit problem with fixed hyper-parameters, n samples around (1.4, -0.8) (tests/test_host_classes.py)."""
    from safebo_amd import synthetic
    m = cls([benoit_f, benoit_g], BOUND, b, grid=grid)
    X, Y = m.Data_sampling(n, np.array([1.4, -.8]), 0.3)
    m.fixed_hyper = synthetic.default_hypopt(2, 2)
    m.GP_initialization(X, Y, "RBF", multi_hyper=5, var_out=True)
    return m


def lower_factor(invK):
    """Lower-triangular M with M^T M = invK (the resident factor): the inverse of the Cholesky factor of K."""
    K = np.linalg.inv(invK)
    return np.tril(np.linalg.inv(np.linalg.cholesky((K + K.T) / 2)))


def remove_update(M, alpha, j):
    """Factor and alpha without observation j, in the prefix form of k_model_remove: m = column j of M, M~ = M without that
    column, r_i = sqrt(sum_{t=j..i} m[t]^2), W_i = sum_{t=j..i} m[t] row_t(M~); rows above j stay, new row i - 1 =
    (r_{i-1} / r_i) row_i(M~) - (m[i] / (r_i r_{i-1})) W_{i-1}; alpha' = alpha_-j - (M~^T m) alpha_j / r_{n-1}^2."""
    n = M.shape[0]
    m = M[:, j].copy()
    Mt = np.delete(M, j, axis=1)
    alpha2 = np.delete(alpha, j) - (Mt.T @ m) * alpha[j] / (m @ m)
    r = np.sqrt(np.cumsum(m[j:] ** 2))
    W = np.cumsum(m[j:, None] * Mt[j:], axis=0)
    N = np.zeros((n - 1, n - 1))
    N[:j] = Mt[:j]
    for i in range(j + 1, n):
        N[i - 1] = (r[i - 1 - j] / r[i - j]) * Mt[i] - (m[i] / (r[i - j] * r[i - 1 - j])) * W[i - 1 - j]
    return N, alpha2


def nerr(got, ref, ystd, power):
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, ystd) ** power))


def with_rows(ds, X_norm, Y_norm):
    """ds over other rows: frozen constants and hyper-parameters, the inverse rebuilt in NumPy from those rows."""
    out = dict(ds)
    out["X_norm"], out["Y_norm"] = np.array(X_norm, dtype=np.float64), np.array(Y_norm, dtype=np.float64)
    out["invKopt"] = oracle.build_invK(out["X_norm"], ds["hypopt"])
    return out


def without(ds, j):
    return with_rows(ds, np.delete(ds["X_norm"], j, axis=0), np.delete(ds["Y_norm"], j, axis=0))


def extended(ds, xn, yn):
    return with_rows(ds, np.vstack([ds["X_norm"], np.atleast_2d(xn)]), np.vstack([ds["Y_norm"], np.atleast_2d(yn)]))


def check_post(eng, ds, pts, tol, label):
    mean, var = eng.posterior()
    om, ov = oracle.gp_inference(pts, ds)
    em, ev = nerr(mean, om, ds["Y_std"], 1), nerr(var, ov, ds["Y_std"], 2)
    assert em < tol and ev < tol, (label, em, ev)


def check_paths(eng, ds, lo, hi, count, grid_pts, list_pts, dtype, label):
    """The posterior of the resident model on every path a 2-D model can take (tests/test_gpu_append.py: _check_paths): K1b (fp64
    only; n <= 16: K1b or the K1g its plan falls back to) and K1g on the grid, the generic kernels (posterior_path 1 and 2) on a
    point list."""
    tol = TOL64 if dtype == "f64" else TOL32
    try:
        paths = (("K1b", 2), ("K1g", 0)) if dtype == "f64" else (("K1g", 1),)
        for name, bl in paths:
            eng.set_option("bilinear", bl)
            eng.set_grid(lo, hi, count)
            eng.posterior_run()
            kernel = eng.profile()["posterior_kernel"]
            # (K1b's plan declines when its two GEMMs issue more than 0.7 of K1g's triangular contraction, bilinear_setup: at one
            # 16-row block the model is K1g's even when K1b is asked for; from npad = 32 on -- the append tests assert K1b from
            # n = 17 -- it must be K1b)
            small = name == "K1b" and ds["X_norm"].shape[0] <= 16
            assert kernel == KERNEL[name] or (small and kernel == KERNEL["K1g"]), (label, name, kernel)
            check_post(eng, ds, grid_pts, tol, (label, name))
    finally:
        eng.set_option("bilinear", 1)
    eng.set_points(list_pts)
    try:
        for path in (1, 2):
            eng.set_option("posterior_path", path)
            eng.posterior_run()
            tile = (8 if dtype == "f64" else 4) * ((ds["X_norm"].shape[0] + 15) // 16 * 16) * 64
            assert eng.profile()["posterior_kernel"] == (2 if path == 2 or tile > 64 * 1024 else 1), (label, path)
            check_post(eng, ds, list_pts, tol, (label, "generic", path))
    finally:
        eng.set_option("posterior_path", 0)


def assert_sharp(sref, floor=1e-9):
    """The oracle's own sweep decides nothing on a tie: S, M and G are non-empty and the smallest decision margins on the grid
    -- min |lcb_1| (the safe set) and min |lcb_0 - u*| over S (the minimisers; u* = the smallest ucb_0 in S) -- exceed
    ``floor``, so a mask that differs is the kernel's fault."""
    assert sref["S"].any() and sref["M"].any() and sref["G"][0].any(), (sref["S"].sum(), sref["M"].sum(), sref["G"][0].sum())
    lcb, S = sref["lcb"], sref["S"]
    m_safe = float(np.min(np.abs(lcb[:, 1])))
    m_min = float(np.min(np.abs(lcb[S, 0] - sref["u_star"])))
    assert m_safe > floor and m_min > floor, (m_safe, m_min)


def assert_safeopt_equal(eng, res, sref):
    for k in ("S", "U", "M"):
        assert np.array_equal(eng.mask(k), sref[k]), k
    assert np.array_equal(eng.mask("G", 1), sref["G"][0])
    assert res["minimizer_index"] == sref["minimizer_index"]
    assert list(res["expander_index_c"]) == list(sref["expander_index"])
    assert (res["count_S"], res["count_U"], res["count_M"]) == (sref["S"].sum(), sref["U"].sum(), sref["M"].sum())
    assert res["count_G"][0] == sref["G"][0].sum()


def assert_goose_equal(eng, g, gref):
    assert np.array_equal(eng.mask("S"), gref["S"]) and np.array_equal(eng.mask("U"), gref["U"])
    assert np.array_equal(eng.mask("O", 1), gref["O"][0])
    assert g["safe_min_index"] == gref["safe_min_index"] and np.array_equal(g["target_index_c"], gref["target_index_c"])
    assert g["target_index"] == gref["target_index"] and g["explore_index"] == gref["explore_index"]
    assert np.array_equal(g["count_O"], gref["O"].sum(1)) and (g["count_S"], g["count_U"]) == (gref["S"].sum(), gref["U"].sum())
