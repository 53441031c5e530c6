"""Shared helpers of the sbo_model_append_batch tests: the committed case list, the NumPy statement of the block update the device
performs next to k one-row updates, the refusal model, and the snapshot of what a resident model gives."""
import numpy as np

import oracle

TOL64, TOL32 = 1e-10, 1e-4           # tests/test_gpu_append.py: the project's bars for the append
SHARP = 1e-11                         # a tenth of TOL64: what the NumPy block route itself must keep against the rebuilt oracle
KERNEL = {"K1g": 3, "K1b": 4, "K1t": 5}
FLOAT32_EPS = float(np.finfo(np.float32).eps)

# (n0, k, d, q, log_sn, source): source "invK" = the caller's inverse, "K" = set_model(..., use_invK=False).
#   (1, 1), (1, 64), (2, 63): a block larger than the model;  (15, 2), (16, 1), (16, 17), (17, 63): crossings of the 16-row padding;
#   (63, 64), (64, 64), (65, 8): wave / strip boundaries;  (250, 64): several row blocks and column strips.
# Every case is sharp (test_model_append_batch_cpu.py: the NumPy block route within SHARP of the rebuilt oracle); from n0 + k of
# about 150 on that needs log_sn = -1.
CASES = [
    (1, 1, 2, 2, -2.0, "invK"),
    (1, 64, 2, 2, -2.0, "K"),
    (2, 63, 2, 1, -2.0, "invK"),
    (15, 2, 1, 2, -2.0, "K"),
    (16, 1, 2, 3, -2.0, "invK"),
    (16, 17, 2, 2, -2.0, "K"),
    (17, 63, 8, 2, -2.0, "invK"),
    (63, 64, 2, 2, -2.0, "K"),
    (64, 64, 2, 3, -2.0, "invK"),
    (65, 8, 1, 1, -2.0, "K"),
    (250, 64, 2, 2, -1.0, "invK"),
]


def case_id(case):
    return "n{}_k{}_d{}_q{}_sn{:g}_{}".format(*case)


def nerr(got, ref, ystd, power):
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, ystd) ** power))


def box(d):
    """The box the data and the test points of a d-dimensional case live in: config B's for d = 2, [-2, 2]^d otherwise."""
    return np.array([[-.6, 1.5], [-1., 1.]]) if d == 2 else np.array([[-2.0, 2.0]] * d)


def plant(X, q):
    """q smooth outputs of X [n, d]: Benoit's objective and constraint for d = 2, a bowl and a dome otherwise, and a third dome."""
    from safebo_amd import synthetic
    r2 = np.sum(X ** 2, axis=1)
    if X.shape[1] == 2:
        base = synthetic.benoit(X)
    else:
        base = np.stack([r2 / X.shape[1] + np.sin(2.0 * X[:, 0]), 3.0 - 0.5 * r2 / X.shape[1] + X[:, -1]], axis=1)
    return np.concatenate([base, (1.5 - 0.3 * r2 + X[:, 0])[:, None]], axis=1)[:, :q]


def case_data(case, seed=0):
    """The model of a case: all n0 + k rows drawn in the box, normalised over all of them (the constants stay frozen), default
    hyper-parameters with the case's log_sn.  Returns (ds of the first n0 rows, xn [k, d], yn [k, q], ds of all rows)."""
    from safebo_amd import synthetic
    n0, k, d, q, log_sn, _ = case
    b = box(d)
    rng = np.random.default_rng(1000 * n0 + k + seed)
    X = rng.uniform(b[:, 0], b[:, 1], size=(n0 + k, d))
    # (d = 8: longer length-scales, so that rows eight dimensions apart still see each other)
    full = synthetic.make_dataset(X, plant(X, q), synthetic.default_hypopt(d, q, log_ell=-0.5 if d <= 2 else 1.0, log_sn=log_sn))
    return with_rows(full, full["X_norm"][:n0], full["Y_norm"][:n0]), full["X_norm"][n0:], full["Y_norm"][n0:], full


def with_rows(ds, X_norm, Y_norm, invK=None):
    """ds over other rows: frozen constants and hyper-parameters, the inverse rebuilt in NumPy from those rows (or given)."""
    out = dict(ds)
    out["X_norm"], out["Y_norm"] = np.array(X_norm, dtype=np.float64), np.array(Y_norm, dtype=np.float64)
    out["invKopt"] = oracle.build_invK(out["X_norm"], ds["hypopt"]) if invK is None else invK
    return out


def extended(ds, xn, yn, invK=None):
    return with_rows(ds, np.vstack([ds["X_norm"], np.atleast_2d(xn)]), np.vstack([ds["Y_norm"], np.atleast_2d(yn)]), invK)


def hyper(ds, o):
    """(ell [d], sf2, sn2 with the float32 eps) of output o."""
    d = ds["X_norm"].shape[1]
    h = ds["hypopt"][:, o]
    return np.exp(2.0 * h[:d]), float(np.exp(2.0 * h[d])), float(np.exp(2.0 * h[d + 1])) + FLOAT32_EPS


def lower_factor(invK):
    """Lower-triangular M with M^T M = invK (the resident factor): the inverse of the Cholesky factor of K."""
    K = np.linalg.inv(invK)
    return np.tril(np.linalg.inv(np.linalg.cholesky((K + K.T) / 2)))


def block_inputs(ds, xn, yn, o):
    """B = K(X, X_new) [n, k], Z = K(X_new, X_new) + sn2 I [k, k] and rho = y_new - mp [k] of output o, expanded distance."""
    ell, sf2, sn2 = hyper(ds, o)
    xn = np.atleast_2d(xn)
    B = oracle.cov_mat(ds["X_norm"], xn, ell, sf2)
    Z = oracle.cov_mat(xn, xn, ell, sf2)
    Z = np.triu(Z) + np.triu(Z, 1).T                        # (the older row is `a` of the expanded distance, as in k one-row appends)
    Z[np.diag_indices_from(Z)] = sf2 + sn2
    return B, Z, np.atleast_2d(yn)[:, o] - oracle.mean_prior(ds)[o]


def append_block_update(M, alpha, B, Z, rho):
    """The block update of DESIGN.md section 18: T = M B, U = M^T T, S = Z - B^T U, g = B^T alpha, S = R R^T, G = R^-1,
    new rows [-G U^T | G], w = G^T G (g - rho), alpha' = (alpha + U w, -w).  Returns (M', alpha', pivots of the Cholesky of S as
    they come up: a pivot that is not > 0 refuses the block, None in place of M' and alpha')."""
    n, k = B.shape
    U = M.T @ (M @ B)
    S = Z - B.T @ U
    g = B.T @ alpha
    R = np.zeros((k, k))
    A = np.tril(S).copy()
    piv = np.empty(k)
    for j in range(k):
        piv[j] = A[j, j]
        if not piv[j] > 0.0:
            return None, None, piv[:j + 1]
        R[j, j] = np.sqrt(piv[j])
        R[j + 1:, j] = A[j + 1:, j] / R[j, j]
        A[j + 1:, j + 1:] -= np.tril(np.outer(R[j + 1:, j], R[j + 1:, j]))
    G = np.tril(np.linalg.inv(R))
    N = np.zeros((n + k, n + k))
    N[:n, :n], N[n:, :n], N[n:, n:] = M, -G @ U.T, G
    w = G.T @ (G @ (g - rho))
    return N, np.concatenate([alpha + U @ w, -w]), piv


def append_rows_update(M, alpha, B, Z, rho):
    """The same rows by k one-row updates (csrc/model.hip: k_model_append), row r against the model that holds rows 0 .. r - 1."""
    n, k = B.shape
    for r in range(k):
        kv = np.concatenate([B[:, r], Z[:r, r]])
        u = M.T @ (M @ kv)
        s, ka = Z[r, r] - kv @ u, kv @ alpha
        m = M.shape[0]
        N = np.zeros((m + 1, m + 1))
        N[:m, :m], N[m, :m], N[m, m] = M, -u / np.sqrt(s), 1.0 / np.sqrt(s)
        M, alpha = N, np.concatenate([alpha + u * (ka - rho[r]) / s, [(rho[r] - ka) / s]])
    return M, alpha


def start_state(ds, o):
    """(M, alpha) of output o as the library holds them for ds."""
    return lower_factor(ds["invKopt"][o]), ds["invKopt"][o] @ (ds["Y_norm"][:, o] - oracle.mean_prior(ds)[o])


def posterior_from(ds_all, Ms, alphas, pts):
    """Physical-unit posterior (mean, var) [N, q] at pts from per-output factors and alphas over the rows of ds_all:
    mean = mp + k^T alpha, var = max(0, sf2 - |M k|^2)."""
    xg = (pts - ds_all["X_mean"]) / ds_all["X_std"]
    mp = oracle.mean_prior(ds_all)
    mean, var = np.empty((pts.shape[0], len(Ms))), np.empty((pts.shape[0], len(Ms)))
    for o, (M, al) in enumerate(zip(Ms, alphas)):
        ell, sf2, _ = hyper(ds_all, o)
        kx = oracle.cov_mat(ds_all["X_norm"], xg, ell, sf2)
        t = M @ kx
        mean[:, o] = (mp[o] + kx.T @ al) * ds_all["Y_std"][o] + ds_all["Y_mean"][o]
        var[:, o] = np.maximum(0.0, sf2 - np.sum(t * t, axis=0)) * ds_all["Y_std"][o] ** 2
    return mean, var


def bordered_invK(ds, xn, o):
    """inv of the block-bordered matrix [[inv(invK), B], [B^T, Z]] of output o: the oracle of a block appended to a caller's
    (possibly inconsistent) inverse."""
    B, Z, _ = block_inputs(ds, xn, np.zeros((np.atleast_2d(xn).shape[0], ds["Y_norm"].shape[1])), o)
    return np.linalg.inv(np.block([[np.linalg.inv(ds["invKopt"][o]), B], [B.T, Z]]))


# ---------------------------------------------------------------------------------------------- refusals
def refusal_model():
    """tests/test_gpu_append.py's: q = 2 on [-2, 2]^2 plus one isolated observation x_iso = (6, 6) far outside the swept box.
    Output 1 gets the caller's invK of D K D, where D scales x_iso's row by 1/2: consistent everywhere the grid looks, but a new
    observation at x_iso has a Schur pivot far below zero on output 1 while output 0 accepts it."""
    from safebo_amd import synthetic
    rng = np.random.default_rng(11)
    X = np.vstack([rng.uniform(-2.0, 2.0, size=(63, 2)), [[6.0, 6.0]]])
    ds = synthetic.make_dataset(X, synthetic.benoit(X), synthetic.default_hypopt(2, 2))
    dvec = np.ones(X.shape[0])
    dvec[-1] = 0.5
    ds["invKopt"] = [ds["invKopt"][0], ds["invKopt"][1] / np.outer(dvec, dvec)]
    return ds


def refusal_block(ds, k, pos, seed=3):
    """k normalised rows inside the box's image with x_iso (the model's last row) at position pos; outputs small and finite."""
    rng = np.random.default_rng(seed + 10 * k + pos)
    xn = (rng.uniform(-1.8, 1.8, size=(k, 2)) - ds["X_mean"]) / ds["X_std"]
    xn[pos] = ds["X_norm"][-1]
    return xn, rng.uniform(-0.5, 0.5, size=(k, 2))


def block_pivots(ds, xn, yn, o):
    """The Schur pivots of the block on output o in NumPy, as far as the factorisation gets."""
    M, alpha = start_state(ds, o)
    return append_block_update(M, alpha, *block_inputs(ds, xn, yn, o))[2]


def snapshot(eng, lo, hi, count, b):
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


def assert_same(a, b):
    assert a["n"] == b["n"]
    for name in ("K1b", "K1g"):
        for x, y in zip(a[name], b[name]):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), name
    for k, v in a["sweep"].items():
        assert np.array_equal(np.asarray(v), np.asarray(b["sweep"][k])), k
    for x, y in zip(a["masks"], b["masks"]):
        assert np.array_equal(x, y)


def check_post(eng, ds, pts, tol, label):
    mean, var = eng.posterior()
    om, ov = oracle.gp_inference(pts, ds)
    em, ev = nerr(mean, om, ds["Y_std"], 1), nerr(var, ov, ds["Y_std"], 2)
    print("posterior", label, "mean", em, "var", ev)
    assert em < tol and ev < tol, (label, em, ev)
    return max(em, ev)


def check_paths(eng, ds, lo, hi, count, grid_pts, list_pts, dtype, label):
    """The posterior of the resident 2-D model on K1b (fp64 only; n <= 16: K1b or the K1g its plan falls back to) and K1g on the
    grid and on the generic kernels (posterior_path 1 and 2) on a point list (tests/test_gpu_append.py: _check_paths)."""
    tol = TOL64 if dtype == "f64" else TOL32
    try:
        paths = (("K1b", 2), ("K1g", 0)) if dtype == "f64" else (("K1g", 1),)
        for name, bl in paths:
            eng.set_option("bilinear", bl)
            eng.set_grid(lo, hi, count)
            eng.posterior_run()
            kernel = eng.profile()["posterior_kernel"]
            small = name == "K1b" and ds["X_norm"].shape[0] <= 16
            assert kernel == KERNEL[name] or (small and kernel == KERNEL["K1g"]), (label, name, kernel)
            check_post(eng, ds, grid_pts, tol, (label, name))
    finally:
        eng.set_option("bilinear", 1)
    check_list_paths(eng, ds, list_pts, tol, label)


def check_list_paths(eng, ds, list_pts, tol, label):
    eng.set_points(list_pts)
    try:
        for path in (1, 2):
            eng.set_option("posterior_path", path)
            eng.posterior_run()
            check_post(eng, ds, list_pts, tol, (label, "generic", path))
    finally:
        eng.set_option("posterior_path", 0)


def assert_sharp(sref, floor=1e-9):
    """The oracle's own sweep decides nothing on a tie (tests/model_remove.py): S, M and G are non-empty and the smallest decision
    margins on the grid exceed ``floor``, so a mask that differs is the kernel's fault."""
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
