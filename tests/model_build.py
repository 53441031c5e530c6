"""Shared helpers of the model-build tests (csrc/model.hip: k_model_build below kBlockedFrom rows, the blocked chain k_invk_reverse /
k_chol_prep -> k_chol_step per 32-row panel -> k_chol_finish from it, k_pack_factor behind both): a model generator for any
(n, d, q), the point list the posterior is probed on, the three probes of the resident factor, and the degenerate inputs a build
must refuse.  Everything in normalised units (mean / max(1, Y_std), var / max(1, Y_std)^2), the bars the project's TOL64 / TOL32."""
import functools

import numpy as np

import oracle

import model_loo as ml
import model_remove as mr

TOL64, TOL32 = mr.TOL64, mr.TOL32
BLOCKED_FROM = 96                     # csrc/model.hip: kBlockedFrom
PANEL = 32                            # csrc/model.hip: kPB
KERNEL_K1G = mr.KERNEL["K1g"]
GRID_COUNT = [23, 19]                 # the small grid of probe 3 (two partial 64-candidate tiles per row of blocks)
N_MIN_ROWS = 16                       # the normalisation constants of a model below this size come from this many rows

SHAPE_RANGE = [1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 255, 257]
WIDE_N, WIDE_DQ = [95, 96, 97, 129], [(1, 1), (3, 8), (8, 8)]
LARGE_N, LARGE_DQ = [2047, 2048], (3, 2)


def log_sn_for(n):
    """The noise at which the fp64 oracle is sharp enough for TOL64 (tests/test_gpu_model_loo.py: -1 from n = 300 up, the default
    -2 below; tests/test_model_build_cpu.py checks the oracle's own error at every shape of the range)."""
    return -1.0 if n >= 300 else -2.0


def box(d):
    """The input box: every axis with its own offset and width."""
    a = np.arange(d, dtype=np.float64)
    return -1.0 - 0.1 * a, 1.5 + 0.2 * a


def hyper(d, q, log_sn):
    """Per-output hyper-parameters that differ between outputs and axes (a stride error between outputs mixes them visibly).  The
    length scale grows with sqrt(d / 2) so that neighbours stay correlated in every dimension."""
    o, a = np.arange(q, dtype=np.float64), np.arange(d, dtype=np.float64)
    hyp = np.empty((d + 2, q))
    hyp[:d] = (-0.5 + 0.5 * np.log(max(d, 2) / 2.0)) + 0.06 * o[None, :] - 0.03 * a[:, None]
    hyp[d] = 0.05 * o - 0.1
    hyp[d + 1] = log_sn + 0.04 * o
    return hyp


def outputs(X, q):
    """q smooth outputs of different frequency and offset."""
    d = X.shape[1]
    s = X.sum(axis=1) / np.sqrt(d)
    cols = [np.sin(0.7 * (o + 1) * s + 0.3 * o) + 0.5 * X[:, o % d] + 0.1 * o * X[:, 0] ** 2 + 0.4 * o for o in range(q)]
    return np.stack(cols, axis=1)


def make_model(n, d, q, seed=None, log_sn=None):
    """(ds, lo, hi): n random inputs in box(d), smooth outputs through oracle.make_inference_dataset, hyper(d, q, log_sn).  Below
    N_MIN_ROWS rows the constants are those of N_MIN_ROWS rows (frozen, model_remove.with_rows), so that n = 1 has a finite std."""
    if log_sn is None:
        log_sn = log_sn_for(n)
    rng = np.random.default_rng(7000 + 131 * n + 17 * d + q if seed is None else seed)
    lo, hi = box(d)
    rows = max(n, N_MIN_ROWS)
    X = lo + (hi - lo) * rng.uniform(size=(rows, d))
    hyp = hyper(d, q, log_sn)
    if rows == n:
        return oracle.make_inference_dataset(X, outputs(X, q), hyp), lo, hi
    X_norm, Y_norm, X_mean, X_std, Y_mean, Y_std = oracle.data_normalization(X, outputs(X, q))
    ds = {"X_mean": X_mean, "X_std": X_std, "Y_mean": Y_mean, "Y_std": Y_std, "hypopt": hyp}
    return mr.with_rows(ds, X_norm[:n], Y_norm[:n]), lo, hi


@functools.lru_cache(maxsize=4)
def cached_model(n, d, q):
    """make_model once per shape (the inverse at n = 2047 / 2048 is the expensive part); callers must not change it."""
    return make_model(n, d, q)


def point_list(ds, lo, hi, npts=300, on_obs=8, seed=11):
    """npts points: uniform in the box widened by 10 % per side, the last min(on_obs, n) placed on observations spread over the
    rows (first, last and between) -- there the variance sf2 - k^T invK k is a near-total cancellation that reads every entry of M."""
    n, d = ds["X_norm"].shape
    rng = np.random.default_rng(seed + n)
    w = hi - lo
    pts = (lo - 0.1 * w) + 1.2 * w * rng.uniform(size=(npts, d))
    rows = np.unique(np.linspace(0, n - 1, min(on_obs, n)).round().astype(int))
    pts[npts - len(rows):] = ds["X_norm"][rows] * ds["X_std"] + ds["X_mean"]
    return pts


def nerrs(mean, var, om, ov, ds):
    return mr.nerr(np.asarray(mean, np.float64), om, ds["Y_std"], 1), mr.nerr(np.asarray(var, np.float64), ov, ds["Y_std"], 2)


def symmetrised(ds):
    out = dict(ds)
    out["invKopt"] = [0.5 * (np.asarray(P) + np.asarray(P).T) for P in ds["invKopt"]]
    return out


def skewed(ds, rel=1e-13, seed=3):
    """ds whose invKopt carry a random skew-symmetric part of relative size ``rel`` (of the largest entry): what a caller's own
    inversion may hand over.  k_invk_alpha reads the matrix as passed; the factor is of its symmetric part."""
    rng = np.random.default_rng(seed)
    out = dict(ds)
    parts = []
    for P in ds["invKopt"]:
        R = rng.standard_normal(P.shape)
        parts.append(np.asarray(P) + rel * np.max(np.abs(P)) * 0.5 * (R - R.T))
    out["invKopt"] = parts
    return out


def list_posterior(eng, pts, path):
    """The posterior of the resident model on the point list through one of the generic kernels (posterior_path 1 / 2)."""
    eng.set_points(pts)
    try:
        eng.set_option("posterior_path", path)
        eng.posterior_run()
        return eng.posterior()
    finally:
        eng.set_option("posterior_path", 0)


def probe(eng, ds, lo, hi, pts, dtype="f64", label="", ref=None, loo=True):
    """The three probes of the resident factor.  1: model_loo.check_loo (alpha, diag(M^T M), log det; fp64 whatever the model
    dtype).  2: the posterior on the point list through both generic kernels against oracle.gp_inference (``ref`` = its (mean, var)
    on ``pts`` when the caller has them).  3, d = 2: a GRID_COUNT grid with bilinear = 0, which must run K1g -- the packed triangle
    images Fpk through the matrix-core path.  Returns the largest normalised error of the posterior probes."""
    tol = TOL64 if dtype == "f64" else TOL32
    np_dtype = np.float64 if dtype == "f64" else np.float32
    n, d = ds["X_norm"].shape
    assert (eng.n, eng.d, eng.q) == (n, d, ds["Y_norm"].shape[1]), label
    if loo:
        ml.check_loo(eng, ds, TOL64, (label, "loo"))
    om, ov = ref if ref is not None else oracle.gp_inference(pts, ds)
    worst = 0.0
    for path in (1, 2):
        mean, var = list_posterior(eng, pts, path)
        assert mean.shape == om.shape and var.shape == ov.shape and mean.dtype == np_dtype, (label, path)
        em, ev = nerrs(mean, var, om, ov, ds)
        print(label, "list path", path, em, ev)
        assert em < tol and ev < tol, (label, "list", path, em, ev)
        worst = max(worst, em, ev)
    if d == 2:
        gpts = oracle.grid_points(lo, hi, GRID_COUNT)
        gm, gv = oracle.gp_inference(gpts, ds)
        try:
            eng.set_option("bilinear", 0)
            eng.set_grid(lo, hi, GRID_COUNT)
            eng.posterior_run()
            assert eng.profile()["posterior_kernel"] == KERNEL_K1G, (label, eng.profile()["posterior_kernel"])
            mean, var = eng.posterior()
        finally:
            eng.set_option("bilinear", 1)
        em, ev = nerrs(mean, var, gm, gv, ds)
        print(label, "grid K1g", em, ev)
        assert em < tol and ev < tol, (label, "K1g", em, ev)
        worst = max(worst, em, ev)
        eng.set_points(pts)               # (no grid stays resident: the next build is not deferred behind a K1b plan)
    return worst


def build_and_probe(eng, ds, lo, hi, use_invK, dtype="f64", label="", npts=300, ref=None, loo=True):
    """set_model with a point list resident (the factor is built inside the call, never deferred), then the three probes."""
    pts = point_list(ds, lo, hi, npts)
    eng.set_points(pts)
    eng.set_model(ds, dtype=dtype, use_invK=use_invK)
    return probe(eng, ds, lo, hi, pts, dtype=dtype, label=label, ref=ref, loo=loo)


# ---- builds that must be refused ------------------------------------------------------------------------------------------------
def indefinite_invK(ds, output, index):
    """ds with one diagonal entry of invKopt[output] negated: that matrix is no longer positive definite, the others are untouched."""
    out = dict(ds)
    parts = [np.array(P, copy=True) for P in ds["invKopt"]]
    parts[output][index, index] = -abs(parts[output][index, index])
    out["invKopt"] = parts
    return out


DUP_ROWS = 32                         # identical input rows of the degenerate mode-1 model (one whole panel)
DUP_LOG_SF = 12.0                     # sf2 = e^24 = 2.6e10: its ulp (3.8e-6) swallows the smallest noise the model format allows
DUP_LOG_SN = -40.0                    # sn2 = e^-80 + float32 eps = 1.19e-7


def degenerate_hyper_model(ds, output, first_row):
    """A model whose K + sn2 I of ``output`` alone is singular as stored: rows first_row .. first_row + DUP_ROWS - 1 of X_norm are
    made identical and that output gets log sigma_f = DUP_LOG_SF, log sigma_n = DUP_LOG_SN.  Then sf2 + (sn2 + float32 eps)
    rounds to sf2, every entry of the DUP_ROWS x DUP_ROWS block is the same fp64 number v, and elimination leaves the block
    e 1 1^T with |e'| <= c eps e from one pivot to the next (e' = fl(e - u^2), u = fl(sqrt e)): a pivot <= 0, or after at most 23
    pivots an underflow to zero (2^35 2^(-49 k) < 2^-1074).  In exact arithmetic on the stored matrix the second of these pivots
    is exactly zero.  The other outputs keep their noise and stay positive definite."""
    out = dict(ds)
    X = np.array(ds["X_norm"], copy=True)
    X[first_row:first_row + DUP_ROWS] = X[first_row]
    hyp = np.array(ds["hypopt"], copy=True)
    d = X.shape[1]
    hyp[d, output], hyp[d + 1, output] = DUP_LOG_SF, DUP_LOG_SN
    out["X_norm"], out["hypopt"] = X, hyp
    out.pop("invKopt", None)           # (never read: the build is from the hyper-parameters)
    return out


def kernel_matrix(ds, output):
    """K + (sn2 + float32 eps) I of one output as oracle.build_invK forms it before inverting."""
    X, hyp = ds["X_norm"], ds["hypopt"]
    n, d = X.shape
    ell, sf2 = np.exp(2.0 * hyp[:d, output]), np.exp(2.0 * hyp[d, output])
    sn2 = np.exp(2.0 * hyp[d + 1, output]) + oracle.FLOAT32_EPS
    return oracle.cov_mat(X, X, ell, sf2) + sn2 * np.eye(n)


# ---- the two sources against the true posterior (extended precision) -------------------------------------------------------------
TRUE_N = [97, 161]
TRUE_LOG_SN = -3.0
TRUE_POINTS = 100
# The bar of the hyper-parameter build: TRUE_MARGIN times the fp64 oracle's own distance from oracle.extended.posterior_true on the
# same points (profiles/model_build_checks.md has the measured distances and the reasoning behind the factor).
TRUE_MARGIN = 4.0


def true_case(n):
    ds, lo, hi = make_model(n, 2, 2, log_sn=TRUE_LOG_SN)
    return ds, lo, hi, point_list(ds, lo, hi, TRUE_POINTS)


def distance_from_truth(mean, var, truth, ds):
    tm, tv = (np.asarray(a, dtype=np.float64) for a in truth)
    return nerrs(mean, var, tm, tv, ds)


def cholesky_route(pts, ds):
    """The posterior the way a hyper-parameter build evaluates it, in NumPy fp64 with IEEE square roots and divisions: K = L L^T,
    M = L^-1, mean = mp + (M k)^T (M rhs), var = sf2 - |M k|^2."""
    from scipy.linalg import solve_triangular
    n, d = ds["X_norm"].shape
    q = ds["Y_norm"].shape[1]
    mp = oracle.mean_prior(ds)
    xn = (np.asarray(pts) - ds["X_mean"]) / ds["X_std"]
    mean, var = np.empty((len(pts), q)), np.empty((len(pts), q))
    for o in range(q):
        ell, sf2 = np.exp(2.0 * ds["hypopt"][:d, o]), np.exp(2.0 * ds["hypopt"][d, o])
        L = np.linalg.cholesky(kernel_matrix(ds, o))
        t = solve_triangular(L, oracle.calc_cov_mat(ds["X_norm"], xn, ell, sf2), lower=True)
        r = solve_triangular(L, ds["Y_norm"][:, o] - mp[o], lower=True)
        mean[:, o] = (mp[o] + t.T @ r) * ds["Y_std"][o] + ds["Y_mean"][o]
        var[:, o] = np.maximum(0.0, sf2 - np.sum(t * t, axis=0)) * ds["Y_std"][o] ** 2
    return mean, var
