"""NumPy restatement of StableOpt's robust problem on a grid (models/StableOpt.py:139-164 on models/GP_Robust.py) -- test
infrastructure for tests/test_robust_cpu.py and tests/test_gpu_robust.py.

GP_Robust's posterior is GP_Safe's with the prior mean zero for every output (models/GP_Robust.py:322-324); ``oracle.gp_inference``
is pinned to GP_Safe's prior, so the prior is a parameter here.  On the joint grid (controls = the fast axes, disturbances = the slow
ones) the robust problem is reductions over the disturbance planes:
    f[xc]   = max_d bound_0(xc, d)            (bound: mean / ucb / lcb)
    g_c[xc] = min_d lcb_c(xc, d)              (c >= 1)
    index   = argmin over {xc: g_c[xc] >= 0 for all c} of f   (ties -> lowest index, np.argmin order), -1 when that set is empty
    worst_d = argmax_d bound_0(xc*, d)        (np.argmax order)
"""
import numpy as np

import oracle


def zero_prior(ds):
    return np.zeros(np.asarray(ds["Y_mean"]).shape[0])


def gp_inference_prior(points, ds, mp, chunk=65536):
    """models/GP_Safe.py:310-352 with the prior mean ``mp`` [q] (normalised units) -- GP_Robust's posterior for mp = 0."""
    points = np.asarray(points, dtype=np.float64)
    N = points.shape[0]
    n, d = ds["X_norm"].shape
    q = ds["Y_norm"].shape[1]
    mp = np.asarray(mp, dtype=np.float64)
    mean = np.empty((N, q))
    var = np.empty((N, q))
    for s in range(0, N, chunk):
        xnorm = (points[s:s + chunk] - ds["X_mean"]) / ds["X_std"]
        for i in range(q):
            hyper = ds["hypopt"][:, i]
            ell, sf2 = np.exp(2 * hyper[:d]), np.exp(2 * hyper[d])
            k = oracle.calc_cov_mat(ds["X_norm"], xnorm, ell, sf2)
            kinv = np.matmul(k.T, ds["invKopt"][i])
            m = mp[i] + np.matmul(kinv, ds["Y_norm"][:, i] - mp[i])
            v = np.maximum(0, sf2 - np.sum(kinv * k.T, axis=1))
            mean[s:s + chunk, i] = m * ds["Y_std"][i] + ds["Y_mean"][i]
            var[s:s + chunk, i] = v * ds["Y_std"][i] ** 2
    return mean, var


def bound_of(mean, var, b, kind):
    if kind == "mean":
        return mean
    s = b * np.sqrt(var)
    return mean + s if kind == "ucb" else mean - s


def robust_from_posterior(mean, var, nc, b, kind="ucb"):
    """The robust reductions of a joint-grid posterior mean / var [N, q] (N = nc x nd, control index fastest)."""
    q = mean.shape[1]
    nd = mean.shape[0] // nc
    f_all = bound_of(mean[:, 0], var[:, 0], b, kind).reshape(nd, nc)
    f = f_all.max(axis=0)
    argd = f_all.argmax(axis=0)
    g = np.stack([bound_of(mean[:, c], var[:, c], b, "lcb").reshape(nd, nc).min(axis=0) for c in range(1, q)]) if q > 1 \
        else np.zeros((0, nc))
    safe = np.all(g >= 0, axis=0)
    if safe.any():
        index = int(np.argmin(np.where(safe, f, np.inf)))
        value = float(f[index])
        worst = int(argd[index])
    else:
        index, value, worst = -1, float("inf"), -1
    return {"f": f, "g": g, "safe": safe, "index": index, "value": value, "worst_d_index": worst,
            "count_safe": int(safe.sum()), "candidate_index": worst * nc + index if index >= 0 else -1}


def robust_sweep(lo, hi, count, n_control_axes, ds, b, kind="ucb", mp=None):
    """Posterior of the joint grid (prior ``mp``, default zero) and its robust reductions."""
    pts = oracle.grid_points(lo, hi, count)
    mean, var = gp_inference_prior(pts, ds, zero_prior(ds) if mp is None else mp)
    nc = int(np.prod(count[:n_control_axes]))
    out = robust_from_posterior(mean, var, nc, b, kind)
    out["mean"], out["var"] = mean, var
    return out


def w_shape(x, d):
    """The W-shape problem of the reference's StableOpt study: f(x, d) = sin(x d) + sqrt(d) x^2 - 0.5 x."""
    return np.sin(x * d) + np.sqrt(d) * x ** 2 - 0.5 * x
