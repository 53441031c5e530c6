"""NumPy / SciPy reference for sbo_refine -- test infrastructure only.

posterior_grad: the exact posterior of oracle.gp_inference at one point with the analytic gradients of mean and var;
bound_grad:     a bound (mean / ucb / lcb / var) and its gradient, ucb / lcb = mean +- b sqrt(var) (models/SafeOpt.py:34-45);
The problem itself -- SLSQP from a seed, the feasible yardstick, the KKT residual -- is refine_sets_oracle's, of which sbo_refine's
is the single-point case.
"""
import numpy as np

import oracle


def posterior_grad(x, ds):
    """mean[q], var[q] (un-normalised, var clamped at 0 as models/GP_Safe.py:343) and their gradients [q, d] at x [d]."""
    x = np.asarray(x, dtype=np.float64)
    Xn = ds["X_norm"]
    n, d = Xn.shape
    q = ds["Y_norm"].shape[1]
    mp = oracle.mean_prior(ds)
    xn = (x - ds["X_mean"]) / ds["X_std"]
    mean, var = np.empty(q), np.empty(q)
    gm, gv = np.empty((q, d)), np.empty((q, d))
    for o in range(q):
        h = ds["hypopt"][:, o]
        ell, sf2 = np.exp(2 * h[:d]), np.exp(2 * h[d])
        diff = Xn - xn                                         # [n, d]
        k = sf2 * np.exp(-0.5 * np.sum(diff * diff / ell, axis=1))
        iK = ds["invKopt"][o]
        alpha = iK @ (ds["Y_norm"][:, o] - mp[o])
        w = iK @ k
        ys = ds["Y_std"][o]
        vn = sf2 - k @ w
        mean[o] = ys * (mp[o] + k @ alpha) + ds["Y_mean"][o]
        var[o] = ys * ys * max(0.0, vn)
        dk = k[:, None] * diff / ell                           # d k_j / d xn_a
        gm[o] = ys * (alpha @ dk) / ds["X_std"]
        gv[o] = -2.0 * ys * ys * (w @ dk) / ds["X_std"]
    return mean, var, gm, gv


def bound_grad(x, ds, b, o, kind):
    """(value, gradient [d]) of bound ``kind`` of output o at x."""
    m, v, gm, gv = posterior_grad(x, ds)
    if kind == "mean":
        return m[o], gm[o]
    if kind == "var":
        return v[o], gv[o]
    s = 1.0 if kind == "ucb" else -1.0
    sd = np.sqrt(v[o])
    return m[o] + s * b * sd, gm[o] + s * b * gv[o] / (2.0 * sd)
