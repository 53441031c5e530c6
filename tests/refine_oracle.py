"""NumPy / SciPy reference for sbo_refine -- test infrastructure only.

posterior_grad: the exact posterior of oracle.gp_inference at one point with the analytic gradients of mean and var;
bound_grad:     a bound (mean / ucb / lcb / var) and its gradient, ucb / lcb = mean +- b sqrt(var) (models/SafeOpt.py:34-45);
slsqp:          SciPy SLSQP from a seed on the same problem the device solves;
kkt_residual:   stationarity residual at a point, multipliers of the (nearly) active constraints from scipy.optimize.nnls.
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


def slsqp(ds, b, seed, objective=0, kind="lcb", maximize=False, constraints=(1,), lo=None, hi=None, x_0=None, r=None):
    """SLSQP from ``seed`` on min (or max) of ``kind``_objective s.t. lcb_c >= 0, the box and the ball: (x, value at x)."""
    from scipy.optimize import minimize
    sg = -1.0 if maximize else 1.0

    def fun(x):
        f, g = bound_grad(x, ds, b, objective, kind)
        return sg * f, sg * g

    cons = [{"type": "ineq", "fun": (lambda x, c=c: bound_grad(x, ds, b, c, "lcb")[0]),
             "jac": (lambda x, c=c: bound_grad(x, ds, b, c, "lcb")[1])} for c in constraints]
    if x_0 is not None:
        x_0 = np.asarray(x_0, dtype=np.float64)
        cons.append({"type": "ineq", "fun": lambda x: r * r - np.sum((x - x_0) ** 2), "jac": lambda x: -2.0 * (x - x_0)})
    res = minimize(fun, np.asarray(seed, dtype=np.float64), jac=True, method="SLSQP", bounds=list(zip(lo, hi)), constraints=cons,
                   options={"maxiter": 500, "ftol": 1e-14})
    x = np.clip(res.x, lo, hi)
    return x, bound_grad(x, ds, b, objective, kind)[0]


def make_feasible(x, seed, ds, b, constraints=(1,), x_0=None, r=None, steps=80):
    """``x`` when lcb_c(x) >= 0 for every constraint (and inside the ball), else the feasible end of a bisection on the segment
    from the feasible ``seed`` towards ``x`` -- an SLSQP answer a hair outside the safe set made into a feasible yardstick."""
    def ok(p):
        if x_0 is not None and np.sqrt(np.sum((p - x_0) ** 2)) > r:
            return False
        return all(bound_grad(p, ds, b, c, "lcb")[0] >= 0.0 for c in constraints)
    x, seed = np.asarray(x, dtype=np.float64), np.asarray(seed, dtype=np.float64)
    if ok(x):
        return x
    lo_t, hi_t = 0.0, 1.0
    for _ in range(steps):
        t = 0.5 * (lo_t + hi_t)
        if ok(seed + t * (x - seed)):
            lo_t = t
        else:
            hi_t = t
    return seed + lo_t * (x - seed)


def kkt_residual(x, ds, b, objective=0, kind="lcb", maximize=False, constraints=(1,), lo=None, hi=None, x_0=None, r=None,
                 active=1e-6):
    """||grad f - sum lambda_i grad g_i||_inf / (1 + ||grad f||_inf) over the constraints within ``active`` (relative) of their
    bound, lambda >= 0 by NNLS.  Box faces: bound constraints x_a >= lo_a / -x_a >= -hi_a.  f is the minimised function."""
    from scipy.optimize import nnls
    x = np.asarray(x, dtype=np.float64)
    d = x.shape[0]
    sg = -1.0 if maximize else 1.0
    f, gf = bound_grad(x, ds, b, objective, kind)
    gf = sg * gf
    G = []
    for c in constraints:
        g, gg = bound_grad(x, ds, b, c, "lcb")
        if g <= active * (abs(ds["Y_std"][c]) + np.linalg.norm(gg)):
            G.append(gg)
    if x_0 is not None:
        h = r * r - np.sum((x - x_0) ** 2)
        if h <= active * r * r:
            G.append(-2.0 * (x - np.asarray(x_0)))
    span = np.asarray(hi) - np.asarray(lo)
    for a in range(d):
        e = np.zeros(d)
        if x[a] <= lo[a] + active * span[a]:
            e[a] = 1.0
            G.append(e)
        elif x[a] >= hi[a] - active * span[a]:
            e[a] = -1.0
            G.append(e)
    if G:
        A = np.array(G).T
        lam, _ = nnls(A, gf)
        res = gf - A @ lam
    else:
        res = gf
    return float(np.max(np.abs(res)) / (1.0 + np.max(np.abs(gf))))
