"""NumPy / SciPy twin of sbo_mean_grad and sbo_lipschitz -- test infrastructure only.

    g_a(x)    = d MEAN_o / d x_a = Y_std_o sum_j alpha_oj k_j (X_ja - xn_a) / ell_a / X_std_a          (oracle.mean_grad)
    dg_a/dx_b = C_a sum_j alpha_oj k_j [(X_ja - xn_a)(X_jb - xn_b) / ell_b - delta_ab] / X_std_b,   C_a = Y_std_o / (ell_a X_std_a)

grad():          g at one point for one output (the twin's own formula; oracle.mean_grad is the checker);
hess_row():      row a of the mean's Hessian;
default_seeds(): the seeds SweepEngine.lipschitz builds when it is given none;
box_L():         the two stages: oracle.mean_grad at the seeds and a stable sort for the top seeds, SciPy L-BFGS-B with the analytic
                 gradient from each, oracle.mean_grad again at the results.
"""
import numpy as np
from scipy.optimize import minimize

import oracle


def _model(ds, o):
    d = ds["X_norm"].shape[1]
    hyper = ds["hypopt"][:, o]
    ell, sf2 = np.exp(2 * hyper[:d]), np.exp(2 * hyper[d])
    alpha = ds["invKopt"][o] @ (ds["Y_norm"][:, o] - oracle.mean_prior(ds)[o])
    return ell, sf2, alpha


def _weights(x, ds, o, model=None):
    """diff [n, d] = X_norm - xn and w [n] = alpha_j k_j at one point."""
    ell, sf2, alpha = _model(ds, o) if model is None else model
    xn = (np.asarray(x, dtype=np.float64) - ds["X_mean"]) / ds["X_std"]
    diff = ds["X_norm"] - xn
    return diff, alpha * sf2 * np.exp(-0.5 * np.sum(diff * diff / ell, axis=1)), ell


def grad(x, ds, o, model=None):
    """d MEAN_o / d x at one point: [d]."""
    diff, w, ell = _weights(x, ds, o, model)
    return ds["Y_std"][o] * (w @ diff) / ell / ds["X_std"]


def hess_row(x, ds, o, a, model=None):
    """d g_a / d x_b for b = 0 .. d - 1 at one point: [d]."""
    diff, w, ell = _weights(x, ds, o, model)
    d = diff.shape[1]
    inner = diff[:, a][:, None] * diff / ell - np.eye(d)[a]
    return ds["Y_std"][o] / (ell[a] * ds["X_std"][a]) * (w @ inner) / ds["X_std"]


def seeds_per_axis(d):
    """min(33, max(2, floor(4096^(1/d)))) in integers."""
    m = 2
    while m < 33 and (m + 1) ** d <= 4096:
        m += 1
    return m


def default_seeds(ds, lo, hi):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    d = lo.shape[0]
    grid = oracle.grid_points(lo, hi, [seeds_per_axis(d)] * d)
    return np.vstack([grid, np.clip(ds["X_norm"] * ds["X_std"] + ds["X_mean"], lo, hi)])


def box_L(ds, lo, hi, seeds=None, top=4, outputs=None):
    """-> dict(L [q], L_seed [q], x [q, d], evaluations, problems): the twin of SweepEngine.lipschitz."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    d, q = lo.shape[0], ds["Y_norm"].shape[1]
    S = default_seeds(ds, lo, hi) if seeds is None else np.asarray(seeds, dtype=np.float64).reshape(-1, d)
    S = S[np.all(np.isfinite(S) & (S >= lo) & (S <= hi), axis=1)]
    if S.shape[0] == 0:
        raise ValueError("no seed is finite and inside the box")
    G = oracle.mean_grad(S, ds)                                  # [S, q, d]
    span = hi - lo
    out = {"L": np.zeros(q), "L_seed": np.zeros(q), "x": np.zeros((q, d)), "evaluations": 0, "problems": 0}
    for o in (range(q) if outputs is None else outputs):
        model = _model(ds, o)
        Lseed = float(np.max(np.abs(G[:, o, :])))
        scale = Lseed if Lseed > 0 and np.isfinite(Lseed) else 1.0
        finals = []
        for a in range(d):
            if not span[a] > 0:
                continue
            for s in (1.0, -1.0):
                order = np.argsort(-s * G[:, o, a], kind="stable")[:top]
                for i in order:
                    def fun(u, s=s, a=a):                        # in box units u = (x - lo) / span (held axes stay at lo)
                        x = lo + u * span
                        return -s * grad(x, ds, o, model)[a] / scale, -s * hess_row(x, ds, o, a, model) * span / scale
                    u0 = np.where(span > 0, (S[i] - lo) / np.where(span > 0, span, 1.0), 0.0)
                    res = minimize(fun, u0, jac=True, method="L-BFGS-B", bounds=[(0.0, 1.0 if span[b] > 0 else 0.0) for b in range(d)],
                                   options={"ftol": 1e-16, "gtol": 1e-13, "maxiter": 500})
                    finals.append(np.clip(lo + res.x * span, lo, hi))
                    out["evaluations"] += int(res.nfev)
                    out["problems"] += 1
        pts = np.vstack([S] + finals) if finals else S
        A = np.abs(oracle.mean_grad(pts[S.shape[0]:], ds)[:, o, :]) if finals else np.zeros((0, d))
        A = np.vstack([np.abs(G[:, o, :]), A])
        e = int(np.argmax(np.max(A, axis=1)))
        out["L"][o], out["L_seed"][o], out["x"][o] = float(np.max(A)), Lseed, pts[e]
    return out


# ---- the configs both test files use: (synthetic config, n, fine grid per axis) -----------------------------------------------------
CASES = {"A": ("A", None, 401), "B64": ("B", 64, 401), "B300": ("B", 300, 401), "C64": ("C", 64, 401), "D128": ("D", 128, 21)}
_case_cache = {}


def case(name):
    """-> dict(ds, lo, hi, fine [q]: the largest ||grad MEAN_o||_inf on the fine grid, twin: box_L from the default seeds, top = 4);
    computed once per process."""
    if name not in _case_cache:
        from safebo_amd import synthetic
        cfg_name, n, fine = CASES[name]
        cfg = synthetic.make_config(cfg_name, n=n)
        ds, lo, hi = cfg["ds"], cfg["bound"][:, 0].copy(), cfg["bound"][:, 1].copy()
        pts = oracle.grid_points(lo, hi, [fine] * lo.shape[0])
        _case_cache[name] = {"ds": ds, "lo": lo, "hi": hi, "fine": np.max(oracle.mean_grad_infnorm(pts, ds), axis=0),
                             "twin": box_L(ds, lo, hi, top=4)}
    return _case_cache[name]
