"""NumPy restatement of GP_Classic's hyper-parameter fit (models/GP_Classic.py:168-240) -- test infrastructure for
tests/test_classic_cpu.py, tests/test_gpu_fit_local.py and tools/fit_bench.py.

The objective is ``oracle.negative_loglikelihood`` (GP_Classic's NLL is GP_Safe's expression).  Its analytic gradient, with
alpha = K^-1 y, Q = K^-1 - alpha alpha^T and Kf the noise-free part of K:
    dNLL/dh_a     = sum_ik Q_ik Kf_ik (x_ia - x_ka)^2 / W_a      (a < d, W_a = exp(2 h_a))
    dNLL/dh_d     = 2 sum_ik Q_ik Kf_ik
    dNLL/dh_{d+1} = 2 sn2 tr Q                                  (sn2 = exp(2 h_{d+1}))
The reference's fit: SciPy SLSQP from each start with jac = grad(NLL), bounds [-4, 4]^(d+1) x [-8, -2], tol = float32 eps,
maxiter 10000; the best start per output by argmin (first of equal values).
"""
import numpy as np
from scipy.optimize import minimize

import oracle

FLOAT32_EPS = float(np.finfo(np.float32).eps)


def classic_bounds(d):
    """models/GP_Classic.py:205-208."""
    return np.array([[-4.0, 4.0]] * (d + 1) + [[-8.0, -2.0]])


def _parts(hyper, X_norm, y):
    X_norm = np.asarray(X_norm, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n, d = X_norm.shape
    h = np.asarray(hyper, dtype=np.float64)
    W, sf2, sn2 = np.exp(2 * h[:d]), np.exp(2 * h[d]), np.exp(2 * h[d + 1])
    R2 = (X_norm[:, None, :] - X_norm[None, :, :]) ** 2 / W           # [n, n, d]
    Kf = sf2 * np.exp(-0.5 * R2.sum(axis=2))
    K = Kf + (sn2 + 1e-8) * np.eye(n)
    return y, R2, Kf, K, sn2


def nll_grad(hyper, X_norm, y):
    """(NLL, grad[d+2]); NLL is ``oracle.negative_loglikelihood``; (inf, NaN) when K has no Cholesky factor."""
    f = oracle.negative_loglikelihood(hyper, X_norm, y)
    d = np.asarray(X_norm).shape[1]
    if not np.isfinite(f):
        return f, np.full(d + 2, np.nan)
    y, R2, Kf, K, sn2 = _parts(hyper, X_norm, y)
    Kinv = np.linalg.inv(K)
    alpha = Kinv @ y
    Q = Kinv - np.outer(alpha, alpha)
    QK = Q * Kf
    g = np.empty(d + 2)
    g[:d] = np.einsum("ik,ika->a", QK, R2)
    g[d] = 2.0 * QK.sum()
    g[d + 1] = 2.0 * sn2 * np.trace(Q)
    return f, g


def grad_scale(hyper, X_norm, y):
    """sum_ik |Q_ik dK_ik / dh| per component: the scale of the cancellation in each gradient component."""
    y, R2, Kf, K, sn2 = _parts(hyper, X_norm, y)
    d = R2.shape[2]
    Kinv = np.linalg.inv(K)
    alpha = Kinv @ y
    A = np.abs(Kinv - np.outer(alpha, alpha))
    s = np.empty(d + 2)
    s[:d] = np.einsum("ik,ika->a", A * Kf, R2)
    s[d] = 2.0 * (A * Kf).sum()
    s[d + 1] = 2.0 * sn2 * np.trace(A)
    return s


def classic_starts(d, multi_hyper, bounds=None):
    """``multi_hyper`` points of the unscrambled Sobol sequence in d + 2 dimensions with the origin skipped, scaled into the
    bounds -- the role of sobol_seq.i4_sobol_generate at models/GP_Classic.py:211, 223."""
    from scipy.stats import qmc
    b = classic_bounds(d) if bounds is None else np.asarray(bounds, dtype=np.float64)
    pts = qmc.Sobol(d + 2, scramble=False).random(multi_hyper + 1)[1:]
    return b[:, 0] + (b[:, 1] - b[:, 0]) * pts


def slsqp_fit(X_norm, y, starts, bounds, maxiter=10000, tol=FLOAT32_EPS):
    """models/GP_Classic.py:221-232 for one output: SLSQP with the analytic gradient from every start.  Returns
    (best_x, best_nll, per-start x [P, d+2], per-start nll [P])."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)

    def fun(h):
        return oracle.negative_loglikelihood(h, X_norm, y)

    def jac(h):
        return nll_grad(h, X_norm, y)[1]

    xs, fs = [], []
    for h0 in np.asarray(starts, dtype=np.float64):
        res = minimize(fun, h0, method="SLSQP", jac=jac, bounds=bounds, tol=tol, options={"disp": False, "maxiter": maxiter})
        xs.append(np.asarray(res.x))
        fs.append(float(res.fun))
    fs = np.array(fs)
    best = int(np.argmin(fs))
    return xs[best], fs[best], np.array(xs), fs
