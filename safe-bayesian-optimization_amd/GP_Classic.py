"""Host-side mirror of the reference's plain GP class (models/GP_Classic.py) on the MI355X engine.

models/GP_Classic.py is the GP that BayesRTOjax builds on.  It shares GP_Safe's objective (``negative_loglikelihood``) and
posterior formula, and differs in these ways, which this class keeps:
  * the prior mean is zero for every output (uploaded with ``sbo_model_set_prior``, as GP_Robust does);
  * the fit runs a gradient-based local search from ``multi_hyper`` starts over [-4, 4]^(d+1) x [-8, -2] (:205-208) instead of
    differential evolution.  The reference runs SciPy SLSQP with ``jac = grad(NLL)`` per start and output and keeps the best
    (:210-232).  By default every (output, start) pair is fitted in one device launch (``sbo_fit_local``: a projected BFGS
    with the analytic gradient); ``fit_on_device = False`` runs SciPy SLSQP on the host with the analytic
    gradient of ``negative_loglikelihood_grad``, as the reference does;
  * the starts are the first ``multi_hyper`` points of the unscrambled Sobol sequence after the origin, scaled into the bounds.
    The reference draws them with ``sobol_seq.i4_sobol_generate``; this class uses ``scipy.stats.qmc.Sobol(scramble=False)``,
    whose points are not claimed to equal sobol_seq's above two dimensions;
  * ``Ball_sampling`` draws directions from scrambled Sobol points of [-1, 1]^d and radii r_i U (no 1/d power, :42-48);
    ``Data_sampling`` calls each plant with ``x`` only (:50-75);
  * ``GP_inference`` with ``var_out = False`` returns the objective's mean only (:343-346).
``invKopt`` is inv(K + (sn2 + float32 eps) I) (:235-238), as in GP_Safe.
"""
from __future__ import annotations

import numpy as np
from scipy.optimize import minimize
from scipy.stats import qmc

from .GP_Safe import GP as _GPSafe, FLOAT32_EPS


class GP(_GPSafe):
    mean_prior_zero = True
    noise_lower_bound = -8.0

    def __init__(self, plant_system, device: int = 0, dtype: str = "f64", seed: int = 42) -> None:
        _GPSafe.__init__(self, plant_system, device=device, dtype=dtype, seed=seed)
        self.fit_on_device = True     # False: SciPy SLSQP per (output, start) on the host, with the analytic gradient
        self.fit_options = {}         # forwarded to SweepEngine.fit_local (maxiter, ftol, gtol)
        self.last_fit = None          # the per-start arrays of the last device fit

    # ---- data sampling (models/GP_Classic.py:29-75) -------------------------------------------------------------
    def Ball_sampling(self, x_dim, n_sample, r_i, key=None):
        rng = key if isinstance(key, np.random.Generator) else np.random.default_rng(key) if key is not None else self.key
        points = qmc.Sobol(d=x_dim, scramble=True, seed=rng).random(n=n_sample) * 2 - 1
        norm = np.linalg.norm(points, axis=-1).reshape(-1, 1)
        r = rng.uniform(size=(n_sample, 1))
        return r_i * r * points / norm

    def Data_sampling(self, n_sample, x_0, r):
        x_0 = np.asarray(x_0, dtype=np.float64)
        X = self.Ball_sampling(x_0.shape[0], n_sample, r, self.key) + x_0
        Y = np.zeros((n_sample, self.n_fun))
        for j in range(self.n_fun):
            for i in range(n_sample):
                Y[i, j] = self.plant_system[j](X[i])
        return X, Y

    # ---- hyper-parameters (models/GP_Classic.py:168-240) ------------------------------------------------------------
    def fit_bounds(self):
        d = self.nx_dim
        return np.array([[-4.0, 4.0]] * (d + 1) + [[-8.0, -2.0]])

    def fit_starts(self):
        b = self.fit_bounds()
        pts = qmc.Sobol(self.nx_dim + 2, scramble=False).random(self.multi_hyper + 1)[1:]
        return b[:, 0] + (b[:, 1] - b[:, 0]) * pts

    def negative_loglikelihood_grad(self, hyper, X, Y):
        """Analytic gradient of ``negative_loglikelihood`` (the reference's ``grad(NLL)``): with alpha = K^-1 y,
        Q = K^-1 - alpha alpha^T and Kf the noise-free K, dh_a = sum Q Kf (x_a - x'_a)^2 / W_a, dh_d = 2 sum Q Kf,
        dh_{d+1} = 2 sn2 tr Q."""
        d = self.nx_dim
        h = np.asarray(hyper, dtype=np.float64)
        y = np.asarray(Y, dtype=np.float64).reshape(-1)
        W, sf2, sn2 = np.exp(2 * h[:d]), np.exp(2 * h[d]), np.exp(2 * h[d + 1])
        R2 = (X[:, None, :] - X[None, :, :]) ** 2 / W
        Kf = sf2 * np.exp(-0.5 * R2.sum(axis=2))
        K = Kf + (sn2 + 1e-8) * np.eye(X.shape[0])
        try:
            np.linalg.cholesky(K)
        except np.linalg.LinAlgError:
            return np.full(d + 2, np.nan)
        Kinv = np.linalg.inv(K)
        alpha = Kinv @ y
        QK = (Kinv - np.outer(alpha, alpha)) * Kf
        g = np.empty(d + 2)
        g[:d] = np.einsum("ik,ika->a", QK, R2)
        g[d] = 2.0 * QK.sum()
        g[d + 1] = 2.0 * sn2 * (np.trace(Kinv) - alpha @ alpha)
        return g

    def determine_hyperparameters(self, X_norm=None, Y_norm=None):
        """Multistart local fit of every output (models/GP_Classic.py:194-240); the reference reads self.X_norm / self.Y_norm."""
        X_norm = self.X_norm if X_norm is None else X_norm
        Y_norm = self.Y_norm if Y_norm is None else Y_norm
        d = self.nx_dim
        bounds = self.fit_bounds()
        if self.fixed_hyper is not None:
            hypopt = np.array(self.fixed_hyper, dtype=np.float64).reshape(d + 2, self.ny_dim)
        elif self.fit_on_device:
            self.last_fit = self.engine.fit_local(X_norm, Y_norm, bounds, self.fit_starts(), **self.fit_options)
            hypopt = self.last_fit["best_x"].T.copy()
        else:
            hypopt = np.zeros((d + 2, self.ny_dim))
            for i in range(self.ny_dim):
                y = Y_norm[:, i:i + 1]
                localsol, localval = [], []
                for h0 in self.fit_starts():
                    res = minimize(self.negative_loglikelihood, h0, args=(X_norm, y), method="SLSQP", bounds=bounds,
                                   jac=lambda h, X, Y: self.negative_loglikelihood_grad(h, X, Y), tol=FLOAT32_EPS,
                                   options={"disp": False, "maxiter": 10000})
                    localsol.append(res.x)
                    localval.append(res.fun)
                hypopt[:, i] = localsol[int(np.argmin(localval))]
        invKopt = []
        for i in range(self.ny_dim):
            ell = np.exp(2.0 * hypopt[:d, i])
            sf2 = np.exp(2.0 * hypopt[d, i])
            sn2 = np.exp(2.0 * hypopt[d + 1, i]) + FLOAT32_EPS
            K = self.Cov_mat(self.kernel, X_norm, X_norm, ell, sf2) + sn2 * np.eye(self.n_point)
            invKopt.append(np.linalg.inv(K))
        return hypopt, invKopt
