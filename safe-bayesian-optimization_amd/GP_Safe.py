"""Host-side mirror of the reference's GP model class (models/GP_Safe.py), NumPy + libsafebo.so.

Same method names, argument meaning and error behaviour as the reference ``GP`` so its drivers keep working
(``from models.GP_Safe import GP`` -> ``from safebo_amd.GP_Safe import GP``); what changes is where the
arithmetic runs: the posterior (``GP_inference``) is evaluated by the HIP kernels behind the C ABI, batched
when the caller passes many points.  Model fitting (normalisation, hyper-parameter search) is host NumPy/SciPy by
default; with ``fit_on_device = True`` the differential-evolution search evaluates its whole population per
generation with the batched device objective ``sbo_nll_batch``; ``"de"`` runs the whole search
on the device, and ``"model"`` the search of every output side by side, the polish and the model build (``sbo_model_fit``).

Differences that are deliberate and documented:
  * no JAX: ``key`` arguments are ``numpy.random.Generator`` objects (or seeds); the reference's threefry
    stream cannot be reproduced without JAX, parity is defined on given X, Y;
  * ``sobol_seq`` multistart vectors are generated with ``scipy.stats.qmc.Sobol`` (same role, unused by the
    reference's DE path as well: models/GP_Safe.py:209 builds them, :224 never reads them);
  * ``fixed_hyper=`` lets a caller skip the DE fit and install given hyper-parameters (benchmarks, tests).
"""
from __future__ import annotations

import numpy as np
from scipy.optimize import differential_evolution

from .engine import SweepEngine

FLOAT32_EPS = float(np.finfo(np.float32).eps)


class LazyInvK:
    """``invKopt`` of a model the device fitted and built itself (``fit_on_device = "model"``): a sequence of q matrices
    inv(K_i + (sn2_i + float32 eps) I), each formed from ``hypopt`` on its first read and kept -- a loop that never reads one never
    pays its O(n^3).  ``materialised`` is True once every element exists; ``SweepEngine.set_model`` uploads such a dataset with
    ``use_invK=False`` until then."""

    def __init__(self, compute, q):
        self._compute = compute      # i -> [n, n]
        self._items = [None] * q

    @property
    def materialised(self):
        return all(a is not None for a in self._items)

    def __len__(self):
        return len(self._items)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self._items)))]
        if self._items[i] is None:
            self._items[i] = self._compute(range(len(self._items))[i])
        return self._items[i]

    def __setitem__(self, i, value):
        self._items[i] = value

    def __iter__(self):
        return (self[i] for i in range(len(self._items)))


class GP:
    noise_lower_bound = -5.0     # lower bound of log sigma_n in the fit (models/GP_Safe.py:205)
    mean_prior_zero = False      # True: prior mean 0 for every output (models/GP_Robust.py:322-324)

    def __init__(self, plant_system, device: int = 0, dtype: str = "f64", seed: int = 42) -> None:
        self.plant_system = plant_system
        self.n_fun = len(plant_system)
        self.key = np.random.default_rng(seed)              # reference: jax.random.PRNGKey(42), GP_Safe.py:15
        self.inference_datasets = {"X_mean": [], "X_std": [], "Y_mean": [], "Y_std": [],
                                   "X_norm": [], "Y_norm": [], "invKopt": [], "hypopt": []}   # GP_Safe.py:16-23
        self.dtype = dtype
        self.device = device
        self._engine = None          # created lazily: constructing a GP must not require a GPU
        self._model_version = 0      # bumped by update_inference_dataset
        self._uploaded_version = -1
        self.fixed_hyper = None
        self.de_options = {}         # forwarded to scipy DE (e.g. {"seed": 0, "maxiter": 50})
        self.fit_on_device = False   # True: DE evaluates whole populations with the batched device NLL (sbo_nll_batch);
                                     # "de": the whole DE search runs on the device (sbo_fit_de), polish on the host;
                                     # "model": search, polish and model build on the device in one call (sbo_model_fit)
        self.var_out = True

    # ---- engine plumbing -----------------------------------------------------------------------------------
    @property
    def engine(self) -> SweepEngine:
        if self._engine is None:
            self._engine = SweepEngine(self.device)
        return self._engine

    def _sync_model(self):
        """Upload ``inference_datasets`` when it changed since the last upload."""
        if self._uploaded_version != self._model_version:
            self.engine.set_model(self.inference_datasets, dtype=self.dtype, kernel=self.kernel, mean_prior=self._mean_prior())
            self._uploaded_version = self._model_version
            self._cand_token = None

    def _mean_prior(self, ds=None):
        ds = self.inference_datasets if ds is None else ds
        return np.zeros(np.asarray(ds["Y_mean"]).shape[0]) if self.mean_prior_zero else None

    # ---- data sampling (models/GP_Safe.py:30-78) -------------------------------------------------------------
    def Ball_sampling(self, x_dim, n_sample, r_i, key=None):
        """Uniform samples in the ball of radius r_i around the origin: normal direction times U^(1/d) radius."""
        rng = key if isinstance(key, np.random.Generator) else np.random.default_rng(key) if key is not None else self.key
        xi = rng.standard_normal((n_sample, x_dim))
        unit = xi / np.linalg.norm(xi, axis=1, keepdims=True)
        radius = rng.uniform(size=(n_sample, 1)) ** (1.0 / x_dim)
        return r_i * radius * unit

    def Data_sampling(self, n_sample, x_0, r, noise=0.):
        x_0 = np.asarray(x_0, dtype=np.float64)
        X = self.Ball_sampling(x_0.shape[0], n_sample, r, self.key) + x_0
        Y = np.zeros((n_sample, self.n_fun))
        for i in range(n_sample):
            for j in range(self.n_fun):
                Y[i, j] = self.plant_system[j](X[i], noise)
        return X, Y

    # ---- GP operations (models/GP_Safe.py:84-245) ------------------------------------------------------------
    def data_normalization(self):
        self.X_mean, self.X_std = np.mean(self.X, axis=0), np.std(self.X, axis=0)     # population std, :92
        self.Y_mean, self.Y_std = np.mean(self.Y, axis=0), np.std(self.Y, axis=0)
        return (self.X - self.X_mean) / self.X_std, (self.Y - self.Y_mean) / self.Y_std

    def squared_seuclidean_jax(self, X, Y, V):
        """Expanded standardised squared distance; V holds the *squared* length-scales (models/GP_Safe.py:98-120)."""
        v = V ** -0.5
        Xa, Ya = X * v, Y * v
        return -2 * np.dot(Xa, Ya.T) + np.sum(Xa ** 2, axis=1)[:, None] + np.sum(Ya ** 2, axis=1)

    def Cov_mat(self, kernel, X_norm, Y_norm, W, sf2):
        if W.shape[0] != X_norm.shape[1]:
            raise ValueError("ERROR W and X_norm dimension should be same")
        elif kernel != "RBF":
            raise ValueError("ERROR no kernel with name ", kernel)
        return sf2 * np.exp(-0.5 * self.squared_seuclidean_jax(X_norm, Y_norm, W))

    def calc_Cov_mat(self, kernel, X_norm, x_norm, ell, sf2):
        x_norm = np.asarray(x_norm).reshape(1, self.nx_dim)
        if ell.shape[0] != X_norm.shape[1]:
            raise ValueError("ERROR W and X_norm dimension should be same")
        elif kernel != "RBF":
            raise ValueError("ERROR no kernel with name ", kernel)
        return sf2 * np.exp(-0.5 * self.squared_seuclidean_jax(X_norm, x_norm, ell))

    def negative_loglikelihood(self, hyper, X, Y):
        """y^T K^-1 y + log|K| with jitter 1e-8 -- no 1/2 and no constant (models/GP_Safe.py:169-192)."""
        d = self.nx_dim
        W, sf2, sn2 = np.exp(2 * hyper[:d]), np.exp(2 * hyper[d]), np.exp(2 * hyper[d + 1])
        K = self.Cov_mat(self.kernel, X, X, W, sf2) + (sn2 + 1e-8) * np.eye(self.n_point)
        K = (K + K.T) * 0.5
        try:
            L = np.linalg.cholesky(K)
        except np.linalg.LinAlgError:
            return np.inf
        alpha = np.linalg.solve(L.T, np.linalg.solve(L, Y))
        return float(np.dot(Y.T, alpha)[0][0] + 2 * np.sum(np.log(np.diag(L))))

    def determine_hyperparameters(self, X_norm, Y_norm):
        """One GP per output; bounds [-1.5, 1.5]^(d+1) x [-5, -2] searched by SciPy DE (models/GP_Safe.py:194-234),
        then invK = inv(K + (sn2 + float32 eps) I)."""
        d = self.nx_dim
        bounds = np.array([[-1.5, 1.5]] * (d + 1) + [[self.noise_lower_bound, -2.0]])
        if self.fit_on_device == "model" and self.fixed_hyper is None:
            return self._fit_model_on_device(X_norm, Y_norm, bounds)
        hypopt = np.zeros((d + 2, self.ny_dim))
        invKopt = []
        for i in range(self.ny_dim):
            if self.fixed_hyper is not None:
                hypopt[:, i] = np.asarray(self.fixed_hyper, dtype=np.float64)[:, i]
            elif self.fit_on_device == "de":
                # the whole DE search on the device (sbo_fit_de): SciPy's defaults as the reference uses them (popsize 15 per
                # dimension, Latin-hypercube start, best1bin, mutation (0.5, 1), recombination 0.7, tol 0.01), deferred
                # updating, then SciPy's own polish step (L-BFGS-B from the best member) on the host objective
                from scipy.optimize import minimize
                from scipy.stats import qmc
                opts = dict(self.de_options)
                seed = int(opts.get("seed", 0) or 0)
                P = int(opts.get("popsize", 15)) * (d + 2)
                pop = qmc.scale(qmc.LatinHypercube(d + 2, seed=seed).random(P), bounds[:, 0], bounds[:, 1])
                y_i = np.ascontiguousarray(Y_norm[:, i])
                best, energy, _ = self.engine.fit_de(X_norm, y_i, bounds, pop, seed=seed + i, maxiter=int(opts.get("maxiter", 1000)),
                                                     tol=float(opts.get("tol", 0.01)), atol=float(opts.get("atol", 0.0)))
                if opts.get("polish", True):
                    res = minimize(self.negative_loglikelihood, best, args=(X_norm, Y_norm[:, i:i + 1]), method="L-BFGS-B",
                                   bounds=bounds)
                    if res.fun < energy:
                        best = res.x
                hypopt[:, i] = best
            elif self.fit_on_device:
                # same objective and bounds; SciPy hands over the whole trial population (vectorized, deferred
                # updating) and the device returns one NLL per member
                y_i = np.ascontiguousarray(Y_norm[:, i])
                res = differential_evolution(lambda H: self.engine.nll_batch(X_norm, y_i, H.T), bounds=bounds,
                                             vectorized=True, updating="deferred", **self.de_options)
                hypopt[:, i] = res.x
            else:
                res = differential_evolution(self.negative_loglikelihood, args=(X_norm, Y_norm[:, i:i + 1]), bounds=bounds,
                                             **self.de_options)
                hypopt[:, i] = res.x
            invKopt.append(self._invK(X_norm, hypopt, i))
        return hypopt, invKopt

    def _invK(self, X_norm, hypopt, i):
        """inv(K_i + (sn2_i + float32 eps) I) of output i (models/GP_Safe.py:226-232)."""
        d = X_norm.shape[1]
        ell = np.exp(2.0 * hypopt[:d, i])
        sf2 = np.exp(2.0 * hypopt[d, i])
        sn2 = np.exp(2.0 * hypopt[d + 1, i]) + FLOAT32_EPS
        K = self.Cov_mat(self.kernel, X_norm, X_norm, ell, sf2) + sn2 * np.eye(X_norm.shape[0])
        return np.linalg.inv(K)

    def _fit_model_on_device(self, X_norm, Y_norm, bounds):
        """``fit_on_device = "model"``: one ``sbo_model_fit`` call -- the DE of every output side by side, the polish and the model
        build on the device -- with the population, seeds and ``de_options`` keys of the "de" mode.  The device model is then
        current (``_device_model_fitted`` makes the caller mark it so); ``invKopt`` is formed on the host only if somebody reads it."""
        from scipy.stats import qmc
        d = self.nx_dim
        opts = dict(self.de_options)
        seed = int(opts.get("seed", 0) or 0)
        P = int(opts.get("popsize", 15)) * (d + 2)
        pop = qmc.scale(qmc.LatinHypercube(d + 2, seed=seed).random(P), bounds[:, 0], bounds[:, 1])
        ds = {"X_mean": self.X_mean, "X_std": self.X_std, "Y_mean": self.Y_mean, "Y_std": self.Y_std, "X_norm": X_norm, "Y_norm": Y_norm}
        self.fit_report = self.engine.model_fit(ds, bounds, pop, seed=seed, maxiter=int(opts.get("maxiter", 1000)),
                                                tol=float(opts.get("tol", 0.01)), atol=float(opts.get("atol", 0.0)),
                                                polish=bool(opts.get("polish", True)), dtype=self.dtype, kernel=self.kernel,
                                                mean_prior=self._mean_prior(ds))
        hypopt = self.fit_report["hypopt"]
        self._device_model_fitted = True
        return hypopt, LazyInvK(lambda i: self._invK(X_norm, hypopt, i), self.ny_dim)

    def update_inference_dataset(self):
        ds = self.inference_datasets
        ds["X_mean"], ds["X_std"], ds["Y_mean"], ds["Y_std"] = self.X_mean, self.X_std, self.Y_mean, self.Y_std
        ds["X_norm"], ds["Y_norm"], ds["invKopt"], ds["hypopt"] = self.X_norm, self.Y_norm, self.invKopt, self.hypopt
        self._model_version += 1
        if self.__dict__.pop("_device_model_fitted", False):
            self._uploaded_version = self._model_version   # sbo_model_fit built this very model on the device: no upload
            self._cand_token = None

    # ---- initialisation / update (models/GP_Safe.py:251-304) ---------------------------------------------------
    def GP_initialization(self, X, Y, kernel, multi_hyper, var_out=True):
        self.X, self.Y, self.kernel = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64), kernel
        self.n_point, self.nx_dim = self.X.shape
        self.ny_dim = self.Y.shape[1]
        self.multi_hyper = multi_hyper
        self.var_out = var_out
        self._refit()

    def _refit(self):
        """The default path on the data the model holds: re-normalise, refit, rebuild (models/GP_Safe.py:283-304)."""
        self.X_norm, self.Y_norm = self.data_normalization()
        self.hypopt, self.invKopt = self.determine_hyperparameters(self.X_norm, self.Y_norm)
        self.update_inference_dataset()

    def _device_followed(self):
        """Behind an incremental update: the host state is complete again and the device model already holds it."""
        self.update_inference_dataset()              # bumps _model_version: the cached sweeps of SafeOpt / GoOSE.BO are stale
        self._uploaded_version = self._model_version  # ... but the device model is already current: no re-upload
        self._cand_token = None

    @staticmethod
    def _check_incremental_args(incremental, window, refit_when, what):
        """``window`` and ``refit_when`` of add_sample / add_samples; ``what``: how that method's default path refits."""
        if refit_when is not None:
            if not incremental:
                raise ValueError(f"refit_when needs incremental=True (the default path refits {what})")
            if not callable(refit_when):
                raise ValueError("refit_when must be callable: it receives the dict of loo()")
        if window is not None:
            if not incremental:
                raise ValueError("window needs incremental=True (the default path refits on all data)")
            if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 1:
                raise ValueError("window must be an integer >= 1")

    def _carry_lazy(self, X_norm):
        """[(i, invKopt[i])] of the outputs whose inverse exists, for an update that carries them over to the rows ``X_norm``.  A
        ``LazyInvK`` is replaced by one over those rows first: an element nobody has read stays unformed and is not in the list."""
        if not isinstance(self.invKopt, LazyInvK):
            return list(enumerate(self.invKopt))
        hypopt, old = self.hypopt, self.invKopt
        self.invKopt = LazyInvK(lambda i: self._invK(X_norm, hypopt, i), self.ny_dim)
        return [(i, P) for i, P in enumerate(old._items) if P is not None]

    def add_sample(self, x_new, y_new, incremental: bool = False, window: int | None = None, refit_when=None):
        """Reference behaviour (models/GP_Safe.py:283-304): re-normalise, refit, rebuild.  ``incremental=True`` is the
        opt-in fast path of SURVEY.md 8(f) rank 2: normalisation constants and hyper-parameters stay frozen and the device
        model gains one row in O(n^2) (``sbo_model_append``); the Python-side ``inference_datasets`` follows with the
        bordered inverse, also O(n^2).  ``window=W`` (with ``incremental=True`` only) keeps a sliding window of the W most
        recent observations: a model that already holds W of them loses its oldest (``remove_sample(0)``) before the new one
        is appended, so n never exceeds W and a model at ``SBO_MAX_N`` keeps running.  ``refit_when=fn`` (with ``incremental=True``
        only) asks whether the frozen constants still describe the data: after the update ``fn(self.loo())`` is called, and if it
        returns true the model is refitted on the data it now holds by exactly the default path (re-normalise, refit, rebuild).
        The policy is the caller's; the library fixes no threshold."""
        self._check_incremental_args(incremental, window, refit_when, "on every sample")
        if window is not None:
            while self.n_point >= window:
                self.remove_sample(0)
        self.X = np.vstack([self.X, np.asarray(x_new, dtype=np.float64)])
        self.Y = np.vstack([self.Y, np.asarray(y_new, dtype=np.float64)])
        self.n_point = self.X.shape[0]
        if incremental:
            self._sync_model()
            xn = (np.asarray(x_new, dtype=np.float64).reshape(-1) - self.X_mean) / self.X_std
            yn = (np.asarray(y_new, dtype=np.float64).reshape(-1) - self.Y_mean) / self.Y_std
            self.engine.append_sample(xn, yn)
            # the host copy of the model follows: bordered inverse of K + sn2 I under the frozen hyper-parameters, so that
            # ``inference_datasets`` stays a complete, uploadable state (X_norm [n+1, d] next to invKopt [n+1, n+1])
            d = self.nx_dim
            for i in range(self.ny_dim):
                ell, sf2 = np.exp(2.0 * self.hypopt[:d, i]), np.exp(2.0 * self.hypopt[d, i])
                sn2 = np.exp(2.0 * self.hypopt[d + 1, i]) + FLOAT32_EPS
                k = self.Cov_mat(self.kernel, self.X_norm, xn[None, :], ell, sf2)[:, 0]
                u = self.invKopt[i] @ k
                s = (sf2 + sn2) - float(k @ u)
                self.invKopt[i] = np.block([[self.invKopt[i] + np.outer(u, u) / s, -u[:, None] / s],
                                            [-u[None, :] / s, np.array([[1.0 / s]])]])
            self.X_norm = np.vstack([self.X_norm, xn])
            self.Y_norm = np.vstack([self.Y_norm, yn])
            self._device_followed()
            if refit_when is None or not refit_when(self.loo()):
                return
        self._refit()

    def add_samples(self, X_new, Y_new, incremental: bool = True, window: int | None = None, refit_when=None):
        """k observations at once -- the other half of ``Batch``: ``X_new`` [k, d], ``Y_new`` [k, q] in physical units.
        ``incremental=True`` (the default here) normalises them with the frozen constants and makes one ``append_samples`` call
        (``sbo_model_append_batch``: one block update of the device model); the Python-side ``inference_datasets`` follows with the
        block-bordered inverse per output, [[invK + U S^-1 U^T, -U S^-1], [-S^-1 U^T, S^-1]] with U = invK K(X, X_new) and
        S = K(X_new, X_new) + sn2 I - K(X_new, X) U; an element of a ``LazyInvK`` nobody has read stays unformed, now over all rows.
        More than ``SBO_MAX_APPEND`` rows are split into consecutive blocks here.  ``window=W`` (1 <= k < W) removes the
        ``max(0, n + k - W)`` oldest observations (``remove_sample(0)``) before the append, so n never exceeds W.  ``refit_when`` is
        asked once, after the block, as in ``add_sample``.  ``incremental=False`` stacks the rows and runs the default path once
        (re-normalise, refit, rebuild) -- the reference, fed the same rows one by one, would have refitted k times."""
        from ._lib import SBO_MAX_APPEND
        X_new, Y_new = np.asarray(X_new, dtype=np.float64), np.asarray(Y_new, dtype=np.float64)
        if X_new.ndim != 2 or Y_new.ndim != 2 or X_new.shape[1] != self.nx_dim or Y_new.shape[1] != self.ny_dim \
                or X_new.shape[0] != Y_new.shape[0]:
            raise ValueError("X_new must be [k, d] and Y_new [k, q]")
        k = X_new.shape[0]
        if k < 1:
            raise ValueError("add_samples needs at least one row")
        if not (np.all(np.isfinite(X_new)) and np.all(np.isfinite(Y_new))):
            raise ValueError("X_new and Y_new must be finite")
        self._check_incremental_args(incremental, window, refit_when, "on the stacked data")
        if window is not None:
            if not k < window:
                raise ValueError(f"a block of k = {k} rows needs window > k")
            for _ in range(max(0, self.n_point + k - int(window))):
                self.remove_sample(0)
        if not incremental:
            self.X, self.Y = np.vstack([self.X, X_new]), np.vstack([self.Y, Y_new])
            self.n_point = self.X.shape[0]
            self._refit()
            return
        self._sync_model()
        d = self.nx_dim
        for b0 in range(0, k, SBO_MAX_APPEND):
            xn = (X_new[b0:b0 + SBO_MAX_APPEND] - self.X_mean) / self.X_std
            yn = (Y_new[b0:b0 + SBO_MAX_APPEND] - self.Y_mean) / self.Y_std
            self.engine.append_samples(xn, yn)
            X_norm = np.vstack([self.X_norm, xn])
            for i, P in self._carry_lazy(X_norm):       # (what nobody has read stays unformed, now over all rows)
                ell, sf2 = np.exp(2.0 * self.hypopt[:d, i]), np.exp(2.0 * self.hypopt[d, i])
                sn2 = np.exp(2.0 * self.hypopt[d + 1, i]) + FLOAT32_EPS
                B = self.Cov_mat(self.kernel, self.X_norm, xn, ell, sf2)
                Z = self.Cov_mat(self.kernel, xn, xn, ell, sf2) + sn2 * np.eye(xn.shape[0])
                U = P @ B
                # (kept exactly symmetric: an asymmetry of P would enter the border through U = P B and grow from block to block)
                Sinv = np.linalg.inv(Z - B.T @ U)
                Sinv = 0.5 * (Sinv + Sinv.T)
                USinv = U @ Sinv
                top = P + USinv @ U.T
                self.invKopt[i] = np.block([[0.5 * (top + top.T), -USinv], [-USinv.T, Sinv]])
            self.X = np.vstack([self.X, X_new[b0:b0 + SBO_MAX_APPEND]])
            self.Y = np.vstack([self.Y, Y_new[b0:b0 + SBO_MAX_APPEND]])
            self.X_norm, self.Y_norm = X_norm, np.vstack([self.Y_norm, yn])
            self.n_point = self.X.shape[0]
        self._device_followed()
        if refit_when is not None and refit_when(self.loo()):
            self._refit()

    def remove_sample(self, index: int):
        """The mirror of ``add_sample(..., incremental=True)``: observation ``index`` leaves the model under the frozen
        normalisation constants and hyper-parameters, O(n^2) on the device (``sbo_model_remove``).  The Python-side
        ``inference_datasets`` follows: with the old inverse split into A (without row and column ``index``), b (that column
        without its diagonal entry) and c (the diagonal entry), the inverse of K without the observation is A - b b^T / c."""
        n = self.n_point
        if isinstance(index, bool) or not isinstance(index, (int, np.integer)) or not 0 <= index < n:
            raise ValueError(f"index {index!r} out of range [0, {n})")
        if n == 1:
            raise ValueError("a model holds at least one observation")
        index = int(index)
        self._sync_model()
        self.engine.remove_sample(index)
        keep = np.arange(n) != index
        X_norm = self.X_norm[keep]
        for i, P in self._carry_lazy(X_norm):           # (what nobody has read stays unformed, now over the remaining rows)
            b = P[keep, index]
            self.invKopt[i] = P[np.ix_(keep, keep)] - np.outer(b, b) / P[index, index]
        self.X, self.Y = self.X[keep], self.Y[keep]
        self.X_norm, self.Y_norm = X_norm, self.Y_norm[keep]
        self.n_point = n - 1
        self._device_followed()

    def loo(self, b=None):
        """Leave-one-out diagnostics of the model as it stands (``sbo_model_loo``: one O(n^2) pass over the device model's factor,
        nothing is changed).  Physical units: ``mean`` [n, q] = Y - resid Y_std, the prediction of every observation from all the
        others, and ``var`` [n, q] = var Y_std^2 (noise included).  ``z`` [n, q] and the per-output summaries ``logdet``, ``lpd``,
        ``z_max``, ``z_argmax``, ``outside`` (= #{|z_i| > b}) and ``nll`` (the fit objective's form at the frozen hyper-parameters)
        are the engine's, in normalised units.  ``b`` defaults to the instance's ``b`` where the class has one, else 3.0."""
        if b is None:
            b = getattr(self, "b", 3.0)
        self._sync_model()
        d = self.engine.model_loo(b, self.Y_norm)
        out = {"mean": self.Y - d["resid"] * self.Y_std, "var": d["var"] * self.Y_std ** 2}
        for k in ("z", "logdet", "lpd", "z_max", "z_argmax", "outside", "nll"):
            out[k] = d[k]
        return out

    # ---- inference (models/GP_Safe.py:310-352) -----------------------------------------------------------------
    def GP_inference(self, x, inference_dataset=None):
        """Posterior of every output at ``x``.  ``x`` of shape [d] returns (mean[q], var[q]) like the reference
        (or the scalar objective mean when ``var_out`` is False, models/GP_Safe.py:349-352); ``x`` of shape [N, d]
        is the batched form the reference reaches with ``vmap`` and returns (mean[N, q], var[N, q])."""
        if inference_dataset is not None and inference_dataset is not self.inference_datasets:
            eng = self.engine
            eng.set_model(inference_dataset, dtype=self.dtype, kernel=getattr(self, "kernel", "RBF"),
                          mean_prior=self._mean_prior(inference_dataset))
            self._uploaded_version = -1
        else:
            self._sync_model()
        x = np.asarray(x, dtype=np.float64)
        single = x.ndim == 1
        pts = x.reshape(1, -1) if single else x
        self.engine.set_points(pts)
        self._cand_token = None
        mean, var = self.engine.posterior()
        if single:
            if self.var_out:
                return mean[0], var[0]
            return mean[0].flatten()[0]
        return mean, var
