"""Host-side mirror of the reference's Bayesian real-time optimisation loop (models/BayesRTOjax.py) on GP_Classic.

    GP_m = BayesRTOjax.BayesianOpt(plant_system)                       # + grid=(G, G): acquisition grid points per axis
    X, Y = GP_m.Data_sampling(n_sample, x_i, r)
    GP_m.GP_initialization(X, Y, 'RBF', multi_hyper=10, var_out=True)
    data = GP_m.RTOminimize(n_iter, x_i, TR_parameters, multi_start, b)

The reference's acquisition (``minimize_acquisition``, :17-85) minimises the objective's LCB subject to every constraint's
LCB >= 0 inside the ball of radius r around x_0, by SLSQP multistarts.  Here it is one device sweep (``sbo_sweep_tr``) of a G^d
grid on the ball's bounding box [x_0 - r, x_0 + r] under the zero-prior model of GP_Classic.

The reference cannot run as written; this mirror reads it as follows:
  * missing argument: ``GP_inference_jit(x)`` / ``GP_inference(x)`` omit the required ``inference_dataset`` (:88, :96, :201,
    :239-240); the mirror passes ``self.inference_datasets``;
  * stay candidate: ``localsol = [x_0.tolist()]`` puts a point among displacements (:35); the mirror's stay candidate is the
    displacement d = 0, valued at ``plant_temporary[0][0]`` (:36);
  * move or stay: the sweep's minimiser replaces the stay candidate only if its LCB is strictly smaller (argmin keeps the first
    of equal values, :82); with no safe grid point inside the ball, d = 0;
  * ``multi_start`` is accepted and ignored: the grid replaces the multistart;
  * ball: the reference's constraint r - ||d + 1e-8|| >= 0 (:104-107) becomes the sweep's unshifted ||x - x_0|| <= r, so a grid
    point within about 1e-8 of the sphere may be admitted here that the reference rejects (``TR_constraint`` keeps the shift);
  * kept exactly: ``update_TR`` with ``plant_temporary`` and the +1e-8 in rho's denominator (:212-259), the order "update_TR
    before add_sample" (:160-164), and ``calculate_GP_cons`` evaluated at ``x_initial`` as the loop does (:153).
"""
from __future__ import annotations

import numpy as np

from . import GP_Classic
from ._lib import EmptySafeSetError


class BayesianOpt(GP_Classic.GP):
    def __init__(self, plant_system, grid=None, device: int = 0, dtype: str = "f64", seed: int = 42, refine: bool = False):
        GP_Classic.GP.__init__(self, plant_system, device=device, dtype=dtype, seed=seed)
        self.grid = None if grid is None else tuple(int(g) for g in grid)
        self.refine = bool(refine)    # the acquisition's winner, x_0 and multi_start ball draws are refined off the grid
        self._ms_rng = np.random.default_rng(seed)

    # ---- acquisition (models/BayesRTOjax.py:17-107) ----------------------------------------------------------------
    def _grid_counts(self):
        g = self.grid if self.grid is not None else (101,) * self.nx_dim
        if len(g) != self.nx_dim or min(g) < 1:
            raise ValueError("grid must give a positive point count per input axis")
        return g

    def _acquisition_sweep(self, r, x_0, b):
        """argmin of lcb_0 over the grid points of the ball with every constraint's lcb >= 0: (index, x, lcb), index -1 if none."""
        x_0 = np.asarray(x_0, dtype=np.float64)
        self._sync_model()
        self.engine.set_grid(x_0 - r, x_0 + r, self._grid_counts())
        try:
            res = self.engine.sweep_tr(b, x_0, r)
        except EmptySafeSetError:
            return -1, None, np.inf
        if res["index"] < 0:
            return -1, None, np.inf
        return res["index"], res["x"], res["lcb"]

    def minimize_acquisition(self, r, x_0, data_storage, b=0, multi_start=5, refine=None):
        """(d, value): the displacement from x_0 of the acquisition's minimiser and its LCB, or (0, plant_temporary[0][0]).
        ``refine`` (default: the constructor's): the sweep's winner, x_0 and ``multi_start`` points drawn in the ball are refined
        off the grid (SweepEngine.refine); draws that are not safe under the model are dropped by their status.  The refined point
        is taken only if x_0 + d itself is safe under the model, inside the ball and no worse than the grid answer."""
        x_0 = np.asarray(x_0, dtype=np.float64)
        stay = float(data_storage.data["plant_temporary"][0][0])
        index, x, lcb = self._acquisition_sweep(r, x_0, b)
        if (self.refine if refine is None else bool(refine)) and r > 0:
            seeds = ([x] if index >= 0 else []) + [x_0]
            m = int(multi_start)
            if m > 0:
                dirs = self._ms_rng.standard_normal((m, self.nx_dim))
                dirs /= np.maximum(np.linalg.norm(dirs, axis=1, keepdims=True), 1e-300)
                rad = r * self._ms_rng.uniform(size=(m, 1)) ** (1.0 / self.nx_dim)
                seeds += list(x_0 + rad * dirs)
            out = self.engine.refine(b, np.asarray(seeds), 0, "lcb", lo=x_0 - r, hi=x_0 + r, x_0=x_0, r=r)
            if out["best"] >= 0:
                # the caller applies x_0 + d: that point, not the refined one, must be safe (x_0 + (x - x_0) need not round to x)
                xa = x_0 + (out["best_x"] - x_0)
                self.engine.set_points(xa[None, :])
                lcb_a = [float(self.engine.bounds(b, c, "lcb")[0]) for c in range(self.n_fun)]
                if all(v >= 0.0 for v in lcb_a[1:]) and np.sqrt(np.sum((xa - x_0) ** 2)) <= r and lcb_a[0] <= lcb:
                    index, x, lcb = out["best"], xa, lcb_a[0]
        if index >= 0 and lcb < stay:
            return x - x_0, lcb
        return np.zeros_like(x_0), stay

    def obj_fun(self, x, b):
        mean, var = self.GP_inference(np.asarray(x, dtype=np.float64), self.inference_datasets)
        return mean[0] - b * np.sqrt(var[0])

    def constraint(self, x, b, index):
        mean, var = self.GP_inference(np.asarray(x, dtype=np.float64), self.inference_datasets)
        return mean[index] - b * np.sqrt(var[index])

    def TR_constraint(self, d, r):
        return r - np.linalg.norm(np.asarray(d) + 1e-8)

    # ---- real-time optimisation (models/BayesRTOjax.py:113-259) ------------------------------------------------------
    def RTOminimize(self, n_iter, x_initial, TR_parameters, multi_start, b):
        keys = ["i", "x_initial", "x_new", "plant_output", "GP_cons", "GP_cons_safe", "TR_radius", "plant_temporary"]
        data_storage = DataStorage(keys)
        x_initial = np.asarray(x_initial, dtype=np.float64)
        radius = TR_parameters["radius"]
        plant_output = self.calculate_plant_outputs(x_initial)
        GP_cons, GP_cons_safe = self.calculate_GP_cons(x_initial, b)
        data_storage.add_data_points(self.create_data_points(0, x_initial, x_initial, plant_output, GP_cons, GP_cons_safe, radius))
        data_storage.data["plant_temporary"].append(plant_output.tolist())
        for i in range(n_iter):
            d_new, obj = self.minimize_acquisition(radius, x_initial, data_storage, multi_start=multi_start, b=b)
            plant_output = self.calculate_plant_outputs(x_initial + d_new)
            GP_cons, GP_cons_safe = self.calculate_GP_cons(x_initial, b)
            data_storage.add_data_points(self.create_data_points(i + 1, x_initial, x_initial + d_new, plant_output, GP_cons,
                                                                 GP_cons_safe, radius))
            x_new, radius_new = self.update_TR(x_initial, x_initial + d_new, radius, TR_parameters, data_storage)
            self.add_sample(x_initial + d_new, plant_output)
            x_initial = np.asarray(x_new, dtype=np.float64)
            radius = radius_new
        return data_storage.get_data()

    def create_data_points(self, iter, x_initial, x_new, plant_output, GP_cons, GP_cons_safe, radius):
        return {"i": iter, "x_initial": np.asarray(x_initial).tolist(), "x_new": np.asarray(x_new).tolist(),
                "plant_output": np.asarray(plant_output).tolist(), "GP_cons": np.asarray(GP_cons).tolist(),
                "GP_cons_safe": np.asarray(GP_cons_safe).tolist(), "TR_radius": radius}

    def calculate_plant_outputs(self, x):
        return np.array([plant(x) for plant in self.plant_system])

    def calculate_GP_cons(self, x, b):
        cons, cons_safe = [], []
        if self.n_fun > 1:
            mean, var = self.GP_inference(np.asarray(x, dtype=np.float64), self.inference_datasets)
            for i in range(1, self.n_fun):
                cons.append(mean[i])
                cons_safe.append(mean[i] - b * np.sqrt(var[i]))
        return np.array(cons), np.array(cons_safe)

    def update_TR(self, x_initial, x_new, radius, TR_parameters, data_storage):
        r = radius
        for i in range(self.n_fun - 1):
            if data_storage.data["plant_output"][-1][i + 1] < 0:
                return x_initial, r * TR_parameters["radius_red"]
        plant_previous = data_storage.data["plant_temporary"][0][0]
        plant_now = data_storage.data["plant_output"][-1][0]
        GP_previous = self.GP_inference(np.asarray(x_initial, dtype=np.float64), self.inference_datasets)[0][0]
        GP_now = self.GP_inference(np.asarray(x_new, dtype=np.float64), self.inference_datasets)[0][0]
        rho = (plant_now - plant_previous) / (GP_now - GP_previous + 1e-8)
        if plant_previous < plant_now:
            return x_initial, r * TR_parameters["radius_red"]
        if rho < TR_parameters["rho_lb"]:
            return x_initial, r * TR_parameters["radius_red"]
        elif rho < TR_parameters["rho_ub"]:
            data_storage.data["plant_temporary"][0][0] = plant_now
            return x_new, r
        data_storage.data["plant_temporary"][0][0] = plant_now
        return x_new, min(r * TR_parameters["radius_inc"], TR_parameters["radius_max"])


class DataStorage:
    def __init__(self, keys):
        self.data = {}
        for key in keys:
            if type(key) == str:       # noqa: E721  (the reference's check, models/BayesRTOjax.py:266)
                self.data[key] = []
            else:
                raise TypeError(f"Key '{key}' is not a string type")

    def add_data_points(self, data_dict):
        for key, new_data_point in data_dict.items():
            if key in self.data:
                self.data[key].append(new_data_point)
            else:
                raise KeyError(f"Key '{key}' not found in data sets")

    def get_data(self):
        for i in self.data.keys():
            self.data[i] = np.array(self.data[i])
        return self.data
