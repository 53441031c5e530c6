"""Host-side mirror of the reference's SafeOpt class (models/SafeOpt.py) on the MI355X sweep engine.

The reference poses S_t / M_t / G_t as continuous constrained problems and solves each with SciPy differential
evolution, one posterior evaluation per Python callback (models/SafeOpt.py:47-124).  Here the same definitions are
evaluated on a candidate grid over ``bound`` by one device sweep; the class keeps the
reference's method names and return conventions so ``test/test_SafeOpt.py``-style drivers run unchanged:

    GP_m = SafeOpt.BO(plant_system, bound, b)                 # + grid=(n0, n1, ..) candidates per axis
                                                              #   or candidates=pts, an [N, d] array of scattered points
    minimizer, std_minimizer = GP_m.Minimizer()
    expander, std_expander = GP_m.Expander()

``mean/ucb/lcb(x, i)`` accept one point [d] (returns a scalar, as the reference) or many [N, d] (the
``vmap(GP_m.lcb, in_axes=(0, None))(points, 1)`` call of test/test_SafeOpt.py:337 becomes ``GP_m.lcb(points, 1)``).
"""
from __future__ import annotations

import numpy as np

from .GP_Safe import GP


class BO(GP):
    def __init__(self, plant_system, bound, b, grid=None, device: int = 0, dtype: str = "f64",
                 reference_quirk_L_index: bool = True, seed: int = 42, candidates=None, list_index: int | None = None,
                 refine: bool = False, lipschitz: str = "grid", expanders: str = "lipschitz", expander_sources: int = 4096):
        GP.__init__(self, plant_system, device=device, dtype=dtype, seed=seed)
        if lipschitz not in ("grid", "box"):
            raise ValueError("lipschitz must be 'grid' or 'box'")
        if expanders not in ("lipschitz", "hallucinated"):
            raise ValueError("expanders must be 'lipschitz' or 'hallucinated'")
        if isinstance(expander_sources, bool) or not isinstance(expander_sources, (int, np.integer)) or expander_sources < 1:
            raise ValueError("expander_sources must be an integer >= 1")
        if expanders == "hallucinated" and refine:
            raise ValueError("refine=True needs expanders='lipschitz': the pair refinement is built on the Lipschitz link")
        # "lipschitz": G_t is the sweep's, the reference's rule.  "hallucinated": Expander() decides by SweepEngine.expander_gain
        #  among the ``expander_sources`` most uncertain safe candidates that could win the acquisition
        self.expanders = expanders
        self.expander_sources = int(expander_sources)
        self.expander_witness = None
        # "grid": L_i is the sweep's, the maximum over the candidates.  "box": the larger of that and SweepEngine.lipschitz over
        # ``bound`` -- a multistart lower bound of the box maximum; the sweeps' own L does not change
        self.lipschitz = lipschitz
        self._box_L_cache = None      # (model_version, L [q])
        self.refine = bool(refine)    # acquisitions polish the sweep's winner off the grid (SweepEngine.refine)
        self.bound = np.asarray(bound, dtype=np.float64)
        self.b = b
        d = self.bound.shape[0]
        if grid is not None and candidates is not None:
            raise ValueError("pass either grid= or candidates=, not both")
        # scattered candidates [N, d] (for d >= 5 a tensor grid cannot resolve the box): masks are flat, in the caller's order, and
        # Minimizer / Expander / Target / explore_safeset return rows of them.  Lists above 2^21 points take the spatial index of
        # the list (engine option "list_index", passed through when given here).
        self.candidates = None
        if candidates is not None:
            pts = np.asarray(candidates)
            pts = np.ascontiguousarray(pts if pts.dtype == np.float32 else pts.astype(np.float64))
            if pts.ndim != 2 or pts.shape[1] != d or pts.shape[0] < 1:
                raise ValueError(f"candidates must be [N, {d}]")
            self.candidates = pts
        self.list_index = list_index
        # candidate grid over the box; default = the 400 points per axis of create_data_for_plot (test_SafeOpt.py:325)
        self.grid = None if self.candidates is not None else tuple(int(g) for g in (grid if grid is not None else (400,) * d))
        self.reference_quirk_L_index = reference_quirk_L_index
        self._sweep_cache = None      # (model_version, result dict)
        self._cand_token = None

    # ---- plant ------------------------------------------------------------------------------------------------
    def calculate_plant_outputs(self, x, noise=0):
        return np.array([plant(x, noise) for plant in self.plant_system])

    # ---- bounds (models/SafeOpt.py:29-45) ------------------------------------------------------------------------
    def _bound_value(self, x, i, kind):
        x = np.asarray(x, dtype=np.float64)
        single = x.ndim == 1
        self._sync_model()
        self.engine.set_points(x.reshape(1, -1) if single else x)
        self._cand_token = None
        out = self.engine.bounds(self.b, i, kind)
        return out[0] if single else out

    def mean(self, x, i):
        return self._bound_value(x, i, "mean")

    def ucb(self, x, i):
        return self._bound_value(x, i, "ucb")

    def lcb(self, x, i):
        return self._bound_value(x, i, "lcb")

    def lcb_constraint_min(self, x):
        """max over the constraints of lcb_i(x) -- '<= 0' therefore means every constraint LCB is <= 0
        (models/SafeOpt.py:73-77)."""
        return max(self.lcb(x, i) for i in range(1, self.n_fun))

    # ---- the sweep ----------------------------------------------------------------------------------------------
    def _grid_resident(self):
        self._sync_model()
        if self.list_index is not None:
            self.engine.set_option("list_index", int(self.list_index))
        token = (self._model_version, self.grid)
        if self._cand_token != token:
            if self.candidates is not None:
                self.engine.set_points(self.candidates)
            else:
                self.engine.set_grid(self.bound[:, 0], self.bound[:, 1], self.grid)
            self._cand_token = token

    def sweep(self, want_masks: bool = False) -> dict:
        """One SafeOpt iteration on the candidate grid (cached until the model changes)."""
        if self._sweep_cache is not None and self._sweep_cache[0] == (self._model_version, self.grid) and not want_masks:
            return self._sweep_cache[1]
        self._grid_resident()
        res = self.engine.sweep_safeopt(self.b, quirk_L_index=self.reference_quirk_L_index, want_masks=want_masks)
        self._sweep_cache = ((self._model_version, self.grid), res)
        return res

    def masks(self) -> dict:
        """S / U / M / G_c masks of the current model, reshaped to the grid (axis 0 fastest -> last array axis); flat, in the
        caller's order, with ``candidates=``."""
        self.sweep(want_masks=True)
        shape = self.grid[::-1] if self.candidates is None else (self.candidates.shape[0],)
        out = {k: self.engine.mask(k).reshape(shape) for k in ("S", "U", "M")}
        for c in range(1, self.n_fun):
            out[f"G{c}"] = self.engine.mask("G", c).reshape(shape)
        return out

    # ---- acquisition (models/SafeOpt.py:47-124) --------------------------------------------------------------------
    def minimize_obj_ucb(self, safe_set_cons=None, refine=None):
        """min over S_t of ucb_0 -> (x, value); ``safe_set_cons`` is accepted for signature parity and ignored:
        the safe-set constraints are the sweep's S mask.  ``refine`` (default: the constructor's): the sweep's arg-min is
        refined off the grid under the same constraints (the sweep's sets are not changed)."""
        res = self.sweep(want_masks=True)
        S = self.engine.mask("S")
        ucb0 = self.engine.bounds(self.b, 0, "ucb")
        g = int(np.argmin(np.where(S, ucb0, np.inf)))
        if self._refining(refine):
            return self._refine_from([self._grid_point(g)], "ucb", (self._grid_point(g), res["u_star"]))
        return self._grid_point(g), res["u_star"]

    def _refining(self, refine):
        return self.refine if refine is None else bool(refine)

    def _refine_from(self, seeds, kind, fallback, x_0=None, r=None, lo=None, hi=None):
        """(best_x, best_value) of SweepEngine.refine from ``seeds`` (objective output 0, every constraint), or ``fallback``
        when no seed is usable."""
        self._sync_model()
        out = self.engine.refine(self.b, np.asarray(seeds, dtype=np.float64), 0, kind,
                                 lo=self.bound[:, 0] if lo is None else lo, hi=self.bound[:, 1] if hi is None else hi, x_0=x_0, r=r)
        if out["best"] < 0:
            return fallback
        return out["best_x"], out["best_value"]

    def Minimizer(self, refine=None):
        """argmax over M_t of var_0 -> (x, std).  ``refine`` (default: the constructor's): the level of M_t is the refined u* of
        ``minimize_obj_ucb(refine=True)``, and the grid's minimiser and that call's arg-min (lcb_0 <= u* holds there by
        construction) are refined off the grid on max var_0 s.t. lcb_c >= 0, lcb_0 <= u* (models/SafeOpt.py:53-66); the grid's
        answer when neither seed is usable."""
        res = self.sweep()
        if not self._refining(refine):
            return res["minimizer_x"], res["minimizer_std"]
        x_u, u_star = self.minimize_obj_ucb(refine=True)
        out = self.engine.refine_sets(self.b, np.stack([res["minimizer_x"], np.asarray(x_u, dtype=np.float64)]), objective=0, kind="var",
                                      maximize=True, level=(0, u_star), lo=self.bound[:, 0], hi=self.bound[:, 1])
        if out["best"] < 0:
            return res["minimizer_x"], res["minimizer_std"]
        return out["best_x"], float(np.sqrt(out["best_value"]))

    def infnorm_mean_grad(self, x, i):
        """max_a |d MEAN_i / d x_a| at one point (analytic form of jax.grad(self.mean), models/SafeOpt.py:68-71)."""
        ds = self.inference_datasets
        d = self.nx_dim
        x = np.asarray(x, dtype=np.float64)
        hyper = ds["hypopt"][:, i]
        ell, sf2 = np.exp(2 * hyper[:d]), np.exp(2 * hyper[d])
        mp = 0.0 if i == 0 else -2 * ds["Y_mean"][i] / ds["Y_std"][i]
        xn = (x - ds["X_mean"]) / ds["X_std"]
        k = self.calc_Cov_mat(self.kernel, ds["X_norm"], xn, ell, sf2)[:, 0]
        w = k * (ds["invKopt"][i] @ (ds["Y_norm"][:, i] - mp))
        grad = ds["Y_std"][i] * ((ds["X_norm"] - xn).T @ w) / ell / ds["X_std"]
        return float(np.max(np.abs(grad)))

    def mean_grad(self, points):
        """d MEAN_o / d x_a at ``points`` [N, d] (or one point [d]) -> [N, q, d], on the device (SweepEngine.mean_grad)."""
        self._sync_model()
        return self.engine.mean_grad(points)

    def maximize_infnorm_mean_grad(self, i, lipschitz=None):
        """L_i = max over the candidate grid of ||grad MEAN_i||_inf (the reference maximises over the box with DE).  ``lipschitz``
        (default: the constructor's) "box": the larger of that -- where the sweep computed it -- and the box maximum found by
        ``SweepEngine.lipschitz`` over ``bound`` from its default seeds (cached until the model changes)."""
        res = self.sweep()
        if not self._box_lipschitz(lipschitz):
            return float(res["L"][i])
        return self._max_L(res, i)

    def _box_lipschitz(self, lipschitz=None):
        mode = self.lipschitz if lipschitz is None else lipschitz
        if mode not in ("grid", "box"):
            raise ValueError("lipschitz must be 'grid' or 'box'")
        return mode == "box"

    def _box_L(self):
        """``SweepEngine.lipschitz`` over ``bound`` for every output, once per model version."""
        if self._box_L_cache is None or self._box_L_cache[0] != self._model_version:
            self._sync_model()
            self._box_L_cache = (self._model_version, self.engine.lipschitz(self.bound[:, 0], self.bound[:, 1])["L"])
        return self._box_L_cache[1]

    def _max_L(self, res, i):
        """max(the sweep's L_i, the box L_i).  (A lean sweep leaves L_0 = 0: the maximum is then the box value.)"""
        return float(max(res["L"][i], self._box_L()[i]))

    def Lipschitz_continuity_constraint(self, x, i, max_infnorm_mean_grad):
        """x = [x, x'] stacked: ucb_i(x) - L ||x - x' + 1e-8|| (models/SafeOpt.py:85-88)."""
        x = np.asarray(x, dtype=np.float64)
        d = self.nx_dim
        return self.ucb(x[:d], i) - max_infnorm_mean_grad * np.linalg.norm(x[:d] - x[d:] + 1e-8)

    def Expander(self, refine=None):
        """The most uncertain expander over the constraints -> (x, std).  ``refine`` (default: the constructor's): for every
        constraint with a non-empty G_c the pair (its grid expander, the U candidate nearest to it under the shifted norm) is
        refined off the grid on max var_0(x) s.t. x in S, x' in U and the link with the sweep's L (models/SafeOpt.py:90-124);
        a constraint whose pair is not usable keeps its grid value.  ``expander_witness`` holds (x', c, L) of the answer, or None
        when the answer is a grid value.  With ``expanders="hallucinated"`` see ``_expander_hallucinated``."""
        if self.expanders == "hallucinated":
            if self._refining(refine):
                raise ValueError("refine=True needs expanders='lipschitz': the pair refinement is built on the Lipschitz link")
            return self._expander_hallucinated()
        res = self.sweep()
        if not self._refining(refine):
            return res["expander_x"], res["expander_std"]
        self.expander_witness = None
        best_x, best_std = res["expander_x"], res["expander_std"]
        if not (res["expander_index_c"] >= 0).any():
            return best_x, best_std
        if 2 * self.nx_dim > 8:
            raise ValueError("refining a pair needs d <= 4")
        res = self.sweep(want_masks=True)
        pts, U = self._all_points(), self.engine.mask("U")
        best_x, best_std, first = res["expander_x"], -np.inf, True
        for c in range(1, self.n_fun):
            g = int(res["expander_index_c"][c - 1])
            if g < 0:
                continue
            xg, std_c, wit = pts[g], float(res["expander_std_c"][c - 1]), None
            Lc = self._sweep_L(res, c)
            h = self._nearest_in_mask(pts, U, xg)
            out = self.engine.refine_sets(self.b, xg, pts[h], objective=0, kind="var", maximize=True, link=(c, Lc),
                                          lo=self.bound[:, 0], hi=self.bound[:, 1], max_eval=self._pair_max_eval)
            if out["best"] >= 0:
                xg, std_c, wit = out["best_x"], float(np.sqrt(out["best_value"])), (out["best_xp"], c, Lc)
            if first or std_c > best_std:          # (first on ties, models/SafeOpt.py:119-122)
                best_x, best_std, self.expander_witness, first = xg, std_c, wit, False
        return best_x, best_std

    def _expander_hallucinated(self):
        """``Expander()`` under ``expanders="hallucinated"``: the SafeOpt paper's G_t, which needs no Lipschitz constant -- a safe
        candidate g is an expander when, were it measured at its optimistic value ucb_c(g), the GP would certify a candidate that
        is not safe today (``SweepEngine.expander_gain``).  Sources: the members of S whose objective std exceeds the sweep's
        minimiser std (no other source can win the acquisition), the ``expander_sources`` largest by std, ties to the lowest
        flat index; targets: every candidate outside S.  Returns the source with count > 0 of largest objective std (ties: the
        lowest flat index) and that std, and stores ``expander_witness = (x', None, None)``, x' the target it certifies best; with no such
        source, what the sweep returns for an empty G and ``expander_witness = None``.  This is not reference behaviour: the
        reference decides expanders by the Lipschitz rule."""
        res = self.sweep(want_masks=True)
        self.expander_witness = None
        d = self.bound.shape[0]
        empty = (np.zeros(d), 0.0)                                    # (the sweep's answer for an empty G: sbo_safeopt_result)
        S = self.engine.mask("S")
        std = np.sqrt(self.engine.bounds(self.b, 0, "var").astype(np.float64))
        cand = np.nonzero(S & (std > res["minimizer_std"]))[0]
        outside = np.nonzero(~S)[0]
        if cand.size == 0 or outside.size == 0:
            return empty
        order = cand[np.argsort(-std[cand], kind="stable")][:self.expander_sources]      # (stable: ties keep the lower flat index first)
        pts = self._all_points()
        out = self.engine.expander_gain(pts[order], pts[outside], self.b, return_margin=True)
        hit = np.nonzero(out["count"] > 0)[0]
        if hit.size == 0:
            return empty
        g = int(hit[0])                                               # (``order`` descends by std)
        self.expander_witness = (pts[outside[int(out["witness"][g])]], None, None)
        return pts[order[g]], float(std[order[g]])

    def Batch(self, k, pending=None, min_std=0.01):
        """``k`` points to evaluate side by side -> (X [j, d], std [j]), j <= k: the greedy batch of ``SweepEngine.batch_select``
        (GP-BUCB, "hallucinated observations") over the candidates of M u G_1 u .. u G_{q-1} of the current model.  Pick j has the
        largest std of the objective conditioned on the data, on ``pending`` [P, d] (points whose experiments are still running) and
        on the picks before it; the batch ends before a pick whose std is below ``min_std`` (default: the stopping threshold of the
        reference's loop, test/test_SafeOpt.py:178).  With k = 1 and nothing pending the std is max(minimizer std, expander std)
        of ``sweep()``.  The sets are those of the current model: they are NOT re-derived between the picks, which is the GP-BUCB
        rule.  Ties go to the lowest flat index of the candidates, whereas the reference's loop prefers the expander on a tie.
        This is not reference behaviour: the reference proposes one point per iteration."""
        from .engine import SweepEngine
        d = self.bound.shape[0]
        _, k, _, pend, min_std = SweepEngine.batch_arguments(d, self.n_fun, np.zeros((1, d)), k, 0, pending, min_std)
        self.sweep(want_masks=True)
        member = self.engine.mask("M")
        for c in range(1, self.n_fun):
            member = member | self.engine.mask("G", c)
        pool = self._all_points()[np.nonzero(member)[0]]          # (ascending flat index)
        if pool.shape[0] == 0:
            return np.empty((0, d)), np.empty(0)
        out = self.engine.batch_select(pool, k, 0, pend, min_std)
        return out["x"], out["std"]

    def Thompson(self, k, seed=0, features=1024, exact=False):
        """``k`` points to evaluate side by side by safe Thompson sampling -> (X [k, d], value [k]): ``k`` functions are drawn
        jointly from the objective's posterior (``SweepEngine.sample_paths``: pathwise conditioning on ``features`` random features,
        the draws of ``SweepEngine.path_draws(d, n, k, features, seed)``), and slot j goes to the minimiser of path j over the safe
        set S of the current model (its members in ascending flat index; ties to the lowest).  ``value`` is the path's value there.
        Proposals come in path order and may repeat; an empty S gives (empty [0, d], empty [0]).  The batch is diversified by the
        posterior itself and needs no ``b`` for the objective.  With ``exact`` the draws are exact: ``SweepEngine.posterior_joint``
        on the same pool (the posterior's full covariance and its Cholesky factor, the draws of ``SweepEngine.joint_draws(|S|, k,
        seed)``); ``features`` is not used, and a safe set above ``SBO_JOINT_MAX_POINTS`` members raises ValueError -- an exact joint
        draw cannot be chunked, and there is no fallback to the paths.  This is not reference behaviour: the reference proposes one
        point per iteration, from bounds."""
        from .engine import SweepEngine
        d = self.bound.shape[0]
        _, k, _, features, seed, _, _ = SweepEngine.path_arguments(d, self.n_fun, 0, np.zeros((1, d)), k, 0, features, seed)
        self.sweep(want_masks=True)
        pool = self._all_points()[np.nonzero(self.engine.mask("S"))[0]]          # (ascending flat index)
        if pool.shape[0] == 0:
            return np.empty((0, d)), np.empty(0)
        if exact:
            from . import _lib
            if pool.shape[0] > _lib.SBO_JOINT_MAX_POINTS:
                raise ValueError(f"Thompson(exact=True): the safe set has {pool.shape[0]} members, above SBO_JOINT_MAX_POINTS = "
                                 f"{_lib.SBO_JOINT_MAX_POINTS}; an exact joint draw cannot be chunked (exact=False draws paths)")
            out = self.engine.posterior_joint(pool, 0, k, seed, return_cov=False)
        else:
            out = self.engine.sample_paths(pool, k, 0, features, seed)
        return out["x"], out["value"]

    def ThompsonRefined(self, k, seed=0, features=1024, starts=1):
        """``Thompson(k, seed, features)`` with every path's minimiser refined off the grid -> (X [k, d], value [k])
        (``SweepEngine.refine_paths``).  The pool and the ``sample_paths`` call are ``Thompson``'s; path s then
        starts from its own grid arg-min and, with ``starts`` = j > 1, also from those of paths s+1 .. s+j-1 (mod k) -- all members
        of S --, and moves to a local minimum of the path over the box and lcb_c >= 0 of every constraint under the class's ``b``,
        on the same draws.  The result is the best start's point and the path's value there, never worse than the grid's and
        feasible under ``lcb``.  Paths only: an exact joint draw (``Thompson(exact=True)``) is a vector, not a function, and has
        nothing to refine.  A method of its own because ``Thompson``'s signature is pinned.  This is not reference behaviour."""
        if isinstance(starts, bool) or not isinstance(starts, (int, np.integer)) or starts < 1:
            raise ValueError("starts must be an integer >= 1")
        X, value = self.Thompson(k, seed, features)
        if X.shape[0] == 0 or np.any(np.isnan(X)):       # (an empty S; a path without a value on the pool has nothing to start from)
            return X, value
        k = X.shape[0]
        seeds = X[(np.arange(k)[:, None] + np.arange(min(int(starts), k))[None, :]) % k]          # [k, j, d]
        ref = self.engine.refine_paths(self.b, seeds, 0, features, seed, lo=self.bound[:, 0], hi=self.bound[:, 1])   # (the same draws)
        return ref["best_x"], ref["best_value"]

    _pair_max_eval = 1600  # evaluations of one point per refined pair (a pair costs two, and has twice the variables)

    def _sweep_L(self, res, c):
        """The Lipschitz constant the sweep used for constraint c (models/SafeOpt.py:110: the loop-leaked index under the quirk);
        with ``lipschitz="box"`` the larger of it and the box value of the same index."""
        i = self.n_fun - 1 if self.reference_quirk_L_index else c
        return self._max_L(res, i) if self._box_lipschitz() else float(res["L"][i])

    def _all_points(self):
        """Every candidate [N, d] in the sweep's flat order (axis 0 fastest on a grid)."""
        if self.candidates is not None:
            return self.candidates.astype(np.float64)
        axes = []
        for a, cnt in enumerate(self.grid):
            lo, hi = self.bound[a]
            ax = lo + np.arange(cnt) * ((hi - lo) / (cnt - 1) if cnt > 1 else 0.0)
            if cnt > 1:
                ax[-1] = hi
            axes.append(ax)
        mesh = np.meshgrid(*axes[::-1], indexing="ij")
        return np.stack([m.reshape(-1) for m in mesh[::-1]], axis=1)

    @staticmethod
    def _nearest_in_mask(pts, mask, x, flip=False):
        """Index of the member of ``mask`` nearest to x under ||x - x_h + 1e-8|| (``flip``: ||x_h - x + 1e-8||); first on ties."""
        idx = np.nonzero(mask)[0]
        diff = (pts[idx] - x if flip else x - pts[idx]) + 1e-8
        return int(idx[np.argmin(np.sqrt(np.sum(diff * diff, axis=1)))])

    # ---- helpers ----------------------------------------------------------------------------------------------------
    def _grid_point(self, g: int):
        if self.candidates is not None:
            return self.candidates[g].astype(np.float64)
        x = np.empty(len(self.grid))
        for a, cnt in enumerate(self.grid):
            i = g % cnt
            g //= cnt
            lo, hi = self.bound[a]
            x[a] = hi if (i == cnt - 1 and cnt > 1) else lo + i * ((hi - lo) / (cnt - 1) if cnt > 1 else 0.0)
        return x
