"""Host-side mirror of the reference's GoOSE class (models/GoOSE.py) on the MI355X sweep engine.

    x_safe_min, min_safe_lcb = GP_m.minimize_obj_lcb()         # argmin_{S_t} lcb_0          models/GoOSE.py:63-67
    x_target, target_lcb     = GP_m.Target()                   # argmin over the optimistic sets   :80-114
    x_new                    = GP_m.explore_safeset(x_target)  # argmin_{S_t} ||x - target||_2     :116-119

all three read one device sweep of the candidate grid, or of ``candidates=`` (an [N, d] array of scattered points, as for
SafeOpt.BO), cached until the model changes.
"""
from __future__ import annotations

import numpy as np

from .SafeOpt import BO as _SafeOptBO


class BO(_SafeOptBO):
    def __init__(self, plant_system, bound, b, grid=None, device: int = 0, dtype: str = "f64",
                 reference_quirk_L_index: bool = True, seed: int = 42, candidates=None, list_index: int | None = None,
                 refine: bool = False, lipschitz: str = "grid"):
        _SafeOptBO.__init__(self, plant_system, bound, b, grid=grid, device=device, dtype=dtype,
                            reference_quirk_L_index=reference_quirk_L_index, seed=seed, candidates=candidates,
                            list_index=list_index, refine=refine, lipschitz=lipschitz)
        self._goose_cache = None

    def goose_sweep(self, want_masks: bool = False) -> dict:
        key = (self._model_version, self.grid)
        if self._goose_cache is not None and self._goose_cache[0] == key and not want_masks:
            return self._goose_cache[1]
        self._grid_resident()
        res = self.engine.sweep_goose(self.b, quirk_L_index=self.reference_quirk_L_index, want_masks=want_masks)
        self._goose_cache = (key, res)
        return res

    def minimize_obj_lcb(self, refine=None):
        """``refine`` (default: the constructor's): the sweep's arg-min refined off the grid under the same constraints; the
        sweep's sets (S, O_c, the target) are not changed by it."""
        res = self.goose_sweep()
        if self._refining(refine):
            return self._refine_from([res["safe_min_x"]], "lcb", (res["safe_min_x"], res["safe_min_lcb"]))
        return res["safe_min_x"], res["safe_min_lcb"]

    def Target(self, refine=None):
        """``refine`` (default: the constructor's): for every constraint with a non-empty O_c the pair (the nearest safe candidate
        that satisfies the link, its grid target) is refined off the grid on min lcb_0(x') s.t. x in S, x' in U and the link with
        the sweep's L (models/GoOSE.py:80-114); a constraint whose pair is not usable keeps its grid value.  ``target_witness``
        holds (x, c, L) of the answer, or None when the answer is a grid value."""
        res = self.goose_sweep()
        if res["target_index"] < 0:      # no optimistic point on this grid
            return np.full(self.bound.shape[0], np.nan), np.inf
        if not self._refining(refine):
            return res["target_x"], res["target_lcb"]
        if 2 * self.nx_dim > 8:
            raise ValueError("refining a pair needs d <= 4")
        self.target_witness = None
        res = self.goose_sweep(want_masks=True)
        pts, S = self._all_points(), self.engine.mask("S")
        best_x, best_lcb, first = res["target_x"], np.inf, True
        for c in range(1, self.n_fun):
            h = int(res["target_index_c"][c - 1])
            if h < 0:
                continue
            xh, lcb_c, wit = pts[h], float(res["target_lcb_c"][c - 1]), None
            Lc = self._sweep_L(res, c)
            diff = pts - xh + 1e-8
            linked = S & (self.engine.bounds(self.b, c, "ucb") - Lc * np.sqrt(np.sum(diff * diff, axis=1)) >= 0)
            if linked.any():
                g = self._nearest_in_mask(pts, linked, xh, flip=True)
                out = self.engine.refine_sets(self.b, pts[g], xh, objective=0, kind="lcb", at="xp", link=(c, Lc),
                                              lo=self.bound[:, 0], hi=self.bound[:, 1], max_eval=self._pair_max_eval)
                if out["best"] >= 0:
                    xh, lcb_c, wit = out["best_xp"], out["best_value"], (out["best_x"], c, Lc)
            if first or lcb_c < best_lcb:          # (first on ties, models/GoOSE.py:110-112)
                best_x, best_lcb, self.target_witness, first = xh, lcb_c, wit, False
        return best_x, best_lcb

    def explore_safeset(self, target, refine=None):
        """Closest safe candidate to ``target`` (cdist Euclidean, models/GoOSE.py:117).  ``refine`` (default: the
        constructor's): that candidate is refined off the grid on min ||x - target|| over the safe set."""
        res = self.goose_sweep()
        target = np.asarray(target, dtype=np.float64)
        if res["target_index"] >= 0 and np.array_equal(target, res["target_x"]):
            x = res["explore_x"]
        else:
            # (a target of the caller's own: the same arg-min on the device, over the safe set the sweep left resident)
            x = self.engine.explore_safeset(target)[1]
        if self._refining(refine) and np.all(np.isfinite(target)) and res["count_S"] > 0:
            out = self.engine.refine_sets(self.b, x, kind="dist", target=target, lo=self.bound[:, 0], hi=self.bound[:, 1])
            if out["best"] >= 0:
                return out["best_x"]
        return x
