"""SweepEngine -- thin NumPy/ctypes host object over libsafebo.so (one per process and per GPU).

Holds what crosses the seam of SURVEY.md section 8(b): the ``inference_datasets`` dict
(models/GP_Safe.py:236-245), ``b`` (models/SafeOpt.py:13) and a candidate set, and exposes the
batched calls that replace ``vmap(BO.lcb)`` (test/test_SafeOpt.py:337), ``Minimizer``/``Expander``
(models/SafeOpt.py:53-124) and ``minimize_obj_lcb``/``Target``/``explore_safeset``
(models/GoOSE.py:63-119).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

FLOAT32_EPS = float(np.finfo(np.float32).eps)

_DTYPES = {"f64": (L.SBO_F64, np.float64), "f32": (L.SBO_F32, np.float32),
           np.float64: (L.SBO_F64, np.float64), np.float32: (L.SBO_F32, np.float32)}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


class SweepEngine:
    def __init__(self, device: int = 0):
        self._lib = L.load()
        self._ctx = C.c_void_p()
        L.check(self._lib.sbo_init(int(device), C.byref(self._ctx)))
        self.device = int(device)
        self.tag, self.np_dtype = _DTYPES["f64"]
        self.n = self.d = self.q = 0
        self.n_local = 0
        self.first = 0
        self.world, self.rank = 1, 0
        self._obs = None       # (X_norm, X_mean, X_std) of the resident model: the observations among lipschitz's default seeds

    # ---- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._lib.sbo_shutdown(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def synchronize(self):
        L.check(self._lib.sbo_synchronize(self._ctx))

    def set_option(self, key: str, value: int):
        L.check(self._lib.sbo_set_option(self._ctx, key.encode(), int(value)))

    # ---- multi-GPU ---------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(L.SBO_COMM_ID_BYTES)
        L.check(L.load().sbo_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, world: int, rank: int, uid: bytes | None):
        buf = C.create_string_buffer(uid, L.SBO_COMM_ID_BYTES) if uid is not None else None
        L.check(self._lib.sbo_comm_init(self._ctx, int(world), int(rank), buf))
        self.world, self.rank = int(world), int(rank)

    def comm_barrier(self):
        L.check(self._lib.sbo_comm_barrier(self._ctx))

    # ---- model -------------------------------------------------------------------------------
    def set_model(self, ds: dict, dtype="f64", kernel: str = "RBF", use_invK: bool = True, mean_prior=None):
        """Upload the ``inference_datasets`` dict.  ``use_invK=False`` lets the library factor
        K + (sn2 + float32 eps) I itself (Cholesky, contraction with L^-1).  ``mean_prior`` [q] (normalised units) replaces
        GP_Safe's prior mean (0 for the objective, -2 Y_mean / Y_std for the constraints); models/GP_Robust.py uses zeros."""
        self.tag, self.np_dtype = _DTYPES[dtype]
        if use_invK and getattr(ds.get("invKopt"), "materialised", True) is False:
            use_invK = False         # a lazy invKopt nobody has read (GP_Safe.LazyInvK): the library factors K itself
        X_norm = _f64(ds["X_norm"])
        Y_norm = _f64(ds["Y_norm"])
        if X_norm.ndim != 2 or Y_norm.ndim != 2 or X_norm.shape[0] != Y_norm.shape[0]:
            raise ValueError("X_norm / Y_norm must be [n, d] and [n, q]")
        n, d = X_norm.shape
        q = Y_norm.shape[1]
        hyp = _f64(ds["hypopt"])
        if hyp.shape != (d + 2, q):
            raise ValueError("ERROR W and X_norm dimension should be same")   # models/GP_Safe.py:134-135
        arrs = [_f64(ds[k]) for k in ("X_mean", "X_std", "Y_mean", "Y_std")]
        if arrs[0].shape != (d,) or arrs[1].shape != (d,) or arrs[2].shape != (q,) or arrs[3].shape != (q,):
            raise ValueError("X_mean/X_std must be [d], Y_mean/Y_std must be [q]")
        args = [self._ctx, self.tag, kernel.encode(), n, d, q, _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]), _ptr(arrs[3]),
                _ptr(X_norm), _ptr(Y_norm), _ptr(hyp)]
        if mean_prior is not None:
            mp = _f64(mean_prior).reshape(-1)
            if mp.shape != (q,):
                raise ValueError("mean_prior must be [q]")
            ptrs = None
            if use_invK:
                parts = [_f64(a) for a in ds["invKopt"]]
                if len(parts) != q or any(a.shape != (n, n) for a in parts):
                    raise ValueError("invKopt must hold q matrices of shape [n, n]")
                ptrs = (C.c_void_p * q)(*[a.ctypes.data for a in parts])
            L.check(self._lib.sbo_model_set_prior(*args, ptrs, _ptr(mp)))
        elif use_invK:
            # `invKopt` is a list of q separate [n, n] arrays in the reference (models/GP_Safe.py:231-232): handed over as such
            parts = [_f64(a) for a in ds["invKopt"]]
            if len(parts) != q or any(a.shape != (n, n) for a in parts):
                raise ValueError("invKopt must hold q matrices of shape [n, n]")
            ptrs = (C.c_void_p * q)(*[a.ctypes.data for a in parts])
            L.check(self._lib.sbo_model_set_list(*args, ptrs))
        else:
            L.check(self._lib.sbo_model_set(*args, None))
        self.n, self.d, self.q = n, d, q
        self._prior = self._prior_mean(arrs[2], arrs[3], mean_prior)
        self._obs = (X_norm.copy(), arrs[0].copy(), arrs[1].copy())

    def model_fit(self, ds: dict, bounds, init_pop, seed: int = 0, maxiter: int = 1000, tol: float = 0.01, atol: float = 0.0,
                  polish: bool = True, polish_maxiter: int = 10000, polish_ftol: float = FLOAT32_EPS, polish_gtol: float = 1e-8,
                  dtype="f64", kernel: str = "RBF", mean_prior=None) -> dict:
        """Fit and build in one call (``sbo_model_fit``): ``ds`` holds the normalisation and the normalised data (``X_mean``,
        ``X_std``, ``Y_mean``, ``Y_std``, ``X_norm``, ``Y_norm`` -- no ``hypopt``, no ``invKopt``).  The DE of every output runs side
        by side on the device (output o with ``seed + o`` from ``init_pop`` [P, d+2] in the box ``bounds`` [d+2, 2]), a projected
        BFGS polishes every output's best, and the model is built as ``set_model(..., use_invK=False)`` builds it.  Returns
        ``hypopt`` [d+2, q] and the fields of ``sbo_fit_report`` (per-output arrays cut to q)."""
        tag, np_dtype = _DTYPES[dtype]
        X_norm = _f64(ds["X_norm"])
        Y_norm = _f64(ds["Y_norm"])
        if X_norm.ndim != 2 or Y_norm.ndim != 2 or X_norm.shape[0] != Y_norm.shape[0]:
            raise ValueError("X_norm / Y_norm must be [n, d] and [n, q]")
        n, d = X_norm.shape
        q, D = Y_norm.shape[1], d + 2
        arrs = [_f64(ds[k]) for k in ("X_mean", "X_std", "Y_mean", "Y_std")]
        if arrs[0].shape != (d,) or arrs[1].shape != (d,) or arrs[2].shape != (q,) or arrs[3].shape != (q,):
            raise ValueError("X_mean/X_std must be [d], Y_mean/Y_std must be [q]")
        B = _f64(bounds)
        pop = _f64(init_pop)
        if d > L.SBO_MAX_D or q > L.SBO_MAX_Q or B.shape != (D, 2) or pop.ndim != 2 or pop.shape[1] != D:
            raise ValueError("bounds [d+2, 2], init_pop [P, d+2], d <= SBO_MAX_D, q <= SBO_MAX_Q")
        mp = None
        if mean_prior is not None:
            mp = _f64(mean_prior).reshape(-1)
            if mp.shape != (q,):
                raise ValueError("mean_prior must be [q]")
        opts = L.FitOpts(P=pop.shape[0], maxiter=int(maxiter), tol=float(tol), atol=float(atol), seed=int(seed) & (2 ** 64 - 1),
                         polish=1 if polish else 0, polish_maxiter=int(polish_maxiter), polish_ftol=float(polish_ftol),
                         polish_gtol=float(polish_gtol))
        for a in range(D):
            opts.lo[a], opts.hi[a] = B[a, 0], B[a, 1]
        hyp = np.empty((D, q), dtype=np.float64)
        rep = L.FitReport()
        L.check(self._lib.sbo_model_fit(self._ctx, tag, kernel.encode(), n, d, q, _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]),
                                        _ptr(arrs[3]), _ptr(X_norm), _ptr(Y_norm), _ptr(mp), C.byref(opts), _ptr(pop), _ptr(hyp),
                                        C.byref(rep)))
        self.tag, self.np_dtype = tag, np_dtype
        self.n, self.d, self.q = n, d, q
        self._prior = self._prior_mean(arrs[2], arrs[3], mp)
        self._obs = (X_norm.copy(), arrs[0].copy(), arrs[1].copy())
        out = {"hypopt": hyp}
        for name, _ in L.FitReport._fields_:
            if name == "reserved":
                continue
            v = getattr(rep, name)
            out[name] = np.array(v[:q]) if hasattr(v, "__len__") else v
        return out

    @staticmethod
    def _prior_mean(Y_mean, Y_std, mean_prior):
        """The prior mean of the resident model in normalised units (models/GP_Safe.py:331-332, or the caller's)."""
        if mean_prior is not None:
            return _f64(mean_prior).reshape(-1).copy()
        mp = -2.0 * Y_mean / Y_std
        mp[0] = 0.0
        return mp

    def append_sample(self, x_norm_new, y_norm_new):
        """One more observation under frozen hyper-parameters and normalisation: O(n^2) on the
        device instead of a rebuild.  ``x_norm_new`` [d] and ``y_norm_new`` [q] are normalised with the constants of the
        last ``set_model``."""
        x = _f64(x_norm_new).reshape(-1)
        y = _f64(y_norm_new).reshape(-1)
        if x.shape != (self.d,) or y.shape != (self.q,):
            raise ValueError("x_norm_new must be [d] and y_norm_new [q]")
        L.check(self._lib.sbo_model_append(self._ctx, _ptr(x), _ptr(y)))
        self._rows_changed(1, np.vstack([self._obs[0], x]))

    def append_samples(self, X_norm_new, Y_norm_new):
        """k observations in one block update (``sbo_model_append_batch``): ``X_norm_new`` [k, d] and
        ``Y_norm_new`` [k, q], normalised with the constants of the last ``set_model``, enter in row order; the resident model is
        the one k calls of ``append_sample`` would leave, with one verdict wait, one re-pack and one plan invalidation.  All or
        nothing: a refused block (``ValueError``: a non-finite value, a Schur pivot that is not positive; ``SafeBOError`` with
        ``SBO_E_UNSUPPORTED``: n + k > ``SBO_MAX_N``) leaves the model as it was.  1 <= k <= ``SBO_MAX_APPEND``."""
        X = _f64(X_norm_new)
        Y = _f64(Y_norm_new)
        if X.ndim != 2 or Y.ndim != 2 or X.shape[1] != self.d or Y.shape[1] != self.q or X.shape[0] != Y.shape[0]:
            raise ValueError("X_norm_new must be [k, d] and Y_norm_new [k, q]")
        k = X.shape[0]
        if not 1 <= k <= L.SBO_MAX_APPEND:
            raise ValueError(f"k = {k} out of range [1, SBO_MAX_APPEND = {L.SBO_MAX_APPEND}]")
        if not (np.all(np.isfinite(X)) and np.all(np.isfinite(Y))):
            raise ValueError("X_norm_new and Y_norm_new must be finite")
        L.check(self._lib.sbo_model_append_batch(self._ctx, k, _ptr(X), _ptr(Y)))
        self._rows_changed(k, np.vstack([self._obs[0], X]))

    def remove_sample(self, index: int):
        """The counterpart of ``append_sample`` (``sbo_model_remove``): observation ``index`` (0-based, in the order of ``X_norm``
        as set and appended) leaves the resident model under the same frozen constants, O(n^2) on the device; the rows behind
        it move up by one.  A model keeps at least one observation."""
        if isinstance(index, bool) or not isinstance(index, (int, np.integer)):
            raise ValueError("index must be an integer")
        if self.n and not 0 <= index < self.n:          # (without a model the library answers: SBO_E_NO_MODEL)
            raise ValueError(f"index {int(index)} out of range [0, {self.n})")
        L.check(self._lib.sbo_model_remove(self._ctx, int(index)))
        self._rows_changed(-1, np.delete(self._obs[0], int(index), axis=0))

    def _rows_changed(self, dn, new_obs0):
        """Behind an accepted append, block append or removal: the row count and the observations follow the resident model."""
        self.n += dn
        self._obs = (new_obs0,) + self._obs[1:]

    def model_loo(self, b: float = 3.0, Y_norm=None) -> dict:
        """Leave-one-out diagnostics of the resident model (``sbo_model_loo``), normalised units, fp64 whatever the model dtype:
        ``resid`` [n, q] = y_i - mu_-i, ``var`` [n, q] (noise included), ``z`` [n, q] = resid / sqrt(var), and per output ``logdet``
        = log det(K + sn2 I), ``lpd`` = sum_i log N(y_i | mu_-i, v_i), ``z_max`` = max |z| with its index ``z_argmax`` (the lowest of a
        tie) and ``outside`` = #{|z_i| > b}.  One O(n^2) pass over the resident factor on the device; the model is not changed.
        With ``Y_norm`` [n, q] (the rows the model holds; the library keeps no copy) it adds the reference's NLL form
        ``nll`` [q] = sum_i r_i e_i / v_i + logdet with r = Y_norm - prior mean (models/GP_Safe.py:169-192 without its jitter)."""
        b = float(b)
        n, q = self.n, self.q
        resid = np.empty((n, q), dtype=np.float64)
        var = np.empty((n, q), dtype=np.float64)
        res = L.ModelLooResult()
        L.check(self._lib.sbo_model_loo(self._ctx, b, _ptr(resid), _ptr(var), C.byref(res)))
        out = {"resid": resid, "var": var, "z": resid / np.sqrt(var), "logdet": np.array(res.logdet[:q]), "lpd": np.array(res.lpd[:q]),
               "z_max": np.array(res.z_max[:q]), "z_argmax": np.array(res.z_argmax[:q], dtype=np.int64),
               "outside": np.array(res.outside[:q], dtype=np.int64)}
        if Y_norm is not None:
            Y = _f64(Y_norm)
            if Y.shape != (n, q):
                raise ValueError("Y_norm must be [n, q]")
            out["nll"] = np.sum((Y - self._prior) * resid / var, axis=0) + out["logdet"]
        return out

    # ---- candidates --------------------------------------------------------------------------
    def set_points(self, points, first: int = 0):
        pts = np.asarray(points)
        if pts.ndim != 2:
            raise ValueError("points must be [N, d]")
        if pts.dtype == np.float32:
            tag = L.SBO_F32
            pts = np.ascontiguousarray(pts)
        else:
            tag = L.SBO_F64
            pts = _f64(pts)
        L.check(self._lib.sbo_candidates_points(self._ctx, _ptr(pts), tag, pts.shape[0], pts.shape[1], int(first)))
        self.n_local, self.first = pts.shape[0], int(first)

    def set_grid(self, lo, hi, count, first: int = 0, n_local: int | None = None):
        lo, hi = _f64(lo), _f64(hi)
        cnt = np.ascontiguousarray(np.asarray(count, dtype=np.int64))
        if not (lo.shape == hi.shape == cnt.shape) or lo.ndim != 1:
            raise ValueError("lo, hi, count must be 1-D of equal length")
        total = int(np.prod([int(c) for c in cnt]))
        if n_local is None:
            n_local = total - int(first)
        L.check(self._lib.sbo_candidates_grid(self._ctx, lo.shape[0], _ptr(lo), _ptr(hi), _ptr(cnt), int(first),
                                              int(n_local)))
        self.n_local, self.first = int(n_local), int(first)

    def set_grid_sharded(self, lo, hi, count):
        """Grid sharded over the communicator's ranks by hyper-planes of the slowest axis."""
        lo, hi = _f64(lo), _f64(hi)
        cnt = np.ascontiguousarray(np.asarray(count, dtype=np.int64))
        if not (lo.shape == hi.shape == cnt.shape) or lo.ndim != 1:
            raise ValueError("lo, hi, count must be 1-D of equal length")
        first, nloc = C.c_int64(), C.c_int64()
        L.check(self._lib.sbo_candidates_grid_sharded(self._ctx, lo.shape[0], _ptr(lo), _ptr(hi), _ptr(cnt),
                                                      C.byref(first), C.byref(nloc)))
        self.n_local, self.first = int(nloc.value), int(first.value)

    # ---- hot path ----------------------------------------------------------------------------
    def posterior_run(self):
        L.check(self._lib.sbo_posterior_run(self._ctx))

    def posterior(self):
        """Batched ``GP_inference`` (models/GP_Safe.py:310-352): (mean[N, q], var[N, q])."""
        mean = np.empty((self.n_local, self.q), dtype=self.np_dtype)
        var = np.empty((self.n_local, self.q), dtype=self.np_dtype)
        L.check(self._lib.sbo_posterior_get(self._ctx, _ptr(mean), _ptr(var)))
        return mean, var

    def bounds(self, b: float, index: int, kind: str):
        """Batched ``BO.mean/ucb/lcb(points, index)`` (models/SafeOpt.py:29-45)."""
        k = {"mean": L.SBO_MEAN, "ucb": L.SBO_UCB, "lcb": L.SBO_LCB, "var": L.SBO_VAR}[kind]
        out = np.empty(self.n_local, dtype=self.np_dtype)
        L.check(self._lib.sbo_bounds(self._ctx, float(b), int(index), k, _ptr(out)))
        return out

    def _opts(self, b, quirk, want_masks, posterior_ready, lean=False):
        return L.SweepOpts(float(b), int(bool(quirk)), int(bool(want_masks)), int(bool(posterior_ready)), int(lean))

    def sweep_safeopt(self, b: float, quirk_L_index: bool = True, want_masks: bool = False,
                      posterior_ready: bool = False, lean: bool = False) -> dict:
        """``lean``: the caller wants the sweep's result only.  1 / True: mean / var may stay unwritten where no stage of the sweep
        reads them; 2: they need not be evaluated there at all (``posterior()`` behind a lean sweep runs K1 again).  A lean sweep of
        a model with constraints reports ``L[0] = 0``: no sweep reads the objective's Lipschitz key (models/SafeOpt.py:110)."""
        res = L.SafeOptResult()
        opts = self._opts(b, quirk_L_index, want_masks, posterior_ready, lean)
        L.check(self._lib.sbo_sweep_safeopt(self._ctx, C.byref(opts), C.byref(res)))
        d, q = self.d, self.q
        return {
            "minimizer_index": int(res.minimizer_index), "minimizer_x": np.array(res.minimizer_x[:d]),
            "minimizer_std": float(res.minimizer_std),
            "expander_index_c": np.array(res.expander_index_c[:q - 1], dtype=np.int64),
            "expander_std_c": np.array(res.expander_std_c[:q - 1]),
            "expander_best_c": int(res.expander_best_c), "expander_index": int(res.expander_index),
            "expander_x": np.array(res.expander_x[:d]), "expander_std": float(res.expander_std),
            "choose_minimizer": bool(res.choose_minimizer), "u_star": float(res.u_star),
            "L": np.array(res.L[:q]), "count_S": int(res.count_S), "count_U": int(res.count_U),
            "count_M": int(res.count_M), "count_G": np.array(res.count_G[:q - 1], dtype=np.int64),
            "n_exact_rechecks": int(res.n_exact_rechecks), "guard_band": int(res.guard_band),
            "guard_rechecks": int(res.guard_rechecks), "guard_passes": int(res.guard_passes),
        }

    def sweep_goose(self, b: float, quirk_L_index: bool = True, want_masks: bool = False,
                    posterior_ready: bool = False) -> dict:
        res = L.GooseResult()
        opts = self._opts(b, quirk_L_index, want_masks, posterior_ready)
        L.check(self._lib.sbo_sweep_goose(self._ctx, C.byref(opts), C.byref(res)))
        d, q = self.d, self.q
        return {
            "safe_min_index": int(res.safe_min_index), "safe_min_x": np.array(res.safe_min_x[:d]),
            "safe_min_lcb": float(res.safe_min_lcb),
            "target_index_c": np.array(res.target_index_c[:q - 1], dtype=np.int64),
            "target_lcb_c": np.array(res.target_lcb_c[:q - 1]), "target_best_c": int(res.target_best_c),
            "target_index": int(res.target_index), "target_x": np.array(res.target_x[:d]),
            "target_lcb": float(res.target_lcb), "explore_index": int(res.explore_index),
            "explore_x": np.array(res.explore_x[:d]), "choose_safe_min": bool(res.choose_safe_min),
            "L": np.array(res.L[:q]), "count_S": int(res.count_S), "count_U": int(res.count_U),
            "count_O": np.array(res.count_O[:q - 1], dtype=np.int64), "n_exact_rechecks": int(res.n_exact_rechecks),
            "guard_band": int(res.guard_band), "guard_rechecks": int(res.guard_rechecks), "guard_passes": int(res.guard_passes),
        }

    def sweep_tr(self, b: float, x_0, r: float, posterior_ready: bool = False) -> dict:
        """Trust-region acquisition of models/GP_TR.py:43-51: argmin lcb_0 over S_t and the ball ||x - x_0|| <= r."""
        res = L.TRResult()
        opts = self._opts(b, True, True, posterior_ready)
        x0 = _f64(x_0)
        if x0.shape != (self.d,):
            raise ValueError("x_0 must have shape [d]")
        L.check(self._lib.sbo_sweep_tr(self._ctx, C.byref(opts), _ptr(x0), float(r), C.byref(res)))
        return {"index": int(res.index), "x": np.array(res.x[:self.d]), "lcb": float(res.lcb),
                "count_S": int(res.count_S), "count_T": int(res.count_T), "guard_band": int(res.guard_band),
                "guard_rechecks": int(res.guard_rechecks), "guard_passes": int(res.guard_passes)}

    def sweep_robust(self, b: float, n_control_axes: int, kind: str = "ucb", posterior_ready: bool = False) -> dict:
        """StableOpt's robust min-max on the resident grid (models/StableOpt.py:139-164): axes 0 .. n_control_axes - 1 are the controls
        xc, the rest the disturbance d.  argmin over xc with min_d lcb_c >= 0 (every constraint) of max_d ``kind``_0; ``index`` is the
        flat index in the control sub-grid (-1 and ``value`` = inf when no control is robust-safe)."""
        k = {"mean": L.SBO_MEAN, "ucb": L.SBO_UCB, "lcb": L.SBO_LCB}.get(kind)
        if k is None:
            raise ValueError("kind must be 'mean', 'ucb' or 'lcb'")
        res = L.RobustResult()
        opts = self._opts(b, True, False, posterior_ready)
        L.check(self._lib.sbo_sweep_robust(self._ctx, C.byref(opts), int(n_control_axes), k, C.byref(res)))
        nc = int(n_control_axes)
        self._robust_shape = (int(res.count_control), self.q)
        return {"index": int(res.index), "xc": np.array(res.xc[:nc]), "value": float(res.value),
                "worst_d_index": int(res.worst_d_index), "worst_d": np.array(res.worst_d[:self.d - nc]),
                "candidate_index": int(res.candidate_index), "count_control": int(res.count_control),
                "count_disturbance": int(res.count_disturbance), "count_safe": int(res.count_safe),
                "guard_band": int(res.guard_band), "guard_rechecks": int(res.guard_rechecks), "guard_passes": int(res.guard_passes)}

    def robust_arrays(self):
        """Per-control arrays of the last robust sweep: f[Nc] = max_d bound_0, g[q - 1, Nc] = min_d lcb_c."""
        nc, q = getattr(self, "_robust_shape", (0, self.q))
        f = np.empty(nc, dtype=np.float64)
        g = np.empty((max(q - 1, 0), nc), dtype=np.float64)
        L.check(self._lib.sbo_robust_get(self._ctx, _ptr(f), _ptr(g) if g.size else None))
        return f, g

    def explore_safeset(self, target):
        """``BO.explore_safeset(target)`` (models/GoOSE.py:116-119) for a caller's own target: (flat index, x) of the candidate of the
        last sweep's safe set closest to ``target`` -- arg-min on the device."""
        t = _f64(target)
        if t.shape != (self.d,):
            raise ValueError("target must have shape [d]")
        idx = C.c_int64()
        x = np.zeros(L.SBO_MAX_D)
        L.check(self._lib.sbo_explore_safeset(self._ctx, _ptr(t), C.byref(idx), _ptr(x)))
        return int(idx.value), x[:self.d].copy()

    def refine(self, b: float, seeds, objective: int = 0, kind: str = "lcb", maximize: bool = False, constraints=None, *, lo, hi,
               x_0=None, r=None, max_eval: int | None = None, tol: float | None = None) -> dict:
        """Local refinement off the grid: each seed [d] of ``seeds`` [S, d] moves to a local optimum of
        ``kind`` ("mean" / "ucb" / "lcb" / "var") of output ``objective`` (minimised, or maximised) over the box [lo, hi], the
        constraints lcb_c >= 0 (``constraints``: output indices, None = every constraint output, [] = none) and, with ``x_0`` and
        ``r``, the ball ||x - x_0|| <= r.  Every returned point is feasible under the exact values ``bounds`` gives there and no worse
        than its seed.  Returns per seed ``x`` [S, d], ``value`` [S], ``status`` [S] (SBO_REFINE_*), and ``best`` (-1 if no seed was
        usable), ``best_x``, ``best_value``, ``evaluations``, ``converged``.  The resident candidates, posterior and masks are not
        touched."""
        k = {"mean": L.SBO_MEAN, "ucb": L.SBO_UCB, "lcb": L.SBO_LCB, "var": L.SBO_VAR}.get(kind)
        if k is None:
            raise ValueError("kind must be 'mean', 'ucb', 'lcb' or 'var'")
        opts, res = L.RefineOpts(), L.RefineResult()
        opts.objective = int(objective)
        opts.kind = k
        opts.maximize = int(bool(maximize))
        masks = {"constraint_mask": range(1, self.q) if constraints is None else constraints}
        return self._refine_call(lambda n, S, Sp, x, xp, val, st: self._lib.sbo_refine(self._ctx, C.byref(opts), n, S, x, val, st, C.byref(res)),
                                 opts, res, b, seeds, None, masks, lo, hi, x_0, r, max_eval, tol)

    def _refine_call(self, call, opts, res, b, seeds, seeds_p, masks, lo, hi, x_0, r, max_eval, tol) -> dict:
        """What ``refine`` and ``refine_sets`` share: the seed arrays, ``masks`` (field of ``opts`` -> output indices), the box, the
        ball, ``max_eval`` and ``tol`` into ``opts``; ``call(n, seeds, seeds_p, x, xp, value, status)``; the result dict."""
        d = self.d
        pair = seeds_p is not None
        S = []
        for s in (seeds, seeds_p) if pair else (seeds,):
            s = _f64(s)
            if s.ndim == 1:
                s = s.reshape(1, -1)
            if d < 1 or s.ndim != 2 or s.shape[1] != d:
                raise ValueError("seeds must be [S, d] for the model's d")
            S.append(np.ascontiguousarray(s))
        if pair and S[1].shape != S[0].shape:
            raise ValueError("seeds and seeds_p must have the same shape")
        opts.b = float(b)
        for field, cs in masks.items():
            m = 0
            for c in cs:
                c = int(c)
                if c < 0 or c >= 32:
                    raise ValueError("constraint index out of range")
                m |= 1 << c
            setattr(opts, field, m)
        lo, hi = _f64(lo).reshape(-1), _f64(hi).reshape(-1)
        if lo.shape != (d,) or hi.shape != (d,):
            raise ValueError("lo and hi must have shape [d]")
        for a in range(d):
            opts.lo[a], opts.hi[a] = lo[a], hi[a]
        if (x_0 is None) != (r is None):
            raise ValueError("the ball needs both x_0 and r")
        if x_0 is not None:
            x0 = _f64(x_0).reshape(-1)
            if x0.shape != (d,):
                raise ValueError("x_0 must have shape [d]")
            opts.use_ball = 1
            for a in range(d):
                opts.x_0[a] = x0[a]
            opts.r = float(r)
        opts.max_eval = int(max_eval) if max_eval is not None else 0
        opts.tol = float(tol) if tol is not None else 0.0
        n = S[0].shape[0]
        x = np.empty((n, d))
        xp = np.empty((n, d)) if pair else None
        val = np.empty(n)
        st = np.empty(n, dtype=np.int32)
        L.check(call(n, _ptr(S[0]), _ptr(S[1]) if pair else None, _ptr(x), _ptr(xp) if pair else None, _ptr(val), _ptr(st)))
        out = {"x": x, "value": val, "status": st, "best": int(res.best), "best_x": np.array(res.best_x[:d]),
               "best_value": float(res.best_value), "evaluations": int(res.evaluations), "converged": int(res.converged)}
        if pair:
            out["xp"] = xp
            out["best_xp"] = np.array(res.best_xp[:d])
        return out

    def refine_sets(self, b: float, seeds, seeds_p=None, *, objective: int = 0, kind: str = "lcb", at: str = "x", maximize: bool = False,
                    safe=None, unsafe=None, level=None, link=None, target=None, lo, hi, x_0=None, r=None,
                    max_eval: int | None = None, tol: float | None = None) -> dict:
        """``refine`` for the set-valued steps (``sbo_refine_sets``).  With ``seeds_p`` [S, d] the variable is
        the pair (x, x') from (``seeds``, ``seeds_p``) -- d <= 4 --, else the point x.  Objective: ``kind`` of output ``objective``
        at x or (``at="xp"``) at x', or ``kind="dist"``: the distance from x to ``target`` [d], minimised.  Terms: lcb_c(x) >= 0 for c
        in ``safe`` (None = every constraint, [] = none); lcb_c(x') <= 0 for c in ``unsafe`` (pair mode: None = every constraint;
        single mode: none); ``level=(o, value)``: lcb_o(x) <= value; ``link=(c, L)``: ucb_c(x) - L ||x - x' + 1e-8|| >= 0; the box
        (both points) and the ball (x).  Returns what ``refine`` returns -- ``evaluations`` counts each point of a pair -- and in
        pair mode ``xp`` [S, d] and ``best_xp``."""
        kinds = {"mean": L.SBO_MEAN, "ucb": L.SBO_UCB, "lcb": L.SBO_LCB, "var": L.SBO_VAR, "dist": L.SBO_REFINE_DIST}
        if kind not in kinds:
            raise ValueError("kind must be 'mean', 'ucb', 'lcb', 'var' or 'dist'")
        if at not in ("x", "xp"):
            raise ValueError("at must be 'x' or 'xp'")
        if (kind == "dist") != (target is not None):
            raise ValueError("kind='dist' and target go together")
        d = self.d
        pair = seeds_p is not None
        opts, res = L.RefineSetsOpts(), L.RefineSetsResult()
        opts.pair = int(pair)
        opts.objective = int(objective)
        opts.kind = kinds[kind]
        opts.objective_point = int(at == "xp")
        opts.maximize = int(bool(maximize))
        if level is not None:
            opts.use_level, opts.level_output, opts.level = 1, int(level[0]), float(level[1])
        if link is not None:
            opts.use_link, opts.link_output, opts.L = 1, int(link[0]), float(link[1])
        if target is not None:
            t = _f64(target).reshape(-1)
            if t.shape != (d,):
                raise ValueError("target must have shape [d]")
            for a in range(d):
                opts.target[a] = t[a]
        masks = {"safe_mask": range(1, self.q) if safe is None else safe,
                 "unsafe_mask": (range(1, self.q) if pair else ()) if unsafe is None else unsafe}
        return self._refine_call(lambda n, S, Sp, x, xp, val, st: self._lib.sbo_refine_sets(self._ctx, C.byref(opts), n, S, Sp, x, xp, val, st,
                                                                                            C.byref(res)),
                                 opts, res, b, seeds, seeds_p, masks, lo, hi, x_0, r, max_eval, tol)

    def refine_robust(self, b: float, xc_seed, n_control_axes: int, lo, hi, count_d, kind: str = "ucb", *, max_rounds: int | None = None,
                      max_scenarios: int | None = None, max_eval: int | None = None, tol: float | None = None) -> dict:
        """StableOpt's robust min-max refined off the grid (``sbo_refine_robust``): from the control ``xc_seed``
        [nxc] -- the winner of ``sweep_robust`` -- to a local solution of min_xc max_d ``kind``_0(xc, d) s.t. min_d lcb_c(xc, d) >= 0
        over the joint box ``lo`` / ``hi`` [d] (controls first), by outer approximation over at most ``max_scenarios`` disturbance
        points.  ``count_d`` [d - nxc]: the check grid of the disturbance box.  Returns ``status`` (SBO_REFINE_*), ``xc``, ``value``
        and ``seed_value`` (max over C = check grid + scenarios of the exact bound at xc / at the seed), ``worst_d``, ``g_min``
        [q - 1] (min over C of lcb_c at xc), ``scenarios`` [K, nd], ``rounds``, ``evaluations`` and ``gap``.  The returned ``xc`` is
        robust-safe on C and no worse than the seed there, the seed itself at worst.  Nothing resident is touched."""
        k = {"mean": L.SBO_MEAN, "ucb": L.SBO_UCB, "lcb": L.SBO_LCB}.get(kind)
        if k is None:
            raise ValueError("kind must be 'mean', 'ucb' or 'lcb'")
        d, nxc = self.d, int(n_control_axes)
        lo, hi = _f64(lo).reshape(-1), _f64(hi).reshape(-1)
        if lo.shape != (d,) or hi.shape != (d,):
            raise ValueError("lo and hi must have shape [d]")
        opts, res = L.RefineRobustOpts(), L.RefineRobustResult()
        opts.b, opts.kind, opts.n_control_axes = float(b), k, nxc
        opts.max_rounds = int(max_rounds) if max_rounds is not None else 0
        opts.max_scenarios = int(max_scenarios) if max_scenarios is not None else 0
        opts.max_eval = int(max_eval) if max_eval is not None else 0
        opts.tol = float(tol) if tol is not None else 0.0
        for a in range(d):
            opts.lo[a], opts.hi[a] = lo[a], hi[a]
        nd = max(d - nxc, 0)
        seed = _f64(xc_seed).reshape(-1)
        cnt = np.asarray(count_d, dtype=np.int64).reshape(-1)
        if 1 <= nxc <= d - 1 and (seed.shape != (nxc,) or cnt.shape != (nd,)):
            raise ValueError("xc_seed must be [n_control_axes] and count_d [d - n_control_axes]")
        for a in range(min(nd, cnt.shape[0])):
            opts.count_d[a] = int(cnt[a])
        scen = np.zeros((L.SBO_ROBUST_MAX_SCEN, max(nd, 1)))
        if seed.shape[0] < L.SBO_MAX_D:
            seed = np.concatenate((seed, np.zeros(L.SBO_MAX_D - seed.shape[0])))
        L.check(self._lib.sbo_refine_robust(self._ctx, C.byref(opts), _ptr(seed), _ptr(scen), C.byref(res)))
        K = int(res.scenarios)
        return {"status": int(res.status), "xc": np.array(res.xc[:nxc]), "value": float(res.value), "seed_value": float(res.seed_value),
                "worst_d": np.array(res.worst_d[:nd]), "g_min": np.array(res.g_min[1:self.q]), "scenarios": scen[:K, :nd].copy(),
                "rounds": int(res.rounds), "evaluations": int(res.evaluations), "gap": float(res.gap)}

    def mean_grad(self, points, infnorm: bool = False):
        """d MEAN_o / d x_a at ``points`` [N, d] (``sbo_mean_grad``): grad [N, q, d], the analytic form of
        ``jax.grad(self.mean)`` (models/SafeOpt.py:68-71).  ``infnorm=True``: also max_a |.| as [N, q].  The value at a point does not
        depend on the list it stands in, bit for bit.  fp64 models; nothing resident is touched."""
        pts = _f64(points)
        if pts.ndim == 1:
            pts = pts.reshape(1, -1)
        if self.d < 1 or pts.ndim != 2 or pts.shape[1] != self.d:
            raise ValueError("points must be [N, d] for the model's d")
        N = pts.shape[0]
        grad = np.empty((N, self.q, self.d))
        inf = np.empty((N, self.q)) if infnorm else None
        L.check(self._lib.sbo_mean_grad(self._ctx, N, _ptr(pts), _ptr(grad), _ptr(inf)))
        return (grad, inf) if infnorm else grad

    def lipschitz_seeds(self, lo, hi) -> np.ndarray:
        """The default seeds of ``lipschitz``: a tensor grid over the box of min(33, max(2, floor(4096^(1/d)))) points per axis -- the
        points of ``sbo_candidates_grid``, axis 0 the fastest --, then the observations (X_norm X_std + X_mean) clipped to the box."""
        lo, hi = _f64(lo).reshape(-1), _f64(hi).reshape(-1)
        d = self.d
        if lo.shape != (d,) or hi.shape != (d,):
            raise ValueError("lo and hi must have shape [d]")
        m = 2
        while m < 33 and (m + 1) ** d <= 4096:
            m += 1
        axes = []
        for a in range(d):
            ax = lo[a] + np.arange(m) * ((hi[a] - lo[a]) / (m - 1))
            ax[-1] = hi[a]
            axes.append(ax)
        mesh = np.meshgrid(*axes[::-1], indexing="ij")
        grid = np.stack([g.reshape(-1) for g in mesh[::-1]], axis=1)
        if self._obs is None:
            raise ValueError("the default seeds need a model")
        X_norm, X_mean, X_std = self._obs
        return np.ascontiguousarray(np.vstack([grid, np.clip(X_norm * X_std + X_mean, lo, hi)]))

    def lipschitz(self, lo, hi, seeds=None, outputs=None, top: int | None = None, max_eval: int | None = None,
                  tol: float | None = None) -> dict:
        """max over the box [lo, hi] of ||grad MEAN_o||_inf by a multistart local search on the device (``sbo_lipschitz``, DESIGN.md
        section 16) -- the reference's ``maximize_infnorm_mean_grad`` (models/SafeOpt.py:79-83), there by DE.  ``seeds`` [S, d] (None:
        ``lipschitz_seeds(lo, hi)``); seeds outside the box are skipped.  ``outputs``: the outputs to bound (None: all).  Returns
        ``L`` [q] (0 for outputs not asked for), ``L_seed`` [q] (the largest value at a seed), ``x`` [q, d] where L is attained,
        ``axis`` and ``sign`` [q] (L = sign * d MEAN_o / d x_axis at x), ``seeds_used``, ``evaluations``, ``problems``, ``converged``.
        L >= L_seed, and L is bit for bit ``mean_grad(x[o], infnorm=True)``'s value: a lower bound of the supremum that is attained
        in the box, not a certificate.  Nothing resident is touched."""
        lo, hi = _f64(lo).reshape(-1), _f64(hi).reshape(-1)
        d, q = self.d, self.q
        if lo.shape != (d,) or hi.shape != (d,):
            raise ValueError("lo and hi must have shape [d]")
        S = self.lipschitz_seeds(lo, hi) if seeds is None else _f64(seeds)
        if S.ndim == 1:
            S = S.reshape(1, -1)
        if d < 1 or S.ndim != 2 or S.shape[1] != d:
            raise ValueError("seeds must be [S, d] for the model's d")
        opts, res = L.LipschitzOpts(), L.LipschitzResult()
        if outputs is not None:
            for o in outputs:
                o = int(o)
                if o < 0 or o >= 32:
                    raise ValueError("output index out of range")
                opts.output_mask |= 1 << o
            if not opts.output_mask:
                raise ValueError("outputs must name at least one output")
        opts.top = int(top) if top is not None else 0
        opts.max_eval = int(max_eval) if max_eval is not None else 0
        opts.tol = float(tol) if tol is not None else 0.0
        for a in range(d):
            opts.lo[a], opts.hi[a] = lo[a], hi[a]
        L.check(self._lib.sbo_lipschitz(self._ctx, C.byref(opts), S.shape[0], _ptr(S), C.byref(res)))
        return {"L": np.array(res.L[:q]), "L_seed": np.array(res.L_seed[:q]), "x": np.array([list(res.x[o][:d]) for o in range(q)]),
                "axis": np.array(res.axis[:q], dtype=np.int64), "sign": np.array(res.sign[:q], dtype=np.int64),
                "seeds_used": int(res.seeds_used), "evaluations": int(res.evaluations), "problems": int(res.problems),
                "converged": int(res.converged)}

    @staticmethod
    def batch_arguments(d: int, q: int, points, k, output=0, pending=None, min_std=0.0):
        """The checks of ``batch_select`` that need no device: (points [m, d], k, output, pending [P, d] or None, min_std), or
        ValueError.  ``d`` / ``q`` < 1 (no model yet): the width of ``points`` and the range of ``output`` are the library's to check."""
        pts = _f64(points)
        if pts.ndim == 1:
            pts = pts.reshape(1, -1)
        if pts.ndim != 2 or pts.shape[0] < 1 or pts.shape[1] < 1 or (d >= 1 and pts.shape[1] != d):
            raise ValueError("points must be [m, d] for the model's d, m >= 1")
        for name, val in (("k", k), ("output", output)):
            if isinstance(val, bool) or not isinstance(val, (int, np.integer)):
                raise ValueError(f"{name} must be an integer")
        if not 1 <= k <= L.SBO_MAX_BATCH:
            raise ValueError(f"k must be in [1, {L.SBO_MAX_BATCH}]")
        if output < 0 or (q >= 1 and output >= q):
            raise ValueError("output out of range [0, q)")
        pend = None
        if pending is not None:
            pend = _f64(pending)
            if pend.ndim == 1:
                pend = pend.reshape(1, -1)
            if pend.ndim != 2 or pend.shape[1] != pts.shape[1]:
                raise ValueError("pending must be [P, d]")
            if pend.shape[0] == 0:
                pend = None
            elif k + pend.shape[0] > L.SBO_MAX_BATCH:
                raise ValueError(f"k + len(pending) must be at most {L.SBO_MAX_BATCH}")
        min_std = float(min_std)
        if not np.isfinite(min_std) or min_std < 0.0:
            raise ValueError("min_std must be finite and >= 0")
        if not np.all(np.isfinite(pts)) or (pend is not None and not np.all(np.isfinite(pend))):
            raise ValueError("points and pending must be finite")
        return pts, int(k), int(output), pend, min_std

    def batch_select(self, points, k: int, output: int = 0, pending=None, min_std: float = 0.0, return_var: bool = False) -> dict:
        """A greedy batch of ``k`` rows of ``points`` [m, d] under hallucinated observations (``sbo_batch_select``, DESIGN.md section
        17; the GP-BUCB rule): pick j maximises the posterior variance of ``output`` conditioned on the data, on ``pending`` [P, d]
        (points whose experiments are still running: conditioned on first, never picked) and on picks 0 .. j-1 -- a GP's variance
        does not depend on the observed values, so nothing has to be measured in between.  Ties go to the lowest index, a row may
        be picked again, and the batch ends before a pick whose std is below ``min_std``.  Returns ``index`` [j] into ``points``,
        ``x`` [j, d], ``std`` [j] (un-normalised, at the time of the pick) and, with ``return_var``, ``var`` [m]: the variance of
        every row after the last pick has been conditioned on.  fp64 whatever the model dtype; the value of a row does not depend
        on the list it stands in, bit for bit; nothing resident is touched."""
        pts, k, output, pend, min_std = self.batch_arguments(self.d, self.q, points, k, output, pending, min_std)
        opts, res = L.BatchOpts(output, k, 0 if pend is None else pend.shape[0], 0, min_std), L.BatchResult()
        var = np.empty(pts.shape[0]) if return_var else None
        L.check(self._lib.sbo_batch_select(self._ctx, C.byref(opts), pts.shape[0], _ptr(pts), _ptr(pend), _ptr(var), C.byref(res)))
        j = int(res.n_selected)
        index = np.array(res.index[:j], dtype=np.int64)
        out = {"index": index, "x": pts[index].reshape(j, pts.shape[1]), "std": np.array(res.std[:j], dtype=np.float64)}
        if return_var:
            out["var"] = var
        return out

    @staticmethod
    def expander_arguments(d: int, q: int, sources, targets, b, constraints=None):
        """The checks of ``expander_gain`` that need no device: (sources [ms, d], targets [mt, d], b, constraint mask), or
        ValueError.  ``d`` / ``q`` < 1 (no model yet): the width of the lists and the range of ``constraints`` are the library's to
        check."""
        src, tgt = _f64(sources), _f64(targets)
        if src.ndim == 1:
            src = src.reshape(1, -1)
        if tgt.ndim == 1:
            tgt = tgt.reshape(1, -1)
        if src.ndim != 2 or src.shape[0] < 1 or src.shape[1] < 1 or (d >= 1 and src.shape[1] != d):
            raise ValueError("sources must be [ms, d] for the model's d, ms >= 1")
        if tgt.ndim != 2 or tgt.shape[0] < 1 or tgt.shape[1] != src.shape[1]:
            raise ValueError("targets must be [mt, d], mt >= 1")
        if src.shape[0] > L.SBO_EXPANDER_MAX_POINTS:
            raise ValueError(f"at most {L.SBO_EXPANDER_MAX_POINTS} sources per call")
        if isinstance(b, bool) or not isinstance(b, (int, float, np.integer, np.floating)):
            raise ValueError("b must be a number")
        b = float(b)
        if not np.isfinite(b) or b < 0.0:
            raise ValueError("b must be finite and >= 0")
        if q == 1:
            raise ValueError("the model has no constraint (q >= 2 is required)")
        mask = 0
        if constraints is not None:
            for c in constraints:
                if isinstance(c, bool) or not isinstance(c, (int, np.integer)):
                    raise ValueError("constraints must be integers")
                if c < 1 or c >= 32 or (q >= 1 and c >= q):
                    raise ValueError("constraint out of range [1, q)")
                mask |= 1 << int(c)
            if not mask:
                raise ValueError("constraints must name at least one constraint")
        if not np.all(np.isfinite(src)) or not np.all(np.isfinite(tgt)):
            raise ValueError("sources and targets must be finite")
        return src, tgt, b, mask

    def _expander_call(self, opts, src, tgt, want_margin):
        """One ``sbo_expander_gain``: (count, margin or None, witness or None) of ``src`` against ``tgt`` (within the caps)."""
        ms = src.shape[0]
        count = np.empty(ms, dtype=np.int64)
        margin = np.empty(ms) if want_margin else None
        witness = np.empty(ms, dtype=np.int64) if want_margin else None
        L.check(self._lib.sbo_expander_gain(self._ctx, C.byref(opts), ms, _ptr(src), tgt.shape[0], _ptr(tgt), _ptr(count), _ptr(margin),
                                            _ptr(witness)))
        return count, margin, witness

    def expander_gain(self, sources, targets, b, constraints=None, return_margin: bool = False) -> dict:
        """Expanders by hallucinated optimistic observations (``sbo_expander_gain``; the G_t of the SafeOpt
        paper, no Lipschitz constant): row g of ``sources`` [ms, d] is an expander when, were it measured at ``ucb_c(g)`` on every
        constraint of ``constraints`` (None: all), the GP would certify some row of ``targets`` [mt, d] on all of them.  Returns
        ``count`` [ms] (int64: the targets g would certify) and ``expander`` [ms] (count > 0); with ``return_margin`` also
        ``margin`` [ms] (the largest Z(x | g) = min_c lcb'_c(x) / Y_std[c] over the targets) and ``witness`` [ms] (its row of
        ``targets``, the lowest on a tie).  Target lists above the library's cap are passed in chunks: counts add, margins take the
        maximum with the lowest row on a tie.  fp64 whatever the model dtype; nothing resident is touched."""
        src, tgt, b, mask = self.expander_arguments(self.d, self.q, sources, targets, b, constraints)
        opts = L.ExpanderOpts(b, mask, 0)
        count = margin = witness = None
        chunk = self._expander_chunk
        if self.n >= 1 and self.q >= 2:  # (the whitened vectors of a call: (ms + mt) * ldt * #constraints * 8 bytes under the library's cap)
            row = 8 * ((self.n + 31) // 32 * 32) * (bin(mask).count("1") if mask else self.q - 1)
            chunk = min(chunk, L.SBO_EXPANDER_MAX_SCRATCH // row - src.shape[0])
            if chunk < 1:
                raise ValueError("too many sources for the scratch of one call at this n: pass them in parts")
        for lo in range(0, tgt.shape[0], chunk):
            c, m, w = self._expander_call(opts, src, np.ascontiguousarray(tgt[lo:lo + chunk]), return_margin)
            if count is None:
                count, margin, witness = c, m, (w if w is None else np.where(w >= 0, w + lo, -1))
                continue
            count = count + c
            if return_margin:            # (chunks in ascending order: a later one wins only when strictly larger -- or the first with a value)
                better = (w >= 0) & ((witness < 0) | (m > margin))
                margin, witness = np.where(better, m, margin), np.where(better, w + lo, witness)
        out = {"count": count, "expander": count > 0}
        if return_margin:
            out["margin"], out["witness"] = margin, witness
        return out

    _expander_chunk = L.SBO_EXPANDER_MAX_POINTS      # targets of one call

    @staticmethod
    def path_draws(d: int, n: int, n_paths: int, features: int = 1024, seed=0):
        """The randomness of ``sample_paths`` in unit scale, from ``np.random.default_rng(seed)`` in this order: ``omega`` [F, d]
        standard normal, ``phase`` [F] uniform on [0, 2 pi), ``weights`` [S, F] and ``noise`` [S, n] standard normal."""
        rng = np.random.default_rng(seed)
        omega = rng.standard_normal((features, d))
        phase = rng.uniform(0.0, 2.0 * np.pi, features)
        weights = rng.standard_normal((n_paths, features))
        noise = rng.standard_normal((n_paths, n))
        return omega, phase, weights, noise

    @staticmethod
    def path_arguments(d: int, q: int, n: int, points, n_paths, output=0, features=1024, seed=0, maximize=False, draws=None):
        """The checks of ``sample_paths`` that need no device: (points [m, d], n_paths, output, features, seed, maximize as 0 | 1,
        draws as four contiguous float64 arrays or None), or ValueError.  With ``draws`` the number of features is that of its
        ``omega``.  ``d`` / ``q`` / ``n`` < 1 (no model yet): what depends on them is the library's to check."""
        pts = _f64(points)
        if pts.ndim == 1:
            pts = pts.reshape(1, -1)
        if pts.ndim != 2 or pts.shape[0] < 1 or pts.shape[1] < 1 or (d >= 1 and pts.shape[1] != d):
            raise ValueError("points must be [m, d] for the model's d, m >= 1")
        for name, val in (("n_paths", n_paths), ("output", output), ("features", features), ("seed", seed)):
            if isinstance(val, bool) or not isinstance(val, (int, np.integer)):
                raise ValueError(f"{name} must be an integer")
        if not 1 <= n_paths <= L.SBO_MAX_PATHS:
            raise ValueError(f"n_paths must be in [1, {L.SBO_MAX_PATHS}]")
        if output < 0 or (q >= 1 and output >= q):
            raise ValueError("output out of range [0, q)")
        if seed < 0:
            raise ValueError("seed must be >= 0")
        if not isinstance(maximize, (bool, np.bool_)) and not (isinstance(maximize, (int, np.integer)) and maximize in (0, 1)):
            raise ValueError("maximize must be a bool")
        if draws is not None:
            if not isinstance(draws, (tuple, list)) or len(draws) != 4:
                raise ValueError("draws must be (omega [F, d], phase [F], weights [S, F], noise [S, n])")
            omega, phase, weights, noise = (np.ascontiguousarray(_f64(a)) for a in draws)
            if omega.ndim != 2 or omega.shape[0] < 1 or omega.shape[1] != pts.shape[1]:
                raise ValueError("omega must be [F, d], F >= 1")
            features = omega.shape[0]
            if phase.shape != (features,) or weights.shape != (n_paths, features):
                raise ValueError("phase must be [F] and weights [n_paths, F]")
            if noise.ndim != 2 or noise.shape[0] != n_paths or (n >= 1 and noise.shape[1] != n):
                raise ValueError("noise must be [n_paths, n] for the model's n")
            if not all(np.all(np.isfinite(a)) for a in (omega, phase, weights, noise)):
                raise ValueError("draws must be finite")
            draws = (omega, phase, weights, noise)
        if not 1 <= features <= L.SBO_MAX_FEATURES:
            raise ValueError(f"features must be in [1, {L.SBO_MAX_FEATURES}]")
        if not np.all(np.isfinite(pts)):
            raise ValueError("points must be finite")
        return pts, int(n_paths), int(output), int(features), int(seed), int(bool(maximize)), draws

    def _paths_call(self, opts, draws, pts, want_values):
        """One ``sbo_sample_paths``: (index [S], value [S], values [m, S] or None) of ``pts`` (within the caps)."""
        S = int(opts.n_paths)
        res = L.PathsResult()
        values = np.empty((pts.shape[0], S)) if want_values else None
        omega, phase, weights, noise = draws
        L.check(self._lib.sbo_sample_paths(self._ctx, C.byref(opts), _ptr(omega), _ptr(phase), _ptr(weights), _ptr(noise), pts.shape[0],
                                           _ptr(pts), _ptr(values), C.byref(res)))
        return np.array(res.index[:S], dtype=np.int64), np.array(res.value[:S], dtype=np.float64), values

    def sample_paths(self, points, n_paths: int, output: int = 0, features: int = 1024, seed: int = 0, maximize: bool = False,
                     draws=None, return_values: bool = False) -> dict:
        """``n_paths`` joint draws from the posterior of ``output``, as functions, at ``points`` [m, d] (``sbo_sample_paths``,
        DESIGN.md section 20; pathwise conditioning: a random-feature draw from the prior plus a data-dependent update, O(F + n)
        per point and path).  The randomness is ``draws`` = (omega, phase, weights, noise) in unit scale, by default
        ``path_draws(d, n, n_paths, features, seed)``; the same draws are the same functions in every call.  Returns ``index``
        [S] (per path its arg-min over the points, ``maximize``: arg-max; the lowest row on a tie, -1 without a value), ``x`` [S, d]
        (NaN rows where index is -1), ``value`` [S] (un-normalised) and, with ``return_values``, ``values`` [m, S].  Pools above
        the library's caps are passed in chunks with the same draws and merged by (value, lowest row).  One set of features fixes
        the prior's kernel to within O(1 / sqrt(F)): the paths' variance differs from the posterior's by that much.  fp64 whatever
        the model dtype; nothing resident is touched.  This is not reference behaviour."""
        pts, S, output, F, seed, maximize, draws = self.path_arguments(self.d, self.q, self.n, points, n_paths, output, features, seed,
                                                                       maximize, draws)
        if draws is None:
            draws = tuple(np.ascontiguousarray(a) for a in self.path_draws(pts.shape[1], max(self.n, 0), S, F, seed))
        opts = L.PathsOpts(output, S, F, maximize)
        m = pts.shape[0]
        chunk = self._paths_chunk
        if return_values:
            chunk = min(chunk, self._paths_values // (8 * S))
        index = value = None
        values = np.empty((m, S)) if return_values else None
        for lo in range(0, m, chunk):
            i, v, vals = self._paths_call(opts, draws, np.ascontiguousarray(pts[lo:lo + chunk]), return_values)
            if return_values:
                values[lo:lo + chunk] = vals
            i = np.where(i >= 0, i + lo, -1)
            if index is None:
                index, value = i, v
                continue
            # (chunks in ascending order: a later one wins only when strictly better -- or the first with a value)
            better = (i >= 0) & ((index < 0) | ((v > value) if maximize else (v < value)))
            index, value = np.where(better, i, index), np.where(better, v, value)
        x = np.full((S, pts.shape[1]), np.nan)
        x[index >= 0] = pts[index[index >= 0]]
        out = {"index": index, "x": x, "value": value}
        if return_values:
            out["values"] = values
        return out

    _paths_chunk = L.SBO_PATHS_MAX_POINTS            # points of one call
    _paths_values = L.SBO_PATHS_MAX_VALUES           # bytes of values_out of one call

    @staticmethod
    def refine_paths_arguments(d: int, q: int, n: int, b, seeds, output=0, features=1024, seed=0, draws=None, maximize=False,
                               constraints=None, lo=None, hi=None, max_eval=None, tol=None):
        """The checks of ``refine_paths`` that need no device: (seeds [S, K, d], b, output, features, seed, maximize as 0 | 1, draws
        or None, constraint mask, lo [d], hi [d], max_eval, tol), or ValueError.  ``seeds`` [S, d] is K = 1; a seed may be
        non-finite (the library reports it infeasible).  The draws, the output, the feature count and ``maximize`` are held to
        ``path_arguments``; ``d`` / ``q`` / ``n`` < 1 (no model yet): what depends on them is the library's to check."""
        sd = _f64(seeds)
        if sd.ndim == 2:
            sd = sd[:, None, :]
        if sd.ndim != 3 or min(sd.shape) < 1 or (d >= 1 and sd.shape[2] != d):
            raise ValueError("seeds must be [S, K, d] or [S, d] for the model's d")
        S, K, dd = sd.shape
        if K > L.SBO_REFINE_PATHS_MAX_STARTS:
            raise ValueError(f"at most {L.SBO_REFINE_PATHS_MAX_STARTS} starts per path")
        _, S, output, features, seed, maximize, draws = SweepEngine.path_arguments(d, q, n, np.zeros((1, dd)), S, output, features, seed,
                                                                                   maximize, draws)
        if isinstance(b, bool) or not isinstance(b, (int, float, np.integer, np.floating)) or not np.isfinite(b) or b < 0:
            raise ValueError("b must be finite and >= 0")
        mask = 0
        for c in (range(1, max(q, 1)) if constraints is None else constraints):
            if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or c < 1 or c >= 32 or (q >= 1 and c >= q):
                raise ValueError("constraints must be output indices in [1, q)")
            mask |= 1 << int(c)
        if lo is None or hi is None:
            raise ValueError("refine_paths needs the box lo, hi")
        lo, hi = _f64(lo).reshape(-1), _f64(hi).reshape(-1)
        if lo.shape != (dd,) or hi.shape != (dd,):
            raise ValueError("lo and hi must have shape [d]")
        if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo <= hi)):
            raise ValueError("the box needs finite lo <= hi")
        if max_eval is not None and (isinstance(max_eval, bool) or not isinstance(max_eval, (int, np.integer))):
            raise ValueError("max_eval must be an integer")
        if tol is not None and np.isnan(tol):
            raise ValueError("tol is NaN")
        return (np.ascontiguousarray(sd), float(b), output, features, seed, maximize, draws, mask, lo, hi,
                int(max_eval) if max_eval is not None else 0, float(tol) if tol is not None else 0.0)

    def refine_paths(self, b: float, seeds, output: int = 0, features: int = 1024, seed: int = 0, draws=None, maximize: bool = False,
                     constraints=None, *, lo, hi, max_eval: int | None = None, tol: float | None = None) -> dict:
        """Sample-path optima off the grid (``sbo_refine_paths``): start k of path s, ``seeds`` [S, K, d] (or
        [S, d]), moves to a local minimum (``maximize``: maximum) of path s of ``output`` -- the function ``sample_paths`` defines for
        the same ``draws``, by default ``path_draws(d, n, S, features, seed)`` -- over the box [lo, hi] and lcb_c >= 0 under ``b``
        (``constraints`` as in ``refine``: None = every constraint output, [] = the box only).  Every returned point is feasible
        under the values ``bounds`` gives there; ``value`` is bit for bit the entry ``sample_paths`` returns at that point and no
        worse than at the seed.  Returns ``x`` [S, K, d], ``value`` [S, K], ``status`` [S, K] (SBO_REFINE_*), per path ``best`` [S]
        (the start, -1: none usable), ``best_x`` [S, d], ``best_value`` [S], and ``evaluations``, ``converged``.  fp64 models only;
        nothing resident is touched."""
        sd, b, output, F, seed, maximize, draws, mask, lo, hi, max_eval, tol = self.refine_paths_arguments(
            self.d, self.q, self.n, b, seeds, output, features, seed, draws, maximize, constraints, lo, hi, max_eval, tol)
        S, K, d = sd.shape
        if draws is None:
            draws = tuple(np.ascontiguousarray(a) for a in self.path_draws(d, max(self.n, 0), S, F, seed))
        opts, res = L.RefinePathsOpts(), L.RefinePathsResult()
        opts.b, opts.output, opts.n_paths, opts.n_features, opts.n_starts = b, output, S, F, K
        opts.maximize, opts.constraint_mask, opts.max_eval, opts.tol = maximize, mask, max_eval, tol
        for a in range(d):
            opts.lo[a], opts.hi[a] = lo[a], hi[a]
        x, val, st = np.empty((S, K, d)), np.empty((S, K)), np.empty((S, K), dtype=np.int32)
        omega, phase, weights, noise = draws
        L.check(self._lib.sbo_refine_paths(self._ctx, C.byref(opts), _ptr(omega), _ptr(phase), _ptr(weights), _ptr(noise), _ptr(sd),
                                           _ptr(x), _ptr(val), _ptr(st), C.byref(res)))
        return {"x": x, "value": val, "status": st, "best": np.array(res.best[:S], dtype=np.int64),
                "best_x": np.array([list(res.best_x[s][:d]) for s in range(S)]), "best_value": np.array(res.best_value[:S]),
                "evaluations": int(res.evaluations), "converged": int(res.converged)}

    @staticmethod
    def joint_draws(m: int, n_draws: int, seed=0):
        """The randomness of ``posterior_joint`` in unit scale: ``z`` [S, m] standard normal from ``np.random.default_rng(seed)``."""
        return np.random.default_rng(seed).standard_normal((n_draws, m))

    @staticmethod
    def joint_arguments(d: int, q: int, points, output=0, n_draws=0, seed=0, z=None, noise=False, jitter=1e-6, maximize=False):
        """The checks of ``posterior_joint`` that need no device: (points [m, d], output, n_draws, seed, z [S, m] contiguous float64
        or None, noise as 0 | 1, jitter, maximize as 0 | 1), or ValueError.  With ``z`` the number of draws is that of its rows.
        ``d`` / ``q`` < 1 (no model yet): what depends on them is the library's to check.  A pool above ``SBO_JOINT_MAX_POINTS`` is
        refused here: a joint draw cannot be chunked."""
        pts = _f64(points)
        if pts.ndim == 1:
            pts = pts.reshape(1, -1)
        if pts.ndim != 2 or pts.shape[0] < 1 or pts.shape[1] < 1 or (d >= 1 and pts.shape[1] != d):
            raise ValueError("points must be [m, d] for the model's d, m >= 1")
        if pts.shape[0] > L.SBO_JOINT_MAX_POINTS:
            raise ValueError(f"at most SBO_JOINT_MAX_POINTS = {L.SBO_JOINT_MAX_POINTS} points per call (a joint draw cannot be chunked)")
        for name, val in (("output", output), ("n_draws", n_draws), ("seed", seed)):
            if isinstance(val, bool) or not isinstance(val, (int, np.integer)):
                raise ValueError(f"{name} must be an integer")
        if output < 0 or (q >= 1 and output >= q):
            raise ValueError("output out of range [0, q)")
        if seed < 0:
            raise ValueError("seed must be >= 0")
        for name, val in (("noise", noise), ("maximize", maximize)):
            if not isinstance(val, (bool, np.bool_)) and not (isinstance(val, (int, np.integer)) and val in (0, 1)):
                raise ValueError(f"{name} must be a bool")
        if isinstance(jitter, bool) or not isinstance(jitter, (int, float, np.integer, np.floating)):
            raise ValueError("jitter must be a number")
        jitter = float(jitter)
        if not np.isfinite(jitter) or jitter < 0.0:
            raise ValueError("jitter must be finite and >= 0")
        if z is not None:
            z = np.ascontiguousarray(_f64(z))
            if z.ndim == 1:
                z = z.reshape(1, -1)
            if z.ndim != 2 or z.shape[0] < 1 or z.shape[1] != pts.shape[0]:
                raise ValueError("z must be [S, m], S >= 1")
            if not np.all(np.isfinite(z)):
                raise ValueError("z must be finite")
            n_draws = z.shape[0]
        if not 0 <= n_draws <= L.SBO_MAX_PATHS:
            raise ValueError(f"n_draws must be in [0, {L.SBO_MAX_PATHS}]")
        if not np.all(np.isfinite(pts)):
            raise ValueError("points must be finite")
        return pts, int(output), int(n_draws), int(seed), z, int(bool(noise)), jitter, int(bool(maximize))

    def posterior_joint(self, points, output: int = 0, n_draws: int = 0, seed: int = 0, z=None, noise: bool = False, jitter: float = 1e-6,
                        maximize: bool = False, return_cov: bool = True, return_chol: bool = False, return_draws: bool = False) -> dict:
        """The posterior of ``output`` at ``points`` [m, d] as a multivariate normal (``sbo_posterior_joint``):
        ``mean`` [m], with ``return_cov`` ``cov`` [m, m] (symmetric bit for bit; ``noise``: of a new observation, sn2 on the diagonal),
        with ``return_chol`` ``chol`` [m, m] (lower, ``chol chol^T = cov + Y_std^2 jitter sf2 I``), and ``n_draws`` exact joint draws
        ``mean + chol z_s`` from ``z`` [S, m] standard normals (default ``joint_draws(m, n_draws, seed)``): ``index`` [S] (per draw its
        arg-min over the points, ``maximize``: arg-max; the lowest row on a tie), ``x`` [S, d], ``value`` [S] and, with
        ``return_draws``, ``draws`` [m, S].  ``pivot_min`` / ``pivot_row``: the smallest pivot of the factorisation relative to its
        diagonal entry and its row (NaN / -1 when no factor was needed).  ``jitter`` (in units of sf2) goes on the diagonal of the
        matrix that is factored and nowhere else; a pivot below 2^-40 of its diagonal entry raises ValueError.  At most
        ``SBO_JOINT_MAX_POINTS`` points: a joint draw cannot be chunked.  fp64 whatever the model dtype; nothing resident is touched.
        This is not reference behaviour."""
        pts, output, S, seed, z, noise, jitter, maximize = self.joint_arguments(self.d, self.q, points, output, n_draws, seed, z, noise,
                                                                                jitter, maximize)
        m = pts.shape[0]
        if z is None and S > 0:
            z = np.ascontiguousarray(self.joint_draws(m, S, seed))
        opts, res = L.JointOpts(output, S, noise, maximize, jitter), L.JointResult()
        mean = np.empty(m)
        cov = np.empty((m, m)) if return_cov else None
        chol = np.empty((m, m)) if return_chol else None
        draws = np.empty((m, S)) if return_draws and S > 0 else None
        L.check(self._lib.sbo_posterior_joint(self._ctx, C.byref(opts), m, _ptr(pts), _ptr(z), _ptr(mean), _ptr(cov), _ptr(chol), _ptr(draws),
                                              C.byref(res)))
        out = {"mean": mean}
        if return_cov:
            out["cov"] = cov
        if return_chol:
            out["chol"] = chol
        if return_draws:
            out["draws"] = draws if draws is not None else np.empty((m, 0))
        if S > 0:
            index = np.array(res.index[:S], dtype=np.int64)
            x = np.full((S, pts.shape[1]), np.nan)
            x[index >= 0] = pts[index[index >= 0]]
            out["index"], out["x"], out["value"] = index, x, np.array(res.value[:S], dtype=np.float64)
        out["pivot_min"], out["pivot_row"] = float(res.pivot_min), int(res.pivot_row)
        return out

    def mask(self, which: str, c: int = 0) -> np.ndarray:
        w = {"S": L.SBO_MASK_S, "U": L.SBO_MASK_U, "M": L.SBO_MASK_M, "G": L.SBO_MASK_G, "O": L.SBO_MASK_O}[which]
        out = np.empty(self.n_local, dtype=np.uint8)
        L.check(self._lib.sbo_masks_get(self._ctx, w, int(c), _ptr(out)))
        return out.astype(bool)

    def nll_batch(self, X_norm, y, hypers):
        """``negative_loglikelihood`` (models/GP_Safe.py:169-192) for a population: hypers[P, d+2] -> NLL[P]."""
        X = _f64(X_norm)
        yv = _f64(np.asarray(y).reshape(-1))
        H = _f64(hypers)
        if X.ndim != 2 or H.ndim != 2 or H.shape[1] != X.shape[1] + 2 or yv.shape[0] != X.shape[0]:
            raise ValueError("X_norm [n, d], y [n], hypers [P, d + 2]")
        out = np.empty(H.shape[0], dtype=np.float64)
        L.check(self._lib.sbo_nll_batch(self._ctx, X.shape[0], X.shape[1], _ptr(X), _ptr(yv), H.shape[0], _ptr(H), _ptr(out)))
        return out

    def fit_de(self, X_norm, y, bounds, init_pop, seed: int = 0, maxiter: int = 1000, tol: float = 0.01, atol: float = 0.0):
        """Differential evolution of ``negative_loglikelihood`` on the device (``sbo_fit_de``).  bounds[d+2, 2],
        init_pop[P, d+2].  Returns (best hyper-parameters [d+2], NLL, generations run)."""
        X = _f64(X_norm)
        yv = _f64(np.asarray(y).reshape(-1))
        B = _f64(bounds)
        pop = _f64(init_pop)
        D = X.shape[1] + 2
        if X.ndim != 2 or B.shape != (D, 2) or pop.ndim != 2 or pop.shape[1] != D or yv.shape[0] != X.shape[0]:
            raise ValueError("X_norm [n, d], y [n], bounds [d+2, 2], init_pop [P, d+2]")
        lo, hi = _f64(B[:, 0]), _f64(B[:, 1])
        best, energy, gens = np.empty(D), C.c_double(), C.c_int()
        L.check(self._lib.sbo_fit_de(self._ctx, X.shape[0], X.shape[1], _ptr(X), _ptr(yv), pop.shape[0], _ptr(lo), _ptr(hi), _ptr(pop),
                                     int(seed), int(maxiter), float(tol), float(atol), _ptr(best), C.byref(energy), C.byref(gens)))
        return best, float(energy.value), int(gens.value)

    def fit_de_batch(self, X_norm, Y_norm, bounds, init_pop, seeds, maxiter: int = 1000, tol: float = 0.01, atol: float = 0.0):
        """``fit_de`` for every column of Y_norm[n, q] side by side (``sbo_fit_de_batch``): one launch per generation for all
        outputs, output o searched with ``seeds[o]`` from the shared ``init_pop``.  Returns (best_x [q, d+2], energies [q],
        generations [q]); row o is bit for bit ``fit_de(X_norm, Y_norm[:, o], ..., seed=seeds[o])``."""
        X = _f64(X_norm)
        Y = _f64(Y_norm)
        if Y.ndim == 1:
            Y = Y[:, None].copy()
        B = _f64(bounds)
        pop = _f64(init_pop)
        if X.ndim != 2 or Y.ndim != 2 or Y.shape[0] != X.shape[0]:
            raise ValueError("X_norm [n, d], Y_norm [n, q]")
        n, d = X.shape
        q, D = Y.shape[1], d + 2
        sd = np.ascontiguousarray(np.array([int(s) & (2 ** 64 - 1) for s in np.atleast_1d(seeds).tolist()], dtype=np.uint64))
        if B.shape != (D, 2) or pop.ndim != 2 or pop.shape[1] != D or sd.shape != (q,):
            raise ValueError("bounds [d+2, 2], init_pop [P, d+2], seeds [q]")
        lo, hi = _f64(B[:, 0]), _f64(B[:, 1])
        best, energy, gens = np.empty((q, D)), np.empty(q), np.empty(q, dtype=np.int32)
        L.check(self._lib.sbo_fit_de_batch(self._ctx, n, d, q, _ptr(X), _ptr(Y), pop.shape[0], _ptr(lo), _ptr(hi), _ptr(pop), _ptr(sd),
                                           int(maxiter), float(tol), float(atol), _ptr(best), _ptr(energy), _ptr(gens)))
        return best, energy, gens

    def nll_grad_batch(self, X_norm, y, hypers):
        """``negative_loglikelihood`` and its analytic gradient (models/GP_Classic.py:219, ``grad(NLL)``) for a population:
        hypers[P, d+2] -> (NLL[P], grad[P, d+2]).  The NLL is bit for bit ``nll_batch``'s; a failed factor gives inf and NaNs."""
        X = _f64(X_norm)
        yv = _f64(np.asarray(y).reshape(-1))
        H = _f64(hypers)
        if X.ndim != 2 or H.ndim != 2 or H.shape[1] != X.shape[1] + 2 or yv.shape[0] != X.shape[0]:
            raise ValueError("X_norm [n, d], y [n], hypers [P, d + 2]")
        nll = np.empty(H.shape[0], dtype=np.float64)
        grad = np.empty(H.shape, dtype=np.float64)
        L.check(self._lib.sbo_nll_grad_batch(self._ctx, X.shape[0], X.shape[1], _ptr(X), _ptr(yv), H.shape[0], _ptr(H), _ptr(nll),
                                             _ptr(grad)))
        return nll, grad

    def fit_local(self, X_norm, Y_norm, bounds, starts, maxiter: int = 10000, ftol: float = FLOAT32_EPS, gtol: float = 1e-8) -> dict:
        """GP_Classic's multistart fit (models/GP_Classic.py:194-240) in one launch (``sbo_fit_local``): a projected BFGS on the box
        bounds[d+2, 2] from every start of starts[P, d+2], for every column of Y_norm[n, q].  Returns ``best_x`` [q, d+2] and
        ``best_nll`` [q] (ties to the lowest start) and the per-start ``x`` [q, P, d+2], ``nll``, ``iters``, ``evals``, ``pgnorm``
        and ``status`` [q, P] (``_lib.SBO_FIT_*``)."""
        X = _f64(X_norm)
        Y = _f64(Y_norm)
        if Y.ndim == 1:
            Y = Y[:, None].copy()
        B = _f64(bounds)
        S = _f64(starts)
        if X.ndim != 2 or Y.ndim != 2 or Y.shape[0] != X.shape[0]:
            raise ValueError("X_norm [n, d], Y_norm [n, q]")
        n, d = X.shape
        q, D = Y.shape[1], d + 2
        if B.shape != (D, 2) or S.ndim != 2 or S.shape[1] != D:
            raise ValueError("bounds [d+2, 2], starts [P, d+2]")
        P = S.shape[0]
        lo, hi = _f64(B[:, 0]), _f64(B[:, 1])
        out = {"best_x": np.empty((q, D)), "best_nll": np.empty(q), "x": np.empty((q, P, D)), "nll": np.empty((q, P)),
               "iters": np.empty((q, P), dtype=np.int32), "evals": np.empty((q, P), dtype=np.int32), "pgnorm": np.empty((q, P)),
               "status": np.empty((q, P), dtype=np.int32)}
        L.check(self._lib.sbo_fit_local(self._ctx, n, d, q, _ptr(X), _ptr(Y), P, _ptr(S), _ptr(lo), _ptr(hi), int(maxiter), float(ftol),
                                        float(gtol), _ptr(out["best_x"]), _ptr(out["best_nll"]), _ptr(out["x"]), _ptr(out["nll"]),
                                        _ptr(out["iters"]), _ptr(out["evals"]), _ptr(out["pgnorm"]), _ptr(out["status"])))
        return out

    def plant_wo(self, U) -> np.ndarray:
        """William-Otto reactor outputs (objective, constraint 1, constraint 2) for input rows U[N, 2] = (Fb, Tr)."""
        u = _f64(np.atleast_2d(U))
        if u.ndim != 2 or u.shape[1] != 2:
            raise ValueError("U must be [N, 2]")
        out = np.empty((u.shape[0], 3), dtype=np.float64)
        L.check(self._lib.sbo_plant_wo(self._ctx, u.shape[0], _ptr(u), _ptr(out)))
        return out

    def profile_struct(self):
        """The raw ``sbo_profile`` of the last sweep (a timing loop keeps these and converts them with ``profile_dict`` afterwards:
        building the dict costs several microseconds of a 0.2 ms sweep)."""
        p = L.Profile()
        L.check(self._lib.sbo_profile_get(self._ctx, C.byref(p)))
        return p

    @staticmethod
    def profile_dict(p) -> dict:
        return {name: (list(getattr(p, name)) if issubclass(tp, C.Array) else getattr(p, name)) for name, tp in L.Profile._fields_}

    def profile(self) -> dict:
        return self.profile_dict(self.profile_struct())
