"""Seeded walks over one SweepEngine's call history -- test infrastructure for tests/test_gpu_history.py (GPU) and
tests/test_history_walk_cpu.py (the generator's coverage, no GPU).

The claim under test: whatever the engine did before, a sweep returns what a fresh context returns for the same model, candidates and
options.  A walk is a list of plain tuples (replayable from the seed alone, printed whole on a failure); the driver runs it on an
engine and checks every step against NumPy references of the current state: the dataset (appends rebuilt with frozen normalisation,
as tests/test_gpu_append.py::_extend does), the candidate set and the sweep's arguments.  Importing this module opens no GPU.
"""
import numpy as np

import oracle
import robust_oracle
from safebo_amd import synthetic

# problems: (config, n) -- B and H (q = 2, Benoit), C (q = 3, the Williams-Otto shape), A (small n)
PROBLEMS = {"A": ("A", 20), "B": ("B", 64), "H": ("H", 96), "C": ("C", 48)}
# 2-D grids: whole 64 x 128 tiles (128 x 64, 256 x 64) and grids that are not (130 x 70, 96 x 50); count[0] is the fast axis.  (Sized
# for the NumPy expander references, whose cost grows with |S| x |U|)
GRIDS = {"t128x64": [128, 64], "t256x64": [256, 64], "r130x70": [130, 70], "r96x50": [96, 50]}
SMALLER = {"t256x64": "r130x70", "r130x70": "r96x50", "t128x64": "r96x50", "r96x50": "r96x50"}
LARGER = {"r96x50": "t256x64", "r130x70": "t256x64", "t128x64": "t256x64", "t256x64": "t256x64"}
LISTS = {"l1000": 1000, "l2000": 2000}
ALL_GRIDS = dict(GRIDS, t256x128=[256, 128])      # (+ the directed tests' grid)
# option whitelist (value sets) and the defaults a walk restores
OPTIONS = {"bilinear": (0, 1, 2), "col_path": (0, 1, 2), "fuse_classify": (-1, 0, 1), "posterior_path": (0, 1, 2), "k1_sched": (0, 1),
           "guard_band": (1, 2), "list_index": (-1, 0, 1), "exact_lazy": (1, 2), "tensor_cheb": (0, 1)}
DEFAULTS = {"bilinear": 1, "col_path": 1, "fuse_classify": -1, "posterior_path": 0, "k1_sched": 1, "guard_band": 1, "list_index": -1,
            "exact_lazy": 1, "tensor_cheb": 1}
READY_KINDS = ("safeopt", "goose", "tr", "robust")
REFUSALS = ("b_nan", "b_neg", "append_nonfinite", "grid_zero", "mask_g_after_goose", "robust_arrays_after_model")
SEEDS = tuple(range(8))
WALK_PROBLEMS = ("B", "H", "C", "A", "B", "C", "H", "B")
SWEEPS = ("safeopt", "goose", "tr", "robust")


# ---- the generator (CPU only) ----------------------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, seed):
        self.rng = np.random.default_rng(1000 + seed)
        self.seed = seed
        self.steps = []
        self.problem = WALK_PROBLEMS[seed % len(WALK_PROBLEMS)]
        self.b = float(synthetic.CONFIGS[PROBLEMS[self.problem][0]]["b"])
        self.grid = None
        self.on_list = False

    def emit(self, *step):
        self.steps.append(tuple(step))

    def bval(self):
        return float(self.b * self.rng.choice([1.0, 0.75, 1.25]))

    def sweep(self, kind=None, ready=None, b=None, lean=None):
        kind = kind or str(self.rng.choice(["safeopt", "safeopt", "goose", "tr"] + ([] if self.on_list else ["robust"])))
        ready = bool(self.rng.integers(2)) if ready is None else ready
        b = self.bval() if b is None else b
        if kind == "safeopt":
            lean = int(self.rng.integers(3)) if lean is None else lean
            self.emit("safeopt", b, lean, ready, bool(self.rng.integers(4) > 0))
        elif kind == "goose":
            self.emit("goose", b, ready)
        elif kind == "tr":
            self.emit("tr", b, float(self.rng.uniform(0.2, 0.6)), ready)
        else:
            self.emit("robust", b, str(self.rng.choice(["ucb", "lcb", "mean"])), ready)

    def to_grid(self, name=None):
        self.grid = name or self.grid
        self.on_list = False
        self.emit("set_grid", self.grid)

    def model(self, dtype="f64"):
        self.emit("set_model", self.problem, dtype)

    # segments: each one emits a required transition with random arguments
    def seg_lean_ready(self, lean, kind):
        if kind == "robust" and self.on_list:
            self.to_grid()
        self.sweep("safeopt", ready=False, lean=lean)
        self.sweep(kind, ready=True, b=self.b, lean=0)

    def seg_append(self, under):
        if under == "K1i":
            self.to_grid("t256x128")          # (K1i wants a grid well finer than its nodes)
        elif self.on_list:
            self.to_grid()
        self.emit("option", "posterior_path", 0)
        self.emit("option", "bilinear", 0 if under == "K1g" else 1)
        self.model()
        self.sweep("safeopt", ready=False, lean=0)
        if under == "K1b":
            self.sweep("safeopt", ready=False)
        self.emit("append", int(self.rng.integers(1, 4)), under)
        self.sweep()
        self.sweep()
        if under == "K1g":
            self.emit("option", "bilinear", 1)

    def seg_refuse(self, kind):
        if kind == "mask_g_after_goose":
            self.sweep("goose", ready=bool(self.rng.integers(2)))
        if kind == "robust_arrays_after_model":
            if self.on_list:
                self.to_grid()
            self.sweep("robust")
            self.model()
        self.emit("refuse", kind)
        self.sweep(ready=True)

    def seg_shrink_grow(self):
        if self.on_list or self.grid in ("r96x50", "t256x64", "t256x128"):
            self.to_grid("t128x64")
        self.to_grid(SMALLER[self.grid])
        self.sweep(ready=False)
        self.to_grid(LARGER[self.grid])
        self.sweep(ready=False)
        self.sweep(ready=True)

    def seg_list_round(self):
        self.emit("option", "list_index", int(self.rng.choice([-1, 0, 1])))
        self.on_list = True
        self.emit("set_points", "l1000")
        self.sweep(ready=False)
        self.to_grid(str(self.rng.choice(list(GRIDS))))
        self.sweep()
        self.on_list = True
        self.emit("set_points", str(self.rng.choice(list(LISTS))))
        self.sweep(ready=False)
        self.sweep(ready=True)

    def seg_dtype_round(self):
        for dt in ("f32", "f64", "f32"):
            self.model(dt)
            self.sweep(str(self.rng.choice(["safeopt", "goose", "tr"])), ready=False)
            self.sweep(str(self.rng.choice(["safeopt", "goose", "tr"])), ready=True)
        self.model("f64")

    def seg_b_change(self):
        self.sweep(ready=False, b=self.b)
        self.sweep(ready=True, b=self.b * 0.8)
        self.sweep(ready=True, b=self.b * 1.2)

    def seg_options(self):
        for _ in range(2):
            key = str(self.rng.choice(list(OPTIONS)))
            self.emit("option", key, int(self.rng.choice(OPTIONS[key])))
            self.sweep()

    def seg_reads(self):
        self.sweep("safeopt", ready=False, lean=int(self.rng.integers(3)))
        self.emit("posterior")
        self.emit("explore", [float(v) for v in self.rng.uniform(0.0, 1.0, size=2)])
        self.emit("posterior_run")
        self.sweep(ready=True)


def make_walk(seed):
    """The step list of walk ``seed`` (deterministic: the seed is all a replay needs)."""
    g = _Gen(seed)
    g.to_grid(str(g.rng.choice(list(GRIDS))))
    g.model()
    g.sweep("safeopt", ready=False, lean=0)
    combos = [(lean, kind) for lean in (0, 1, 2) for kind in READY_KINDS]
    segs = [("lean_ready",) + combos[(2 * seed + j) % len(combos)] for j in range(2)]
    segs += [("append", {"A": "K1i", "C": "K1i", "B": "K1b", "H": "K1g"}[g.problem]), ("refuse", REFUSALS[(2 * seed) % 6]), ("refuse", REFUSALS[(2 * seed + 1) % 6]),
             ("shrink_grow",), ("list_round",), ("b_change",), ("options",), ("reads",)]
    if seed % 2 == 0:
        segs.append(("dtype_round",))
    for i in g.rng.permutation(len(segs)):
        name, *args = segs[i]
        getattr(g, "seg_" + name)(*args)
    for key, val in DEFAULTS.items():
        g.emit("option", key, val)
    return g.steps


def transitions(steps):
    """Names of the required transitions a step list contains (what the CPU test asserts over the fixed seeds)."""
    out = set()
    last_sweep = None
    model_sweeps = 0
    opts = dict(DEFAULTS)
    on_list = False
    dtypes = []
    cands = []
    grid = None
    for i, s in enumerate(steps):
        kind = s[0]
        if kind in SWEEPS:
            ready = s[2] if kind == "goose" else s[3]
            if ready and last_sweep is not None and last_sweep[0] == "safeopt":
                out.add(f"lean{last_sweep[2]}->{kind}_ready")
            if ready and last_sweep is not None and last_sweep[1] != s[1]:
                out.add("b_change_between_ready")
            if steps[i - 1][0] == "refuse":
                out.add("refused->sweep")
            last_sweep = s
            model_sweeps += 1
        elif kind == "set_model":
            model_sweeps = 0
            last_sweep = None
            dtypes.append(s[2])
        elif kind == "append":
            out.add("append_under_" + s[2])
            # (the generator's label agrees with the state it left: K1i after one sweep, K1b after two, K1g with bilinear 0)
            expect = "K1g" if opts["bilinear"] == 0 else ("K1i" if model_sweeps == 1 else "K1b")
            assert not on_list and expect == s[2], (i, s, model_sweeps, opts["bilinear"])
        elif kind == "option":
            opts[s[1]] = s[2]
        elif kind == "set_grid":
            if grid is not None and not on_list:
                a, b = np.prod(ALL_GRIDS[grid]), np.prod(ALL_GRIDS[s[1]])
                out.add("grid_shrink" if b < a else ("grid_grow" if b > a else "grid_same"))
            grid = s[1]
            on_list = False
            cands.append("grid")
        elif kind == "set_points":
            on_list = True
            cands.append("list")
        elif kind in ("posterior", "posterior_run", "explore"):
            out.add(kind)
    if any(cands[j:j + 3] == ["list", "grid", "list"] for j in range(len(cands))):
        out.add("list->grid->list")
    if any(dtypes[j:j + 3] == ["f32", "f64", "f32"] for j in range(len(dtypes))):
        out.add("f32->f64->f32")
    return out


REQUIRED = ({f"lean{lv}->{k}_ready" for lv in (0, 1, 2) for k in READY_KINDS} |
            {"append_under_K1i", "append_under_K1b", "append_under_K1g", "refused->sweep", "grid_shrink", "grid_grow",
             "list->grid->list", "f32->f64->f32", "b_change_between_ready"})


# ---- the driver (GPU) ------------------------------------------------------------------------------------------------------------
def _problem(name):
    cfg_name, n = PROBLEMS[name]
    cfg = synthetic.make_config(cfg_name, n=n)
    return cfg


def _list_points(problem, name):
    cfg = _problem(problem)
    bound = cfg["bound"]
    rng = np.random.default_rng(7 + LISTS[name])
    return rng.uniform(bound[:, 0], bound[:, 1], size=(LISTS[name], bound.shape[0]))


def _nerr(got, ref, ystd, power):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref) / np.maximum(1.0, ystd) ** power)) if np.size(ref) else 0.0


class Walk:
    """Runs a step list on ``eng`` and checks every step.  ``record`` collects (step index, posterior_kernel, set_path)."""

    def __init__(self, eng, seed, steps, problem=None):
        self.eng, self.seed, self.steps = eng, seed, steps
        self.record = []
        self.ds = None
        self.ds_ver = 0
        self.problem = None
        self.dtype = "f64"
        self.cand = None
        self.pts = None
        self.last = None           # (kind, oracle result) of the last sweep that left masks
        self.robust_ok = False
        self.cache = {}
        self.rng = np.random.default_rng(5000 + seed)
        self.walk_problem = problem or WALK_PROBLEMS[seed % len(WALK_PROBLEMS)]
        self.bound = _problem(self.walk_problem)["bound"]
        self.append_kernels = set()     # posterior kernel of the sweep before each append

    # references, cached on (dataset, candidates, arguments)
    def _ref(self, kind, *args):
        key = (kind, self.ds_ver, self.cand) + args
        if key not in self.cache:
            if ("post", self.ds_ver, self.cand) not in self.cache:
                self.cache[("post", self.ds_ver, self.cand)] = oracle.gp_inference(self.pts, self.ds)
            mv = self.cache[("post", self.ds_ver, self.cand)]
            if kind == "post":
                return mv
            if kind == "safeopt":
                self.cache[key] = oracle.safeopt_sweep(self.pts, self.ds, args[0], quirk_L_index=args[1], mean_var=mv)
            elif kind == "goose":
                self.cache[key] = oracle.goose_sweep(self.pts, self.ds, args[0], mean_var=mv)
            elif kind == "tr":
                self.cache[key] = oracle.tr_sweep(self.pts, self.ds, args[0], args[1], args[2], mean_var=mv)
            elif kind == "robust":
                self.cache[key] = robust_oracle.robust_from_posterior(mv[0], mv[1], ALL_GRIDS[self.cand[1]][0], args[0], args[1])
        return self.cache[key]

    def run(self, start=0):
        for i, step in enumerate(self.steps[start:], start):
            try:
                self.step(step)
            except Exception as e:                                 # noqa: BLE001
                listing = "\n".join(f"  {j:3d} {s!r}" for j, s in enumerate(self.steps[:i + 1]))
                raise AssertionError(f"history walk seed {self.seed}, step {i}: {step!r}\n"
                                     f"replay: history_walk.make_walk({self.seed})[:{i + 1}] =\n{listing}\n"
                                     f"{type(e).__name__}: {e}") from e
            prof = self.eng.profile()
            self.record.append((i, step[0], int(prof["posterior_kernel"]), int(prof["set_path"])))
        return self.record

    def step(self, s):
        eng, kind = self.eng, s[0]
        if kind == "set_grid":
            bound = self.bound
            eng.set_grid(bound[:, 0], bound[:, 1], ALL_GRIDS[s[1]])
            self.cand = ("grid", s[1])
            self.pts = oracle.grid_points(bound[:, 0], bound[:, 1], ALL_GRIDS[s[1]])
            self.last, self.robust_ok = None, False
        elif kind == "set_points":
            pts = _list_points(self.walk_problem, s[1])
            eng.set_points(pts)
            self.cand = ("list", s[1])
            self.pts = pts
            self.last, self.robust_ok = None, False
        elif kind == "set_model":
            self.problem, self.dtype = s[1], s[2]
            cfg = _problem(s[1])
            self.ds = {k: (list(v) if k == "invKopt" else np.array(v)) for k, v in cfg["ds"].items()}
            self.ds_ver += 1
            eng.set_model(self.ds, dtype=s[2], use_invK=s[2] == "f64")
            self.last, self.robust_ok = None, False
        elif kind == "append":
            n_new = s[1]
            self.append_kernels.add(int(eng.profile()["posterior_kernel"]))
            bound = _problem(self.problem)["bound"]
            for _ in range(n_new):
                x = self.rng.uniform(bound[:, 0], bound[:, 1])
                y = (synthetic.williams_otto if self.problem == "C" else synthetic.benoit)(x[None])[0]
                xn = (x - self.ds["X_mean"]) / self.ds["X_std"]
                yn = (y - self.ds["Y_mean"]) / self.ds["Y_std"]
                eng.append_sample(xn, yn)
                out = dict(self.ds)
                out["X_norm"] = np.vstack([self.ds["X_norm"], xn[None]])
                out["Y_norm"] = np.vstack([self.ds["Y_norm"], yn[None]])
                out["invKopt"] = oracle.build_invK(out["X_norm"], self.ds["hypopt"])
                self.ds = out
                self.ds_ver += 1
            self.last, self.robust_ok = None, False
        elif kind == "option":
            eng.set_option(s[1], s[2])
        elif kind == "refuse":
            self.refuse(s[1])
        elif kind == "safeopt":
            self.safeopt(*s[1:])
        elif kind == "goose":
            self.goose(*s[1:])
        elif kind == "tr":
            self.tr(*s[1:])
        elif kind == "robust":
            self.robust(*s[1:])
        elif kind == "posterior":
            self.check_posterior()
        elif kind == "posterior_run":
            eng.posterior_run()
            self.check_posterior()
        elif kind == "explore":
            lo, hi = self.pts.min(axis=0), self.pts.max(axis=0)
            t = lo + np.asarray(s[1]) * (hi - lo)
            if self.last is None:
                return
            S = self.last[1]["S"]
            idx, x = eng.explore_safeset(t)
            d2 = np.sqrt(np.sum((self.pts - t) ** 2, axis=1))
            assert idx == int(np.argmin(np.where(S, d2, np.inf))), ("explore", idx)
            assert np.array_equal(x, self.pts[idx])
        else:
            raise KeyError(kind)

    # ---- checks ---------------------------------------------------------------------------------------------------------------
    def _ys(self, o=0):
        return max(1.0, float(self.ds["Y_std"][o]))

    def check_posterior(self):
        mean, var = self.eng.posterior()
        om, ov = self._ref("post")
        tol = 1e-10 if self.dtype == "f64" else 1e-4
        em, ev = _nerr(mean, om, self.ds["Y_std"], 1), _nerr(var, ov, self.ds["Y_std"], 2)
        assert em < tol and ev < tol, ("posterior", em, ev)

    def _raises(self, fn):
        try:
            fn()
        except AssertionError:
            raise
        except Exception:                                          # noqa: BLE001
            return
        raise AssertionError("the call was not refused")

    def refuse(self, kind):
        eng = self.eng
        if kind == "b_nan":
            self._raises(lambda: eng.sweep_safeopt(float("nan"), want_masks=True))
        elif kind == "b_neg":
            self._raises(lambda: eng.sweep_goose(-1.0, want_masks=True))
        elif kind == "append_nonfinite":
            d, q = self.ds["X_norm"].shape[1], self.ds["Y_norm"].shape[1]
            self._raises(lambda: eng.append_sample(np.full(d, 0.1), np.array([np.inf] + [0.0] * (q - 1))))
        elif kind == "grid_zero":
            bound = self.bound
            self._raises(lambda: eng.set_grid(bound[:, 0], bound[:, 1], [0, 64]))
        elif kind == "mask_g_after_goose":
            self._raises(lambda: eng.mask("G", 1))
        elif kind == "robust_arrays_after_model":
            self._raises(lambda: eng.robust_arrays())

    def _empty(self, ref, call):
        try:
            call()
        except AssertionError:
            raise
        except Exception as e:                                     # noqa: BLE001
            assert type(e).__name__ == "EmptySafeSetError", e
            return
        raise AssertionError("the oracle's safe set is empty; the sweep did not say so")

    def safeopt(self, b, lean, ready, quirk):
        ref = self._ref("safeopt", b, quirk)
        q = self.ds["Y_norm"].shape[1]
        call = lambda: self.eng.sweep_safeopt(b, quirk_L_index=quirk, want_masks=True, posterior_ready=ready, lean=lean)  # noqa: E731
        if ref["empty_safe_set"]:
            self.last = None
            return self._empty(ref, call)
        res = call()
        eng = self.eng
        for k in ("S", "U", "M"):
            assert np.array_equal(eng.mask(k), ref[k]), k
        for c in range(1, q):
            assert np.array_equal(eng.mask("G", c), ref["G"][c - 1]), f"G{c}"
        assert (res["count_S"], res["count_U"], res["count_M"]) == (ref["S"].sum(), ref["U"].sum(), ref["M"].sum())
        assert list(res["count_G"]) == list(ref["G"].sum(1))
        assert res["minimizer_index"] == ref["minimizer_index"]
        assert list(res["expander_index_c"]) == list(ref["expander_index"])
        assert res["expander_best_c"] == ref["expander_best"] and res["choose_minimizer"] == ref["choose_minimizer"]
        assert abs(res["u_star"] - ref["u_star"]) < 1e-10 * self._ys(0), ("u_star", res["u_star"], ref["u_star"])
        assert abs(res["minimizer_std"] - ref["minimizer_std"]) < (1e-10 if self.dtype == "f64" else 1e-9) * max(self._ys(0), ref["minimizer_std"])
        if lean and q >= 2:
            assert res["L"][0] == 0.0, ("a lean sweep reports L[0] = 0", res["L"])
            assert np.allclose(res["L"][1:], ref["L"][1:], rtol=1e-9), ("L", res["L"], ref["L"])
        else:
            assert np.allclose(res["L"], ref["L"], rtol=1e-9), ("L", res["L"], ref["L"])
        self.last = ("safeopt", ref)

    def goose(self, b, ready):
        ref = self._ref("goose", b)
        q = self.ds["Y_norm"].shape[1]
        call = lambda: self.eng.sweep_goose(b, want_masks=True, posterior_ready=ready)  # noqa: E731
        if ref["empty_safe_set"]:
            self.last = None
            return self._empty(ref, call)
        res = call()
        eng = self.eng
        for k in ("S", "U"):
            assert np.array_equal(eng.mask(k), ref[k]), k
        for c in range(1, q):
            assert np.array_equal(eng.mask("O", c), ref["O"][c - 1]), f"O{c}"
        assert (res["count_S"], res["count_U"]) == (ref["S"].sum(), ref["U"].sum())
        assert list(res["count_O"]) == list(ref["O"].sum(1))
        assert res["safe_min_index"] == ref["safe_min_index"]
        assert list(res["target_index_c"]) == list(ref["target_index_c"])
        assert res["target_index"] == ref["target_index"] and res["explore_index"] == ref["explore_index"]
        assert res["choose_safe_min"] == ref["choose_safe_min"]
        assert np.allclose(res["L"], ref["L"], rtol=1e-9), ("L", res["L"], ref["L"])
        self.last = ("goose", ref)

    def tr(self, b, r, ready):
        x0 = self.pts[len(self.pts) // 3]
        ref = self._ref("tr", b, tuple(x0), r)
        call = lambda: self.eng.sweep_tr(b, x0, r, posterior_ready=ready)  # noqa: E731
        if ref["empty"] and not ref["S"].any():
            return self._empty(ref, call)
        res = call()
        assert res["count_S"] == ref["S"].sum() and res["count_T"] == ref["T"].sum(), ("counts", res["count_S"], res["count_T"])
        assert res["index"] == (ref["index"] if not ref["empty"] else -1), ("index", res["index"])

    def robust(self, b, kind, ready):
        ref = self._ref("robust", b, kind)
        res = self.eng.sweep_robust(b, 1, kind, posterior_ready=ready)
        assert res["index"] == ref["index"] and res["count_safe"] == ref["count_safe"], ("robust", res["index"], ref["index"])
        assert res["worst_d_index"] == ref["worst_d_index"]
        f, g = self.eng.robust_arrays()
        tol = 1e-10 if self.dtype == "f64" else 1e-4
        assert _nerr(f, ref["f"], self.ds["Y_std"][0], 1) < tol
        for c in range(g.shape[0]):
            assert _nerr(g[c], ref["g"][c], self.ds["Y_std"][c + 1], 1) < tol
