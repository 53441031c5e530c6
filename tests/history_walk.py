"""Seeded walks over one SweepEngine's call history -- test infrastructure for tests/test_gpu_history.py (GPU) and
tests/test_history_walk_cpu.py (the generator's coverage, no GPU).

The claim under test: whatever the engine did before, a sweep returns what a fresh context returns for the same model, candidates and
options.  A walk is a list of plain tuples (replayable from the seed alone, printed whole on a failure); the driver runs it on an
engine and checks every step against NumPy references of the current state: the dataset (appends rebuilt with frozen normalisation,
as tests/test_gpu_append.py::_extend does), the candidate set and the sweep's arguments.  Importing this module opens no GPU.

Seeds 0 .. 7 are the walks of the first version, step for step (tests/test_history_walk_cpu.py pins their digests): set_model, single
appends, the four sweeps, options and three reads.  Seeds 8 .. 15 add what has joined the ABI since: removals, block appends, the
on-device fit and a caller's prior (model-changing steps, each under a resident K1i, K1b or K1g plan and followed by two sweeps), and
the read-only calls -- model_loo, mean_grad, lipschitz, batch_select, the three refines, the likelihood kernels -- each checked
against the oracle its own suite uses and followed by a sweep on ``posterior_ready``.  A new step never returns early: the generator
establishes its precondition and the driver raises when it is missing.  ``Walk(None, ...)`` is the dry mode: no engine, references
only, and per sweep the smallest margin of any decision (``Walk.margins``).

Seeds 16 .. 23 (the third generation, _Gen3) add expander_gain and sample_paths -- each against the NumPy statement of its own suite
(expander_oracle.gain_naive, paths_oracle.paths_solve) on the rows the walk holds, sharp by assertion, and repeated with the same
arguments behind the posterior_ready sweep that follows it: the same bytes -- and three situations the earlier walks forbid: a
read-only call directly behind a model change with no sweep in between (mask("S") is refused before the call and still refused after
it), model_loo / batch_select / expander_gain / sample_paths on an fp32 model and behind its updates at their fp64 bars, and a caller's
prior that is not zero.  Seeds 0 .. 15 are untouched by all of this: READ_ONLY stays the tuple _make_walk2 indexes.
"""
import numpy as np

import batch_oracle
import de_twin
import expander_oracle
import model_append_batch as mb
import model_loo
import model_remove as mr
import nll_grad_oracle
import oracle
import paths_oracle
import refine_sets_oracle as rso
import robust_oracle
import robust_refine_oracle
from safebo_amd import SweepEngine, synthetic

# problems: (config, n) -- B and H (q = 2, Benoit), C (q = 3, the Williams-Otto shape), A (small n)
PROBLEMS = {"A": ("A", 20), "B": ("B", 64), "H": ("H", 96), "C": ("C", 48)}
# 2-D grids: whole 64 x 128 tiles (128 x 64, 256 x 64) and grids that are not (130 x 70, 96 x 50); count[0] is the fast axis.  (Sized
# for the NumPy expander references, whose cost grows with |S| x |U|)
GRIDS = {"t128x64": [128, 64], "t256x64": [256, 64], "r130x70": [130, 70], "r96x50": [96, 50]}
SMALLER = {"t256x64": "r130x70", "r130x70": "r96x50", "t128x64": "r96x50", "r96x50": "r96x50"}
LARGER = {"r96x50": "t256x64", "r130x70": "t256x64", "t128x64": "t256x64", "t256x64": "t256x64"}
LISTS = {"l1000": 1000, "l2000": 2000}
# a grid over a small box inside the safe set (_inside_box): every control is robust-safe there, so a robust sweep has a winner for
# refine_robust to start from -- on the whole domain of these problems no control is safe against every disturbance
INSIDE = {"i128x64": [128, 64]}
ALL_GRIDS = dict(GRIDS, t256x128=[256, 128], **INSIDE)      # (+ the directed tests' grid)
# option whitelist (value sets) and the defaults a walk restores
OPTIONS_V1 = {"bilinear": (0, 1, 2), "col_path": (0, 1, 2), "fuse_classify": (-1, 0, 1), "posterior_path": (0, 1, 2), "k1_sched": (0, 1),
           "guard_band": (1, 2), "list_index": (-1, 0, 1), "exact_lazy": (1, 2), "tensor_cheb": (0, 1)}
DEFAULTS_V1 = {"bilinear": 1, "col_path": 1, "fuse_classify": -1, "posterior_path": 0, "k1_sched": 1, "guard_band": 1, "list_index": -1,
            "exact_lazy": 1, "tensor_cheb": 1}
# (seeds 8 ..: the options that have joined the column path and the set phase since)
OPTIONS = dict(OPTIONS_V1, k1_skip_safe=(0, 1), col_overlap=(0, 1), set_fuse=(0, 1), set_lanes=(0, 1), grad_defer=(0, 1, 2, 3))
DEFAULTS = dict(DEFAULTS_V1, k1_skip_safe=1, col_overlap=1, set_fuse=1, set_lanes=1, grad_defer=1)
READY_KINDS = ("safeopt", "goose", "tr", "robust")
REFUSALS = ("b_nan", "b_neg", "append_nonfinite", "grid_zero", "mask_g_after_goose", "robust_arrays_after_model")
OLD_SEEDS = tuple(range(8))
NEW_SEEDS = tuple(range(8, 16))
THIRD_SEEDS = tuple(range(16, 24))
SEEDS = OLD_SEEDS + NEW_SEEDS + THIRD_SEEDS
READ_ONLY = ("loo", "mean_grad", "lipschitz", "batch_select", "refine", "refine_sets", "refine_robust", "nll")     # (_make_walk2 indexes this)
NEW_CALLS = ("expander_gain", "sample_paths")
READ_ONLY3 = READ_ONLY + NEW_CALLS
F32_READS = ("loo", "batch_select", "expander_gain", "sample_paths")      # fp64 data and factor "for every model dtype" 
F64_ONLY = ("mean_grad", "lipschitz", "refine")                           # refused on an fp32 model
MODEL_STEPS = ("remove", "append_block", "fit", "set_prior_zero", "set_prior")
# the model-changing steps a read-only call stands directly behind (seeds 16 ..), as the driver and transitions() label them
CHANGES = ("set_model_invK1", "set_model_invK0", "append", "remove_first", "remove_middle", "remove_last", "append_block_1",
           "append_block_3", "append_block_17", "fit", "set_prior")
F32_UPDATES = ("append", "append_block_3", "remove_middle")
PRIOR = (0.3, -0.7, 0.4)        # set_prior: a caller's prior that is not zero, normalised units, cut to q
EG_SOURCES, EG_TARGETS = 9, 257                  # expander_gain: off the 64 x 64 tile edges of csrc/expander.hip
SP_POINTS, SP_PATHS, SP_FEATURES = 257, 17, 257  # sample_paths: off the 128-point tiles, the 16-path blocks and the 32-column slabs
SHARP = 1e-8                    # the sharpness above which counts, witnesses and path indices are compared exactly (a condition on the inputs)
UNDER = ("K1i", "K1b", "K1g")
RTOL_GRAD = 1e-9            # tests/test_gpu_lipschitz.py: RTOL, per output, of the largest |grad_o| over the step's points
FIT_BOX = np.array([[-1.0, 0.5], [-1.0, 0.5], [-0.5, 0.5], [-2.5, -1.5]])     # (d = 2: a box of well-conditioned models)
FIT_P, FIT_MAXITER, FIT_SEED = 8, 4, 77
WALK_PROBLEMS = ("B", "H", "C", "A", "B", "C", "H", "B")
WALK3_PROBLEMS = ("B", "H", "C", "A", "B", "H", "C", "A")      # seeds 16 ..: the four problems, two seeds each
SWEEPS = ("safeopt", "goose", "tr", "robust")


def walk_problem(seed):
    return WALK3_PROBLEMS[seed - THIRD_SEEDS[0]] if seed >= THIRD_SEEDS[0] else WALK_PROBLEMS[seed % len(WALK_PROBLEMS)]


# ---- the generator (CPU only) ----------------------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, seed):
        self.rng = np.random.default_rng(1000 + seed)
        self.seed = seed
        self.steps = []
        self.problem = walk_problem(seed)
        self.b = float(synthetic.CONFIGS[PROBLEMS[self.problem][0]]["b"])
        self.grid = None
        self.on_list = False
        self.options = OPTIONS_V1

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
            key = str(self.rng.choice(list(self.options)))
            self.emit("option", key, int(self.rng.choice(self.options[key])))
            self.sweep()

    def seg_reads(self):
        self.sweep("safeopt", ready=False, lean=int(self.rng.integers(3)))
        self.emit("posterior")
        self.emit("explore", [float(v) for v in self.rng.uniform(0.0, 1.0, size=2)])
        self.emit("posterior_run")
        self.sweep(ready=True)


class _Gen2(_Gen):
    """Seeds 8 ..: the old segments plus one per step added since."""

    def __init__(self, seed):
        super().__init__(seed)
        self.options = OPTIONS
        self.touched = []

    def emit(self, *step):
        if step[0] == "option" and step[1] not in self.touched:
            self.touched.append(step[1])
        super().emit(*step)

    def under(self, under, robust=False):
        """A fresh fp64 model with the plan `under` resident (seg_append's way there); `robust`: the last sweep in front of the
        step is a robust one, whose arrays the step has to drop."""
        if under == "K1i":
            self.to_grid("t256x128")
        elif self.on_list or self.grid == "t256x128":
            self.to_grid(self.grid if self.grid in GRIDS else "t128x64")
        self.emit("option", "posterior_path", 0)
        self.emit("option", "bilinear", 0 if under == "K1g" else 1)
        self.model()
        self.sweep("safeopt", ready=False, lean=0)
        if under == "K1b":
            self.sweep("safeopt", ready=False)
        if robust:
            assert under != "K1i"            # (K1i is the model's first sweep alone)
            self.sweep("robust", ready=bool(self.rng.integers(2)))

    def after(self, under):
        self.sweep()
        self.sweep()
        if under == "K1g":
            self.emit("option", "bilinear", 1)

    def seg_remove(self, under, index_kind, robust=False):
        self.under(under, robust)
        self.emit("remove", index_kind, under)
        self.after(under)

    def seg_append_block(self, under, k, robust=False):
        self.under(under, robust)
        self.emit("append_block", k, under)
        self.after(under)

    def seg_fit(self, under, robust=False):
        self.under(under, robust)
        self.emit("fit", under)
        self.after(under)

    def seg_set_prior_zero(self):
        if self.on_list:
            self.to_grid()
        self.model()
        self.sweep("safeopt", ready=False, lean=0)
        self.emit("set_prior_zero")
        self.sweep()
        self.sweep()
        self.model()
        self.sweep("safeopt", ready=False, lean=0)

    def seg_remove_on_list(self):
        self.emit("option", "list_index", 1)
        self.on_list = True
        self.emit("set_points", "l2000")
        self.model()
        self.sweep("safeopt", ready=False, lean=0)
        self.emit("remove", "middle", "list")
        self.sweep()
        self.sweep()
        self.emit("option", "list_index", -1)

    def seg_new_options(self, *settings):
        """The options added since the first version at the values the drawn ones of seg_options do not reach: each followed by a
        lean-2 SafeOpt sweep (the column path's) and a random one, and left standing until the walk's end."""
        if self.on_list or self.grid not in GRIDS:
            self.to_grid(self.grid if self.grid in GRIDS else "t128x64")
        for key, val in settings:
            self.emit("option", key, val)
            self.sweep("safeopt", ready=False, lean=2)
            self.sweep()

    def seg_read_only(self, step, kind):
        """A sweep that leaves the step what it reads, the step, a sweep of `kind` on posterior_ready."""
        if kind == "robust" and self.on_list:
            self.to_grid(self.grid if self.grid in GRIDS else "t128x64")
        if self.grid == "t256x128" and not self.on_list:
            self.to_grid("r130x70")
        back = self.grid
        if step == "refine_robust":
            self.to_grid("i128x64")
            self.model()
            self.sweep("robust", ready=False, b=self.b)
        else:
            self.sweep("safeopt" if step == "refine_sets" else str(self.rng.choice(["safeopt", "goose"])), ready=False, b=self.b, lean=0)
        if step == "batch_select":
            self.emit(step, 4)
        else:
            self.emit(step)
        self.sweep(kind, ready=True, b=self.b, lean=0)
        if step == "refine_robust":
            self.to_grid(back if back in GRIDS else "t128x64")

    def seg_dtype_round(self):
        """The old round with an append, a block append and a removal while the model is fp32 with its twin, and one single append
        after the last set_model(f64): the twin left behind is not that model's."""
        if self.on_list or self.grid == "t256x128":
            self.to_grid(self.grid if self.grid in GRIDS else "t128x64")
        three = ["safeopt", "goose", "tr"]
        self.model("f32")
        self.sweep(str(self.rng.choice(three)), ready=False)
        for step in (("append", 1, "f32"), ("append_block", 3, "f32"), ("remove", "middle", "f32")):
            self.emit(*step)
            self.sweep(str(self.rng.choice(three)), ready=bool(self.rng.integers(2)))
        self.model("f64")
        self.sweep(str(self.rng.choice(three)), ready=False)
        self.model("f32")
        self.sweep(str(self.rng.choice(three)), ready=False)
        self.sweep(str(self.rng.choice(three)), ready=True)
        self.model("f64")
        self.emit("append", 1, "f64_after_f32")
        self.sweep()
        self.sweep(ready=True)


# seeds 8 ..: (model-changing segments, old segments); every seed also gets four read-only segments (make_walk)
NEW_PLAN = {
    8: ([("remove", "K1b", "first"), ("append_block", "K1b", 3), ("dtype_round",)], [("b_change",), ("new_options", ("set_fuse", 0))]),
    9: ([("remove", "K1g", "middle", True), ("append_block", "K1g", 17), ("set_prior_zero",)],
        [("options",), ("reads",), ("new_options", ("k1_skip_safe", 0), ("set_lanes", 0))]),
    10: ([("remove", "K1g", "last"), ("append_block", "K1g", 1)],
         [("shrink_grow",), ("options",), ("refuse", "b_nan"), ("new_options", ("set_lanes", 0), ("set_fuse", 0))]),
    11: ([("remove", "K1i", "first"), ("append_block", "K1i", 17), ("remove_on_list",)], [("options",), ("new_options", ("grad_defer", 0))]),
    12: ([("append_block", "K1b", 17, True), ("remove", "K1b", "last"), ("fit", "K1b")],
         [("list_round",), ("options",), ("new_options", ("k1_skip_safe", 0))]),
    13: ([("append_block", "K1g", 3), ("set_prior_zero",), ("remove_on_list",)], [("options",), ("b_change",), ("new_options", ("set_lanes", 0))]),
    14: ([("remove", "K1g", "last"), ("append_block", "K1g", 1), ("remove_on_list",)],
         [("options",), ("shrink_grow",), ("new_options", ("col_overlap", 0), ("k1_skip_safe", 0))]),
    15: ([("fit", "K1b", True), ("remove", "K1b", "middle"), ("append_block", "K1b", 1)],
         [("options",), ("reads",), ("refuse", "mask_g_after_goose"), ("new_options", ("grad_defer", 2), ("set_fuse", 0))]),
}
# (every value of the five options that is not its default and the one a new_options segment of some seed sets)
NEW_OPTION_VALUES = {("set_fuse", 0), ("set_lanes", 0), ("k1_skip_safe", 0), ("col_overlap", 0), ("grad_defer", 0), ("grad_defer", 2)}


def _make_walk2(seed):
    g = _Gen2(seed)
    g.to_grid(str(g.rng.choice(["t128x64", "r130x70", "r96x50"])))     # (the NumPy references of the larger grids take seconds each)
    g.model()
    g.sweep("safeopt", ready=False, lean=0)
    changing, old = NEW_PLAN[seed]
    j0 = 4 * (seed - NEW_SEEDS[0])
    reads = [("read_only", READ_ONLY[(j0 + j) % len(READ_ONLY)], READY_KINDS[(seed + j + (j0 + j) // len(READ_ONLY)) % len(READY_KINDS)]) for j in range(4)]
    segs = list(changing) + list(old) + reads
    for i in g.rng.permutation(len(segs)):
        name, *args = segs[i]
        getattr(g, "seg_" + name)(*args)
    for key in g.touched:
        g.emit("option", key, DEFAULTS[key])
    return g.steps


class _Gen3(_Gen2):
    """Seeds 16 ..: expander_gain and sample_paths among the read-only calls, read-only calls directly behind a model change, on an
    fp32 model and behind a caller's prior.  The sweeps of these segments are named, not drawn: a SafeOpt or GoOSE sweep of a changed
    model is a NumPy expander reference of its own."""

    def __init__(self, seed):
        super().__init__(seed)
        self.paths = 0             # sample_paths steps so far: output q - 1 and 0 in turn, maximize alternates
        self.turn = seed           # the sweep kinds behind direct calls, in turn

    def plain_grid(self):
        if self.on_list or self.grid not in GRIDS:
            self.to_grid(self.grid if self.grid in GRIDS else "t128x64")

    def call(self, name, under="", mask=0):
        if name == "expander_gain":
            self.emit(name, mask, under)
        elif name == "sample_paths":
            self.emit(name, "first" if self.paths % 2 else "last", (self.paths + self.seed) % 2 == 0, int(self.rng.integers(1 << 30)), under)
            self.paths += 1
        elif name == "batch_select":
            self.emit(name, 4)
        else:
            self.emit(name)

    def change(self, label):
        if label.startswith("set_model_invK"):
            self.emit("set_model", self.problem, "f64", label.endswith("1"))
        elif label == "append":
            self.emit("append", 1, "direct")
        elif label.startswith("remove_"):
            self.emit("remove", label[len("remove_"):], "direct")
        elif label.startswith("append_block_"):
            self.emit("append_block", int(label[len("append_block_"):]), "direct")
        elif label == "fit":
            self.emit("fit", "direct")
        else:
            assert label == "set_prior", label
            self.emit("set_prior")

    def next_kind(self):
        self.turn += 1
        return ("tr", "robust", "goose", "tr", "safeopt", "robust")[self.turn % 6]

    def seg_single(self, name, ctx, kind):
        """One of the two new calls with K1i, K1b or K1g resident, or on a list: behind a sweep, in front of a sweep of `kind` on
        posterior_ready, and again behind that sweep."""
        if ctx == "list":
            self.emit("option", "list_index", int(self.rng.choice([-1, 0, 1])))
            self.on_list = True
            self.emit("set_points", str(self.rng.choice(list(LISTS))))
            self.sweep(str(self.rng.choice(["safeopt", "goose"])), ready=False, b=self.b, lean=0)
        else:
            self.under(ctx)
        self.call(name, under=ctx if ctx in UNDER else "")
        self.sweep(kind, ready=True, b=self.b, lean=0)
        self.emit("again", name)
        if ctx == "K1g":
            self.emit("option", "bilinear", 1)
        if ctx == "list":
            self.emit("option", "list_index", -1)

    def seg_pair(self, first, kind):
        """Both new calls, the second directly behind the first, between a sweep and a sweep of `kind` on posterior_ready; then both
        again.  Problem C: expander_gain runs with a one-bit mask too."""
        if kind == "robust":
            self.plain_grid()
        if self.grid == "t256x128" and not self.on_list:
            self.to_grid("r130x70")
        self.sweep(str(self.rng.choice(["safeopt", "goose"])), ready=False, b=self.b, lean=0)
        for name in (first, NEW_CALLS[1 - NEW_CALLS.index(first)]):
            self.call(name)
            if name == "expander_gain" and self.problem == "C":
                self.call(name, mask=int(self.rng.choice([2, 4])))
        self.sweep(kind, ready=True, b=self.b, lean=0)
        self.emit("again", NEW_CALLS[0])
        self.emit("again", NEW_CALLS[1])

    def seg_direct(self, *pairs):
        """A fresh model and a sweep; then, per (change, call): the model-changing step, the read-only call directly behind it, a sweep.
        The refine calls start from the winner of the sweep before the change, so they stand first, behind a set_model of the same model."""
        self.plain_grid()
        back, first = self.grid, pairs[0][1]
        if first == "refine_robust":
            self.to_grid("i128x64")
            self.model()
            self.sweep("robust", ready=False, b=self.b)
        else:
            self.model()
            self.sweep("safeopt" if first in ("refine", "refine_sets") else str(self.rng.choice(["safeopt", "goose"])), ready=False, b=self.b, lean=0)
        for label, name in pairs:
            self.change(label)
            self.call(name)
            self.sweep(self.next_kind(), ready=bool(self.rng.integers(2)), b=self.b, lean=0)
        if first == "refine_robust":
            self.to_grid(back)
        self.model()                                      # (the segments behind this one start from the problem's own model)
        self.sweep("safeopt", ready=False, lean=0)

    def seg_set_prior(self, first):
        """A caller's prior that is not zero: both new calls (the first directly behind the change) and two sweeps, then the model back."""
        self.plain_grid()
        self.model()
        self.sweep("safeopt", ready=False, lean=0)
        self.change("set_prior")
        self.call(first)
        self.sweep(self.next_kind(), ready=bool(self.rng.integers(2)), b=self.b, lean=0)
        self.call(NEW_CALLS[1 - NEW_CALLS.index(first)])
        self.sweep(self.next_kind(), ready=True, b=self.b, lean=0)
        self.model()
        self.sweep("safeopt", ready=False, lean=0)

    def seg_f32_reads(self, behind, tail):
        """An fp32 model with its twin: the four calls that read fp64 data whatever the model's dtype, each between two sweeps; the
        fp64-only calls refused; an append, a block append and a removal, each with one of `behind` directly behind it; then
        set_model(f64), an append and `tail`: the twin left behind is not that model's."""
        self.plain_grid()
        three = ["safeopt", "goose", "tr"]
        self.model("f32")
        self.sweep(str(self.rng.choice(three)), ready=False, b=self.b, lean=0)
        for name in F32_READS:
            self.call(name)
            self.sweep(str(self.rng.choice(three)), ready=True, b=self.b, lean=0)
        self.emit("refuse", "f64_only_on_f32")
        self.sweep(str(self.rng.choice(three)), ready=True, b=self.b, lean=0)
        for step, name in zip((("append", 1, "f32"), ("append_block", 3, "f32"), ("remove", "middle", "f32")), behind):
            self.emit(*step)
            self.call(name)
            self.sweep(str(self.rng.choice(["goose", "tr"])), ready=bool(self.rng.integers(2)), b=self.b)
        self.model("f64")
        self.emit("append", 1, "f64_after_f32")
        self.call(tail)
        self.sweep("tr", ready=bool(self.rng.integers(2)), b=self.b)


# seeds 16 ..: per seed the segments of _Gen3 (and seg_read_only of _Gen2 for one of the eight older calls), in the order the seed shuffles
THIRD_PLAN = {
    16: [("single", "expander_gain", "K1b", "safeopt"), ("pair", "expander_gain", "goose"), ("read_only", "loo", "tr"),
         ("direct", ("set_model_invK1", "refine"), ("append", "expander_gain"), ("remove_first", "sample_paths"),
          ("append_block_1", "expander_gain"), ("fit", "sample_paths"))],
    17: [("single", "sample_paths", "K1g", "goose"), ("pair", "sample_paths", "tr"), ("read_only", "mean_grad", "robust"),
         ("direct", ("set_model_invK0", "refine_sets"), ("append", "sample_paths"), ("remove_middle", "expander_gain"),
          ("append_block_3", "sample_paths"), ("fit", "expander_gain"))],
    18: [("single", "expander_gain", "K1i", "tr"), ("pair", "expander_gain", "robust"), ("read_only", "lipschitz", "safeopt"),
         ("direct", ("set_model_invK1", "expander_gain"), ("remove_last", "sample_paths"), ("append_block_17", "expander_gain"),
          ("remove_middle", "loo"))],
    19: [("single", "sample_paths", "K1i", "robust"), ("pair", "sample_paths", "safeopt"), ("read_only", "batch_select", "goose"),
         ("direct", ("set_model_invK0", "sample_paths"), ("remove_first", "expander_gain"), ("append_block_1", "sample_paths"),
          ("append_block_3", "mean_grad"))],
    20: [("single", "expander_gain", "list", "goose"), ("pair", "expander_gain", "tr"), ("read_only", "refine", "robust"),
         ("direct", ("set_model_invK1", "sample_paths"), ("remove_middle", "sample_paths"), ("append_block_3", "expander_gain"),
          ("append_block_17", "lipschitz")),
         ("f32_reads", ("loo", "expander_gain", "batch_select"), "sample_paths")],
    21: [("single", "sample_paths", "list", "safeopt"), ("pair", "sample_paths", "goose"), ("read_only", "refine_sets", "tr"),
         ("direct", ("set_model_invK0", "expander_gain"), ("remove_last", "expander_gain"), ("append_block_17", "sample_paths"),
          ("append", "batch_select")),
         ("f32_reads", ("sample_paths", "batch_select", "expander_gain"), "expander_gain")],
    22: [("single", "expander_gain", "K1g", "robust"), ("pair", "expander_gain", "safeopt"), ("read_only", "refine_robust", "goose"),
         ("direct", ("set_model_invK1", "refine_robust"), ("remove_first", "nll")), ("set_prior", "expander_gain")],
    23: [("single", "sample_paths", "K1b", "tr"), ("pair", "sample_paths", "robust"), ("read_only", "nll", "safeopt"),
         ("direct", ("remove_middle", "expander_gain"), ("append_block_17", "sample_paths")), ("set_prior", "sample_paths")],
}


def _make_walk3(seed):
    g = _Gen3(seed)
    g.to_grid(str(g.rng.choice(["t128x64", "r130x70", "r96x50"])))
    g.model()
    g.sweep("safeopt", ready=False, lean=0)
    segs = THIRD_PLAN[seed]
    for i in g.rng.permutation(len(segs)):
        name, *args = segs[i]
        getattr(g, "seg_" + name)(*args)
    for key in g.touched:
        g.emit("option", key, DEFAULTS[key])
    return g.steps


def make_walk(seed):
    """The step list of walk ``seed`` (deterministic: the seed is all a replay needs)."""
    if seed >= THIRD_SEEDS[0]:
        return _make_walk3(seed)
    if seed >= NEW_SEEDS[0]:
        return _make_walk2(seed)
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
    for key, val in DEFAULTS_V1.items():
        g.emit("option", key, val)
    return g.steps


def change_label(s):
    """The name of a model-changing step as CHANGES has it (None: the step changes no model)."""
    kind = s[0]
    if kind == "set_model":
        return "set_model_f32" if s[2] != "f64" else "set_model_invK%d" % int(s[3] if len(s) > 3 else True)
    if kind == "remove":
        return "remove_" + s[1]
    if kind == "append_block":
        return "append_block_%d" % s[1]
    return kind if kind in ("append", "fit", "set_prior", "set_prior_zero") else None


def transitions(steps, third=False):
    """Names of the required transitions a step list contains (what the CPU test asserts over the fixed seeds).  ``third``: the walk
    is one of seeds 16 .., where a read-only call may stand directly behind a model change and on an fp32 model."""
    out = set()
    last_sweep = None
    model_sweeps = 0
    opts = dict(DEFAULTS)
    on_list = False
    dtypes = []
    cands = []
    grid = None
    pending = None               # a read-only step waiting for its sweep: (step name, directly behind a model change)
    prev_change = None           # the label of the model-changing step directly in front of this step
    stale_sweep = None           # the last sweep in front of that change
    recent, swept = [], []       # the new calls since the last sweep; those a posterior_ready sweep has followed since
    prior_seg = None             # behind set_prior, until the next set_model: [new calls, sweeps]
    for i, s in enumerate(steps):
        kind = s[0]
        if kind == "again":
            assert third and s[1] in swept, (i, s, "a repeated call stands behind the posterior_ready sweep that followed the first")
            out.add("again_" + s[1])
            continue
        if pending is not None:
            name, direct = pending
            pending = None
            if third and kind in NEW_CALLS and name in NEW_CALLS and not direct:
                out.add(f"{name}->{kind}")                  # the second of a pair stands directly behind the first
            else:
                ready = kind in SWEEPS and (s[2] if kind == "goose" else s[3])
                assert ready or (direct and kind in SWEEPS), (i, s, "a read-only step is followed by a sweep (on posterior_ready unless "
                                                                    "the step stood directly behind a model change)")
                if not direct:
                    out.add(f"{name}->{kind}_ready")
        if kind not in SWEEPS:
            swept = []
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
            swept, recent = (recent if ready else []), []
            if prior_seg is not None:
                prior_seg[1] += 1
        elif kind == "set_model":
            if prior_seg is not None and set(prior_seg[0]) == set(NEW_CALLS) and prior_seg[1] >= 2:
                out.add("set_prior_segment")
            prior_seg = None
            stale_sweep = last_sweep
            model_sweeps = 0
            last_sweep = None
            dtypes.append(s[2])
        elif kind in READ_ONLY3:
            direct = prev_change is not None
            f32 = dtypes[-1] != "f64"
            if not third:
                assert kind in READ_ONLY and not f32 and model_sweeps >= 1 and not direct, (i, s)
            assert kind in F32_READS or not f32, (i, s)
            assert direct == (last_sweep is None), (i, s, "a read-only step stands behind a sweep, or directly behind a model change")
            before = stale_sweep if direct else last_sweep
            assert kind != "refine_robust" or (before[0] == "robust" and not on_list), (i, s)
            assert kind != "refine_sets" or before[0] == "safeopt", (i, s)
            assert kind not in ("refine", "refine_sets", "refine_robust") or not direct or prev_change.startswith("set_model_invK"), (i, s)
            if kind in NEW_CALLS:
                if s[-1] in UNDER:
                    expect = "K1g" if opts["bilinear"] == 0 else ("K1i" if model_sweeps == 1 else "K1b")
                    assert not on_list and not direct and not f32 and expect == s[-1], (i, s, model_sweeps, opts["bilinear"])
                    out.add(f"{kind}_under_{s[-1]}")
                if on_list and not direct:
                    out.add(kind + "_on_list")
                if kind == "expander_gain" and s[1] != 0:
                    out.add("expander_gain_one_bit")
                if kind == "sample_paths":
                    out.add("sample_paths_output_" + {"first": "0", "last": "last"}[s[1]])
                    out.add("sample_paths_max" if s[2] else "sample_paths_min")
                if not direct:
                    recent.append(kind)
                if prior_seg is not None:
                    prior_seg[0].append(kind)
            if direct:
                out.add(f"direct:{'f32:' if f32 else ''}{prev_change}->{kind}")
                if stale_sweep is not None and stale_sweep[0] == "robust":
                    out.add("direct_read_robust_refused")
                if steps[i - 1][-1] == "f64_after_f32":
                    out.add("append_after_f32_then_f64->" + kind)
            elif f32:
                out.add("f32_read_" + kind)
            pending = (kind, direct)
        elif kind in MODEL_STEPS or (kind == "append" and s[2] not in UNDER):
            under = s[-1] if kind not in ("set_prior_zero", "set_prior") else None
            if last_sweep is not None and last_sweep[0] in ("safeopt", "goose"):
                out.add("mask_refused_after_model_change")
            if last_sweep is not None and last_sweep[0] == "robust":
                out.add("robust_arrays_refused_after_" + kind)
            if under in UNDER:
                out.add(f"{kind}_under_{under}")
                expect = "K1g" if opts["bilinear"] == 0 else ("K1i" if model_sweeps == 1 else "K1b")
                assert not on_list and expect == under and dtypes[-1] == "f64", (i, s, model_sweeps, opts["bilinear"])
            elif under == "list":
                assert kind == "remove" and on_list and opts["list_index"] == 1, (i, s)
                out.add("remove_on_list")
            elif under == "f32":
                assert dtypes[-1] == "f32", (i, s)
                out.add("f32_" + kind)
            elif under == "f64_after_f32":
                assert kind == "append" and dtypes[-2:] == ["f32", "f64"] and model_sweeps == 0, (i, s)
                out.add("append_after_f32_then_f64")
            elif under == "direct":
                assert third and dtypes[-1] == "f64" and last_sweep is not None, (i, s)
            else:
                assert kind in ("set_prior_zero", "set_prior") and (third or kind == "set_prior_zero"), (i, s)
                model_sweeps = 0
                if kind == "set_prior":
                    prior_seg = [[], 0]
            stale_sweep = last_sweep
            last_sweep = None
        elif kind == "append":
            out.add("append_under_" + s[2])
            # (the generator's label agrees with the state it left: K1i after one sweep, K1b after two, K1g with bilinear 0)
            expect = "K1g" if opts["bilinear"] == 0 else ("K1i" if model_sweeps == 1 else "K1b")
            assert not on_list and expect == s[2], (i, s, model_sweeps, opts["bilinear"])
        elif kind == "option":
            opts[s[1]] = s[2]
            if (s[1], s[2]) in NEW_OPTION_VALUES:
                out.add(f"option_{s[1]}_{s[2]}")
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
        elif kind == "refuse" and s[1] == "f64_only_on_f32":
            assert third and dtypes[-1] == "f32" and last_sweep is not None, (i, s)
            out.add("refuse_f64_only_on_f32")
        prev_change = change_label(s) if kind == "set_model" or kind in MODEL_STEPS or (kind == "append" and s[2] not in UNDER) else None
    if any(cands[j:j + 3] == ["list", "grid", "list"] for j in range(len(cands))):
        out.add("list->grid->list")
    if any(dtypes[j:j + 3] == ["f32", "f64", "f32"] for j in range(len(dtypes))):
        out.add("f32->f64->f32")
    assert pending is None, "a walk does not end on a read-only step"
    return out


def walk_transitions(seed):
    return transitions(make_walk(seed), third=seed >= THIRD_SEEDS[0])


REQUIRED = ({f"lean{lv}->{k}_ready" for lv in (0, 1, 2) for k in READY_KINDS} |
            {"append_under_K1i", "append_under_K1b", "append_under_K1g", "refused->sweep", "grid_shrink", "grid_grow",
             "list->grid->list", "f32->f64->f32", "b_change_between_ready"} |
            {f"{k}_under_{u}" for k in ("remove", "append_block") for u in UNDER} |
            {"fit_under_K1b", "remove_on_list", "f32_append", "f32_append_block", "f32_remove", "append_after_f32_then_f64",
             "mask_refused_after_model_change", "robust_arrays_refused_after_remove", "robust_arrays_refused_after_append_block",
             "robust_arrays_refused_after_fit"} |
            {f"option_{k}_{v}" for k, v in NEW_OPTION_VALUES})
# what seeds 16 .. add: the two new calls in front of every sweep kind, with each plan resident, on a list, behind each other, repeated
# around a sweep and directly behind every model-changing step; each of the ten read-only calls directly behind some model change
# (direct_leaders); the four dtype-free calls on an fp32 model and behind its updates; the prior and the new refusal
REQUIRED3 = ({f"{c}->{k}_ready" for c in READ_ONLY3 for k in READY_KINDS if c in NEW_CALLS} |
             {f"{c}_under_{u}" for c in NEW_CALLS for u in UNDER} | {c + "_on_list" for c in NEW_CALLS} | {"again_" + c for c in NEW_CALLS} |
             {"expander_gain->sample_paths", "sample_paths->expander_gain", "expander_gain_one_bit", "sample_paths_output_0",
              "sample_paths_output_last", "sample_paths_max", "sample_paths_min"} |
             {f"direct:{m}->{c}" for m in CHANGES for c in NEW_CALLS} |
             {"direct_read_robust_refused", "set_prior_segment", "refuse_f64_only_on_f32", "f32_append", "f32_append_block", "f32_remove",
              "append_after_f32_then_f64"} |
             {"f32_read_" + c for c in F32_READS})


def read_only_followers(seen, calls=READ_ONLY):
    """{read-only step: sweep kinds found behind it on posterior_ready} of a set of transition names."""
    out = {k: set() for k in calls}
    for name in seen:
        head, _, tail = name.partition("->")
        if head in out and tail.endswith("_ready"):
            out[head].add(tail[:-len("_ready")])
    return out


def direct_leaders(seen, f32=False):
    """{read-only step: the model-changing steps found directly in front of it} of a set of transition names (``f32``: on an fp32
    model, behind its updates)."""
    out = {k: set() for k in (F32_READS if f32 else READ_ONLY3)}
    head = "direct:f32:" if f32 else "direct:"
    for name in seen:
        if name.startswith(head) and (f32 or not name.startswith("direct:f32:")):
            change, _, call = name[len(head):].partition("->")
            out[call].add(change)
    return out


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


_INSIDE = {}


def _inside_box(problem):
    """(lo, hi): 2 % of the problem's domain around the coarse-grid candidate whose smallest constraint lcb is largest (the way of
    tests/skip_safe_cases.py: grid)."""
    if problem not in _INSIDE:
        cfg = _problem(problem)
        lo, hi = cfg["bound"][:, 0], cfg["bound"][:, 1]
        coarse = oracle.grid_points(lo, hi, [64, 64])
        mean, var = oracle.gp_inference(coarse, cfg["ds"])
        lcb = (mean - float(cfg["b"]) * np.sqrt(var))[:, 1:].min(axis=1)
        c, w = coarse[int(np.argmax(lcb))], 0.01 * (hi - lo)
        _INSIDE[problem] = (np.maximum(lo, c - w), np.minimum(hi, c + w))
    return _INSIDE[problem]


def _nerr(got, ref, ystd, power):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref) / np.maximum(1.0, ystd) ** power)) if np.size(ref) else 0.0


class Walk:
    """Runs a step list on ``eng`` and checks every step.  ``record`` collects (step index, posterior_kernel, set_path).  With
    ``eng`` None (the dry mode) nothing runs: the references are computed and ``margins`` collects, per sweep, (step index, kind, the
    smallest normalised distance of any S / U / M / G / O / T decision of the oracle from its threshold: _margin)."""

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
        self.cache = {}
        self.rng = np.random.default_rng(5000 + seed)
        self.walk_problem = problem or walk_problem(seed)
        self.bound = _problem(self.walk_problem)["bound"]
        self.box = (self.bound[:, 0], self.bound[:, 1])     # of the resident candidates: the domain, or an INSIDE grid's small box
        self.append_kernels = set()     # posterior kernel of the sweep before each append
        self.remove_kernels, self.block_kernels = set(), set()      # ... before each removal / block append on a grid
        self.dry = eng is None
        self.robust_refusals = 0        # model-changing steps behind a robust sweep: robust_arrays() was asserted refused
        self.margins = []
        self.index = 0
        self.masks = None               # what the engine's masks held behind the last sweep: {(name, c): array}
        self.rob_kept = None              # robust_arrays() behind the last robust sweep
        self.winner = None              # the last sweep's winner x [d], the seed of the refine steps
        self.last_sweep = None          # the last sweep's step
        self.has_masks = False          # the last sweep left masks or robust arrays (also kept in the dry mode)
        self.changed_by = None          # change_label of the model-changing step since which nothing has swept
        self.stale = None               # (winner, last_sweep, last) of the last sweep in front of that change, and whether it was robust
        self.stale_robust = False
        self.kept = {}                  # new call -> (ds_ver, arguments, result) of its last run, for the "again" step
        self.calls = []                 # per new call: {step, kind, kernel resident, on_list, dtype, direct (a change label or None)}
        self.direct = {}                # read-only call -> the change labels it stood directly behind
        self.devs = {}                  # new call -> the largest deviation from its reference
        self.direct_robust = 0          # direct read-only calls around which robust_arrays() was asserted refused

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
            self.index = i
            try:
                self.step(step)
                if step[0] in SWEEPS:
                    self.changed_by = None
                elif self.last_sweep is None and change_label(step) is not None:
                    self.changed_by = change_label(step)
            except Exception as e:                                 # noqa: BLE001
                listing = "\n".join(f"  {j:3d} {s!r}" for j, s in enumerate(self.steps[:i + 1]))
                raise AssertionError(f"history walk seed {self.seed}, step {i}: {step!r}\n"
                                     f"replay: history_walk.make_walk({self.seed})[:{i + 1}] =\n{listing}\n"
                                     f"{type(e).__name__}: {e}") from e
            if not self.dry:
                prof = self.eng.profile()
                self.record.append((i, step[0], int(prof["posterior_kernel"]), int(prof["set_path"])))
        return self.record

    def _changed(self):
        """A candidate or model change: nothing the last sweep left is readable any more."""
        if self.last_sweep is not None:
            self.stale, self.stale_robust = (self.winner, self.last_sweep, self.last), self.last_sweep[0] == "robust"
        self.last, self.masks, self.rob_kept, self.winner, self.last_sweep = None, None, None, None, None
        self.has_masks = False

    def _model_changed(self):
        """Behind a model-changing step: the masks are refused, and so are the robust arrays of an earlier robust sweep."""
        if not self.dry:
            self._raises(lambda: self.eng.mask("S"))
            if self.rob_kept is not None:
                self._raises(lambda: self.eng.robust_arrays())
                self.robust_refusals += 1
        self.ds_ver += 1
        self._changed()

    def _unchanged(self):
        """Behind a read-only step: the masks of the last sweep are still readable, byte for byte; so are the robust arrays."""
        if not self.has_masks:
            raise RuntimeError("a read-only step stands behind a sweep that left masks or robust arrays")
        if self.dry:
            return
        for (k, c), m in (self.masks or {}).items():
            assert np.array_equal(self.eng.mask(k, c), m), ("mask changed by a read-only call", k, c)
        if self.rob_kept is not None:
            f, g = self.eng.robust_arrays()
            assert f.tobytes() == self.rob_kept[0].tobytes() and g.tobytes() == self.rob_kept[1].tobytes(), "robust arrays changed"

    def _still_refused(self):
        """Around a read-only call directly behind a model change: the masks stay refused, and so do the robust arrays of a robust
        sweep in front of the change -- a reader waits for the factor, it does not make the last sweep's results readable again."""
        if self.dry:
            return
        self._raises(lambda: self.eng.mask("S"))
        if self.stale_robust:
            self._raises(lambda: self.eng.robust_arrays())
            self.direct_robust += 1

    def _keep_masks(self, names):
        self.has_masks = True
        self.masks = None if self.dry else {(k, c): self.eng.mask(k, c) for k, c in names}
        self.rob_kept = None

    def _reach_margin(self, ref, over_safe):
        """Smallest |max over the other set of (ucb_c(g) - L_c ||x_g - x_h + 1e-8||)| / max(1, Y_std[c]): the distance of a G_c decision
        (per g in S, the best h in U) or of an O_c decision (per h in U, the best g in S) from its threshold."""
        gi, hi = np.nonzero(ref["S"])[0], np.nonzero(ref["U"])[0]
        if gi.size == 0 or hi.size == 0:
            return np.inf
        ys, m = np.maximum(1.0, self.ds["Y_std"]), np.inf
        rows, cols = (gi, hi) if over_safe else (hi, gi)
        for s in range(0, rows.size, 1024):
            idx = rows[s:s + 1024]
            g, h = (idx[:, None], cols[None, :]) if over_safe else (cols[None, :], idx[:, None])
            dist = oracle.shifted_norm(self.pts[g], self.pts[h])
            for c in range(1, ref["ucb"].shape[1]):
                best = np.max(ref["ucb"][g, c] - ref["L_used"][c] * dist, axis=1)
                m = min(m, float(np.min(np.abs(best))) / ys[c])
        return m

    def _margin(self, kind, ref, x0=None, r=None):
        """Dry mode: the smallest normalised distance of any decision of the oracle's sweep from its threshold -- S / U (|lcb_c|), M
        (|lcb_0 - u*| over S), G_c / O_c (_reach_margin), and for the trust region T (| ||x - x_0|| - r | over S, relative to r)."""
        if not self.dry:
            return
        ys = np.maximum(1.0, self.ds["Y_std"])
        m = float(np.min(np.abs(ref["lcb"][:, 1:]) / ys[1:]))
        if kind == "tr":
            if ref["S"].any():
                m = min(m, float(np.min(np.abs(np.sqrt(np.sum((self.pts[ref["S"]] - x0) ** 2, axis=1)) - r))) / r)
        elif not ref["empty_safe_set"]:
            if kind == "safeopt":
                m = min(m, float(np.min(np.abs(ref["lcb"][ref["S"], 0] - ref["u_star"])) / ys[0]))
            m = min(m, self._reach_margin(ref, kind == "safeopt"))
        self.margins.append((self.index, kind, float(m)))

    def _plant_rows(self, k):
        bound = _problem(self.problem)["bound"]
        x = self.rng.uniform(bound[:, 0], bound[:, 1], size=(k, bound.shape[0]))
        y = (synthetic.williams_otto if self.problem == "C" else synthetic.benoit)(x)
        return (x - self.ds["X_mean"]) / self.ds["X_std"], (y - self.ds["Y_mean"]) / self.ds["Y_std"]

    def _kernel(self, under, into):
        if not self.dry and under in UNDER:
            into.add(int(self.eng.profile()["posterior_kernel"]))

    def step(self, s):
        eng, kind = self.eng, s[0]
        if kind == "set_grid":
            self.box = _inside_box(self.walk_problem) if s[1] in INSIDE else (self.bound[:, 0], self.bound[:, 1])
            if not self.dry:
                eng.set_grid(self.box[0], self.box[1], ALL_GRIDS[s[1]])
            self.cand = ("grid", s[1])
            self.pts = oracle.grid_points(self.box[0], self.box[1], ALL_GRIDS[s[1]])
            self._changed()
            self.changed_by = None
        elif kind == "set_points":
            pts = _list_points(self.walk_problem, s[1])
            if not self.dry:
                eng.set_points(pts)
            self.cand = ("list", s[1])
            self.pts = pts
            self.box = (self.bound[:, 0], self.bound[:, 1])
            self._changed()
            self.changed_by = None
        elif kind == "set_model":
            self.problem, self.dtype = s[1], s[2]
            cfg = _problem(s[1])
            self.ds = {k: (list(v) if k == "invKopt" else np.array(v)) for k, v in cfg["ds"].items()}
            self.ds_ver += 1
            use_invK = s[3] if len(s) > 3 else s[2] == "f64"
            if s[2] == "f64" and not use_invK:          # (the library factors K itself: the oracle's inverse of the hyper-parameters)
                self.ds["invKopt"] = oracle.build_invK(self.ds["X_norm"], self.ds["hypopt"])
            if not self.dry:
                eng.set_model(self.ds, dtype=s[2], use_invK=use_invK)
            self._changed()
        elif kind == "append":
            n_new = s[1]
            if not self.dry and s[2] in UNDER:
                self.append_kernels.add(int(eng.profile()["posterior_kernel"]))
            bound = _problem(self.problem)["bound"]
            for _ in range(n_new):
                x = self.rng.uniform(bound[:, 0], bound[:, 1])
                y = (synthetic.williams_otto if self.problem == "C" else synthetic.benoit)(x[None])[0]
                xn = (x - self.ds["X_mean"]) / self.ds["X_std"]
                yn = (y - self.ds["Y_mean"]) / self.ds["Y_std"]
                if not self.dry:
                    eng.append_sample(xn, yn)
                out = dict(self.ds)
                out["X_norm"] = np.vstack([self.ds["X_norm"], xn[None]])
                out["Y_norm"] = np.vstack([self.ds["Y_norm"], yn[None]])
                out["invKopt"] = oracle.build_invK(out["X_norm"], self.ds["hypopt"])
                self.ds = out
                self.ds_ver += 1
            if s[2] in UNDER:
                self._changed()
            else:
                self._model_changed()
        elif kind == "remove":
            n = self.ds["X_norm"].shape[0]
            if n <= 8:
                raise RuntimeError("a walk never takes a model below 8 rows")
            j = {"first": 0, "middle": n // 2, "last": n - 1}[s[1]]
            self._kernel(s[2], self.remove_kernels)
            if not self.dry:
                eng.remove_sample(j)
            self.ds = mr.without(self.ds, j)
            self._model_changed()
        elif kind == "append_block":
            xn, yn = self._plant_rows(s[1])
            self._kernel(s[2], self.block_kernels)
            if not self.dry:
                eng.append_samples(xn, yn)
            self.ds = mb.extended(self.ds, xn, yn)
            self._model_changed()
        elif kind == "fit":
            self.fit()
        elif kind == "set_prior_zero":
            self.ds = dict(self.ds, mean_prior=np.zeros(self.ds["Y_norm"].shape[1]))
            if not self.dry:
                eng.set_model(self.ds, dtype="f64", use_invK=True, mean_prior=self.ds["mean_prior"])
            self._model_changed()
        elif kind == "set_prior":
            mp = np.array(PRIOR[:self.ds["Y_norm"].shape[1]])
            self.ds = dict(self.ds, mean_prior=mp)
            if not self.dry:
                eng.set_model(self.ds, dtype="f64", use_invK=True, mean_prior=mp)
            self._model_changed()
        elif kind in READ_ONLY3:
            self.read_only(kind, s[1:])
        elif kind == "again":
            ver, args, first = self.kept[s[1]]
            if ver != self.ds_ver or self.last_sweep is None:
                raise RuntimeError("again: the call is repeated on the same model, behind a sweep")
            if not self.dry:
                second = self.run_new(s[1], args)
                for k in first:
                    assert first[k].tobytes() == second[k].tobytes(), (s[1], "repeated behind a sweep", k)
            self._unchanged()
        elif kind == "option":
            if not self.dry:
                eng.set_option(s[1], s[2])
        elif kind == "refuse":
            if s[1] == "f64_only_on_f32":
                self.refuse_f64_only()
            elif not self.dry:
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
            if not self.dry:
                self.check_posterior()
        elif kind == "posterior_run":
            if not self.dry:
                eng.posterior_run()
                self.check_posterior()
        elif kind == "explore":
            lo, hi = self.pts.min(axis=0), self.pts.max(axis=0)
            t = lo + np.asarray(s[1]) * (hi - lo)
            if self.last is None or self.dry:
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
        self._margin("safeopt", ref)
        self.last_sweep = ("safeopt", b, lean, ready, quirk)
        if ref["empty_safe_set"]:
            self.last, self.masks, self.rob_kept, self.winner, self.has_masks = None, None, None, None, False
            return None if self.dry else self._empty(ref, call)
        self.winner, self.has_masks = self.pts[ref["minimizer_index"]], True
        if self.dry:
            self.last = ("safeopt", ref)
            return
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
        self._keep_masks([("S", 0), ("U", 0), ("M", 0)] + [("G", c) for c in range(1, q)])

    def goose(self, b, ready):
        ref = self._ref("goose", b)
        q = self.ds["Y_norm"].shape[1]
        call = lambda: self.eng.sweep_goose(b, want_masks=True, posterior_ready=ready)  # noqa: E731
        self._margin("goose", ref)
        self.last_sweep = ("goose", b, ready)
        if ref["empty_safe_set"]:
            self.last, self.masks, self.rob_kept, self.winner, self.has_masks = None, None, None, None, False
            return None if self.dry else self._empty(ref, call)
        self.winner, self.has_masks = self.pts[ref["safe_min_index"]], True
        if self.dry:
            self.last = ("goose", ref)
            return
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
        self._keep_masks([("S", 0), ("U", 0)] + [("O", c) for c in range(1, q)])

    def tr(self, b, r, ready):
        x0 = self.pts[len(self.pts) // 3]
        ref = self._ref("tr", b, tuple(x0), r)
        call = lambda: self.eng.sweep_tr(b, x0, r, posterior_ready=ready)  # noqa: E731
        self._margin("tr", ref, x0, r)
        self.last_sweep = ("tr", b, r, ready)
        # (an empty trust region, or an empty safe set, is no error of sbo_sweep_tr: index -1 -- include/safebo.h: sbo_tr_result)
        self.winner, self.has_masks = (self.pts[ref["index"]] if not ref["empty"] else None), True
        if self.dry:
            return
        res = call()
        self._keep_masks([("S", 0), ("M", 0)])
        assert res["count_S"] == ref["S"].sum() and res["count_T"] == ref["T"].sum(), ("counts", res["count_S"], res["count_T"])
        assert res["index"] == (ref["index"] if not ref["empty"] else -1), ("index", res["index"])

    def robust(self, b, kind, ready):
        ref = self._ref("robust", b, kind)
        self.last_sweep = ("robust", b, kind, ready)
        self.winner = self.pts[ref["index"]][:1] if ref["index"] >= 0 else None      # (axis 0 is the control, the fastest)
        self.has_masks = True
        if self.dry:
            g = ref["g"] / np.maximum(1.0, self.ds["Y_std"])[1:, None]
            self.margins.append((self.index, "robust", float(np.min(np.abs(g))) if g.size else np.inf))
            return
        res = self.eng.sweep_robust(b, 1, kind, posterior_ready=ready)
        assert res["index"] == ref["index"] and res["count_safe"] == ref["count_safe"], ("robust", res["index"], ref["index"])
        assert res["worst_d_index"] == ref["worst_d_index"]
        f, g = self.eng.robust_arrays()
        tol = 1e-10 if self.dtype == "f64" else 1e-4
        assert _nerr(f, ref["f"], self.ds["Y_std"][0], 1) < tol
        for c in range(g.shape[0]):
            assert _nerr(g[c], ref["g"][c], self.ds["Y_std"][c + 1], 1) < tol
        self.masks, self.rob_kept = None, (f, g)

    # ---- the steps added since the first version ------------------------------------------------------------------------------------
    def fit(self):
        """engine.model_fit on the current data (P = 8, four generations, no polish, a fixed seed); the reference is the oracle of the
        returned hyper-parameters, built as use_invK=False builds it.  Dry: the host twin of the DE on the oracle's likelihood."""
        ds = self.ds
        d, q = ds["X_norm"].shape[1], ds["Y_norm"].shape[1]
        if d != 2:
            raise RuntimeError("the fit step's box is two-dimensional")
        pop = np.random.default_rng(FIT_SEED).uniform(FIT_BOX[:, 0], FIT_BOX[:, 1], size=(FIT_P, d + 2))
        if self.dry:
            hyp = np.empty((d + 2, q))
            for o in range(q):
                nll = lambda P, o=o: np.array([oracle.negative_loglikelihood(h, ds["X_norm"], ds["Y_norm"][:, o]) for h in P])  # noqa: E731
                hyp[:, o] = de_twin.fit_de(nll, FIT_BOX, pop, FIT_SEED + o, FIT_MAXITER, 0.0)[0]
        else:
            data = {k: ds[k] for k in ("X_mean", "X_std", "Y_mean", "Y_std", "X_norm", "Y_norm")}
            out = self.eng.model_fit(data, FIT_BOX, pop, seed=FIT_SEED, maxiter=FIT_MAXITER, tol=0.0, polish=False)
            hyp = out["hypopt"]
            assert hyp.shape == (d + 2, q) and np.all(hyp >= FIT_BOX[:, :1]) and np.all(hyp <= FIT_BOX[:, 1:]), hyp
        self.ds = dict(ds, hypopt=hyp, invKopt=oracle.build_invK(ds["X_norm"], hyp))
        self.ds.pop("mean_prior", None)
        self._model_changed()

    def ro_loo(self):
        if not self.dry:
            model_loo.check_loo(self.eng, self.ds, model_loo.TOL64, f"walk {self.seed} step {self.index}")

    def ro_mean_grad(self):
        lo, hi = self.box
        pts = self.rng.uniform(lo, hi, size=(257, len(lo)))
        if self.dry:
            return
        got, inf = self.eng.mean_grad(pts, infnorm=True)
        want = oracle.mean_grad(pts, self.ds)
        for o in range(want.shape[1]):
            scale, dev = np.max(np.abs(want[:, o, :])), np.max(np.abs(got[:, o, :] - want[:, o, :]))
            assert dev <= RTOL_GRAD * scale, ("mean_grad", o, dev, scale)
        assert np.array_equal(inf, np.max(np.abs(got), axis=2))

    def ro_lipschitz(self):
        if self.dry:
            return
        lo, hi = self.box
        out = self.eng.lipschitz(lo, hi)
        for o in range(self.ds["Y_norm"].shape[1]):
            x = out["x"][o]
            assert np.all(x >= lo) and np.all(x <= hi), ("lipschitz", o, x)
            assert out["L"][o] >= out["L_seed"][o] > 0.0, ("lipschitz", o, out["L"][o], out["L_seed"][o])
            _, inf = self.eng.mean_grad(x, infnorm=True)
            assert out["L"][o].tobytes() == inf[0, o].tobytes(), ("lipschitz", o, out["L"][o], inf[0, o])

    def ro_batch_select(self, k):
        lo, hi = self.box
        pool = self.rng.uniform(lo, hi, size=(500, len(lo)))
        ref = batch_oracle.select_naive(self.ds, 0, pool, k)
        if self.dry:
            return
        got = self.eng.batch_select(pool, k, 0, return_var=True)
        assert len(got["index"]) == k, got["index"]
        ys = float(self.ds["Y_std"][0])
        for j in range(k):
            # (picks are compared while the oracle's own arg-max is decided by more than GAP; behind a closer call the batches differ)
            if not ref["gaps"][j] > batch_oracle.GAP:
                break
            assert got["index"][j] == ref["index"][j], ("batch_select", j, got["index"], ref["index"], ref["gaps"])
            assert abs(got["std"][j] / ys - np.sqrt(max(0.0, ref["v_pick"][j]))) < batch_oracle.TOL64, ("batch_select std", j)
        else:
            assert np.max(np.abs(got["var"] / ys ** 2 - np.maximum(0.0, ref["v"]))) < batch_oracle.TOL64, "batch_select var"

    def _refine_contract(self, P, out, seed):
        """The contract of the refine calls: the oracle's posterior at the returned point satisfies every term, the reported value is
        the oracle's bound there, and it is no worse than the seed's -- all within 1e-10 max(1, Y_std)."""
        tol = 1e-10 * max(1.0, float(np.max(self.ds["Y_std"])))
        x = out["x"][0]
        assert out["best"] == 0 and np.all(x >= P["lo"]) and np.all(x <= P["hi"]), (out["best"], x)
        for name, g, _ in rso.terms(P, x):
            assert g >= -tol, ("refine term", name, g)
        val, val0 = rso.value(P, x), rso.value(P, seed)
        assert abs(out["value"][0] - val) <= tol, ("refine value", out["value"][0], val)
        worse = (val0 - out["value"][0]) if P["maximize"] else (out["value"][0] - val0)
        assert worse <= tol, ("refine: worse than its seed", out["value"][0], val0)

    def _seed(self, what):
        if self.winner is None or self.last_sweep[0] == "robust":
            raise RuntimeError(f"{what}: the last sweep left no winner to start from")
        return np.array(self.winner)

    def ro_refine(self):
        seed, b = self._seed("refine"), self.last_sweep[1]
        lo, hi = self.box
        P = rso.problem(self.ds, b, lo, hi, "lcb", objective=0)
        if not self.dry:
            self._refine_contract(P, self.eng.refine(b, seed, 0, "lcb", lo=lo, hi=hi), seed)

    def ro_refine_sets(self):
        """The M_t problem from the sweep's minimiser: max var_0 s.t. lcb_c >= 0 and lcb_0 <= u*."""
        if self.last_sweep[0] != "safeopt" or self.last is None:
            raise RuntimeError("refine_sets: the last sweep was no SafeOpt sweep with a safe set")
        seed, b = self._seed("refine_sets"), self.last_sweep[1]
        lo, hi = self.box
        P = rso.problem(self.ds, b, lo, hi, "var", objective=0, maximize=True, level=(0, float(self.last[1]["u_star"])))
        if not self.dry:
            self._refine_contract(P, self.eng.refine_sets(b, seed, **rso.engine_args(P)), seed)

    def ro_refine_robust(self):
        if self.last_sweep[0] != "robust" or self.cand[0] != "grid" or self.winner is None:
            raise RuntimeError("refine_robust: the last sweep was no robust sweep on a grid with a robust-safe control")
        _, b, kind, _ = self.last_sweep
        lo, hi = self.box
        count_d = [17]
        if self.dry:
            return
        out = self.eng.refine_robust(b, self.winner, 1, lo, hi, count_d, kind)
        ds, mp = self.ds, oracle.mean_prior(self.ds)
        tol = 1e-10 * max(1.0, float(np.max(ds["Y_std"])))
        Cset = np.vstack((robust_refine_oracle.check_grid(lo, hi, 1, count_d), out["scenarios"]))
        f, l = robust_refine_oracle.exact_on(out["xc"], Cset, ds, mp, b, kind)
        f0, _ = robust_refine_oracle.exact_on(self.winner, Cset, ds, mp, b, kind)
        assert lo[0] <= out["xc"][0] <= hi[0] and np.all(out["scenarios"] >= lo[1:]) and np.all(out["scenarios"] <= hi[1:])
        assert abs(out["value"] - np.max(f)) <= tol and abs(out["seed_value"] - np.max(f0)) <= tol, (out["value"], np.max(f), out["seed_value"], np.max(f0))
        assert np.max(np.abs(out["g_min"] - l[:, 1:].min(axis=0))) <= tol and np.all(l[:, 1:].min(axis=0) >= -tol), out["g_min"]
        assert out["value"] <= out["seed_value"] + tol

    def ro_nll(self):
        """nll_batch with P = 8 and nll_grad_batch on the current rows, output 0, at the tolerances of tests/test_gpu_fit_shapes.py."""
        X, y = self.ds["X_norm"], self.ds["Y_norm"][:, 0]
        d = X.shape[1]
        H = self.rng.uniform([-0.5] * d + [-0.5, -2.0], [0.5] * d + [0.5, -1.0], size=(8, d + 2))
        if self.dry:
            return
        nll = self.eng.nll_batch(X, y, H)
        nll2, grad = self.eng.nll_grad_batch(X, y, H)
        assert np.array_equal(nll.view(np.uint64), nll2.view(np.uint64))
        for p, h in enumerate(H):
            ref, g = nll_grad_oracle.nll_grad(h, X, y)
            assert abs(nll[p] - ref) <= 1e-9 * max(1.0, abs(ref)), ("nll", p, nll[p], ref)
            assert np.all(np.abs(grad[p] - g) <= 1e-8 * nll_grad_oracle.grad_scale(h, X, y) + 1e-300), ("nll grad", p, grad[p], g)

    # ---- seeds 16 ..: the two new calls, and read-only calls directly behind a model change or on an fp32 model ----------------------
    def read_only(self, kind, args):
        """A read-only step.  Behind a sweep: checked, and the sweep's masks and robust arrays are unchanged afterwards.  Directly
        behind a model change (nothing has swept since): checked with the arguments the sweep in front of the change left -- its b,
        its winner --, and mask("S") is refused before the call and still refused after it."""
        if self.dtype != "f64" and kind not in F32_READS:
            raise RuntimeError(f"{kind}: needs an fp64 model")
        direct = self.last_sweep is None
        if direct and (self.changed_by is None or self.stale is None):
            raise RuntimeError(f"{kind}: needs a sweep before it, or a model change behind a sweep")
        kernel = None if self.dry else int(self.eng.profile()["posterior_kernel"])
        if direct:
            self._still_refused()
            self.winner, self.last_sweep, self.last = self.stale
        try:
            getattr(self, "ro_" + kind)(*args)
        finally:
            if direct:
                self.winner, self.last_sweep, self.last = None, None, None
        if direct:
            self._still_refused()
            self.direct.setdefault(kind, set()).add(("f32:" if self.dtype != "f64" else "") + self.changed_by)
        else:
            self._unchanged()
        if kind in NEW_CALLS:
            self.calls.append({"step": self.index, "kind": kind, "kernel": kernel, "on_list": self.cand[0] == "list", "dtype": self.dtype,
                               "direct": self.changed_by if direct else None})

    def _sharp(self, kind, *figures):
        """A condition on the inputs, not on the device: the reference decides every count, witness and index by more than SHARP."""
        self.margins.append((self.index, kind, float(min(figures))))
        if not min(figures) > SHARP:
            raise RuntimeError(f"{kind}: the reference is blunt {figures}: change this seed's draw, not the bar")

    def _dev(self, kind, err):
        self.devs[kind] = max(self.devs.get(kind, 0.0), err)

    def run_new(self, kind, args):
        """The engine's call of a new step from its kept arguments: every array it returns."""
        if kind == "expander_gain":
            S, T, b, cons = args
            return self.eng.expander_gain(S, T, b, cons, return_margin=True)
        pts, o, draws, maximize = args
        return self.eng.sample_paths(pts, SP_PATHS, o, draws=draws, maximize=maximize, return_values=True)

    def ro_expander_gain(self, mask, under=""):
        """9 sources (the first the last sweep's winner, where there is one) against 257 targets in the box, b of the last sweep: count
        and witness are expander_oracle.gain_naive's on the walk's rows exactly, margin within TOL64."""
        lo, hi = self.box
        S = self.rng.uniform(lo, hi, size=(EG_SOURCES, len(lo)))
        T = self.rng.uniform(lo, hi, size=(EG_TARGETS, len(lo)))
        if self.winner is not None and len(self.winner) == len(lo):
            S[0] = self.winner
        b, q = self.last_sweep[1], self.ds["Y_norm"].shape[1]
        ref = expander_oracle.gain_naive(self.ds, b, S, T, mask)
        self._sharp("expander_gain", *expander_oracle.sharpness(ref))
        args = (S, T, b, None if mask == 0 else expander_oracle.constraints_of(q, mask))
        self.kept["expander_gain"] = (self.ds_ver, args, None)
        if self.dry:
            return
        got = self.run_new("expander_gain", args)
        self.kept["expander_gain"] = (self.ds_ver, args, got)
        assert np.array_equal(got["count"], ref["count"]), ("expander_gain count", got["count"], ref["count"])
        assert np.array_equal(got["witness"], ref["witness"]), ("expander_gain witness", got["witness"], ref["witness"])
        assert np.array_equal(got["expander"], ref["count"] > 0)
        err = float(np.max(np.abs(got["margin"] - ref["margin"])))
        self._dev("expander_gain", err)
        assert err < expander_oracle.TOL64, ("expander_gain margin", err)

    def ro_sample_paths(self, which, maximize, seed, under=""):
        """257 points in the box, 17 paths of 257 features from SweepEngine.path_draws(seed), output 0 or q - 1 (whose prior mean is not
        zero): the indices are paths_oracle.paths_solve's on the walk's rows exactly, the normalised values within TOL64."""
        lo, hi = self.box
        pts = self.rng.uniform(lo, hi, size=(SP_POINTS, len(lo)))
        n, q = self.ds["Y_norm"].shape
        o = q - 1 if which == "last" else 0
        draws = SweepEngine.path_draws(len(lo), n, SP_PATHS, SP_FEATURES, seed)
        f = paths_oracle.paths_solve(self.ds, o, draws, pts)
        self._sharp("sample_paths", paths_oracle.sharpness(f, maximize))
        args = (pts, o, draws, bool(maximize))
        self.kept["sample_paths"] = (self.ds_ver, args, None)
        if self.dry:
            return
        got = self.run_new("sample_paths", args)
        self.kept["sample_paths"] = (self.ds_ver, args, got)
        idx, _ = paths_oracle.best(f, maximize)
        assert np.array_equal(got["index"], idx), ("sample_paths index", got["index"], idx)
        assert got["value"].tobytes() == got["values"][got["index"], np.arange(SP_PATHS)].tobytes()
        err = float(np.max(np.abs((got["values"] - self.ds["Y_mean"][o]) / self.ds["Y_std"][o] - f)))
        self._dev("sample_paths", err)
        assert err < paths_oracle.TOL64, ("sample_paths values", err)

    def refuse_f64_only(self):
        """mean_grad, lipschitz and refine on an fp32 model: refused, and the masks of the sweep before are unchanged."""
        if self.dtype != "f32" or self.last_sweep is None:
            raise RuntimeError("f64_only_on_f32: needs an fp32 model and a sweep before it")
        lo, hi = self.box
        x = np.array(self.winner) if self.winner is not None and len(self.winner) == len(lo) else 0.5 * (lo + hi)
        if not self.dry:
            self._raises(lambda: self.eng.mean_grad(x[None], infnorm=True))
            self._raises(lambda: self.eng.lipschitz(lo, hi))
            self._raises(lambda: self.eng.refine(self.last_sweep[1], x, 0, "lcb", lo=lo, hi=hi))
        self._unchanged()
