"""The shape range of the refine solver's posterior gradient (csrc/refine.hip: ref_eval, shared by k_refine and k_refine_robust) --
the case table of tests/test_refine_shapes_cpu.py (the reference alone: the preconditions) and tests/test_gpu_refine_shapes.py (the
device against the reference).  Importable without a GPU.

What a case is: a model (``source``), a box, b, one refine problem in refine_sets_oracle.problem's arguments, the seeds and the
evaluation budget.  ``n`` is the size of the model itself.  The classes:

    launch   ref_eval's launch shape: 256 threads up to n = 256 and 1024 above, one wave per row of M, 64 columns per wave pass
    tier     the largest n whose packed triangles of M are staged in LDS, and the first that streams them, per slot count
    slots    more than two outputs: every constraint of a q = 4, 5, 8 fan model enforced
    dim      d = 1 and d = 8 for one point; a pair (x, x') at d = 4 (8 solver variables, the ceiling)

The models after removals (REMOVALS, WINDOW, TINY) are compared with the same dataset set afresh, not with the yardstick.
"""
import functools

import numpy as np

import many_constraints as mc
import model_remove as mr
import oracle
import refine_oracle as ro
import refine_sets_oracle as rs
import robust_refine_oracle as rr
from safebo_amd import synthetic

# ---- the host rules of csrc/refine.hip, restated -----------------------------------------------------------------------------------
LDS_M = 144 * 1024           # kRefLdsM: the staged triangles, beside the vectors of every point but the first, fit in this
POINT_BYTES = 16             # per row of the model and per point: k and u = M k, one double each
DEFAULT_EVAL, MAX_EVAL = 400, 20000      # kRefDefaultEval, kRefMaxEval
RAISED_EVAL = 4000                       # for the cases the default budget ends MAX_EVAL (tests/test_gpu_refine_sets.py's budget)
KKT_BOX, KKT_TERMS = 1e-6, 1e-4          # tests/test_gpu_refine.py's bars: box-only problems / with constraint terms


def staged(n, slots, points=1, extra=0):
    """refine_lds_bytes' rule: M's packed triangles of ``slots`` outputs are staged in LDS at n rows."""
    return 8 * slots * n * (n + 1) // 2 + (points - 1) * POINT_BYTES * n + extra <= LDS_M


def largest_staged(slots, points=1, extra=0):
    n = 1
    while staged(n + 1, slots, points, extra):
        n += 1
    return n


def threads(n):
    return 1024 if n > 256 else 256


def eval_cap(n):
    """refine_eval_cap: the ceiling of max_eval."""
    return int(min(MAX_EVAL, max(DEFAULT_EVAL, 4e9 / (float(n) * n))))


# ---- models -----------------------------------------------------------------------------------------------------------------------
def _synthetic(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, size=(n, d))
    Y = np.stack([np.sum(X ** 2, axis=1) + 0.3 * np.sin(3 * X[:, 0]), 0.8 - np.sum(np.abs(X), axis=1) / d], axis=1)
    return synthetic.make_dataset(X, Y, synthetic.default_hypopt(d, 2))


@functools.lru_cache(maxsize=None)
def _model(source):
    kind, args = source[0], source[1:]
    return _synthetic(*args) if kind == "synthetic" else mc.fan_model(*args)


def dataset(case):
    """The case's model (computed once per process, never modified)."""
    return _model(case["source"])


# ---- the case table ---------------------------------------------------------------------------------------------------------------
CASES = {}


def _add(name, cls, source, seeds, kind, maximize=False, b=2.0, box=1.0, max_eval=None, tiers=False, **prob):
    """source: ("synthetic", n, d, seed) of _synthetic or ("fan", q, d, n, seed) of many_constraints.fan_model; seeds: ("points",
    rows), ("pair", x, x'), ("grid", count): the safe grid point with the best objective, ("data", k[, skip]): observed inputs;
    prob: further arguments of refine_sets_oracle.problem (link: the constraint, its L is set from the seed)."""
    synth = source[0] == "synthetic"
    d = source[2]
    q = 2 if synth else source[1]
    n = source[1] if synth else source[3]
    CASES[name] = dict(name=name, cls=cls, source=source, d=d, q=q, n=n, lo=np.full(d, -box), hi=np.full(d, box), b=b, kind=kind,
                       maximize=maximize, prob=prob, seeds=seeds, max_eval=max_eval, tiers=tiers)


def _pts(d, *vals):
    return ("points", tuple(tuple([v] * d) if np.isscalar(v) else tuple(v) for v in vals))


# launch shape: one point, objective 0 with constraint 1 (2 slots).  lcb and ucb at b = 2 weigh the mean's and the variance's
# gradient alike; var is maximised at d = 4 only (at d = 2 and n >= 1000 the variance is ~1e-4 of Y_std^2: its gradient tests nothing)
for _n, _d in ((63, 2), (64, 4), (65, 2), (255, 4), (256, 2), (257, 4), (1023, 2), (1025, 4)):
    _seeds = _pts(_d, 0.0, 0.1) if _n < 1000 else _pts(_d, 0.1)
    for _kind in ("lcb", "ucb") + (("var",) if _d == 4 else ()):
        # (n = 1025, var: from 0.1 SLSQP's first step jumps to another local maximum on the box, 0.0751 against the 0.0643 of the
        # maximum next to the seed, where the device converges with a KKT residual of 3e-9; from 0 both climb the same one)
        _add(f"launch_n{_n}_d{_d}_{_kind}", "launch", ("synthetic", _n, _d, _n + _d), _pts(_d, 0.0) if (_n, _kind) == (1025, "var") else _seeds,
             _kind, maximize=_kind == "var")
for _kind in ("lcb", "var"):
    _add(f"launch_n2048_d4_{_kind}", "launch", ("synthetic", 2048, 4, 2052), _pts(4, 0.1), _kind, maximize=_kind == "var",
         max_eval=eval_cap(2048))

# tier boundary: the largest staged n and the first streamed n of every slot count, under both values of option refine_lds
N1, N2, N3, N8, NP2 = (largest_staged(1), largest_staged(2), largest_staged(3), largest_staged(8), largest_staged(2, 2))
for _n in (N1, N1 + 1):
    _add(f"tier_1slot_n{_n}", "tier", ("synthetic", _n, 2, 7 * _n + 2), _pts(2, 0.1, 0.3), "lcb", safe=(), tiers=True)
for _n in (N2, N2 + 1):
    _add(f"tier_2slot_n{_n}", "tier", ("synthetic", _n, 2, 7 * _n + 2), _pts(2, 0.0, 0.1, -0.2), "lcb", tiers=True)
for _n in (N3, N3 + 1):
    _add(f"tier_3slot_n{_n}", "tier", ("fan", 3, 4, _n, 0), ("grid", (7, 6, 5, 5)), "lcb", b=mc.B, box=1.2, tiers=True)
for _n in (N8, N8 + 1):
    _add(f"tier_8slot_n{_n}", "tier", ("fan", 8, 2, _n, 3), ("grid", (40, 36)), "lcb", b=mc.B, box=1.2, tiers=True)
for _n in (NP2, NP2 + 1):
    _add(f"tier_pair_n{_n}", "tier", ("synthetic", _n, 2, 7 * _n + 2), ("pair", (0.2, -0.1), (0.95, 0.9)), "var", maximize=True,
         pair=True, link=1, tiers=True)

# slots: every constraint of a q = 4, 5, 8 fan enforced, at n = 40 and at one n > 256; the seed is the safe grid point with the best
# objective.  (q, d, n, data seed, grid) per objective.  The data seeds are those
#   - at which the yardstick moves off that grid point: on others -- q = 4 and 5 at n = 40 with data seed 0 for lcb, q = 5 at d = 3,
#     n = 257 with data seeds 0 to 3 for var -- the winner is a corner of the box SLSQP leaves in place with no term active;
#   - at which SLSQP and a local ascent from the seed climb the same maximum (q = 4, d = 3, n = 300, var: not with data seed 0);
#   - on which the solver's twin on the reference gradients (refine_solver_twin.py) converges within RAISED_EVAL: with data seed 0
#     the lcb cases of q = 4 (d = 3, n = 300) and q = 5 (d = 3, n = 257) and the var case of q = 8 (d = 4, n = 260) end with one face
#     and one constraint active, where twin and device stall alike (tests/test_refine_shapes_cpu.py asserts the twin's end)
_G2, _G3, _G4 = (40, 36), (13, 11, 10), (7, 6, 5, 5)
for _kind, _rows in (("lcb", ((4, 2, 40, 1, _G2), (5, 2, 40, 3, _G2), (8, 2, 40, 3, _G2), (4, 3, 300, 1, _G3), (5, 3, 257, 4, _G3),
                              (8, 4, 260, 0, _G4))),
                     ("var", ((4, 2, 40, 0, _G2), (5, 2, 40, 0, _G2), (8, 2, 40, 3, _G2), (4, 3, 300, 2, _G3), (5, 2, 257, 4, _G2),
                              (8, 3, 260, 4, _G3)))):
    for _q, _d, _n, _seed, _count in _rows:
        _add(f"slots_q{_q}_d{_d}_n{_n}_{_kind}", "slots", ("fan", _q, _d, _n, _seed), ("grid", _count), _kind, maximize=_kind == "var",
             b=mc.B, box=1.2, max_eval=RAISED_EVAL)

# dimension: d = 1 and d = 8 for one point; a pair at d = 4 with a link and an unsafe term (refine_sets_oracle.grid_case's "G").  No
# pair launch stages M above n = NP2 = 134, so the pair runs once above 256 rows (1024 threads, streamed) and once staged
_add("dim_d1_n30_lcb", "dim", ("synthetic", 30, 1, 31), _pts(1, 0.0, 0.2), "lcb")
_add("dim_d1_n30_ucb", "dim", ("synthetic", 30, 1, 31), _pts(1, 0.0, 0.2), "ucb")
# (in eight dimensions 200 rows leave the centre of the box unsafe: the seeds are the two observed inputs with the largest lcb_1)
# (var: from the first of them SLSQP ends on another local maximum than a local ascent, so the second and the third)
_add("dim_d8_n200_lcb", "dim", ("synthetic", 200, 8, 208), ("data", 2), "lcb")
_add("dim_d8_n200_var", "dim", ("synthetic", 200, 8, 208), ("data", 2, 1), "var", maximize=True, max_eval=RAISED_EVAL)
_add("dim_pair_d4_n300", "dim", ("synthetic", 300, 4, 304), ("pair", (0.2, -0.1, 0.1, 0.0), (0.95, 0.9, -0.95, 0.9)), "var",
     maximize=True, pair=True, link=1)
_add("dim_pair_d4_n120", "dim", ("synthetic", 120, 4, 124), ("pair", (0.2, -0.1, 0.1, 0.0), (0.95, 0.9, -0.95, 0.9)), "var",
     maximize=True, pair=True, link=1, tiers=True, max_eval=RAISED_EVAL)


def slots(case):
    """Distinct outputs a case's launch evaluates (RefineArgs.nu)."""
    P = problem(case)
    outs = {P["objective"]} | set(P["safe"]) | set(P["unsafe"])
    if P["link"] is not None:
        outs.add(P["link"][0])
    return len(outs)


@functools.lru_cache(maxsize=None)
def _grid_seed(name):
    """The safe grid point with the best objective on the case's box: the seed a host class would hand over."""
    case = CASES[name]
    ds, b = dataset(case), case["b"]
    pts = oracle.grid_points(case["lo"], case["hi"], list(case["seeds"][1]))
    m, v = oracle.gp_inference(pts, ds)
    sd = np.sqrt(v)
    safe = np.all(m[:, 1:] - b * sd[:, 1:] >= 0, axis=1)
    f = {"lcb": m[:, 0] - b * sd[:, 0], "ucb": m[:, 0] + b * sd[:, 0], "mean": m[:, 0], "var": v[:, 0]}[case["kind"]]
    sg = -1.0 if case["maximize"] else 1.0
    assert safe.any(), name
    return pts[int(np.argmin(np.where(safe, sg * f, np.inf)))][None, :].copy()


@functools.lru_cache(maxsize=None)
def _data_seeds(name):
    """The observed inputs with the largest lcb of constraint 1."""
    case = CASES[name]
    ds = dataset(case)
    X = ds["X_norm"] * ds["X_std"] + ds["X_mean"]
    m, v = oracle.gp_inference(X, ds)
    order = np.argsort(-(m[:, 1] - case["b"] * np.sqrt(v[:, 1])), kind="stable")
    k, skip = case["seeds"][1], case["seeds"][2] if len(case["seeds"]) > 2 else 0
    return X[order[skip:skip + k]].copy()


@functools.lru_cache(maxsize=None)
def _problem(name):
    case = CASES[name]
    ds, b, prob = dataset(case), case["b"], dict(case["prob"])
    if prob.get("link") is not None:
        # a caller's L that leaves the link a quarter of ucb_c at the seed (tests/test_gpu_refine_sets.py: _cases)
        c = prob["link"]
        x, xp = np.array(case["seeds"][1]), np.array(case["seeds"][2])
        prob["link"] = (c, float(0.75 * ro.bound_grad(x, ds, b, c, "ucb")[0] / rs.shifted(x, xp)[0]))
    if "safe" in prob:
        prob["safe"] = list(prob["safe"])
    return rs.problem(ds, b, case["lo"], case["hi"], case["kind"], maximize=case["maximize"], **prob)


def problem(case):
    return _problem(case["name"])


def seeds(case):
    """[S, nz] seeds of a case (pair: x then x')."""
    how = case["seeds"]
    if how[0] == "points":
        return np.array(how[1], dtype=np.float64)
    if how[0] == "pair":
        return np.concatenate([how[1], how[2]])[None, :].astype(np.float64)
    if how[0] == "data":
        return _data_seeds(case["name"])
    return _grid_seed(case["name"])


def kkt_bar(case):
    P = problem(case)
    return KKT_TERMS if (P["safe"] or P["unsafe"] or P["link"] is not None or P["level"] is not None) else KKT_BOX


@functools.lru_cache(maxsize=None)
def _yardstick(name):
    case = CASES[name]
    P = problem(case)
    out = []
    for s in seeds(case):
        z, res = rs.slsqp(P, s)
        z = rs.make_feasible(P, z, s)
        out.append({"seed_value": rs.value(P, s), "value": rs.value(P, z), "z": z, "kkt": rs.kkt_residual(P, z), "nit": int(res.nit)})
    return tuple(out)


def yardstick(case):
    """Per seed: SLSQP from the seed, made feasible (refine_sets_oracle.yardstick) -- its value, point, KKT residual and iterations.
    Computed once per process and never modified."""
    return _yardstick(case["name"])


def gradient_shares(P, z):
    """(||grad mean||_inf, ||b grad var / (2 sd)||_inf, ||grad objective||_inf, var / Y_std^2) of the objective's output at its point."""
    x, xp = rs.split(P, z)
    pt = xp if P["at"] == "xp" else x
    o = P["objective"]
    m, v, gm, gv = ro.posterior_grad(pt, P["ds"])
    sd = np.sqrt(v[o])
    gvar = P["b"] * gv[o] / (2.0 * sd)
    gobj = rs.objective(P, z)[1]
    return float(np.max(np.abs(gm[o]))), float(np.max(np.abs(gvar))), float(np.max(np.abs(gobj))), float(v[o] / P["ds"]["Y_std"][o] ** 2)


# ---- models that lost rows ----------------------------------------------------------------------------------------------------------
def removal_order(n0, k):
    """k indices to remove one after the other from a model of n0 rows: first, middle, last, in turn (each in the numbering of the
    model at that moment)."""
    out, n = [], n0
    for i in range(k):
        out.append((0, n // 2, n - 1)[i % 3])
        n -= 1
    return out


def after_removals(ds, order):
    """The oracle's dataset after the removals: frozen constants, the inverse rebuilt from the remaining rows."""
    for j in order:
        ds = mr.without(ds, j)
    return ds


REMOVE_K = 6                                       # 140 -> 134: below the switch of two slots (135) and of a pair (134)
REMOVALS = (20, 140, 300)                          # n0


def removal_problems(ds, n0):
    """(label, problem, seed z) of the refine and refine_sets calls after removals, on the dataset ``ds`` the calls see."""
    lo, hi = -np.ones(2), np.ones(2)
    x, xp = np.array([0.05, -0.1]), np.array([0.95, 0.9])
    L = float(0.75 * ro.bound_grad(x, ds, 2.0, 1, "ucb")[0] / rs.shifted(x, xp)[0])
    return [("refine", rs.problem(ds, 2.0, lo, hi, "lcb"), x.copy()),
            ("pair", rs.problem(ds, 2.0, lo, hi, "var", maximize=True, link=(1, L), pair=True), np.concatenate([x, xp]))]


def robust_case(n0):
    """robust_refine_oracle's model of d2_q2 / n150 at n0 rows: what build_case returns, without ``ds`` and ``rows``.  (Model seed and
    constraint shift at n0 = 20 are those that leave the 14 remaining rows a robust-safe control strictly inside the control box.)"""
    seed, shift = (1, 1.5) if n0 < 100 else (7, 0.3)
    ds0, lo, hi = rr.make_model(2, 2, n0, seed, shift=(0.0, shift))
    return {"ds0": ds0, "lo": lo, "hi": hi, "nxc": 1, "count": [9, 7], "count_d": [7], "q": 2, "mp": np.zeros(2)}


# ---- the sliding window and the smallest models ---------------------------------------------------------------------------------------
WINDOW = (20, 140)                                 # n0: remove row 0, append one row, five times
WINDOW_STEPS = 5


def window_model(n0):
    """(ds0 to set, normalised rows to append [steps, d] / [steps, q], the oracle's dataset after the window has moved)."""
    full = _synthetic(n0 + WINDOW_STEPS, 2, 5)
    X = full["X_norm"] * full["X_std"] + full["X_mean"]
    Y = full["Y_norm"] * full["Y_std"] + full["Y_mean"]
    ds0 = synthetic.make_dataset(X[:n0], Y[:n0], full["hypopt"])
    Xn, Yn = (X - ds0["X_mean"]) / ds0["X_std"], (Y - ds0["Y_mean"]) / ds0["Y_std"]
    return ds0, Xn[n0:], Yn[n0:], mr.with_rows(ds0, Xn[WINDOW_STEPS:], Yn[WINDOW_STEPS:])


TINY_PARENT = (4, 2, 6)                            # _synthetic's arguments: four rows, reachable sizes 2 and 1 by removals only
TINY_ORDER = {2: (0, 2), 1: (0, 2, 0)}


def tiny_model(n):
    """(the 4-row parent, the removals, the oracle's dataset of the n rows left, the seeds: the rows left and the origin)."""
    ds0 = _synthetic(*TINY_PARENT)
    ds = after_removals(ds0, TINY_ORDER[n])
    X = ds["X_norm"] * ds["X_std"] + ds["X_mean"]
    return ds0, TINY_ORDER[n], ds, np.vstack([X, np.zeros((1, 2))])
