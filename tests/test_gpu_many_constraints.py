"""Sweeps with three to seven constraints (q = 4, 5, 8 = SBO_MAX_Q) on every set-phase path (run with -m gpu on an MI355X): the
device against the NumPy oracle on the fan-of-half-planes models of tests/many_constraints.py, whose preconditions (no empty
input, every constraint at work, both lanes twice, winners of the tie rules beyond constraint 1, margins far above rounding)
tests/test_many_constraints_cpu.py checks without a GPU.  Masks, counts and indices are bit-exact; the posterior is within 1e-10
in normalised units; floats that come out of reductions (u*, L, std, lcb) within the suite's 1e-9."""
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import many_constraints as mc
import oracle
import robust_oracle
import safebo_amd
from safebo_amd import GoOSE, SafeOpt, _lib
from test_gpu_parity import _free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL64 = 1e-10
B = mc.B
DEFAULTS = {"posterior_path": 0, "bilinear": 1, "tensor_cheb": 1, "fuse_classify": -1, "set_fuse": 1, "set_lanes": 1, "result_mirror": 1,
            "scan_waves": 1, "list_index": -1, "guard_band": 1}


@contextlib.contextmanager
def options(engine, **kv):
    """Engine options for the block, every one restored to its default afterwards."""
    try:
        for k, v in kv.items():
            engine.set_option(k, v)
        yield
    finally:
        for k in kv:
            engine.set_option(k, DEFAULTS[k])


def bundle(engine, ds, quirk, dtype="f64", lean=0, fresh=False):
    """SafeOpt on a fresh posterior of the resident candidates (the posterior kernel runs inside the sweep), then GoOSE, the
    explore step for a caller's target and the trust-region sweep -- on that resident posterior, or (``fresh``, fp32, lean) each
    on a posterior of its own: results, masks, the kernel that ran and the set path."""
    q, d = ds["Y_norm"].shape[1], ds["X_norm"].shape[1]
    f64 = dtype == "f64"
    ready = f64 and not lean and not fresh

    def renew():
        engine.set_model(ds, dtype=dtype, use_invK=f64)
    renew()
    s = engine.sweep_safeopt(B, quirk_L_index=quirk, want_masks=True, lean=lean)
    prof = engine.profile()
    out = {"s": s, "kernel": prof["posterior_kernel"], "set_path": prof["set_path"], "prof": prof, "q": q}
    m = {k: engine.mask(k) for k in ("S", "U", "M")}
    m.update({f"G{c}": engine.mask("G", c) for c in range(1, q)})
    if ready:
        out["mean"], out["var"] = engine.posterior()
    if fresh:
        renew()
    out["g"] = engine.sweep_goose(B, quirk_L_index=quirk, want_masks=True, posterior_ready=ready)
    m.update({f"O{c}": engine.mask("O", c) for c in range(1, q)})
    m["S_g"], m["U_g"] = engine.mask("S"), engine.mask("U")
    out["e"], out["ex"] = engine.explore_safeset(mc.EXPLORE_TARGET[d])
    if fresh:
        renew()
    out["t"] = engine.sweep_tr(B, mc.TR_BALL[d][0], mc.TR_BALL[d][1], posterior_ready=ready)
    m["T"] = engine.mask("M")
    out["masks"] = m
    return out


def _close(got, want, scale=1.0):
    return abs(got - want) <= 1e-9 * max(1.0, abs(want), scale)


def check_oracle(bn, ref, pts, ds, what=""):
    """Every mask, count, index and choice of a bundle against the oracle's SafeOpt / GoOSE / trust-region results."""
    sref, gref, tref = ref
    m, q, s, g, t = bn["masks"], bn["q"], bn["s"], bn["g"], bn["t"]
    d = pts.shape[1]
    if "mean" in bn:
        ys = np.maximum(1.0, ds["Y_std"])
        em, ev = np.max(np.abs(bn["mean"] - sref["mean"]) / ys), np.max(np.abs(bn["var"] - sref["var"]) / ys ** 2)
        assert em < TOL64 and ev < TOL64, (what, em, ev)
    for k in ("S", "U", "M"):
        assert np.array_equal(m[k], sref[k]), (what, k, int(np.sum(m[k] != sref[k])))
    assert np.array_equal(m["S_g"], gref["S"]) and np.array_equal(m["U_g"], gref["U"]), what
    for c in range(1, q):
        assert np.array_equal(m[f"G{c}"], sref["G"][c - 1]), (what, f"G{c}", int(np.sum(m[f"G{c}"] != sref["G"][c - 1])))
        assert np.array_equal(m[f"O{c}"], gref["O"][c - 1]), (what, f"O{c}", int(np.sum(m[f"O{c}"] != gref["O"][c - 1])))
    assert np.array_equal(m["T"], tref["T"]), what
    # SafeOpt
    assert (s["count_S"], s["count_U"], s["count_M"]) == (sref["S"].sum(), sref["U"].sum(), sref["M"].sum()), what
    assert list(s["count_G"]) == sref["G"].sum(axis=1).tolist(), what
    assert _close(s["u_star"], sref["u_star"]), what
    assert np.allclose(s["L"], sref["L"], rtol=1e-9, atol=0.0), (what, s["L"], sref["L"])       # (never a lean bundle: L[0] too)
    assert s["minimizer_index"] == sref["minimizer_index"] and np.array_equal(s["minimizer_x"], pts[sref["minimizer_index"]]), what
    assert s["minimizer_std"] == pytest.approx(sref["minimizer_std"], rel=1e-9), what
    assert list(s["expander_index_c"]) == list(sref["expander_index"]), (what, s["expander_index_c"], sref["expander_index"])
    assert np.allclose(s["expander_std_c"], sref["expander_std"], rtol=1e-9, atol=0.0), what
    assert s["expander_best_c"] == sref["expander_best"] and s["expander_index"] == sref["expander_best_index"], what
    assert s["expander_best_c"] >= 1 and np.array_equal(s["expander_x"], pts[sref["expander_best_index"]]), what
    assert s["expander_std"] == pytest.approx(sref["expander_best_std"], rel=1e-9), what
    assert s["choose_minimizer"] == sref["choose_minimizer"], what
    # GoOSE
    assert (g["count_S"], g["count_U"]) == (gref["S"].sum(), gref["U"].sum()) and list(g["count_O"]) == gref["O"].sum(axis=1).tolist(), what
    assert g["safe_min_index"] == gref["safe_min_index"] and _close(g["safe_min_lcb"], gref["safe_min_lcb"]), what
    assert np.array_equal(g["safe_min_x"], pts[gref["safe_min_index"]]), what
    assert list(g["target_index_c"]) == list(gref["target_index_c"]), (what, g["target_index_c"], gref["target_index_c"])
    for c in range(q - 1):
        if gref["target_index_c"][c] >= 0:
            assert _close(g["target_lcb_c"][c], gref["target_lcb_c"][c]), (what, c)
        else:
            assert g["target_lcb_c"][c] == np.inf, (what, c)
    assert g["target_best_c"] == gref["target_best"] and g["target_index"] == gref["target_index"], what
    assert g["explore_index"] == gref["explore_index"] and g["choose_safe_min"] == gref["choose_safe_min"], what
    assert g["target_best_c"] >= 1 and _close(g["target_lcb"], gref["target_lcb"]), what
    assert np.array_equal(g["target_x"], pts[gref["target_index"]]) and np.array_equal(g["explore_x"], pts[gref["explore_index"]]), what
    assert np.allclose(g["L"], sref["L"], rtol=1e-9, atol=0.0), what
    assert bn["e"] == mc.explore_reference(pts, gref["S"], mc.EXPLORE_TARGET[d]), what
    assert np.array_equal(bn["ex"], pts[bn["e"]]), what
    # trust region
    assert (t["index"], t["count_S"], t["count_T"]) == (tref["index"], tref["S"].sum(), tref["T"].sum()), what
    assert _close(t["lcb"], tref["lcb_min"]) and np.array_equal(t["x"], pts[tref["index"]]), what


_INT_KEYS = {"s": ("minimizer_index", "minimizer_x", "expander_index_c", "expander_best_c", "expander_index", "expander_x", "choose_minimizer",
                   "count_S", "count_U", "count_M", "count_G"),
             "g": ("safe_min_index", "safe_min_x", "target_index_c", "target_best_c", "target_index", "target_x", "explore_index", "explore_x",
                   "choose_safe_min", "count_S", "count_U", "count_O"),
             "t": ("index", "x", "count_S", "count_T")}


def same_decisions(a, b_, what=""):
    """Every mask, count, index and choice equal (bundles whose floats come from different posterior kernels)."""
    for k, v in a["masks"].items():
        assert np.array_equal(v, b_["masks"][k]), (what, k, int(np.sum(v != b_["masks"][k])))
    for part, keys in _INT_KEYS.items():
        for k in keys:
            assert np.array_equal(np.asarray(a[part][k]), np.asarray(b_[part][k])), (what, part, k, a[part][k], b_[part][k])
    assert a["e"] == b_["e"], what


def same_bundle(a, b_, what="", lean=False):
    """Identical: every mask and every field of every result, floats bitwise (one posterior kernel, work launched differently)."""
    for k, v in a["masks"].items():
        assert np.array_equal(v, b_["masks"][k]), (what, k, int(np.sum(v != b_["masks"][k])))
    for part in ("s", "g", "t"):
        for k, v in a[part].items():
            w = b_[part][k]
            if lean and part == "s" and k == "L":
                assert w[0] == 0.0 and np.array_equal(v[1:], w[1:]), (what, v, w)
                continue
            assert np.array_equal(np.asarray(v), np.asarray(w)), (what, part, k, v, w)
    assert a["e"] == b_["e"], what


def check_tails(engine, quirk, q):
    """The per-constraint arrays of the raw result structs past entry q - 2 (include/safebo.h): indices -1, everything else 0."""
    lib = engine._lib
    opts = _lib.SweepOpts(B, int(quirk), 0, 1, 0)
    s, g = _lib.SafeOptResult(), _lib.GooseResult()
    _lib.check(lib.sbo_sweep_safeopt(engine._ctx, C.byref(opts), C.byref(s)))
    _lib.check(lib.sbo_sweep_goose(engine._ctx, C.byref(opts), C.byref(g)))
    assert list(s.expander_index_c[q - 1:]) == [-1] * (9 - q) and list(g.target_index_c[q - 1:]) == [-1] * (9 - q)
    for arr in (s.expander_std_c, s.count_G, g.target_lcb_c, g.count_O):
        assert list(arr[q - 1:]) == [0] * (9 - q)
    assert list(s.L[q:]) == [0.0] * (8 - q) and list(g.L[q:]) == [0.0] * (8 - q)
    assert all(x >= 0 or x == -1 for x in s.expander_index_c[:q - 1])


# --------------------------------------------------------------------------------------------- (a) every posterior path
# path -> (case suffix, options, kernel, candidates as an explicit list)
PATHS = {
    "generic": ("", {"posterior_path": 1}, 1, False),
    "chunked": ("", {"posterior_path": 2}, 2, False),
    "table": ("", {"bilinear": 0, "tensor_cheb": 0}, 3, False),
    "k1i": ("_gemm", {"bilinear": 1}, 6, False),
    "k1b": ("_gemm", {"bilinear": 2}, 4, False),
    "exact3d": ("_3d", {}, 3, False),
    "list": ("", {"list_index": 0}, 1, True),
    "list_index": ("", {"list_index": 1}, 1, True),
}


@pytest.mark.parametrize("path,q", [(p, q) for p in PATHS for q in (4, 5, 8)] + [("table_perm", 5), ("table_perm", 8)])
def test_sweeps_against_the_oracle_on_every_posterior_path(engine, path, q):
    """SafeOpt, GoOSE (+ explore_safeset with a caller's target) and trust-region sweeps of a model with q - 1 constraints, both
    values of reference_quirk_L_index, against the oracle: generic and chunked generic kernel, separable-table kernel (also with
    permuted constraint columns: expander_best_c / target_best_c beyond constraint 1), K1i (a model's first sweep with the
    caller's invK), K1b, a 3-D grid, and an explicit list with the exhaustive expander and with the spatial index."""
    if path == "table_perm":
        suffix, opts, kernel, as_list = ("_perm",) + PATHS["table"][1:]
    else:
        suffix, opts, kernel, as_list = PATHS[path]
    name = f"q{q}{suffix}"
    k = mc.CASES[name]
    ds, pts = mc.model(name), mc.points(name)
    lo, hi = mc.box(k["d"])
    with options(engine, **opts):
        if as_list:
            engine.set_points(pts)
        else:
            engine.set_grid(lo, hi, k["count"])
        for quirk in (True, False):
            bn = bundle(engine, ds, quirk)
            assert bn["kernel"] == kernel and bn["set_path"] == 0, (path, q, bn["kernel"], bn["set_path"])
            check_oracle(bn, mc.reference(name, quirk), pts, ds, what=(path, q, quirk))
            if as_list and opts["list_index"] == 0:
                # (the exhaustive expander: every safe candidate re-decided for every constraint)
                assert bn["s"]["n_exact_rechecks"] == (q - 1) * mc.reference(name, quirk)[0]["S"].sum()
            if as_list and opts["list_index"] == 1:
                assert bn["prof"]["list_index_leaf_pairs"] + bn["prof"]["list_index_nodes_skipped"] > 0    # (the index was walked)
            check_tails(engine, quirk, q)
    print(f"[many-constraints] path {path} q {q}: posterior_kernel {kernel}")


@pytest.mark.parametrize("q", [5, 8])
def test_tensor_interpolation_and_its_forced_guard_band_equal_the_exact_kernel(engine, q):
    """K1t (three axes, 4.3 M candidates: no brute-force oracle): every decision of the SafeOpt, GoOSE and trust-region sweeps equals
    the exact grid kernel's, with the forced re-evaluation (guard_band 2, q = 5) too; a sample of the posterior is the oracle's."""
    d, count = 3, [160, 168, 160]
    ds = mc.model(f"q{q}_3d")
    lo, hi = mc.box(d)
    out = {}
    variants = [("exact", {"tensor_cheb": 0}), ("k1t", {})] + ([("forced", {"guard_band": 2})] if q == 5 else [])
    for key, opts in variants:
        with options(engine, **opts):
            engine.set_grid(lo, hi, count)
            out[key] = bundle(engine, ds, True)
    assert out["exact"]["kernel"] == 3 and out["k1t"]["kernel"] == 5
    m = out["exact"]["masks"]
    assert all(m[f"G{c}"].any() and m[f"O{c}"].any() for c in range(1, q)) and m["M"].any() and 0 < m["T"].sum() < m["S"].sum()
    same_decisions(out["k1t"], out["exact"], "k1t")
    if q == 5:
        assert out["forced"]["kernel"] == 5 and all(out["forced"][p]["guard_passes"] >= 1 for p in ("s", "g", "t"))
        same_decisions(out["forced"], out["exact"], "forced")
    ys = np.maximum(1.0, ds["Y_std"])
    assert np.max(np.abs(out["k1t"]["mean"] - out["exact"]["mean"]) / ys) < TOL64
    assert np.max(np.abs(out["k1t"]["var"] - out["exact"]["var"]) / ys ** 2) < TOL64
    total = int(np.prod(count))
    idx = np.unique(np.concatenate([np.random.default_rng(3).integers(0, total, size=2000), [0, total - 1]]))
    sub = oracle.grid_points(lo, hi, count)[idx]
    om, ov = oracle.gp_inference(sub, ds)
    assert np.max(np.abs(out["k1t"]["mean"][idx] - om) / ys) < TOL64 and np.max(np.abs(out["k1t"]["var"][idx] - ov) / ys ** 2) < TOL64


# --------------------------------------------------------------------------------------------- (b) lanes
@pytest.mark.parametrize("q", [4, 5, 8])
def test_two_lanes_equal_one_lane_when_a_lane_runs_several_constraints(engine, q):
    """q = 4: lane 0 runs constraints 1 and 3 on one scratch, lane 1 constraint 2; q = 5: both lanes twice; q = 8: four and three.
    A sequence of candidate sets of changing size (small grid, list, large grid, list, small grid, all of it twice) with
    set_lanes 1 and 0: every mask and every result field bitwise equal, and the small steps equal to the oracle -- so a lane's
    second constraint that saw what its first left behind cannot hide behind "both wrong the same way"."""
    name = f"q{q}"
    ds = mc.model(name)
    lo, hi = mc.box(2)
    rng = np.random.default_rng(11)
    lists = [rng.uniform(lo, hi, size=(m, 2)) for m in (3000, 700)]
    steps = [("grid", mc.CASES[name]["count"]), ("list", 0), ("grid", [264, 256]), ("list", 1), ("grid", mc.CASES[name]["count"])] * 2
    out = {}
    for lanes in (1, 0):
        with options(engine, set_lanes=lanes):
            rows = []
            for kind, arg in steps:
                if kind == "grid":
                    engine.set_grid(lo, hi, arg)
                else:
                    engine.set_points(lists[arg])
                rows.append(bundle(engine, ds, True))
            out[lanes] = rows
    for i, (a, b_) in enumerate(zip(out[1], out[0])):
        same_bundle(a, b_, what=(q, i, steps[i]))
    small = (oracle.safeopt_sweep(lists[1], ds, B), oracle.goose_sweep(lists[1], ds, B),
             oracle.tr_sweep(lists[1], ds, B, *mc.TR_BALL[2]))
    assert small[0]["G"].any(axis=1).sum() >= q - 2 and small[1]["O"].any(axis=1).sum() >= q - 2
    for i, (kind, arg) in enumerate(steps):
        if kind == "grid" and arg != [264, 256]:
            check_oracle(out[1][i], mc.reference(name, True), mc.points(name), ds, what=(q, i, "grid"))
        elif kind == "list" and arg == 1:
            check_oracle(out[1][i], small, lists[1], ds, what=(q, i, "list"))
    big = out[1][2]["masks"]
    assert sum(big[f"G{c}"].any() and big[f"O{c}"].any() for c in range(1, q)) >= q - 2


# --------------------------------------------------------------------------------------------- (c) launch switches
SWITCHES = {"fuse_classify": ({"fuse_classify": 0}, {"fuse_classify": 1}), "set_fuse": ({"set_fuse": 0},), "scan_waves": ({"scan_waves": 0},),
            "result_mirror": ({"result_mirror": 0},), "lean": ({"lean": 1}, {"lean": 2})}


@pytest.mark.parametrize("q", [5, 8])
@pytest.mark.parametrize("count", [[72, 70], [264, 256]])
@pytest.mark.parametrize("switch", list(SWITCHES))
def test_launch_switches_do_not_change_a_many_constraint_sweep(engine, switch, count, q):
    """Options that only change how the work is launched, on K1b with every sweep on a posterior of its own (the fused
    classification over q - 1 planes runs inside each): fuse_classify 0 / 1 (k_classify_and over the planes), set_fuse, scan_waves,
    result_mirror (GoOSE's short tail against k_sweep_finals + k_pick_target) and lean 0 / 1 / 2.  The bundles must be identical
    to the default one's (lean: apart from L[0] = 0), and on the 72 x 70 grid the default one is the oracle's."""
    ds = mc.model(f"q{q}_gemm")
    lo, hi = mc.box(2)
    engine.set_grid(lo, hi, count)
    with options(engine, bilinear=2):
        base = bundle(engine, ds, True, fresh=True)
        assert base["kernel"] == 4 and base["set_path"] == 0
        for variant in SWITCHES[switch]:
            lean = variant.get("lean", 0)
            with options(engine, **{k: v for k, v in variant.items() if k != "lean"}):
                bn = bundle(engine, ds, True, lean=lean, fresh=True)
            assert bn["kernel"] == 4 and bn["set_path"] == 0, (variant, bn["kernel"], bn["set_path"])
            same_bundle(base, bn, what=(variant, count, q), lean=bool(lean))
    m = base["masks"]
    assert sum(m[f"G{c}"].any() and m[f"O{c}"].any() for c in range(1, q)) >= q - 2
    if count == [72, 70]:
        check_oracle(base, mc.reference(f"q{q}_gemm", True), mc.points(f"q{q}_gemm"), ds, what=(switch, q))


# --------------------------------------------------------------------------------------------- (d) guard band
@pytest.mark.parametrize("mode,kernel", [(2, 4), (1, 6)])
def test_forced_guard_reevaluation_with_four_constraints_equals_the_exact_kernel(engine, mode, kernel):
    """guard_band 2 on the GEMM posteriors at q = 5: the re-evaluation of every output's band, the exact Lipschitz keys and the second
    set phase must give the exact kernel's decisions -- and the oracle's."""
    name = "q5_gemm"
    ds, pts = mc.model(name), mc.points(name)
    lo, hi = mc.box(2)
    engine.set_grid(lo, hi, mc.CASES[name]["count"])
    with options(engine, bilinear=0):
        exact = bundle(engine, ds, True)
    with options(engine, bilinear=mode, guard_band=2):
        forced = bundle(engine, ds, True, fresh=True)
    assert exact["kernel"] == 3 and forced["kernel"] == kernel
    assert all(forced[p]["guard_passes"] >= 1 for p in ("s", "g", "t"))
    same_decisions(forced, exact, "forced")
    check_oracle(forced, mc.reference(name, True), pts, ds, what="forced")


# --------------------------------------------------------------------------------------------- (e) fp32
@pytest.mark.parametrize("as_list", [False, True])
def test_fp32_sweeps_with_four_constraints_equal_the_fp64_oracle(engine, as_list):
    """dtype f32 with the fp64 recheck at q = 5, on a grid and on an explicit list: the recheck bands of every output
    (rc_band.dm[kMaxQ]) and the re-evaluation must leave SafeOpt, GoOSE and trust-region results that are the fp64 oracle's bit
    for bit; the band the sweep used is non-zero for every output of the model and zero beyond."""
    name, q = "q5", 5
    ds, pts = mc.model(name), mc.points(name)
    lo, hi = mc.box(2)
    for quirk in (True, False):
        if as_list:
            engine.set_points(pts)
        else:
            engine.set_grid(lo, hi, mc.CASES[name]["count"])
        bn = bundle(engine, ds, quirk, dtype="f32")
        prof = engine.profile()
        assert bn["prof"]["fp64_rechecks"] > 0
        check_oracle(bn, mc.reference(name, quirk), pts, ds, what=("f32", as_list, quirk))
        for key in ("fp32_band_dm", "fp32_band_dv"):
            for p in (bn["prof"], prof):
                assert all(v > 0 for v in p[key][:q]) and all(v == 0 for v in p[key][q:]), (key, p[key])
    mean, _ = engine.posterior()
    assert mean.dtype == np.float32


# --------------------------------------------------------------------------------------------- (f) ranks
def _run_ranks(tmp_path, world, cfg_name, n, count, b, timeout=150):
    """The rank workers, each under its own time limit; their exit status is checked before anything else runs."""
    port, out = _free_port(), str(tmp_path / "res.json")
    worker = os.path.join(HERE, "_gpu_rank_worker.py")
    procs = [subprocess.Popen(["timeout", "-k", "10", str(timeout), sys.executable, worker, str(r), str(world), port, out, cfg_name, str(n),
                               json.dumps(count), json.dumps(b)]) for r in range(world)]
    try:
        codes = [p.wait(timeout=timeout + 30) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert codes == [0] * world, codes
    return out, [np.load(out + f".rank{r}.npz") for r in range(world)]


@pytest.mark.parametrize("world,q", [(2, 5), (3, 5), (2, 8), (3, 8)])
def test_multi_rank_sweeps_with_many_constraints_match_the_oracle(tmp_path, world, q):
    """2 and 3 ranks on the one GPU, 37 lines (uneven shards): halo_guess[c], the 1 + kMaxQ + c layout of the exchanged keys and
    the merged arg slots for every constraint -- the stitched masks and rank 0's results are the oracle's."""
    name = f"q{q}_ranks"
    k = mc.CASES[name]
    out, parts = _run_ranks(tmp_path, world, f"mc:{q}", k["n"], k["count"], B)
    res = json.load(open(out))
    sref, gref, _ = mc.reference(name, True)
    assert int(parts[0]["first"]) == 0 and len({int(p["n_local"]) for p in parts}) > 1
    for r in range(1, world):
        assert int(parts[r]["first"]) == int(parts[r - 1]["first"]) + int(parts[r - 1]["n_local"])
    for key in ("S", "U", "M"):
        assert np.array_equal(np.concatenate([p[key] for p in parts]), sref[key]), key
    for c in range(1, q):
        assert np.array_equal(np.concatenate([p[f"G{c}"] for p in parts]), sref["G"][c - 1]), f"G{c}"
        assert np.array_equal(np.concatenate([p[f"O{c}"] for p in parts]), gref["O"][c - 1]), f"O{c}"
    assert res["minimizer_index"] == sref["minimizer_index"] and res["expander_index_c"] == [int(x) for x in sref["expander_index"]]
    assert res["expander_best_c"] == sref["expander_best"] and res["expander_index"] == sref["expander_best_index"]
    assert res["choose_minimizer"] == sref["choose_minimizer"]
    assert np.allclose(res["expander_std_c"], sref["expander_std"], rtol=1e-9, atol=0.0)
    pts = mc.points(name)
    assert np.array_equal(res["minimizer_x"], pts[sref["minimizer_index"]]) and np.array_equal(res["expander_x"], pts[sref["expander_best_index"]])
    assert (res["count_S"], res["count_U"], res["count_M"]) == (sref["S"].sum(), sref["U"].sum(), sref["M"].sum())
    assert res["count_G"] == sref["G"].sum(axis=1).tolist()
    assert _close(res["u_star"], sref["u_star"]) and np.allclose(res["L"], sref["L"], rtol=1e-9, atol=0.0)
    g = res["goose"]
    assert g["safe_min_index"] == gref["safe_min_index"] and g["target_index_c"] == [int(x) for x in gref["target_index_c"]]
    assert g["target_best_c"] == gref["target_best"] and g["target_index"] == gref["target_index"]
    assert g["explore_index"] == gref["explore_index"] and g["choose_safe_min"] == gref["choose_safe_min"]
    assert g["count_O"] == gref["O"].sum(axis=1).tolist()
    for c in range(q - 1):
        if gref["target_index_c"][c] >= 0:
            assert _close(g["target_lcb_c"][c], gref["target_lcb_c"][c]), c
        else:
            assert g["target_lcb_c"][c] == np.inf, c
    assert np.array_equal(g["target_x"], pts[gref["target_index"]]) and np.array_equal(g["explore_x"], pts[gref["explore_index"]])


@pytest.mark.parametrize("world,q", [(3, 5), (2, 8)])
def test_multi_rank_speculative_halo_with_many_constraints(engine, tmp_path, world, q):
    """Three sweeps with growing b on 131 lines: the first sizes the halo windows of every constraint from its own keys (the host
    waits), the later ones from the previous sweep's (no wait inside the sweep, or -- the radii grew past the window -- one rerun
    of the set phase).  Every sweep's sets equal the single-rank engine's."""
    bs, count = [2.0, 2.5, 3.0], [96, 131]
    ds = mc.model(f"q{q}")
    out, parts = _run_ranks(tmp_path, world, f"mc:{q}", mc.CASES[f"q{q}"]["n"], count, bs)
    rows = json.load(open(out))
    lo, hi = mc.box(2)
    engine.set_grid(lo, hi, count)
    for i, (b, row) in enumerate(zip(bs, rows)):
        engine.set_model(ds)
        r = engine.sweep_safeopt(b, want_masks=True)
        m = {key: engine.mask(key) for key in ("S", "M")}
        m.update({f"G{c}": engine.mask("G", c) for c in range(1, q)})
        g = engine.sweep_goose(b, want_masks=True, posterior_ready=True)
        m.update({f"O{c}": engine.mask("O", c) for c in range(1, q)})
        for key, want in m.items():
            assert np.array_equal(np.concatenate([p[f"{i}_{key}"] for p in parts]), want), (i, key)
        assert sum(m[f"G{c}"].any() and m[f"O{c}"].any() for c in range(1, q)) >= q - 2, i
        for key in ("minimizer_index", "expander_index", "count_S", "count_M", "u_star"):
            assert row[key] == r[key], (i, key)
        assert row["count_G"] == r["count_G"].tolist() and row["count_O"] == g["count_O"].tolist(), i
        assert row["target_index"] == g["target_index"] and row["explore_index"] == g["explore_index"], i
    print("[many-constraints] ranks", world, "q", q, [(x["host_syncs"], x["halo_reruns"], x["goose_halo_reruns"]) for x in rows])
    assert rows[0]["host_syncs"] >= 2 and rows[0]["halo_reruns"] == 0            # the first sweep waits for its own keys
    for row in rows[1:]:
        assert row["halo_reruns"] in (0, 1)
        assert row["host_syncs"] == 1 if row["halo_reruns"] == 0 else row["host_syncs"] >= 2, row


# --------------------------------------------------------------------------------------------- (g) robust sweep
def test_robust_sweep_with_four_constraints_matches_the_oracle(engine):
    """StableOpt's min-max on one joint grid at q = 5 (controls: axis 0, disturbance: axis 1): min_d lcb_c for every one of the four
    constraints.  On the exact kernel the per-control arrays are the NumPy reductions of the device posterior bit for bit, and
    count_safe, index, worst_d_index and value are the oracle's."""
    name = "q5"
    ds = mc.model(name)
    lo, hi = mc.box(2)
    count, nc = mc.ROBUST_COUNT, mc.ROBUST_COUNT[0]
    ref = mc.robust_reference()
    with options(engine, bilinear=0, tensor_cheb=0):
        engine.set_model(ds, mean_prior=np.zeros(5))
        engine.set_grid(lo, hi, count)
        res = engine.sweep_robust(mc.ROBUST_B, 1, "ucb")
        assert engine.profile()["posterior_kernel"] == 3
        f, g = engine.robust_arrays()
        mean, var = engine.posterior()
    r = robust_oracle.robust_from_posterior(mean, var, nc, mc.ROBUST_B, "ucb")
    assert g.shape == (4, nc) and np.array_equal(f, r["f"]) and np.array_equal(g, r["g"])
    assert res["value"] == r["value"]
    for key in ("index", "worst_d_index", "count_safe", "candidate_index"):
        assert res[key] == r[key] == ref[key], (key, res[key], r[key], ref[key])
    assert 0 < res["count_safe"] < nc and res["count_control"] == nc and res["count_disturbance"] == count[1]
    tol = 1e-9 * max(1.0, float(np.max(ds["Y_std"])) ** 2)
    assert np.max(np.abs(f - ref["f"])) < tol and np.max(np.abs(g - ref["g"])) < tol and abs(res["value"] - ref["value"]) < tol


# --------------------------------------------------------------------------------------------- (h) host classes and limits
def _host_model(cls, q=5):
    name = f"q{q}"
    k = mc.CASES[name]
    plant = [lambda u, noise=0, i=i: float(mc.fan_outputs(np.asarray(u, dtype=np.float64)[None, :], q)[0, i]) for i in range(q)]
    lo, hi = mc.box(2)
    m = cls(plant, np.stack([lo, hi], axis=1), B, grid=tuple(k["count"]))
    X = mc.fan_inputs(2, k["n"], k["seed"])
    m.fixed_hyper = mc.hyper_parameters(2, q)
    m.GP_initialization(X, mc.fan_outputs(X, q), "RBF", multi_hyper=5, var_out=True)
    return m, mc.points(name)


def test_safeopt_class_with_a_five_output_model_follows_the_oracle():
    m, pts = _host_model(SafeOpt.BO)
    ref = oracle.safeopt_sweep(pts, m.inference_datasets, B)
    assert ref["G"].any(axis=1).sum() >= 3
    x, std = m.Minimizer()
    assert np.array_equal(x, pts[ref["minimizer_index"]]) and std == pytest.approx(ref["minimizer_std"], rel=1e-9)
    x, std = m.Expander()
    assert np.array_equal(x, pts[ref["expander_best_index"]]) and std == pytest.approx(ref["expander_best_std"], rel=1e-9)
    masks = m.masks()
    assert np.array_equal(masks["S"].ravel(), ref["S"])
    for c in range(1, 5):
        assert np.array_equal(masks[f"G{c}"].ravel(), ref["G"][c - 1]), c
        assert m.maximize_infnorm_mean_grad(c) == pytest.approx(ref["L"][c], rel=1e-9)


def test_goose_class_with_a_five_output_model_follows_the_oracle():
    m, pts = _host_model(GoOSE.BO)
    ref = oracle.goose_sweep(pts, m.inference_datasets, B)
    assert ref["O"].any(axis=1).sum() >= 3
    x, lcb = m.minimize_obj_lcb()
    assert np.array_equal(x, pts[ref["safe_min_index"]]) and lcb == pytest.approx(ref["safe_min_lcb"], abs=1e-9)
    t, tl = m.Target()
    assert np.array_equal(t, pts[ref["target_index"]]) and tl == pytest.approx(ref["target_lcb"], abs=1e-9)
    assert np.array_equal(m.explore_safeset(t), pts[ref["explore_index"]])
    other = mc.EXPLORE_TARGET[2]
    assert np.array_equal(m.explore_safeset(other), pts[mc.explore_reference(pts, ref["S"], other)])


def test_nine_outputs_and_foreign_mask_planes_are_refused(engine):
    """q = SBO_MAX_Q + 1 is a ValueError in the reference's style and leaves the resident model alone; mask("G" / "O", c) with c
    outside 1 .. q - 1 is refused instead of reading a neighbouring plane."""
    name, q = "q5", 5
    ds = mc.model(name)
    engine.set_model(ds)
    engine.set_grid(*mc.box(2), mc.CASES[name]["count"])
    engine.sweep_safeopt(B, want_masks=True)
    for c in (0, q, q + 1, 8, -1):
        with pytest.raises(ValueError, match="constraint index out of range"):
            engine.mask("G", c)
    with pytest.raises(ValueError, match="not produced by the last sweep"):
        engine.mask("O", 1)
    engine.sweep_goose(B, want_masks=True, posterior_ready=True)
    for c in (0, q, 8):
        with pytest.raises(ValueError, match="constraint index out of range"):
            engine.mask("O", c)
    assert engine.mask("O", q - 1).shape == (40 * 36,)
    X = mc.fan_inputs(2, 40, 0)
    Y = np.concatenate([mc.fan_outputs(X, 8), mc.fan_outputs(X, 2)[:, 1:]], axis=1)
    assert Y.shape[1] == 9
    with pytest.raises(ValueError, match="q out of range"):
        engine.set_model(safebo_amd.synthetic.make_dataset(X, Y, mc.hyper_parameters(2, 9)))
    assert engine.profile()["set_path"] == 0
