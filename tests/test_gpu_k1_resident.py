"""GPU tests of option k1_resident (csrc/bilinear_post.inc.hpp: k_bres, k_bl_sched_tiles1 with the plan's Lipschitz rows,
k_bl_sched_list2 split by the residency bytes): from a plan's second lean-2 column-path sweep on, the listed tiles of the constraint
and the objective's tiles whose stored values are the plan's are classified from memory, without their GEMM phases.

Every comparison is one engine with k1_resident 1 against another with 0 on the same steps, bit for bit: every entry of the result
(the Lipschitz keys among them), the masks S, U, M and G_1, both skip counts, and the posterior arrays read back at the end of the
sequence (reading them runs the posterior in full, so it cannot stand between the sweeps).  sbo_profile.k1_tiles_resident_c / _o
prove which path a sweep took: the constraint's count is the tiles the sweep listed and evaluated (all tiles less the two skip
counts), the objective's the tiles that hold a safe candidate and whose residency byte stands.

Shapes: the smallest of tests/test_gpu_colpath_pins.py -- 384 x 192 on config H, n = 96, on the window of
tests/test_gpu_k1sched_head.py (3 x 3 tiles, tiles proved safe at b <= 2 and unsafe from b = 3), and 128 x 64 on config A, n = 20
(one tile)."""
import numpy as np
import pytest

import safebo_amd
from safebo_amd import synthetic
from safebo_amd._lib import EmptySafeSetError

pytestmark = pytest.mark.gpu

WIN_LO, WIN_HI = np.array([0.2, -1.0]), np.array([1.5, -0.2])        # tests/test_gpu_k1sched_head.py
GRIDS = {"Hwin": ("H", 96, [384, 192], (WIN_LO, WIN_HI)), "A128x64": ("A", 20, [128, 64], None)}
B_EMPTY = 64.0                                                      # no safe candidate on either grid
DEFAULTS = {"fuse_classify": -1, "col_path": 1, "k1_sched": 1, "k1_skip_safe": 1, "guard_band": 1, "k1_resident": 1}
_CFG = {}


def _config(grid):
    name, n = GRIDS[grid][:2]
    if (name, n) not in _CFG:
        _CFG[(name, n)] = synthetic.make_config(name, n=n)
    return _CFG[(name, n)]


def _ntiles(grid):
    w, h = GRIDS[grid][2]
    return (w // 128) * (h // 64)


@pytest.fixture(scope="module")
def other():
    """The second engine: k1_resident 0, audited on every sweep like the shared one."""
    eng = safebo_amd.SweepEngine(0)
    eng.set_option("guard_audit_every", 1)
    yield eng
    prof = eng.profile()
    eng.close()
    assert prof["guard_audit_violations"] == 0, (prof["guard_audit_violations"], prof["guard_audit_samples"], prof["guard_audit_worst"])


@pytest.fixture
def pair(engine, other):
    for eng, res in ((engine, 1), (other, 0)):
        eng.set_option("fuse_classify", 1)
        eng.set_option("col_path", 2)
        eng.set_option("k1_resident", res)
    yield engine, other
    for eng in (engine, other):
        for k, v in DEFAULTS.items():
            eng.set_option(k, v)
    assert other.profile()["guard_audit_violations"] == 0


def _start(eng, grid):
    cfg, (_, _, count, win) = _config(grid), GRIDS[grid]
    lo, hi = (cfg["bound"][:, 0], cfg["bound"][:, 1]) if win is None else win
    eng.set_grid(lo, hi, count)
    eng.set_model(cfg["ds"], dtype="f64")


def _sweep(eng, grid, b, lean):
    """One SafeOpt sweep: its result (or what it raised), the four masks, the skip and residency counts, the tiles with a safe candidate."""
    try:
        res = eng.sweep_safeopt(b, want_masks=True, lean=lean)
    except EmptySafeSetError as exc:
        res = ("empty", str(exc))
    prof = eng.profile()
    masks = {"S": eng.mask("S"), "U": eng.mask("U"), "M": eng.mask("M"), "G": eng.mask("G", 1)}
    w, h = GRIDS[grid][2]
    has_S = np.asarray(masks["S"]).reshape(h // 64, 64, w // 128, 128).any(axis=(1, 3))
    return {"res": res, "masks": masks, "skips": (prof["k1_tiles_skipped"], prof["k1_tiles_skipped_safe"]),
            "resident": (prof["k1_tiles_resident_c"], prof["k1_tiles_resident_o"]), "kernel": prof["posterior_kernel"],
            "set_path": prof["set_path"], "has_S": has_S}


def _same(a, b, what):
    assert a["skips"] == b["skips"], (what, a["skips"], b["skips"])
    assert a["kernel"] == b["kernel"] and a["set_path"] == b["set_path"], what
    ra, rb = a["res"], b["res"]
    if isinstance(ra, tuple) or isinstance(rb, tuple):
        assert ra == rb, (what, ra, rb)
    else:
        assert ra.keys() == rb.keys()
        for k in ra:
            np.testing.assert_array_equal(np.asarray(ra[k]), np.asarray(rb[k]), err_msg=f"{what}: {k}")
    for k in a["masks"]:
        assert np.array_equal(a["masks"][k], b["masks"][k]), (what, k)


def _walk(pair, grid, steps):
    """The same steps on both engines -- ("sweep", b, lean), ("opt", key, value), ("posterior_run",), ("model",) --; every sweep
    compared, the engine without the option never reports a resident tile, the posterior arrays compared at the end.  Returns the
    records of the engine with the option, one per sweep."""
    on, off = pair
    recs = {on: [], off: []}
    for eng in pair:
        _start(eng, grid)
        for step in steps:
            if step[0] == "sweep":
                recs[eng].append(_sweep(eng, grid, step[1], step[2]))
            elif step[0] == "opt":
                eng.set_option(step[1], step[2])
            elif step[0] == "posterior_run":
                eng.posterior_run()
            else:
                eng.set_model(_config(grid)["ds"], dtype="f64")
    assert len(recs[on]) == len(recs[off])
    for i, (a, b) in enumerate(zip(recs[on], recs[off])):
        _same(a, b, f"{grid} sweep {i}")
        assert b["resident"] == (0, 0), (i, b["resident"])
    (m_on, v_on), (m_off, v_off) = on.posterior(), off.posterior()
    assert np.array_equal(m_on, m_off) and np.array_equal(v_on, v_off)
    print(grid, [(r["kernel"], r["skips"], r["resident"], int(r["has_S"].sum())) for r in recs[on]])
    return recs[on]


def _listed(rec, grid):
    """constraint tiles a lean-2 sweep listed and evaluated: all less the proved unsafe and the proved safe"""
    return _ntiles(grid) - rec["skips"][0] - rec["skips"][1]


def _b_first(grid):
    return _config(grid)["b"]


@pytest.mark.parametrize("grid,b", [("Hwin", 6.0), ("Hwin", 2.0), ("A128x64", 1.0)])
def test_same_b_three_times(pair, grid, b):
    """The model's first sweep (K1i where the grid gets it), K1b at lean 0 (records enclosures and rows, stores every tile), then lean 2
    three times at one b: the first of them already finds every tile resident -- the lean-0 sweep stored them all --, and so do the others."""
    recs = _walk(pair, grid, [("sweep", _b_first(grid), 0), ("sweep", _b_first(grid), 0)] + [("sweep", b, 2)] * 3)
    assert recs[1]["kernel"] == 4 and recs[1]["resident"] == (0, 0), recs[1]
    for r in recs[2:]:
        assert r["set_path"] == 1 and r["kernel"] == 4
        assert r["resident"] == (_listed(r, grid), int(r["has_S"].sum())), (r["resident"], r["skips"], r["has_S"])
    assert int(recs[2]["has_S"].sum()) > 0
    if grid == "Hwin":
        assert recs[2]["skips"][0 if b >= 3.0 else 1] > 0, recs[2]["skips"]


def test_plan_recorded_by_a_lean2_sweep(pair):
    """A plan whose first K1b sweep is already lean 2: the recording sweep stores the objective on the tiles with a safe candidate only.
    Lean 2 at b = 6, at b = 1 and at b = 6 again: at b = 1 the tiles that had no safe candidate at b = 6 take the GEMM path (their
    count is the difference), and they are resident in the sweep after."""
    grid = "Hwin"
    steps = [("sweep", _b_first(grid), 0), ("sweep", 6.0, 2), ("sweep", 6.0, 2), ("sweep", 1.0, 2), ("sweep", 1.0, 2), ("sweep", 6.0, 2)]
    recs = _walk(pair, grid, steps)
    assert recs[0]["kernel"] == 6 and recs[1]["kernel"] == 4
    rec6, s6, s1, s1b, s6b = recs[1:]
    assert rec6["resident"] == (0, 0) and rec6["skips"] == (0, 0)            # (the recording sweep: every constraint tile evaluated)
    n6, n1 = int(s6["has_S"].sum()), int(s1["has_S"].sum())
    assert 0 < n6 < n1, (n6, n1)
    assert np.all(s1["has_S"][s6["has_S"]])
    assert s6["resident"] == (_listed(s6, grid), n6)
    assert s1["resident"] == (_listed(s1, grid), n6) and n1 - n6 > 0         # (n1 - n6 tiles of the objective ran their GEMM phases)
    assert s1b["resident"] == (_listed(s1b, grid), n1)
    assert s6b["resident"] == (_listed(s6b, grid), n6)


def test_posterior_run_between(pair):
    """sbo_posterior_run between two lean-2 sweeps writes the resident posterior through another epilogue: nothing is resident in the
    sweep behind it (it evaluates, stores and records again), and the counts are back one sweep later."""
    grid, b = "Hwin", 6.0
    steps = [("sweep", _b_first(grid), 0), ("sweep", _b_first(grid), 0), ("sweep", b, 2), ("posterior_run",), ("sweep", b, 2), ("sweep", b, 2)]
    recs = _walk(pair, grid, steps)
    before, behind, after = recs[2:]
    assert before["resident"] == (_listed(before, grid), int(before["has_S"].sum())) and before["resident"][1] > 0
    assert behind["resident"] == (0, 0) and behind["skips"] == (0, 0)
    assert after["resident"] == before["resident"] and after["skips"] == before["skips"]


def test_guard_recheck_between(pair):
    """guard_band 2 (exact re-evaluation on every sweep: the patch path) between two lean-2 sweeps."""
    grid, b = "Hwin", 1.0
    steps = [("sweep", _b_first(grid), 0), ("sweep", _b_first(grid), 0), ("sweep", b, 2), ("opt", "guard_band", 2), ("sweep", b, 2),
             ("opt", "guard_band", 1), ("sweep", b, 2), ("sweep", b, 0), ("sweep", b, 2), ("sweep", b, 2)]
    recs = _walk(pair, grid, steps)
    assert recs[2]["resident"][1] > 0
    assert recs[3]["resident"] == (0, 0)
    last = recs[-1]
    assert last["kernel"] == 4 and last["resident"] == (_listed(last, grid), int(last["has_S"].sum()))


def test_set_model_between(pair):
    """set_model of the same data: a new plan -- nothing is resident in its first sweeps, whatever the old plan's bytes said."""
    grid, b = "Hwin", 6.0
    steps = [("sweep", _b_first(grid), 0), ("sweep", _b_first(grid), 0), ("sweep", b, 2), ("model",), ("sweep", b, 2), ("sweep", b, 2),
             ("sweep", b, 2)]
    recs = _walk(pair, grid, steps)
    assert recs[2]["resident"][1] > 0
    assert recs[3]["kernel"] == 6 and recs[3]["resident"] == (0, 0)
    assert recs[4]["kernel"] == 4 and recs[4]["resident"] == (0, 0)          # (the new plan's recording sweep)
    assert recs[5]["resident"] == (_listed(recs[5], grid), int(recs[5]["has_S"].sum()))


@pytest.mark.parametrize("key", ["k1_skip_safe", "k1_sched"])
def test_other_options_off(pair, key):
    """k1_skip_safe 0 with k1_resident 1: the path is taken, the proved-safe tiles are listed and classified from memory as well.
    k1_sched 0: no lists, the parent's sweep, both counters 0."""
    grid, b = "Hwin", 2.0
    steps = [("opt", key, 0), ("sweep", _b_first(grid), 0), ("sweep", _b_first(grid), 0), ("sweep", b, 2), ("sweep", b, 2)]
    recs = _walk(pair, grid, steps)
    for r in recs[2:]:
        if key == "k1_sched":
            assert r["resident"] == (0, 0), r["resident"]
        else:
            assert r["skips"][1] == 0 and r["resident"] == (_listed(r, grid), int(r["has_S"].sum())), (r["skips"], r["resident"])


def test_empty_safe_set_between(pair):
    """A sweep without any safe candidate between two ordinary ones: both of its lists are empty, the sweep behind it equals the one
    in front of it."""
    grid, b = "Hwin", 6.0
    steps = [("sweep", _b_first(grid), 0), ("sweep", _b_first(grid), 0), ("sweep", b, 2), ("sweep", B_EMPTY, 2), ("sweep", b, 2)]
    recs = _walk(pair, grid, steps)
    before, empty, after = recs[2:]
    assert isinstance(empty["res"], tuple) and empty["resident"] == (_listed(empty, grid), 0), (empty["res"], empty["resident"])
    _same(after, before, "behind the empty sweep")
    assert after["resident"] == before["resident"] and before["resident"][1] > 0
