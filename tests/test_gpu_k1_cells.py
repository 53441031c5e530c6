"""GPU tests of option k1_cells (csrc/bilinear_post.inc.hpp: k_bhead): on a resident plan -- where k1_resident classifies the
constraint's listed tiles from memory -- ONE launch decides every tile and classifies the others per 8 x 8 cell: a cell its enclosure
proves safe or unsafe takes its bits from the proof, only the rest load their stored values.  With k1_cells 0 the tile-list kernel and
k_bres<1> run as before.

Every comparison is one engine with k1_cells 1 against another with 0 on the same steps, both audited on every sweep, bit for bit:
every entry of the result, the masks S, U, M and G_1, both skip counts, k1_tiles_resident_c / _o, and the posterior arrays read back
at the end.  sbo_profile.k1_cells_evaluated proves which path a sweep took: it counts the cells whose values were loaded, so it is
positive on a sweep that took the path and listed a tile, at most 128 per listed tile, and 0 on the engine without the option.

Shapes (tests/test_gpu_k1_resident.py): the 384 x 192 window of config H, n = 96 (3 x 3 tiles), and 128 x 64 on config A, n = 20 (one
tile).  The census of the window by the NumPy predicates of tests/skip_safe_cases.py on the oracle's posterior (no band test: the
device proves a few cells fewer), as tiles proved safe / proved unsafe / mixed (of those: with cells of both proved signs), and the
undecided cells of the mixed tiles:
    b = 0     6 / 0 / 3 (2)    25 of  384        b = 2.5   1 / 0 / 8 (6)    98 of 1024
    b = 1     5 / 0 / 4 (3)    61 of  512        b = 3     0 / 1 / 8 (7)   110 of 1024
    b = 2     2 / 0 / 7 (7)    77 of  896        b = 6     0 / 3 / 6 (6)    88 of  768
    b = 64    0 / 9 / 0         --
so the walk 1, 2, 2.5, 3, 6, 2.5, 64, 1 holds proved tiles of each sign, mixed tiles with cells of both proved signs and undecided
cells, and tiles that change between class 4, mixed and class 0 from sweep to sweep (tests/test_k1_cells_cpu.py asserts this census).
The one tile of config A is mixed at every b below 64 (25 of its 128 cells undecided at b = 0, 40 at b = 1).

A sweep in which NO predicate decides cannot be reached through the ABI: b < 0 is refused (both engines raise the same ValueError, and
the sweep behind it is unchanged); at b = 0 the predicates would decide (Q = 0: a cell with m_lo > 0 is proved safe, one with
m_hi < 0 unsafe), but such a sweep does not stay on the resident path at all (measured: no tile resident on either engine, as behind a
guard re-evaluation); a finite b whose square overflows (1e155) fails both predicates' range tests and leaves the path the same way.
Whole tiles with all 128 cells evaluated are reached with k1_skip_safe 0 instead: the five tiles of the window proved safe at b = 1
are then listed, and none of their cells is proved unsafe.  The one tile of config A always holds cells proved unsafe (60 at b = 0,
79 at b = 1 by the census), so it is never evaluated whole."""
import numpy as np
import pytest

import safebo_amd
from safebo_amd import synthetic
from safebo_amd._lib import EmptySafeSetError

pytestmark = pytest.mark.gpu

WIN_LO, WIN_HI = np.array([0.2, -1.0]), np.array([1.5, -0.2])        # tests/test_gpu_k1sched_head.py
GRIDS = {"Hwin": ("H", 96, [384, 192], (WIN_LO, WIN_HI)), "A128x64": ("A", 20, [128, 64], None)}
B_EMPTY = 64.0                                                      # no safe candidate on either grid
DEFAULTS = {"fuse_classify": -1, "col_path": 1, "k1_sched": 1, "k1_skip_safe": 1, "guard_band": 1, "k1_resident": 1, "k1_cells": 1}
WALK_B = (1.0, 2.0, 2.5, 3.0, 6.0, 2.5, B_EMPTY, 1.0)
# The CPU census (tests/test_k1_cells_cpu.py asserts these figures from the oracle's posterior): undecided cells of the mixed tiles per b.
# Without a band the device's predicates are the census' predicates, so with guard_band 0 k1_cells_evaluated must EQUAL them.
CENSUS_UNDECIDED = {"Hwin": {1.0: 61, 2.0: 77, 2.5: 98, 3.0: 110, 6.0: 88, B_EMPTY: 0},
                    "A128x64": {1.0: 40, 2.0: 13, 2.5: 8, 3.0: 5, 6.0: 2, B_EMPTY: 0}}
CENSUS_UNSAFE_CELLS_B1 = 133          # the window at b = 1: cells proved unsafe (20 + 103 + 10 in three mixed tiles); the other 1019 of 1152 are
                                      # evaluated when no cell may be taken as proved safe (k1_skip_safe 0)
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
    """The second engine: k1_cells 0, audited on every sweep like the shared one."""
    eng = safebo_amd.SweepEngine(0)
    eng.set_option("guard_audit_every", 1)
    yield eng
    prof = eng.profile()
    eng.close()
    assert prof["guard_audit_violations"] == 0, (prof["guard_audit_violations"], prof["guard_audit_samples"], prof["guard_audit_worst"])


@pytest.fixture
def pair(engine, other):
    for eng, cells in ((engine, 1), (other, 0)):
        eng.set_option("fuse_classify", 1)
        eng.set_option("col_path", 2)
        eng.set_option("k1_cells", cells)
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
    """One SafeOpt sweep: its result (or what it raised), the four masks, the skip, residency and cell counts."""
    try:
        res = eng.sweep_safeopt(b, want_masks=True, lean=lean)
    except EmptySafeSetError as exc:
        res = ("empty", str(exc))
    except ValueError as exc:
        return {"res": ("refused", str(exc))}
    prof = eng.profile()
    masks = {"S": eng.mask("S"), "U": eng.mask("U"), "M": eng.mask("M"), "G": eng.mask("G", 1)}
    return {"res": res, "masks": masks, "skips": (prof["k1_tiles_skipped"], prof["k1_tiles_skipped_safe"]),
            "resident": (prof["k1_tiles_resident_c"], prof["k1_tiles_resident_o"]), "cells": prof["k1_cells_evaluated"],
            "kernel": prof["posterior_kernel"], "set_path": prof["set_path"], "lean": lean}


def _same(a, b, what):
    ra, rb = a["res"], b["res"]
    if isinstance(ra, tuple) or isinstance(rb, tuple):
        assert ra == rb, (what, ra, rb)
    else:
        assert ra.keys() == rb.keys()
        for k in ra:
            np.testing.assert_array_equal(np.asarray(ra[k]), np.asarray(rb[k]), err_msg=f"{what}: {k}")
    if "masks" not in a or "masks" not in b:
        assert "masks" not in a and "masks" not in b, what
        return
    assert a["skips"] == b["skips"], (what, a["skips"], b["skips"])
    assert a["resident"] == b["resident"], (what, a["resident"], b["resident"])
    assert a["kernel"] == b["kernel"] and a["set_path"] == b["set_path"], what
    for k in a["masks"]:
        assert np.array_equal(a["masks"][k], b["masks"][k]), (what, k)


def _walk(pair, grid, steps):
    """The same steps on both engines -- ("sweep", b, lean), ("opt", key, value), ("posterior_run",), ("model",) --; every sweep
    compared, the engine without the option never reports an evaluated cell, the one with it at most 128 a tile it classified from memory (where it
    reports some: the tests, sweep by sweep), the posterior arrays compared at the end.  Returns the records of the engine with the option."""
    on, off = pair
    recs = {on: [], off: []}
    for eng in pair:
        _start(eng, grid)
        for step in steps:
            if step[0] == "sweep":
                recs[eng].append(_sweep(eng, grid, step[1], step[2]))
            elif step[0] == "opt":
                if step[1] != "k1_cells" or eng is on:
                    eng.set_option(step[1], step[2])
            elif step[0] == "posterior_run":
                eng.posterior_run()
            else:
                eng.set_model(_config(grid)["ds"], dtype="f64")
    assert len(recs[on]) == len(recs[off])
    print(grid, [(r.get("kernel"), r.get("skips"), r.get("resident"), r.get("cells")) for r in recs[on]])
    for i, (a, b) in enumerate(zip(recs[on], recs[off])):
        _same(a, b, f"{grid} sweep {i}")
        if "cells" in a:
            assert b["cells"] == 0, (i, b["cells"])
            assert a["cells"] <= 128 * a["resident"][0], (i, a["cells"], a["resident"])
    (m_on, v_on), (m_off, v_off) = on.posterior(), off.posterior()
    assert np.array_equal(m_on, m_off) and np.array_equal(v_on, v_off)
    return recs[on]


def _listed(rec, grid):
    """constraint tiles a lean-2 sweep listed and evaluated: all less the proved unsafe and the proved safe"""
    return _ntiles(grid) - rec["skips"][0] - rec["skips"][1]


def _b_first(grid):
    return _config(grid)["b"]


def _plan(grid):
    """the model's first sweep (K1i where the grid gets it) and K1b at lean 0, which records enclosures and rows and stores every tile"""
    return [("sweep", _b_first(grid), 0), ("sweep", _b_first(grid), 0)]


@pytest.mark.parametrize("band", [1, 0])
@pytest.mark.parametrize("grid", ["Hwin", "A128x64"])
def test_b_walked_up_and_down(pair, grid, band):
    """One plan, b = 1, 2, 2.5, 3, 6, 2.5, 64, 1 at lean 2: tiles change between proved safe, mixed and proved unsafe from sweep to sweep;
    at b = 64 both engines raise EmptySafeSetError with the same text (no tile is listed: no cell is evaluated).  guard_band 1 and 0."""
    recs = _walk(pair, grid, [("opt", "guard_band", band)] + _plan(grid) + [("sweep", b, 2) for b in WALK_B])
    lean2 = recs[2:]
    for r, b in zip(lean2, WALK_B):
        assert r["set_path"] == 1 and r["kernel"] == 4
        assert r["resident"][0] == _listed(r, grid), (b, r["resident"], r["skips"])
        if b == B_EMPTY:
            assert isinstance(r["res"], tuple) and r["res"][0] == "empty" and r["skips"][0] == _ntiles(grid) and r["cells"] == 0, (r["res"], r["skips"])
        else:
            assert not isinstance(r["res"], tuple) and 0 < r["cells"] < 128 * r["resident"][0], (b, r["cells"], r["resident"])
        if band == 0:
            assert r["cells"] == CENSUS_UNDECIDED[grid][b], (grid, b, r["cells"])
        else:
            assert r["cells"] >= CENSUS_UNDECIDED[grid][b], (grid, b, r["cells"])          # (the band test proves no cell the census leaves open)
    assert lean2[0]["cells"] == lean2[-1]["cells"] and lean2[2]["cells"] == lean2[5]["cells"]
    if grid == "Hwin":
        # (proved tiles of each sign beside mixed ones: safe at b = 1, unsafe at b = 6)
        assert lean2[0]["skips"][1] > 0 and lean2[4]["skips"][0] > 0 and lean2[4]["resident"][0] > 0, (lean2[0]["skips"], lean2[4]["skips"])
        assert len({r["skips"] for r in lean2}) >= 3


@pytest.mark.parametrize("grid", ["Hwin", "A128x64"])
def test_a_refused_b_and_b_zero(pair, grid):
    """b < 0: refused by the ABI on both engines with the same text, and the sweep behind it equals the one in front.  b = 0: both
    engines agree bit for bit; the sweep does not stay on the resident path on either (no tile is reported resident), so no cell is
    counted, and the sweep behind it agrees again."""
    steps = _plan(grid) + [("sweep", 1.0, 2), ("sweep", -1.0, 2), ("sweep", 1.0, 2), ("sweep", 0.0, 2), ("sweep", 1.0, 2)]
    recs = _walk(pair, grid, steps)
    first, refused, again, zero, last = recs[2:]
    assert refused["res"][0] == "refused"
    _same(again, first, "behind the refused sweep")
    assert again["cells"] == first["cells"] > 0
    assert not isinstance(zero["res"], tuple) and (zero["cells"] > 0) == (zero["resident"][0] > 0)
    if grid == "Hwin":
        assert zero["cells"] == 0 and zero["resident"] == (0, 0), (zero["cells"], zero["resident"])      # (off the path, as the docstring says)
    assert not isinstance(last["res"], tuple)


@pytest.mark.parametrize("band", [1, 0])
def test_skip_safe_off_whole_tiles_evaluated(pair, band):
    """k1_skip_safe 0 with k1_cells 1: no cell is taken as proved safe.  The tiles proved safe with the option are listed without it and
    EVERY one of their 128 cells is evaluated (none is proved unsafe: the predicates exclude each other) -- the case of a tile that
    costs its workgroup what k_bres<1> cost --, and the mixed tiles evaluate their proved-safe cells on top of the undecided ones: the
    counter exceeds the k1_skip_safe 1 figure at the same b by at least 128 per such tile.  Without a band the count is exact: every cell
    of the nine tiles that the census does not prove unsafe, 1152 - 133 = 1019."""
    grid, b = "Hwin", 1.0
    recs = _walk(pair, grid, [("opt", "guard_band", band)] + _plan(grid) + [("sweep", b, 2), ("opt", "k1_skip_safe", 0), ("sweep", b, 2), ("sweep", b, 2), ("opt", "k1_skip_safe", 1),
                                           ("sweep", b, 2)])
    with_safe, off1, off2, back = recs[2:]
    assert with_safe["skips"][1] > 0 and with_safe["cells"] > 0
    assert off1["skips"][1] == 0 and off1["resident"][0] == _listed(off1, grid) == with_safe["resident"][0] + with_safe["skips"][1]
    assert off1["cells"] > with_safe["cells"] + 128 * with_safe["skips"][1], (with_safe["cells"], with_safe["skips"], off1["cells"])
    assert off2["cells"] == off1["cells"]
    if band == 0:
        assert with_safe["cells"] == CENSUS_UNDECIDED[grid][b] and off1["cells"] == 128 * _ntiles(grid) - CENSUS_UNSAFE_CELLS_B1, (with_safe["cells"], off1["cells"])
    assert back["cells"] == with_safe["cells"] and back["skips"] == with_safe["skips"]


def test_path_left_and_re_entered(pair):
    """What takes a sweep off the path, each between lean-2 sweeps of one grid: sbo_posterior_run (the stored values are rewritten
    through another epilogue: the sweep behind it evaluates and records again), set_model (a new plan: its first two sweeps), a lean-0
    sweep (it runs the GEMM phases, and leaves the plan resident), k1_resident 0 and k1_sched 0.  The counter is 0 exactly there."""
    grid, b = "Hwin", 2.0
    steps = _plan(grid) + [("sweep", b, 2), ("posterior_run",), ("sweep", b, 2), ("sweep", b, 2), ("model",), ("sweep", b, 2), ("sweep", b, 2),
                           ("sweep", b, 2), ("sweep", b, 0), ("sweep", b, 2), ("opt", "k1_resident", 0), ("sweep", b, 2), ("opt", "k1_resident", 1),
                           ("sweep", b, 2), ("opt", "k1_sched", 0), ("sweep", b, 2), ("opt", "k1_sched", 1), ("sweep", b, 2)]
    recs = _walk(pair, grid, steps)
    on = recs[2]
    assert on["cells"] > 0 and on["resident"][0] == _listed(on, grid)
    taken = [r["cells"] > 0 for r in recs[2:]]
    #        lean 2, behind posterior_run, lean 2, new model: K1i, recording K1b, lean 2, lean 0, lean 2, resident 0, resident 1, sched 0, sched 1
    assert taken == [True, False, True, False, False, True, False, True, False, True, False, True], taken
    for r, t in zip(recs[2:], taken):
        if t:
            assert r["cells"] == on["cells"] and r["resident"][0] == on["resident"][0] and r["skips"] == on["skips"], (r["cells"], r["resident"])
        else:
            assert r["resident"][0] == 0, r["resident"]
    assert recs[5]["kernel"] == 6 and recs[6]["kernel"] == 4


def test_option_switched_between_sweeps(pair):
    """k1_cells 1 -> 0 -> 1 on one engine between lean-2 sweeps at one b (the other engine stays at 0): the launches change, nothing else."""
    grid, b = "Hwin", 2.5
    recs = _walk(pair, grid, _plan(grid) + [("sweep", b, 2), ("opt", "k1_cells", 0), ("sweep", b, 2), ("opt", "k1_cells", 1), ("sweep", b, 2)])
    assert [r["cells"] > 0 for r in recs[2:]] == [True, False, True]
    assert recs[3]["resident"] == recs[2]["resident"] == recs[4]["resident"] and recs[2]["cells"] == recs[4]["cells"]
