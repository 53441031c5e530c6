"""launch_posterior_gemm (csrc/bilinear_post.inc.hpp) and col_set_phase (csrc/sets_colpath.inc.hpp), the two host functions that drive a
column-path sweep, return what they returned before they became drivers over named steps and their reset flags one type:
tests/golden/colpath_steps/record_before_steps.npz holds what the commit named in its ``commit`` entry returned on an MI355X for the
cases listed here (tests/golden/colpath_steps/record.py writes it).  The column path's other tests compare a switch's two positions
(k1_sched 1 against 0, lean 2 against 0) or the oracle's masks: a change that breaks a switch in both positions at once, a block that is
not neutral on the SECOND sweep, a launch that skips other tiles while the masks stay right pass them.  Here everything is compared for
equality, floats bit for bit (the device code is the same): every entry of the result of ``sweep_safeopt`` (``guard_band`` and
``n_exact_rechecks`` among them), the masks S, U, M and G_1, and from the profile ``set_path``, ``posterior_kernel``,
``k1_tiles_skipped``, ``k1_tiles_skipped_safe`` and ``host_syncs``.  Masks of more than 100 000 candidates are pinned as the SHA-256
digest of their packed bits and their count, smaller ones as packed bits.  A sweep that ends in ``EmptySafeSetError`` is pinned as its
message and the masks it left.

Every case is a SEQUENCE on one engine, because the flags of the blocks a sweep's last reader resets live between sweeps.  Options
fuse_classify = 1 and col_path = 2 force the column path; fp64 models of synthetic.make_config.  Shapes (a tile is 64 rows x 128
columns): 128 x 64, config A, n = 20 -- one tile, one shard with an entry, one coarse block; 384 x 192, config H, n = 96 -- 3 x 3 tiles,
on the window of tests/test_gpu_k1sched_head.py (every tile holds a safe candidate at small b, tiles proved SAFE at b <= 2, tiles proved
unsafe from b = 3) and on config H's whole box (tiles proved unsafe at every b); 512 x 64 and 4096 x 64, config B, n = 64 -- 4 and 32
tiles, rows of 16 and of 128 blocks of the fine image (col_row_search's bound past the end of a short row showed on the first, not on the second).
tests/test_colpath_pins_cpu.py asserts with the oracle that these b give the tile populations named here.

  seq_s<k1_sched>_f<k1_skip_safe>_o<col_overlap>
                   one model on the window: K1i, K1b at lean 0 (records the enclosures), lean 2 at b = 6, lean 2 at b = 1, lean 1, lean 0
  box              the same on the whole box at b = 2 and 6, default options
  first_d<grad_defer>_o<col_overlap>
                   a model's first sweep (K1i) and the one behind it: the deferred gradient launch and the chain on the other stream
  grids            128 x 64 -> 512 x 64 -> 128 x 64 -> 384 x 192 -> 4096 x 64 on one engine, K1i / K1b / lean 2 on each: new buffers, the
                   coarse minima's key, list counters on a buffer that moved
  lazy2_col        exact_lazy = 2 on the column path ...
  lazy2_bytes      ... and with col_path = 0 on the byte-mask path: both callers of the late exhaustive pass
  guard2           guard_band = 2 (forced re-evaluation: the column path's first pass, then the byte masks -- set_path 0) between two lean-2
                   sweeps, then lean 0 and lean 2 again.  Setting the option makes the plans stale: the sweep behind it is a first sweep
  between_<what>   something else between two lean-2 sweeps: posterior_run; a byte-mask sweep (col_path = 0) with mask() calls; a GoOSE
                   sweep (it rewrites the capacity of the partial rows); set_model of the same data
  empty            a sweep that finds no safe candidate between two ordinary ones
"""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from safebo_amd import synthetic  # noqa: E402
from safebo_amd._lib import EmptySafeSetError  # noqa: E402

import test_gpu_recheck_pins as rpins  # noqa: E402  (arrays / pack / unpack: the fixture's form)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(HERE, "golden", "colpath_steps", "record_before_steps.npz")
PROFILE_KEYS = ("set_path", "posterior_kernel", "k1_tiles_skipped", "k1_tiles_skipped_safe", "host_syncs")
DIGEST_ABOVE = 100_000
MARK = None                  # record.py --marks: called with "<case>/<step>" in front of every sweep (a kernel trace is cut at these)
DEFAULTS = {"fuse_classify": -1, "col_path": 1, "k1_sched": 1, "k1_skip_safe": 1, "col_overlap": 1, "grad_defer": 1, "exact_lazy": 1,
            "guard_band": 1}
FORCE = {"fuse_classify": 1, "col_path": 2}

WIN_LO, WIN_HI = np.array([0.2, -1.0]), np.array([1.5, -0.2])        # tests/test_gpu_k1sched_head.py
# grid name -> (config, n, count, window or None for the config's box)
GRIDS = {"A128x64": ("A", 20, [128, 64], None), "Hwin": ("H", 96, [384, 192], (WIN_LO, WIN_HI)), "Hbox": ("H", 96, [384, 192], None),
         "B512x64": ("B", 64, [512, 64], None), "B4096x64": ("B", 64, [4096, 64], None)}
# the b of the lean sweeps on each grid: (one with tiles proved unsafe, another one)
LEAN_B = {"A128x64": (3.0, 1.0), "Hwin": (6.0, 1.0), "Hbox": (6.0, 2.0), "B512x64": (4.0, 1.0), "B4096x64": (4.0, 1.0)}
# grids on which the device proves tiles unsafe at the first lean b (the CPU test asserts that the oracle's enclosures allow it; on config
# B's two grids they do as well, but K1b's recorded enclosures prove no tile unsafe at any b that leaves a safe candidate: those shapes are
# pinned for their image rows and their tile counts)
UNSAFE_TILES = {"Hwin", "Hbox"}
B_EMPTY = 64.0                                               # no safe candidate on any of the grids

_CFG = {}


def config(grid):
    name, n = GRIDS[grid][:2]
    if (name, n) not in _CFG:
        _CFG[(name, n)] = synthetic.make_config(name, n=n)
    return _CFG[(name, n)]


def box(grid):
    cfg, win = config(grid), GRIDS[grid][3]
    return (cfg["bound"][:, 0], cfg["bound"][:, 1]) if win is None else win


# ---- a case: its grid(s), the options it sets, and its steps.  A step is
#   ("grid", name)                    set_grid
#   ("model",)                        set_model of the current grid's config
#   ("opt", key, value)               set_option (restored to DEFAULTS / FORCE behind the case)
#   ("sweep", label, b, lean[, kernel])   a SafeOpt sweep, pinned; b None: the config's own.  label ends in "!" where the byte-mask path is
#                                     meant; kernel: the posterior_kernel that is meant (6 K1i, 4 K1b), where it is not "k1i" in the label -> 6, else 4
#   ("posterior_run",) ("goose", b)   not pinned themselves: what stands between two pinned sweeps
def _triple(grid, tag=""):
    """(K1i's plan needs more of a grid than the column path does: of these grids only the 384 x 192 ones get it, the others' first sweep is K1b's)"""
    return [("grid", grid), ("model",), ("sweep", grid + tag + "_first", None, 0, 6 if grid[0] == "H" else 4), ("sweep", grid + tag + "_second", None, 0),
            ("sweep", grid + tag + "_lean2", LEAN_B[grid][0], 2)]


def _start(grid):
    return [("grid", grid), ("model",), ("sweep", "k1i", None, 0), ("sweep", "k1b", None, 0)]


def _sequence(grid):
    b1, b2 = LEAN_B[grid]
    return _start(grid) + [("sweep", "lean2", b1, 2), ("sweep", "lean2_other_b", b2, 2), ("sweep", "lean1", b1, 1), ("sweep", "lean0", b1, 0)]


def _between(*steps):
    b1 = LEAN_B["Hwin"][0]
    return _start("Hwin") + [("sweep", "lean2_before", b1, 2), *steps, ("sweep", "lean2_after", b1, 2), ("sweep", "lean2_again", b1, 2)]


CASES = {}
for _s in (0, 1):
    for _f in (0, 1):
        for _o in (0, 1):
            CASES[f"seq_s{_s}_f{_f}_o{_o}"] = ({"k1_sched": _s, "k1_skip_safe": _f, "col_overlap": _o}, _sequence("Hwin"), "Hwin")
CASES["box"] = ({}, _sequence("Hbox"), "Hbox")
for _d in (0, 1):
    for _o in (0, 1):
        CASES[f"first_d{_d}_o{_o}"] = ({"grad_defer": _d, "col_overlap": _o}, _start("Hwin"), None)
CASES["grids"] = ({}, _triple("A128x64") + _triple("B512x64") + _triple("A128x64", "_again") + _triple("Hwin") + _triple("B4096x64"), "B4096x64")
CASES["lazy2_col"] = ({"exact_lazy": 2}, _start("Hwin") + [("sweep", "lean2", 6.0, 2), ("sweep", "lean0", 6.0, 0)], "Hwin")
CASES["lazy2_bytes"] = ({"exact_lazy": 2, "col_path": 0}, [("grid", "Hwin"), ("model",), ("sweep", "k1i!", None, 0), ("sweep", "k1b!", None, 0),
                                                          ("sweep", "k1b_other_b!", 6.0, 0)], None)
CASES["guard2"] = ({}, _start("Hwin") + [("sweep", "lean2_before", 1.0, 2), ("opt", "guard_band", 2), ("sweep", "lean2_forced!", 1.0, 2),
                                          ("opt", "guard_band", 1), ("sweep", "lean2_after", 1.0, 2, 6), ("sweep", "lean0", 1.0, 0),
                                          ("sweep", "lean2_again", 1.0, 2)], None)
CASES["between_posterior_run"] = ({}, _between(("posterior_run",)), "Hwin")
CASES["between_bytemask"] = ({}, _between(("opt", "col_path", 0), ("sweep", "bytemask!", 6.0, 0), ("opt", "col_path", 2)), "Hwin")
CASES["between_goose"] = ({}, _between(("goose", 3.0)), "Hwin")
CASES["between_set_model"] = ({}, _between(("model",))[:-2] + [("sweep", "lean2_after", 6.0, 2, 6), ("sweep", "lean2_again", 6.0, 2)], None)
CASES["empty"] = ({}, _start("Hwin") + [("sweep", "lean2_before", 6.0, 2), ("sweep", "lean2_empty", B_EMPTY, 2), ("sweep", "lean2_after", 6.0, 2),
                                         ("sweep", "lean0_empty", B_EMPTY, 0), ("sweep", "lean0_after", 6.0, 0)], "Hwin")


def _mask(m):
    """packed bits, or above DIGEST_ABOVE candidates the SHA-256 digest of the packed bits followed by the count's eight bytes"""
    bits = np.packbits(m)
    if m.size <= DIGEST_ABOVE:
        return bits
    return np.concatenate([np.frombuffer(hashlib.sha256(bits.tobytes()).digest(), dtype=np.uint8),
                           np.frombuffer(np.int64(np.count_nonzero(m)).tobytes(), dtype=np.uint8)])


def _record(engine, res):
    out = dict(res)
    prof = engine.profile()
    for k in PROFILE_KEYS:
        out["profile_" + k] = prof[k]
    for k in "SUM":
        out["mask_" + k] = _mask(engine.mask(k))
    out["mask_G1"] = _mask(engine.mask("G", 1))
    return out


def run_case(engine, name):
    options, steps, _ = CASES[name]
    out, kernels, touched, grid = {}, {}, set(), None
    try:
        for k, val in {**FORCE, **options}.items():
            touched.add(k)
            engine.set_option(k, val)
        for step in steps:
            if step[0] == "grid":
                grid = step[1]
                engine.set_grid(*box(grid), GRIDS[grid][2])
            elif step[0] == "model":
                engine.set_model(config(grid)["ds"], dtype="f64")
            elif step[0] == "opt":
                touched.add(step[1])
                engine.set_option(step[1], step[2])
            elif step[0] == "posterior_run":
                engine.posterior_run()
            elif step[0] == "goose":
                engine.sweep_goose(step[1], want_masks=True)
            else:
                label, b, lean = step[1:4]
                assert label not in out, label
                kernels[label] = step[4] if len(step) > 4 else (6 if "k1i" in label else 4)
                if MARK:
                    MARK(f"{name}/{label}")
                try:
                    res = engine.sweep_safeopt(config(grid)["b"] if b is None else b, want_masks=True, lean=lean)
                except EmptySafeSetError as exc:
                    res = {"empty": np.frombuffer(str(exc).encode(), dtype=np.uint8)}
                out[label] = _record(engine, res)
    finally:
        for k in touched:
            engine.set_option(k, DEFAULTS[k])
    return out, kernels


def check_case(name, got, kernels):
    """what makes a case worth pinning: the path that is meant ran, on sets with something to expand, and where the case names unsafe
    tiles at least one lean-2 sweep left some unevaluated"""
    skipped = []
    for step, v in got.items():
        assert v["profile_set_path"] == (0 if step.endswith("!") else 1), (step, v["profile_set_path"])
        assert v["profile_posterior_kernel"] == kernels[step], (step, v["profile_posterior_kernel"])
        if "empty" in v:
            assert "empty" in step, step
            continue
        assert "empty" not in step, step
        assert v["count_S"] > 0 and v["count_U"] > 0, (step, v["count_S"], v["count_U"])
        if "lean2" in step:
            skipped.append(v["profile_k1_tiles_skipped"])
    if CASES[name][2] in UNSAFE_TILES:
        assert any(s > 0 for s in skipped), skipped
    if name == "guard2":
        safe = {step: v["profile_k1_tiles_skipped_safe"] for step, v in got.items()}
        assert safe["lean2_before"] > 0 and safe["lean2_forced!"] == 0 and safe["lean0"] == 0, safe
        # (an option that makes the plans stale: the sweep behind it is a first sweep again, the next records, the one after skips as before)
        assert safe["lean2_after"] == 0 and safe["lean2_again"] == safe["lean2_before"], safe
        assert got["lean2_forced!"]["guard_passes"] >= 1, got["lean2_forced!"]
    if name == "empty":
        assert sum("empty" in v for v in got.values()) == 2


def _compare(case, got):
    z = rpins.unpack(np.load(FIXTURE))
    assert got
    bad = []
    for name, a in got.items():
        want = z[name]
        same = a.dtype == want.dtype and np.array_equal(a, want)
        print(f"{name}: {a.tolist() if a.size <= 8 else a.size} {'==' if same else '!= ' + str(want.tolist() if want.size <= 8 else want.size)}")
        if not same:
            bad.append(name)
    assert not bad, bad
    recorded = {k for k in z if k.split("/")[0] == case}
    assert recorded == set(got), recorded ^ set(got)


@pytest.mark.parametrize("name", list(CASES))
def test_column_path_returns_what_it_returned_before_the_steps(engine, name):
    got, kernels = run_case(engine, name)
    check_case(name, got, kernels)
    _compare(name, rpins.arrays(name, got))
