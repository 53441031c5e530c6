"""Shared cases of the safe-tile skip (option k1_skip_safe; csrc/bilinear_post.inc.hpp: encl_safe / encl_unsafe / encl_keys): config H's
model with n = 96 on small grids, a NumPy restatement of the two enclosure predicates on the oracle's posterior, and the census of tile
classes they give.  tests/test_skip_safe_cpu.py checks the census itself; tests/test_gpu_skip_safe.py compares the device with it.

A tile is 64 rows x 128 columns of the grid (axis 0 fastest), a cell 8 x 8 candidates, 128 cells per tile.  The device takes its
enclosures from what K1b stored, the census from the oracle's values: the two differ by the plan's guard band (~1e-9 relative), so the
census is the device's only where no cell comes near a threshold -- `margin` below is the smallest relative distance of any cell's
corner test from its threshold, and the CPU test asserts it is above 1e-6."""
import functools
import os

import numpy as np

import oracle
from safebo_amd import synthetic

C48 = 1.0 + 2.0 ** -48
WHOLE = "whole"
INSIDE = "inside"


@functools.lru_cache(maxsize=None)
def config():
    return synthetic.make_config("H", n=96)


@functools.lru_cache(maxsize=None)
def grid(name):
    """(lo, hi, count) of a case: the whole domain on [512, 256] (4 x 4 tiles), or the box inside the safe set of
    tests/test_gpu_k1skip.py::test_no_skip_where_every_tile_holds_a_safe_candidate on [256, 128] (4 tiles)."""
    cfg = config()
    lo, hi = cfg["bound"][:, 0], cfg["bound"][:, 1]
    if name == WHOLE:
        return lo, hi, (512, 256)
    coarse = oracle.grid_points(lo, hi, [64, 64])
    cref = oracle.safeopt_sweep(coarse, cfg["ds"], cfg["b"])
    mean, var = cref["mean"][:, 1], cref["var"][:, 1]
    c = coarse[int(np.argmax(mean - cfg["b"] * np.sqrt(np.maximum(var, 0.0))))]
    w = 0.002 * (hi - lo)
    return c - w, c + w, (256, 128)


@functools.lru_cache(maxsize=None)
def posterior(name):
    """The oracle's (mean, var) of a case's grid, [N, q]: computed once, shared by every b."""
    lo, hi, count = grid(name)
    return oracle.gp_inference(oracle.grid_points(lo, hi, list(count)), config()["ds"])


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "skip_safe", "whole.npz")
GOLDEN_B = (1.0, 0.25, 3.0)
_REF_KEYS = ("S", "U", "M", "G")
_REF_SCALARS = ("u_star", "minimizer_index", "minimizer_std", "expander_index", "expander_best", "expander_best_std", "L")


def _oracle_sweep(name, b):
    lo, hi, count = grid(name)
    return oracle.safeopt_sweep(oracle.grid_points(lo, hi, list(count)), config()["ds"], b, mean_var=posterior(name))


@functools.lru_cache(maxsize=None)
def reference(name, b):
    """The oracle's sweep of a case.  The whole-domain grid's expander set takes the oracle a minute per b (every safe candidate against
    every unsafe one), so its sweeps are recorded in tests/golden/skip_safe/whole.npz (masks as packed bits, the scalars; `PYTHONPATH=.
    python tests/skip_safe_cases.py` from the repository root writes the file from the oracle); tests/test_skip_safe_cpu.py checks everything in the record but G
    against the oracle.  The inside box (no unsafe candidate, G empty) is swept by the oracle when asked."""
    if name != WHOLE:
        return _oracle_sweep(name, b)
    _, _, (c0, c1) = grid(name)
    n = c0 * c1
    with np.load(GOLDEN) as z:
        tag = f"b{b:g}_"
        ref = {k: np.unpackbits(z[tag + k])[:n].astype(bool) for k in ("S", "U", "M")}
        ref["G"] = np.unpackbits(z[tag + "G"])[:n].astype(bool)[None, :]
        for k in _REF_SCALARS:
            v = z[tag + k]
            ref[k] = v if v.ndim else v.item()
    return ref


def write_golden():
    out = {}
    for b in GOLDEN_B:
        r = _oracle_sweep(WHOLE, b)
        tag = f"b{b:g}_"
        for k in ("S", "U", "M"):
            out[tag + k] = np.packbits(r[k])
        out[tag + "G"] = np.packbits(r["G"][0])
        for k in _REF_SCALARS:
            out[tag + k] = np.asarray(r[k])
    np.savez_compressed(GOLDEN, **out)


def cells(name):
    """[tile rows, tile cols, 8, 16] arrays m_lo, m_hi, v_lo, v_hi of the constraint over the 8 x 8 cells."""
    _, _, (c0, c1) = grid(name)
    mean, var = posterior(name)
    out = []
    for a, red in ((mean[:, 1], np.min), (mean[:, 1], np.max), (var[:, 1], np.min), (var[:, 1], np.max)):
        x = a.reshape(c1 // 64, 8, 8, c0 // 128, 16, 8)        # (tile row, cell row, row in cell, tile col, cell col, col in cell)
        out.append(red(x, axis=(2, 5)).transpose(0, 2, 1, 3))
    return out


def encl_safe(mlo, mhi, vlo, vhi, b):
    """csrc/bilinear_post.inc.hpp: encl_safe without its band test (on these grids the band does not change which tiles are proved safe:
    the device's count is compared with this census)."""
    tiny, huge = 1e-250, 1e300
    bb = b * b
    return (b >= 0) & (vlo >= 0) & (mlo > 0) & (mhi * mhi < huge) & (bb * vhi < huge) & (mlo * mlo > tiny) & (mlo * mlo >= bb * vhi * C48)


def encl_unsafe(mlo, mhi, vlo, vhi, b):
    """encl_unsafe without its band test.  The device's predicate, which has that test, proves fewer tiles unsafe than this one (7 of
    these 9 at b = 1, 5 of 11 at b = 3): its count is compared between option settings, not with this census."""
    tiny, huge = 1e-250, 1e300
    bb = b * b
    pos = (mhi * mhi < huge) & (bb * vhi < huge) & (bb * vlo > tiny) & (mhi * mhi * C48 <= bb * vlo)
    return (b >= 0) & (vlo >= 0) & ((mhi < 0) | pos)


def census(name, b):
    """dict: safe / unsafe [tile rows, tile cols] bool (every cell of the tile passes), margin = the smallest relative distance of a
    cell's corner test from its threshold over the whole grid."""
    mlo, mhi, vlo, vhi = cells(name)
    safe = encl_safe(mlo, mhi, vlo, vhi, b).all(axis=(2, 3))
    unsafe = encl_unsafe(mlo, mhi, vlo, vhi, b).all(axis=(2, 3))
    bb = b * b
    ps, qs = np.where(mlo > 0, mlo * mlo, 0.0), bb * vhi              # safe:   P_lo against Q_hi
    pu, qu = np.where(mhi > 0, mhi * mhi, 0.0), bb * vlo              # unsafe: P_hi against Q_lo
    margin = min(float(np.min(np.abs(ps - qs) / np.maximum(ps, qs))), float(np.min(np.abs(pu - qu) / np.maximum(pu, qu))))
    return {"safe": safe, "unsafe": unsafe, "margin": margin}


def key_bounds(name, b):
    """Per tile: the variance key (min v_lo), the upper bound of max ucb_1 (max over cells of m_hi + b sqrt v_hi) and the lower bound of
    min ucb_1 (min of m_lo + b sqrt v_lo), as encl_keys forms them up to its outward rounding."""
    mlo, mhi, vlo, vhi = cells(name)
    return (vlo.min(axis=(2, 3)), (mhi + b * np.sqrt(vhi)).max(axis=(2, 3)), (mlo + b * np.sqrt(vlo)).min(axis=(2, 3)))


def tiles_of(name, a):
    """A per-candidate array [N] as [tile rows, 64, tile cols, 128]."""
    _, _, (c0, c1) = grid(name)
    return a.reshape(c1 // 64, 64, c0 // 128, 128)


# ---- what the GPU tests of a case share (tests/test_gpu_skip_safe.py, tests/test_gpu_history.py); nothing here opens a GPU on import ----
KEYS = ("minimizer_index", "expander_index", "expander_best_c", "choose_minimizer", "count_S", "count_U", "count_M", "u_star",
        "minimizer_std", "expander_std")


def masks(eng):
    return {"S": eng.mask("S"), "U": eng.mask("U"), "M": eng.mask("M"), "G": eng.mask("G", 1)}


def sweep(eng, b, lean):
    res = eng.sweep_safeopt(b, want_masks=True, lean=lean)
    return res, masks(eng)


def same(a, b):
    (ra, ma), (rb, mb) = a, b
    for k in KEYS:
        assert ra[k] == rb[k], (k, ra[k], rb[k])
    assert list(ra["count_G"]) == list(rb["count_G"]) and list(ra["expander_index_c"]) == list(rb["expander_index_c"])
    assert ra["L"][1] == rb["L"][1]
    for k in ma:
        assert np.array_equal(ma[k], mb[k]), k


def check_oracle(res, masks, ref):
    for k in ("S", "U", "M"):
        assert np.array_equal(masks[k], ref[k]), k
    assert np.array_equal(masks["G"], ref["G"][0])
    assert res["minimizer_index"] == ref["minimizer_index"]
    assert list(res["expander_index_c"]) == list(ref["expander_index"])
    assert abs(res["u_star"] - ref["u_star"]) < 1e-10
    assert (res["count_S"], res["count_U"], res["count_M"], res["count_G"][0]) == (ref["S"].sum(), ref["U"].sum(), ref["M"].sum(), ref["G"][0].sum())
    assert np.allclose(res["L"][1:], ref["L"][1:], rtol=1e-9)
    assert abs(res["minimizer_std"] - ref["minimizer_std"]) < 1e-10
    if ref["expander_best"] > 0:
        assert abs(res["expander_std"] - ref["expander_best_std"]) < 1e-10


def census_safe(name, b):
    """Tiles the CPU census proves safe.  (The device's count of tiles proved UNSAFE is not compared with the census, which leaves the
    band test out and proves more -- encl_unsafe --; it is compared between option settings instead.)"""
    return int(census(name, b)["safe"].sum())


def skips(eng):
    p = eng.profile()
    return p["k1_tiles_skipped_safe"], p["k1_tiles_skipped"]


def colpath_options(eng):
    eng.set_option("fuse_classify", 1)
    eng.set_option("col_path", 2)


def start(eng, name, b):
    """Grid and model of a case, the model's first sweep (K1i) and the plan's first K1b sweep, which evaluates every tile and records."""
    lo, hi, count = grid(name)
    eng.set_grid(lo, hi, list(count))
    eng.set_model(config()["ds"], dtype="f64")
    eng.sweep_safeopt(b, want_masks=True)
    eng.sweep_safeopt(b, want_masks=True)
    assert eng.profile()["posterior_kernel"] == 4 and skips(eng) == (0, 0)


_FRESH = {}


def fresh(name, b):
    """What a fresh engine returns for the case at lean 0 on its K1b plan (nothing skipped): computed once per (grid, b)."""
    if (name, b) not in _FRESH:
        import safebo_amd
        with safebo_amd.SweepEngine(0) as eng:
            colpath_options(eng)
            start(eng, name, b)
            _FRESH[(name, b)] = sweep(eng, b, 0)
            assert eng.profile()["set_path"] == 1
    return _FRESH[(name, b)]


if __name__ == "__main__":
    write_golden()
