"""The populations tests/test_gpu_col_decide_units.py relies on, asserted with the oracle alone (no GPU): k_col_decide
(csrc/sets_colpath.inc.hpp) walks HALF-WIDTH units -- (tile of 64 rows x 128 columns with a safe candidate, one of its eight 8-row
octets, one of its two 64-column halves) -- and the GPU tests need grids on which the boundary of G_1 runs through both halves of an
octet, a tile keeps all its safe candidates in one half, and a tile row lists one tile or all of them.  The windows and b values
below were picked on synthetic config H with n = 96; a drift of that config shows here first.

The cases and helpers are shared with the GPU tests (imported from this module); the oracle's sweeps are computed once per
(window, grid, b) and left unchanged."""
import numpy as np
import pytest

import oracle
from safebo_amd import synthetic

# windows of config H's box: the box itself (None), the window of tests/test_gpu_k1sched_head.py, and one whose safe set hugs the
# right edge at large b
BOX = None
WIN = ((0.2, -1.0), (1.5, -0.2))
EDGE = ((0.9, -1.0), (1.5, -0.15))

# test 1 / 4: the boundary of G_1 crosses column 64 of a tile -- (window, grid, b).  [128, 64] is a single tile: the smallest grid
# at which unit indexing can go wrong meets the assertion.
BOUNDARY = [(BOX, (128, 64), 1.0), (BOX, (256, 128), 3.0), (WIN, (128, 64), 0.25), (WIN, (256, 128), 0.25)]
# test 2: a listed tile with a half that holds no safe candidate at b_sparse and some at b_dense -- (window, grid, b_sparse, b_dense,
# (tile row, tile column, half))
EMPTY_HALF = [(BOX, (128, 64), 3.0, 1.0, (0, 0, 0)), (WIN, (256, 128), 8.0, 6.0, (1, 1, 1))]
# test 3: tile rows by the tiles they list -- (window, grid, b, listed tiles per row)
ROWS = [(EDGE, (256, 128), 8.0, ((1, 1), (1, 0))),          # all listed | the left one alone
        (WIN, (256, 128), 6.0, ((1, 1), (0, 1))),           # all listed | the right one alone
        (WIN, (384, 192), 9.0, ((0, 0, 1), (0, 0, 1), (0, 0, 0)))]      # three tiles, the right one alone | no tile
# test 5: lean levels and K1i / K1b
LEAN = (WIN, (256, 128), 6.0)


def config():
    return synthetic.make_config("H", n=96)


def window(cfg, win):
    if win is None:
        return cfg["bound"][:, 0].copy(), cfg["bound"][:, 1].copy()
    return np.array(win[0]), np.array(win[1])


_POST, _REF = {}, {}


def reference(cfg, win, count, b):
    """oracle.safeopt_sweep on the grid, computed once per case and read-only."""
    key = (win, tuple(count), float(b))
    if key not in _REF:
        lo, hi = window(cfg, win)
        pts = oracle.grid_points(lo, hi, list(count))
        if key[:2] not in _POST:
            _POST[key[:2]] = oracle.gp_inference(pts, cfg["ds"])
        ref = oracle.safeopt_sweep(pts, cfg["ds"], b, mean_var=_POST[key[:2]])
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def units(x, count):
    """[tile row][octet][8 rows][tile column][half][64 columns] view of a flat per-candidate array (axis 0 fastest)."""
    W, H = count
    return np.asarray(x).reshape(H // 64, 8, 8, W // 128, 2, 64)


def mixed_octets(ref, count):
    """(tile row, octet, tile column) of the octets BOTH of whose half-width units hold safe members and safe non-members of G_1."""
    S, G = ref["S"], ref["G"][0]
    inside = units(S & G, count).any(axis=(2, 5))
    outside = units(S & ~G, count).any(axis=(2, 5))
    return np.argwhere((inside & outside).all(axis=3))


def half_counts(mask, count):
    """[tile row][tile column][half] counts of a mask."""
    return units(mask, count).sum(axis=(1, 2, 5))


def listed(ref, count):
    """[tile row][tile column]: does the tile hold a safe candidate."""
    return half_counts(ref["S"], count).sum(axis=2) > 0


@pytest.fixture(scope="module")
def cfg():
    return config()


@pytest.mark.parametrize("win,count,b", BOUNDARY)
def test_boundary_crosses_column_64(cfg, win, count, b):
    ref = reference(cfg, win, count, b)
    assert not ref["empty_safe_set"] and ref["U"].any()
    assert len(mixed_octets(ref, count)) >= 1


@pytest.mark.parametrize("win,count,b_sparse,b_dense,where", EMPTY_HALF)
def test_half_without_safe_candidates(cfg, win, count, b_sparse, b_dense, where):
    r, t, h = where
    sparse = half_counts(reference(cfg, win, count, b_sparse)["S"], count)
    dense = half_counts(reference(cfg, win, count, b_dense)["S"], count)
    assert sparse[r, t, h] == 0 and sparse[r, t, 1 - h] > 0, sparse.tolist()
    assert dense[r, t, h] > 0, dense.tolist()
    # (the half that gains safe candidates gains members of G_1 too: stale or missing G bytes would show)
    assert half_counts(reference(cfg, win, count, b_dense)["G"][0], count)[r, t, h] > 0


@pytest.mark.parametrize("win,count,b,rows", ROWS)
def test_row_masks(cfg, win, count, b, rows):
    got = listed(reference(cfg, win, count, b), count)
    assert got.astype(int).tolist() == [list(r) for r in rows], got.astype(int).tolist()


def test_lean_case_is_not_trivial(cfg):
    win, count, b = LEAN
    ref = reference(cfg, win, count, b)
    assert ref["S"].any() and ref["M"].any() and ref["G"][0].any() and not ref["S"].all()
