"""CPU check of the cases tests/test_gpu_colpath_pins.py pins: with the oracle's posterior, the b values chosen there give the tile
populations its docstring names (a tile is 64 rows x 128 columns; the enclosure predicates are those of tests/skip_safe_cases.py on the
8 x 8 cells, without the band test)."""
import numpy as np
import pytest

import oracle
import skip_safe_cases as ssc
import test_gpu_colpath_pins as pins


def _census(grid, b):
    """(tiles with a safe candidate, tiles proved safe, tiles proved unsafe, |S|, |U|) of a grid at b"""
    c0, c1 = pins.GRIDS[grid][2]
    mean, var = _posterior(grid)
    cells = []
    for a, red in ((mean[:, 1], np.min), (mean[:, 1], np.max), (var[:, 1], np.min), (var[:, 1], np.max)):
        cells.append(red(a.reshape(c1 // 64, 8, 8, c0 // 128, 16, 8), axis=(2, 5)).transpose(0, 2, 1, 3))
    lcb, _ = oracle.bounds(mean, var, b)
    S = lcb[:, 1] >= 0
    has_S = S.reshape(c1 // 64, 64, c0 // 128, 128).any(axis=(1, 3))
    return (int(has_S.sum()), int(ssc.encl_safe(*cells, b).all(axis=(2, 3)).sum()), int(ssc.encl_unsafe(*cells, b).all(axis=(2, 3)).sum()),
            int(S.sum()), int((lcb[:, 1] <= 0).sum()))


_POST = {}


def _posterior(grid):
    if grid not in _POST:
        _POST[grid] = oracle.gp_inference(oracle.grid_points(*pins.box(grid), pins.GRIDS[grid][2]), pins.config(grid)["ds"])
    return _POST[grid]


@pytest.mark.parametrize("grid", list(pins.GRIDS))
def test_the_pinned_b_values_give_the_tile_populations_named(grid):
    c0, c1 = pins.GRIDS[grid][2]
    tiles = (c0 // 128) * (c1 // 64)
    for b in pins.LEAN_B[grid] + (pins.config(grid)["b"],):
        has_S, _, unsafe, nS, nU = _census(grid, b)
        assert has_S > 0 and nS > 0 and nU > 0, (grid, b, has_S, nS, nU)
        assert has_S + unsafe <= tiles
    unsafe = _census(grid, pins.LEAN_B[grid][0])[2]
    assert unsafe > 0 or grid not in pins.UNSAFE_TILES, (grid, unsafe)
    assert _census(grid, pins.B_EMPTY)[0] == 0
    if grid == "Hwin":
        assert _census(grid, 0.25)[0] == tiles                    # every tile holds a safe candidate at small b
        assert _census(grid, 1.0)[1] > 0                          # tiles proved safe: what guard2's forced re-evaluation drops
