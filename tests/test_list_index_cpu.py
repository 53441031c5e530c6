"""Host side of scattered candidate lists in the classes (no GPU: the engine is created lazily, after the argument checks)."""
import numpy as np
import pytest

from safebo_amd import GoOSE, SafeOpt


@pytest.mark.parametrize("cls", [SafeOpt.BO, GoOSE.BO])
def test_grid_and_candidates_together_are_refused(cls):
    with pytest.raises(ValueError):
        cls([lambda x, noise=0: 0.0] * 2, [[-1.0, 1.0]] * 2, 2.0, grid=(10, 10), candidates=np.zeros((5, 2)))


@pytest.mark.parametrize("cls", [SafeOpt.BO, GoOSE.BO])
def test_candidates_shape_is_checked_and_kept(cls):
    with pytest.raises(ValueError):
        cls([lambda x, noise=0: 0.0] * 2, [[-1.0, 1.0]] * 2, 2.0, candidates=np.zeros((5, 3)))
    pts = np.random.default_rng(0).uniform(-1, 1, size=(7, 2))
    m = cls([lambda x, noise=0: 0.0] * 2, [[-1.0, 1.0]] * 2, 2.0, candidates=pts, list_index=1)
    assert m.grid is None and m.candidates.shape == (7, 2) and m.list_index == 1
    assert np.array_equal(m._grid_point(3), pts[3])
