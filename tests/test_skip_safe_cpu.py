"""CPU checks of the cases tests/test_gpu_skip_safe.py runs on the device (option k1_skip_safe): the NumPy restatement of encl_safe /
encl_unsafe (tests/skip_safe_cases.py) on the oracle's posterior gives the census of tile classes the cases were chosen for, no cell
of these grids comes within 1e-6 (relative) of either threshold -- the device's enclosures are K1b's values, ~1e-9 from the oracle's, so
its counts must equal the census --, the predicates agree with the candidates' own classification, and the key bounds a proved-safe
tile hands the set phase bracket the true range of ucb_1 over the tile."""
import numpy as np
import pytest

import skip_safe_cases as cases

# (grid, b) -> (proved safe, proved unsafe, evaluated) tiles
CENSUS = {
    (cases.WHOLE, 1.0): (2, 9, 5),
    (cases.WHOLE, 0.25): (2, 9, 5),
    (cases.WHOLE, 3.0): (0, 11, 5),
    (cases.INSIDE, None): (4, 0, 0),
}


def _b(b):
    return cases.config()["b"] if b is None else b


@pytest.mark.parametrize("name,b", list(CENSUS))
def test_census_of_tile_classes(name, b):
    c = cases.census(name, _b(b))
    safe, unsafe = int(c["safe"].sum()), int(c["unsafe"].sum())
    print(f"{name} b={_b(b)}: safe {safe} unsafe {unsafe} evaluated {c['safe'].size - safe - unsafe} margin {c['margin']:.3e}")
    assert not (c["safe"] & c["unsafe"]).any()
    assert (safe, unsafe, c["safe"].size - safe - unsafe) == CENSUS[(name, b)]
    assert c["margin"] > 1e-6, c["margin"]


@pytest.mark.parametrize("name,b", list(CENSUS))
def test_proved_tiles_agree_with_the_candidates(name, b):
    """Every candidate of a proved-safe tile is in S and none in U; of a proved-unsafe tile every one is in U and none in S."""
    mean, var = cases.posterior(name)
    lcb = mean[:, 1] - _b(b) * np.sqrt(var[:, 1])
    S, U = cases.tiles_of(name, lcb >= 0), cases.tiles_of(name, lcb <= 0)
    c = cases.census(name, _b(b))
    for r, t in zip(*np.nonzero(c["safe"])):
        assert S[r, :, t, :].all() and not U[r, :, t, :].any(), (r, t)
    for r, t in zip(*np.nonzero(c["unsafe"])):
        assert U[r, :, t, :].all() and not S[r, :, t, :].any(), (r, t)


@pytest.mark.parametrize("name,b", list(CENSUS))
def test_key_bounds_bracket_ucb(name, b):
    """Section 3 of the skip: the variance key is the exact minimum over the tile, the radius key an upper bound of max ucb_1, field 0
    a lower bound of min ucb_1 -- on every proved-safe tile."""
    mean, var = cases.posterior(name)
    ucb = cases.tiles_of(name, mean[:, 1] + _b(b) * np.sqrt(var[:, 1]))
    v = cases.tiles_of(name, var[:, 1])
    vmin, up, lo = cases.key_bounds(name, _b(b))
    c = cases.census(name, _b(b))
    for r, t in zip(*np.nonzero(c["safe"])):
        assert vmin[r, t] == v[r, :, t, :].min()
        assert up[r, t] >= ucb[r, :, t, :].max() and lo[r, t] <= ucb[r, :, t, :].min()
        assert lo[r, t] > 0.0


def test_a_proved_safe_tile_runs_gradient_phases_on_the_inside_box():
    """The gradient gate (k_bpost, k_bl_sched_tiles1) keeps every tile whose largest coarse gradient sample + slack reaches the grid's
    largest sample -- the tile that holds the largest sample always passes.  On the inside box all four tiles are proved safe, so the
    tiles the gate keeps are proved-safe tiles that run gradient phases (class 5): that case covers the class, and L[1] of its lean-2
    sweep must equal lean 0's and the oracle's (tests/test_gpu_skip_safe.py)."""
    c = cases.census(cases.INSIDE, cases.config()["b"])
    assert c["safe"].all() and c["safe"].size == 4


@pytest.mark.parametrize("b", cases.GOLDEN_B)
def test_recorded_reference_of_the_whole_domain(b):
    """tests/golden/skip_safe/whole.npz against the oracle, for everything that does not need the expander set (which is why the record
    exists: the oracle takes a minute per b for G on this grid): S, U, u*, M and the minimiser from the oracle's posterior; G within S."""
    ref = cases.reference(cases.WHOLE, b)
    mean, var = cases.posterior(cases.WHOLE)
    s = np.sqrt(var)
    lcb, ucb = mean - b * s, mean + b * s
    S, U = lcb[:, 1] >= 0, lcb[:, 1] <= 0
    assert np.array_equal(ref["S"], S) and np.array_equal(ref["U"], U)
    u_star = ucb[S, 0].min()
    M = S & (lcb[:, 0] <= u_star)
    assert ref["u_star"] == u_star and np.array_equal(ref["M"], M)
    assert ref["minimizer_index"] == int(np.argmax(np.where(M, var[:, 0], -np.inf)))
    assert not (ref["G"][0] & ~S).any() and ref["G"][0].any()
