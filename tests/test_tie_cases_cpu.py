"""What the constructions of tests/tie_cases.py promise, asserted with NumPy: a construction that loses its property fails here,
before a GPU is involved."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle  # noqa: E402
import robust_oracle  # noqa: E402
import tie_cases as tc  # noqa: E402

B = 2.0
TR_X0, TR_R = np.array([0.25, 0.0]), 0.75


@pytest.mark.parametrize("name", sorted(tc.MIRROR_GRIDS))
def test_mirror_grids_are_bitwise_symmetric_in_the_last_axis(name):
    lo, hi, count = tc.mirror_grid(name)
    axes = oracle.grid_axes(lo, hi, count)
    assert np.array_equal(axes[-1], -axes[-1][::-1])
    if int(np.prod(count)) <= 1 << 21:
        pts = oracle.grid_points(lo, hi, count)
        idx = np.arange(pts.shape[0])
        partner = tc.mirror_partner(idx, count)
        assert np.array_equal(pts[partner, :-1], pts[:, :-1]) and np.array_equal(pts[partner, -1], -pts[:, -1])
        assert np.array_equal(tc.mirror_partner(partner, count), idx)
    # the steps are dyadic: lo + i * step is exact, which is how the device forms the coordinates too
    for ax in axes:
        step = ax[1] - ax[0]
        assert np.log2(step) == np.round(np.log2(step)) and np.array_equal(ax, ax[0] + np.arange(ax.size) * step)


@pytest.mark.parametrize("d,axis", [(2, 1), (2, 0), (3, 2)])
def test_mirror_model_observations_lie_on_the_mirror_plane(d, axis):
    ds = tc.mirror_model(q=3, d=d, axis=axis, n=30)
    assert not ds["X_norm"][:, axis].any() and ds["X_mean"][axis] == 0.0 and ds["X_std"][axis] == 1.0
    assert ds["hypopt"].shape == (d + 2, 3) and len(ds["invKopt"]) == 3
    same = tc.mirror_model(q=3, d=d, axis=axis, n=30, same_constraints=True)
    assert np.array_equal(same["Y_norm"][:, 1], same["Y_norm"][:, 2]) and np.array_equal(same["invKopt"][1], same["invKopt"][2])
    assert same["Y_mean"][1] == same["Y_mean"][2] and same["Y_std"][1] == same["Y_std"][2]


def _sym_sweeps(ds, grid, b, x0=TR_X0):
    lo, hi, count = tc.mirror_grid(grid)
    pts = oracle.grid_points(lo, hi, count)
    mean, var = oracle.gp_inference(pts, ds)
    # the oracle's own posterior is symmetric to rounding only; the symmetrised one is what a per-candidate kernel returns
    ys = ds["Y_std"]
    ms, vs = tc.symmetrise(mean, var, count)
    assert np.max(np.abs(ms - mean) / ys) < 1e-12 and np.max(np.abs(vs - var) / ys ** 2) < 1e-12
    mv = (ms, vs)
    return pts, count, mv, oracle.safeopt_sweep(pts, ds, b, mean_var=mv), oracle.goose_sweep(pts, ds, b, mean_var=mv), \
        oracle.tr_sweep(pts, ds, b, x0, TR_R, mean_var=mv)


def _assert_tie(values, mask, winner, count, worlds=()):
    t = tc.tied(values, mask, winner)
    assert t.size >= 2 and winner == t[0], (winner, t)
    assert int(tc.mirror_partner(winner, count)) in t
    for w in worlds:
        assert len({tc.rank_of(i, count, w) for i in t}) >= 2, (w, t)


@pytest.mark.parametrize("grid,q,same,worlds", [("small", 2, False, ()), ("even", 3, False, ()), ("small", 3, True, ()), ("even", 2, False, ()),
                                                 ("tiles", 2, False, ()), ("planes33", 3, False, (2, 3)), ("planes33", 2, False, (2, 3))])
def test_mirror_model_ties_every_reduction(grid, q, same, worlds):
    """On the symmetrised oracle posterior the minimiser, every expander, the safe minimum, every target and the trust-region
    winner are tied with their mirror partners, which sit in other shards for the world sizes the GPU test uses."""
    ds = tc.mirror_model(q=q, same_constraints=same)
    pts, count, (mean, var), s, g, t = _sym_sweeps(ds, grid, B)
    var0, lcb0 = var[:, 0], s["lcb"][:, 0]
    assert s["S"].any() and s["U"].any() and s["M"].sum() >= 2
    _assert_tie(var0, s["M"], s["minimizer_index"], count, worlds)
    for c in range(1, q):
        assert s["G"][c - 1].any() and g["O"][c - 1].any()
        _assert_tie(var0, s["G"][c - 1], int(s["expander_index"][c - 1]), count, worlds)
        _assert_tie(lcb0, g["O"][c - 1], int(g["target_index_c"][c - 1]), count, worlds)
    _assert_tie(lcb0, s["S"], g["safe_min_index"], count, worlds)
    _assert_tie(lcb0, t["T"], t["index"], count, worlds)
    assert t["T"].sum() < s["S"].sum()
    if same:
        assert np.array_equal(s["G"][0], s["G"][1]) and s["expander_index"][0] == s["expander_index"][1] and s["expander_best"] == 1
        assert np.array_equal(g["O"][0], g["O"][1]) and g["target_index_c"][0] == g["target_index_c"][1] and g["target_best"] == 1
    if grid == "small" and q == 2:
        # the numbers this construction was designed on
        assert (s["minimizer_index"], int(tc.mirror_partner(96, count))) == (96, 2046)
        assert (s["S"].sum(), s["U"].sum(), s["M"].sum(), s["G"][0].sum()) == (1097, 1048, 352, 580)


def test_mirror_model_3d_small_ties():
    ds = tc.mirror_model(q=2, d=3, n=40)
    pts, count, (mean, var), s, g, t = _sym_sweeps(ds, "cube_small", B, x0=np.array([0.25, 0.0, 0.0]))
    _assert_tie(var[:, 0], s["M"], s["minimizer_index"], count)
    _assert_tie(s["lcb"][:, 0], s["S"], g["safe_min_index"], count)
    _assert_tie(s["lcb"][:, 0], t["T"], t["index"], count)
    assert s["U"].any()


def test_b_zero_makes_m_a_tie_set():
    ds = tc.mirror_model(q=2)
    pts, count, (mean, var), s, g, t = _sym_sweeps(ds, "even", 0.0)
    M = s["M"]
    assert M.sum() >= 2 and M.sum() % 2 == 0 and np.all(mean[M, 0] == s["u_star"])
    _assert_tie(var[:, 0], M, s["minimizer_index"], count)
    _assert_tie(s["lcb"][:, 0], s["S"], g["safe_min_index"], count)
    _assert_tie(s["lcb"][:, 0], t["T"], t["index"], count)


@pytest.mark.parametrize("axis", [1, 0])
@pytest.mark.parametrize("kind", ["ucb", "mean"])
def test_robust_mirror_ties(axis, kind):
    """Mirrored in the disturbance axis: the worst disturbance ties; mirrored in the control axis: the robust control ties."""
    ds = tc.mirror_model(q=2, axis=axis)
    lo, hi, count = tc.robust_mirror_grid(axis)
    pts = oracle.grid_points(lo, hi, count)
    mean, var = robust_oracle.gp_inference_prior(pts, ds, np.zeros(2))
    nc, nd = count
    if axis == 1:
        mean, var = tc.symmetrise(mean, var, count)
    else:
        M, V = mean.reshape(nd, nc, 2).copy(), var.reshape(nd, nc, 2).copy()
        M[:, nc - nc // 2:] = M[:, :nc // 2][:, ::-1]
        V[:, nc - nc // 2:] = V[:, :nc // 2][:, ::-1]
        mean, var = M.reshape(-1, 2), V.reshape(-1, 2)
    r = robust_oracle.robust_from_posterior(mean, var, nc, B, kind)
    assert r["index"] >= 0 and 0 < r["count_safe"] < nc
    f_all = robust_oracle.bound_of(mean[:, 0], var[:, 0], B, kind).reshape(nd, nc)
    if axis == 1:
        t = np.flatnonzero(f_all[:, r["index"]] == r["value"])
        assert t.size >= 2 and t[0] == r["worst_d_index"] and nd - 1 - t[0] in t
        for w in (2, 3):
            assert len({tc.rank_of(int(j) * nc, [nc, nd], w) for j in t}) >= 2
    else:
        t = np.flatnonzero(r["safe"] & (r["f"] == r["value"]))
        assert t.size >= 2 and t[0] == r["index"] and nc - 1 - t[0] in t


def test_plane_shards_cover_the_grid_unevenly():
    assert tc.plane_shards([64, 33], 2) == [(0, 16), (16, 33)] and tc.plane_shards([64, 33], 3) == [(0, 11), (11, 22), (22, 33)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_duplicate_list_repeats_every_point_below_and_above(dtype):
    pts, origin = tc.duplicate_list([-1.0, 0.0], [2.0, 3.0], dtype=dtype)
    assert pts.dtype == dtype and pts.shape == (2100, 2)
    m = 700
    for g in (0, 17, 699):
        pos = np.flatnonzero(origin == g)
        assert pos.size == 3 and pos[0] < m <= pos[1] < 2 * m <= pos[2]
        assert np.array_equal(pts[pos[0]], pts[pos[1]]) and np.array_equal(pts[pos[1]], pts[pos[2]])
    # scattered: the repeats are not in the order of the first segment
    assert not np.array_equal(origin[:m], origin[m:2 * m]) and not np.array_equal(origin[m:2 * m], origin[2 * m:])
    assert np.unique(pts, axis=0).shape[0] == m


def test_cell_targets_tie_the_corners():
    lo, hi, count, targets = tc.cell_targets()
    pts = oracle.grid_points(lo, hi, count)
    S = np.ones(pts.shape[0], dtype=bool)
    sizes = {}
    for name, (t, nearest) in targets.items():
        want, dist = tc.nearest_in(pts, S, t)
        tied = np.flatnonzero(dist == dist[want]).tolist()
        assert tied == nearest and want == nearest[0], (name, tied, nearest)
        sizes[name] = len(tied)
    assert sizes == {"centre": 4, "edge_x": 2, "edge_y": 2, "point": 1}


def test_corner_model_leaves_the_lowest_tied_corners_unsafe():
    lo, hi, count, targets = tc.cell_targets()
    pts = oracle.grid_points(lo, hi, count)
    ds = tc.corner_model()
    mean, var = oracle.gp_inference(pts, ds)
    m32, v32 = oracle.gp_inference(pts, ds, dtype=np.float32)
    t, nearest = targets["centre"]
    for i, safe in zip(nearest, (False, True, False, True)):
        # decided with a margin no posterior kernel's rounding (fp32 included) can cross
        assert (mean[i, 1] >= 0) == safe and abs(mean[i, 1]) > 1e-3 and (m32[i, 1] >= 0) == safe
    S = mean[:, 1] >= 0
    want, dist = tc.nearest_in(pts, S, t)
    assert np.flatnonzero(S & (dist == dist[want])).tolist() == [nearest[1], nearest[3]] and want == nearest[1]


def test_sphere_points_are_on_the_sphere():
    lo, hi, count, x0, r, r_below, on = tc.sphere_case()
    pts = oracle.grid_points(lo, hi, count)
    assert np.array_equal(pts[16 * 33 + 16], x0) and r == 5 * 2.0 ** -5 and r_below < r
    dist = np.sqrt(((pts - x0) ** 2).sum(axis=1))
    assert np.flatnonzero(dist == r).tolist() == on and len(on) == 12
    assert (dist <= r).sum() - (dist <= r_below).sum() == 12
    # the same in fp32 arithmetic (every coordinate and square is exact in either format)
    d32 = np.sqrt(((pts.astype(np.float32) - x0.astype(np.float32)) ** 2).sum(axis=1))
    assert np.flatnonzero(d32 == np.float32(r)).tolist() == on


def test_fp32_near_tie_flips_the_arg_min_under_float_rounding():
    pts, target, near, far = tc.near_tie_list()
    d = np.sqrt(((pts - target) ** 2).sum(axis=1))
    assert int(np.argmin(d)) == near == pts.shape[0] - 1 and int(np.argmin(d.astype(np.float32))) == far == 0
    assert np.sort(d)[2] >= 1.5
    lo, hi, count, t, gnear, gfar = tc.near_tie_grid()
    gp = oracle.grid_points(lo, hi, count)
    d = np.sqrt(((gp - t) ** 2).sum(axis=1))
    assert int(np.argmin(d)) == gnear and int(np.argmin(d.astype(np.float32))) == gfar and gfar < gnear
    assert d[gnear] < d[gfar] and np.float32(d[gnear]) == np.float32(d[gfar])


def test_near_tie_goose_targets_the_origin():
    ds, b, pts, t, near, far = tc.near_tie_goose()
    g = oracle.goose_sweep(pts, ds, b)
    assert not pts[t].any() and g["U"].sum() == 1 and g["U"][t] and g["S"].sum() == pts.shape[0] - 1
    assert g["target_index"] == t and g["explore_index"] == near
    d = np.sqrt(((pts - pts[t]) ** 2).sum(axis=1))
    assert int(np.argmin(np.where(g["S"], d.astype(np.float32), np.inf))) == far
    # the classification is decided with a margin fp32 posteriors keep
    assert g["lcb"][g["S"], 1].min() > 0.1 and g["lcb"][t, 1] < -0.1
