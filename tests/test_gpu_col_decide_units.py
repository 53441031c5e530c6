"""GPU tests of k_col_decide's half-width units (csrc/sets_colpath.inc.hpp): a wave takes (tile with a safe candidate, octet, 64-column
half), one column per lane, and queues its open candidates in 128 LDS entries (option col_queue: 64 forces a flush before every
append).  Modelled on tests/test_gpu_k1sched_head.py: column path forced, config H with n = 96, populations picked and asserted with
the oracle on the CPU (tests/test_col_decide_units_cpu.py holds the cases and asserts them without a GPU), masks and results against
oracle.safeopt_sweep bit for bit, everything with the expander chain on its own stream (col_overlap 1) and on the main stream (0).

[128, 64] is a single tile, the smallest grid at which unit indexing can go wrong; it meets the CPU assertions of tests 1, 2 and 4.

The two boundary cases on the window (0.2, -1.0) .. (1.5, -0.2) at b = 0.25 -- nearly every candidate safe, U a small corner -- are
also the regression test of the row search (col_row_search): with no U point inside a candidate's cap its running minimum is +inf,
and a block marked "not to be searched" by a large finite bound was searched all the same -- on rows of fewer than 128 blocks that is
the next rows of the image, whose U points made 480 ([128, 64]) and 897 ([256, 128]) candidates along the right edge members of G_1.
Such blocks carry +inf now."""
import numpy as np
import pytest

from test_col_decide_units_cpu import (BOUNDARY, EMPTY_HALF, LEAN, ROWS, config, half_counts, listed, mixed_octets, reference, units,
                                       window)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cfg():
    return config()


@pytest.fixture(params=[0, 1], ids=["one_stream", "overlap"])
def colpath(engine, request):
    engine.set_option("fuse_classify", 1)
    engine.set_option("col_path", 2)
    engine.set_option("col_overlap", request.param)
    yield engine
    engine.set_option("col_queue", 128)
    engine.set_option("col_overlap", 1)
    engine.set_option("fuse_classify", -1)
    engine.set_option("col_path", 1)


def _masks(eng):
    return {"S": eng.mask("S"), "U": eng.mask("U"), "M": eng.mask("M"), "G": eng.mask("G", 1)}


def _model(engine, cfg, win, count):
    lo, hi = window(cfg, win)
    engine.set_grid(lo, hi, list(count))
    engine.set_model(cfg["ds"], dtype="f64")


def _sweep(engine, b, lean, ref):
    """One SafeOpt sweep on the column path, checked against the oracle: (result, masks)."""
    res = engine.sweep_safeopt(b, want_masks=True, lean=lean)
    assert engine.profile()["set_path"] == 1
    masks = _masks(engine)
    for k in ("S", "U", "M"):
        assert np.array_equal(masks[k], ref[k]), k
    bad = np.flatnonzero(masks["G"] != ref["G"][0])
    assert bad.size == 0, ("G", bad.size, bad[:8].tolist(), masks["G"][bad[:8]].tolist())
    assert res["minimizer_index"] == ref["minimizer_index"]
    assert list(res["expander_index_c"]) == list(ref["expander_index"])
    assert (res["count_S"], res["count_U"], res["count_M"], res["count_G"][0]) == (ref["S"].sum(), ref["U"].sum(), ref["M"].sum(), ref["G"][0].sum())
    assert res["choose_minimizer"] == ref["choose_minimizer"]
    assert res["guard_band"] == 0
    return res, masks


def _same(a, b, what, skip=()):
    (ra, ma), (rb, mb) = a, b
    assert ra.keys() == rb.keys()
    for k in ra:
        if k not in skip:
            np.testing.assert_array_equal(np.asarray(ra[k]), np.asarray(rb[k]), err_msg=f"{what}: {k}")
    for k in ma:
        assert np.array_equal(ma[k], mb[k]), (what, k)


@pytest.mark.parametrize("win,count,b", BOUNDARY)
def test_boundary_inside_a_tile(colpath, cfg, win, count, b):
    """The boundary of G_1 crosses column 64 of a tile: both half-width units of an octet hold members and non-members of G_1, so both
    take the per-candidate path.  A model's first sweep (K1i), its second (K1b), and a lean-2 one."""
    ref = reference(cfg, win, count, b)
    assert len(mixed_octets(ref, count)) >= 1
    _model(colpath, cfg, win, count)
    for lean in (0, 0, 2):
        _sweep(colpath, b, lean, ref)


@pytest.mark.parametrize("win,count,b_sparse,b_dense,where", EMPTY_HALF)
def test_half_without_safe_candidates(colpath, cfg, win, count, b_sparse, b_dense, where):
    """A listed tile whose safe candidates all lie in one 64-column half: the other half-unit writes zero G bytes.  Then the same engine
    at a b where that half holds safe candidates (and members of G_1), and back: no G byte survives a sweep."""
    r, t, h = where
    sparse, dense = reference(cfg, win, count, b_sparse), reference(cfg, win, count, b_dense)
    assert half_counts(sparse["S"], count)[r, t, h] == 0 and half_counts(sparse["S"], count)[r, t, 1 - h] > 0
    assert half_counts(dense["G"][0], count)[r, t, h] > 0
    _model(colpath, cfg, win, count)
    _sweep(colpath, b_sparse, 0, sparse)               # (the model's first sweep runs K1i: the sweeps compared below all run K1b)
    for lean in (0, 2):
        first = _sweep(colpath, b_sparse, lean, sparse)
        assert not units(first[1]["G"], count)[r, :, :, t, h, :].any()
        filled = _sweep(colpath, b_dense, lean, dense)
        assert units(filled[1]["G"], count)[r, :, :, t, h, :].any()
        back = _sweep(colpath, b_sparse, lean, sparse)
        assert not units(back[1]["G"], count)[r, :, :, t, h, :].any()
        _same(back, first, f"lean {lean}: back at b_sparse")


@pytest.mark.parametrize("win,count,b,rows", ROWS)
def test_row_with_one_listed_tile_and_with_all(colpath, cfg, win, count, b, rows):
    """Tile rows that list one tile (at the left end, at the right end) and all of them: the unit map's prefix with the half index at
    both ends of a row mask."""
    ref = reference(cfg, win, count, b)
    assert listed(ref, count).astype(int).tolist() == [list(x) for x in rows]
    _model(colpath, cfg, win, count)
    for lean in (0, 0, 2):
        _sweep(colpath, b, lean, ref)


@pytest.mark.parametrize("win,count,b", BOUNDARY)
def test_forced_flushes(colpath, cfg, win, count, b):
    """col_queue = 64: every append to a wave's queue is preceded by a flush.  Masks, results and count_G equal those of the default
    queue and the oracle's."""
    ref = reference(cfg, win, count, b)
    assert len(mixed_octets(ref, count)) >= 1
    _model(colpath, cfg, win, count)
    _sweep(colpath, b, 0, ref)                         # (K1i; the sweeps compared below all run K1b)
    got = {}
    for q in (64, 128):
        colpath.set_option("col_queue", q)
        got[q] = [_sweep(colpath, b, lean, ref) for lean in (0, 2)]
    for i, (x, y) in enumerate(zip(got[64], got[128])):
        _same(x, y, f"col_queue 64 against 128, sweep {i}")
        assert x[0]["count_G"][0] == y[0]["count_G"][0] == ref["G"][0].sum()


def test_lean_levels_and_both_posterior_kernels(colpath, cfg):
    """The first (K1i) and the second (K1b) sweep of a model at lean 0, 1 and 2: identical results (a lean sweep reports L[0] = 0: no
    sweep reads the objective's Lipschitz key)."""
    win, count, b = LEAN
    ref = reference(cfg, win, count, b)
    got = {}
    for lean in (0, 1, 2):
        _model(colpath, cfg, win, count)
        got[lean] = []
        for sweep in range(2):
            got[lean].append(_sweep(colpath, b, lean, ref))
            assert colpath.profile()["posterior_kernel"] in (4, 6)
    for lean in (1, 2):
        for i in range(2):
            _same(got[lean][i], got[0][i], f"lean {lean} against 0, sweep {i}", skip=("L",))
