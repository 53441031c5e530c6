"""GPU tests of the head of a lean-2 column-path sweep (option k1_sched; csrc/bilinear_post.inc.hpp: k_bl_sched_tiles1): the
constraint's tile list is appended by the classifying kernel itself -- sharded, two ends per shard, counters bumped by atomics and
reset by k_bl_sched_list2 for the next sweep.  tests/test_gpu_k1sched.py stays the bit-for-bit yardstick of k1_sched 1 against 0;
here are the cases that list can get wrong: a classifier workgroup with idle waves, empty ends, counters that survive a sweep, an
error between sweeps, many workgroups racing for both ends.  test_no_stale_M_bits is a regression test of code this change leaves
alone (k_col_a clears the M words, the minimiser's M part waits for its event): it pins down what any later move of that clear to
another stream has to keep.

The b values and windows are chosen with the oracle on the CPU (and asserted there), so that the tile populations named in each test
occur: a tile (64 rows x 128 columns) with lcb_1 >= 0 somewhere cannot be skipped, a tile the device skips has lcb_1 < 0 everywhere."""
import numpy as np
import pytest

import oracle
from safebo_amd import synthetic
from safebo_amd._lib import EmptySafeSetError

pytestmark = pytest.mark.gpu

# a window of config H's box in which every tile of a 384 x 192 grid holds a safe candidate at small b
WIN_LO, WIN_HI = np.array([0.2, -1.0]), np.array([1.5, -0.2])


def _masks(eng):
    return {"S": eng.mask("S"), "U": eng.mask("U"), "M": eng.mask("M"), "G": eng.mask("G", 1)}


def _step(engine, b, lean):
    """One SafeOpt sweep: (result, masks, k1_tiles_skipped).  A sweep that finds no safe candidate runs to its end and then raises:
    its record is ("empty", message) with the masks and the skip count it left."""
    try:
        res = engine.sweep_safeopt(b, want_masks=True, lean=lean)
    except EmptySafeSetError as exc:
        res = ("empty", str(exc))
    return res, _masks(engine), engine.profile()["k1_tiles_skipped"]


def _plan(engine, lo, hi, count, cfg):
    """A new plan, swept twice at lean 0: the second sweep runs K1b and records the enclosures the skips rest on."""
    engine.set_grid(lo, hi, count)
    engine.set_model(cfg["ds"], dtype="f64")
    return [_step(engine, cfg["b"], 0) for _ in range(2)]


def _run(engine, sched, lo, hi, count, cfg, sweeps):
    engine.set_option("k1_sched", sched)
    return _plan(engine, lo, hi, count, cfg) + [_step(engine, b, lean) for b, lean in sweeps]


def _same_rec(a, b, what=""):
    (ra, ma, sa), (rb, mb, sb) = a, b
    assert sa == sb, (what, sa, sb)
    if isinstance(ra, tuple) or isinstance(rb, tuple):
        assert ra == rb, (what, ra, rb)
    else:
        assert ra.keys() == rb.keys()
        for k in ra:
            np.testing.assert_array_equal(np.asarray(ra[k]), np.asarray(rb[k]), err_msg=f"{what}: {k}")
    assert ma.keys() == mb.keys()
    for k in ma:
        assert np.array_equal(ma[k], mb[k]), (what, k)


def _ab(engine, lo, hi, count, cfg, sweeps):
    """The same sweeps with the tile lists and without, bit for bit; returns the records of the run with lists (plan sweeps dropped)."""
    a = _run(engine, 1, lo, hi, count, cfg, sweeps)
    b = _run(engine, 0, lo, hi, count, cfg, sweeps)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        _same_rec(x, y, f"sweep {i}")
    return a[2:]


@pytest.fixture
def colpath(engine):
    engine.set_option("fuse_classify", 1)
    engine.set_option("col_path", 2)
    yield engine
    engine.set_option("k1_sched", 1)
    engine.set_option("col_overlap", 1)
    engine.set_option("fuse_classify", -1)
    engine.set_option("col_path", 1)


@pytest.fixture(scope="module")
def cfg():
    return synthetic.make_config("H", n=96)


_POST = {}


def _posterior(cfg, lo, hi, count):
    """The oracle's posterior on a grid, computed once per grid and left unchanged."""
    key = (tuple(lo), tuple(hi), tuple(count))
    if key not in _POST:
        mean, var = oracle.gp_inference(oracle.grid_points(lo, hi, count), cfg["ds"])
        mean.setflags(write=False)
        var.setflags(write=False)
        _POST[key] = (mean, var)
    return _POST[key]


def _tiles(x, count):
    """[tile rows][64][tiles per row][128] view of a flat per-candidate array (axis 0 fastest)."""
    W, H = count
    return np.asarray(x).reshape(H // 64, 64, W // 128, 128)


def _cpu(cfg, lo, hi, count, b):
    """Per tile at this b: does it hold a safe candidate; its count of M bits; and the M mask itself (None without a safe candidate)."""
    mean, var = _posterior(cfg, lo, hi, count)
    lcb, ucb = oracle.bounds(mean, var, b)
    S = lcb[:, 1] >= 0
    M = (S & (lcb[:, 0] <= np.min(ucb[S, 0]))) if S.any() else None
    has_S = _tiles(S, count).any(axis=(1, 3))
    n_M = _tiles(M, count).sum(axis=(1, 3)) if M is not None else np.zeros_like(has_S, dtype=np.int64)
    return has_S, n_M, M


def test_last_classifier_workgroup_has_idle_waves(colpath, cfg):
    """3 x 3 tiles: the classifier's second workgroup has one live wave.  b from "every tile holds a safe candidate" (nothing skipped, and
    the tile with the largest gradient is evaluated: the front of the list holds an evaluated tile) to "no safe candidate at all" (every
    tile skipped, every end of the list empty, the sweep raises), and a sweep behind that one (the counters after a sweep that found
    nothing)."""
    count = [384, 192]
    bs = (0.25, 2.0, 4.0, 6.0, 8.0, 64.0, 6.0)
    holds = [int(_cpu(cfg, WIN_LO, WIN_HI, count, b)[0].sum()) for b in bs]
    assert holds[0] == 9 and holds[5] == 0 and any(0 < h < 9 for h in holds), holds
    recs = _ab(colpath, WIN_LO, WIN_HI, count, cfg, [(b, 2) for b in bs])
    skipped = [r[2] for r in recs]
    print("tiles with a safe candidate (oracle)", holds, "tiles skipped (device)", skipped)
    assert skipped[0] == 0, skipped
    for i, (h, s, r) in enumerate(zip(holds, skipped, recs)):
        assert isinstance(r[0], tuple) == (i == 5), (i, r[0])
        assert 0 <= s <= 9 - h, (holds, skipped)
    res, masks, s_none = recs[5]
    assert res[0] == "empty" and s_none == 9, (res, s_none)
    assert not masks["S"].any() and masks["U"].all() and not masks["M"].any() and not masks["G"].any()
    assert any(0 < s < 9 for s in skipped), skipped
    _same_rec(recs[6], recs[3], "the sweep behind the empty one")


def test_counters_are_reset_between_sweeps(colpath, cfg):
    """One plan, the same b twelve times: a counter that kept a count would lengthen the list (or shift its back end) from the second
    sweep on.  Then a sweep without lists, one with; a lean-0 sweep, a lean-2 one."""
    count = [384, 192]
    b = 6.0
    assert 0 < int(_cpu(cfg, WIN_LO, WIN_HI, count, b)[0].sum()) < 9
    colpath.set_option("k1_sched", 1)
    _plan(colpath, WIN_LO, WIN_HI, count, cfg)
    first = _step(colpath, b, 2)
    assert not isinstance(first[0], tuple) and 0 < first[2] < 9, first[2]
    for i in range(11):
        _same_rec(_step(colpath, b, 2), first, f"repeat {i + 1}")
    colpath.set_option("k1_sched", 0)
    _same_rec(_step(colpath, b, 2), first, "without lists")
    colpath.set_option("k1_sched", 1)
    _same_rec(_step(colpath, b, 2), first, "with lists again")
    r0 = _step(colpath, b, 0)
    assert not isinstance(r0[0], tuple)
    _same_rec(_step(colpath, b, 2), first, "behind a lean-0 sweep")


def test_error_between_sweeps(colpath, cfg):
    """A sweep the ABI refuses (b < 0) between two lean-2 sweeps: the second equals the first."""
    count = [384, 192]
    b = 6.0
    colpath.set_option("k1_sched", 1)
    _plan(colpath, WIN_LO, WIN_HI, count, cfg)
    first = _step(colpath, b, 2)
    assert not isinstance(first[0], tuple) and 0 < first[2] < 9, first[2]
    with pytest.raises(ValueError):
        colpath.sweep_safeopt(-1.0, want_masks=True, lean=2)
    _same_rec(_step(colpath, b, 2), first, "behind the refused sweep")


def test_many_workgroups_fill_both_ends(colpath, cfg):
    """8 x 8 tiles, 16 classifier workgroups appending at once.  On config H's box the tile with the constraint's largest gradient holds
    no safe candidate at these b (skipped, but it runs the gradient phases: a front entry with bit 31), and the tiles with a safe
    candidate have gradients below half the maximum (evaluated without gradient phases: back entries)."""
    lo, hi = cfg["bound"][:, 0], cfg["bound"][:, 1]
    count = [1024, 512]
    bs = (1.0, 3.0, 6.0)
    g = _tiles(oracle.mean_grad_infnorm(oracle.grid_points(lo, hi, count), cfg["ds"])[:, 1], count).max(axis=(1, 3))
    top = np.unravel_index(int(np.argmax(g)), g.shape)
    for b in bs:
        has_S = _cpu(cfg, lo, hi, count, b)[0]
        assert not has_S[top] and 2 <= int(has_S.sum()) < 62 and np.all(g[has_S] < 0.5 * g.max()), (b, has_S.sum())
    recs = _ab(colpath, lo, hi, count, cfg, [(b, 2) for b in bs])
    for r in recs:
        assert not isinstance(r[0], tuple) and 0 < r[2] < 64, r[2]
        assert len(np.asarray(r[0]["L"])) >= 2 and "count_G" in r[0]


@pytest.mark.parametrize("count,b_stale", [([384, 192], 6.0), ([256, 128], 3.0)])
def test_no_stale_M_bits(colpath, cfg, count, b_stale):
    """A sweep with a large M region, then one at a b for which a tile that held M bits has no safe candidate: the minimiser's M part does
    not visit that tile, so its M words are zero only if THIS sweep cleared them.  Lean 0, 1 and 2; with the tile lists, without, and with
    every kernel on the main stream."""
    lo, hi = cfg["bound"][:, 0], cfg["bound"][:, 1]
    b_big = 2.0
    _, nM_big, _ = _cpu(cfg, lo, hi, count, b_big)
    has_S, _, M_ref = _cpu(cfg, lo, hi, count, b_stale)
    gone = (nM_big > 0) & ~has_S
    assert gone.any() and M_ref is not None and M_ref.any(), (nM_big, has_S)
    rows, cols = gone.nonzero()
    got = {}
    for sched, overlap in ((1, 1), (0, 1), (1, 0)):
        colpath.set_option("k1_sched", sched)
        colpath.set_option("col_overlap", overlap)
        _plan(colpath, lo, hi, count, cfg)
        for lean in (0, 1, 2):
            big = _step(colpath, b_big, lean)
            assert not isinstance(big[0], tuple) and _tiles(big[1]["M"], count)[rows, :, cols, :].any(), big[0]
            res, masks, _ = _step(colpath, b_stale, lean)
            assert not isinstance(res, tuple), res
            got[(sched, overlap, lean)] = masks["M"]
            assert res["count_M"] == int(masks["M"].sum())
    ref = got[(1, 1, 2)]
    assert not _tiles(ref, count)[rows, :, cols, :].any()
    for k, m in got.items():
        assert np.array_equal(m, ref), k
    if count == [256, 128]:
        assert np.array_equal(ref, M_ref)
