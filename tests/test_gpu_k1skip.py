"""GPU tests of the constraint tiles a lean sweep leaves unevaluated (r06, csrc/bilinear.hip: k_bl_enclose / encl_unsafe): from a
plan's second K1b sweep on, a lean = 2 column-path sweep skips the constraint's posterior on 64 x 128 tiles whose per-cell enclosures
prove every candidate unsafe and outside the guard band.  Masks, counts, indices, u* and L[1] must stay bit-identical to a full
sweep's and equal the oracle's; the posterior asked for afterwards is complete; the audit checks samples on skipped tiles against the
enclosure."""
import numpy as np
import pytest

import oracle
from safebo_amd import synthetic

pytestmark = pytest.mark.gpu

KEYS = ("minimizer_index", "expander_index", "expander_best_c", "choose_minimizer", "count_S", "count_U", "count_M", "u_star",
        "minimizer_std", "expander_std")


def _masks(eng):
    return {"S": eng.mask("S"), "U": eng.mask("U"), "M": eng.mask("M"), "G": eng.mask("G", 1)}


def _same(a, b):
    (ra, ma), (rb, mb) = a, b
    for k in KEYS:
        assert ra[k] == rb[k], (k, ra[k], rb[k])
    assert list(ra["count_G"]) == list(rb["count_G"]) and list(ra["expander_index_c"]) == list(rb["expander_index_c"])
    assert ra["L"][1] == rb["L"][1]
    for k in ma:
        assert np.array_equal(ma[k], mb[k]), k


def _check_oracle(res, masks, ref):
    for k in ("S", "U", "M"):
        assert np.array_equal(masks[k], ref[k]), k
    assert np.array_equal(masks["G"], ref["G"][0])
    assert res["minimizer_index"] == ref["minimizer_index"]
    assert list(res["expander_index_c"]) == list(ref["expander_index"])
    assert abs(res["u_star"] - ref["u_star"]) < 1e-10
    assert (res["count_S"], res["count_U"], res["count_M"], res["count_G"][0]) == (ref["S"].sum(), ref["U"].sum(), ref["M"].sum(), ref["G"][0].sum())
    assert np.allclose(res["L"][1:], ref["L"][1:], rtol=1e-9)


def _sweeps(engine, cfg, lo, hi, count, b):
    """K1i (first sweep), K1b full (records the enclosures), then lean 2 and lean 0 on the same plan: (skipped, lean-2 result, lean-0 result)."""
    engine.set_grid(lo, hi, count)
    engine.set_model(cfg["ds"], dtype="f64")
    engine.sweep_safeopt(b, want_masks=True)
    engine.sweep_safeopt(b, want_masks=True)
    assert engine.profile()["posterior_kernel"] == 4
    assert engine.profile()["k1_tiles_skipped"] == 0            # (the plan's first K1b launch evaluates every tile and records them)
    res2 = engine.sweep_safeopt(b, want_masks=True, lean=2)
    prof = engine.profile()
    assert prof["set_path"] == 1 and prof["posterior_kernel"] == 4
    out2 = (res2, _masks(engine))
    res0 = engine.sweep_safeopt(b, want_masks=True, lean=0)
    assert engine.profile()["k1_tiles_skipped"] == 0
    return prof["k1_tiles_skipped"], out2, (res0, _masks(engine))


@pytest.fixture
def colpath(engine):
    engine.set_option("fuse_classify", 1)
    engine.set_option("col_path", 2)
    yield engine
    engine.set_option("fuse_classify", -1)
    engine.set_option("col_path", 1)
    engine.set_option("guard_band", 1)


def test_lean_sweep_skips_unsafe_constraint_tiles(colpath):
    """An H-shaped grid (config H's model, 256 x 128: two of its four tiles hold no safe candidate): some constraint tiles are skipped, the lean-2 result equals lean 0 and the
    oracle bit for bit, and the posterior asked for afterwards (K1 again, in full) matches the oracle."""
    engine = colpath
    cfg = synthetic.make_config("H", n=96)
    lo, hi, count = cfg["bound"][:, 0], cfg["bound"][:, 1], [256, 128]
    ref = oracle.safeopt_sweep(oracle.grid_points(lo, hi, count), cfg["ds"], cfg["b"])
    skipped, lean2, lean0 = _sweeps(engine, cfg, lo, hi, count, cfg["b"])
    assert 0 < skipped <= 2, skipped
    _same(lean2, lean0)
    _check_oracle(*lean2, ref)
    engine.sweep_safeopt(cfg["b"], want_masks=True, lean=2)
    assert engine.profile()["k1_tiles_skipped"] == skipped
    mean, var = engine.posterior()
    ys = np.maximum(1.0, cfg["ds"]["Y_std"])
    assert np.max(np.abs(mean - ref["mean"]) / ys) < 1e-10 and np.max(np.abs(var - ref["var"]) / ys ** 2) < 1e-10


def test_lean_sweep_skips_with_forced_reevaluation(colpath):
    """guard_band = 2: the exact re-evaluation behind a lean-2 first pass that skipped tiles runs K1 in full and returns the oracle's sets."""
    engine = colpath
    cfg = synthetic.make_config("H", n=96)
    lo, hi, count = cfg["bound"][:, 0], cfg["bound"][:, 1], [256, 128]
    ref = oracle.safeopt_sweep(oracle.grid_points(lo, hi, count), cfg["ds"], cfg["b"])
    engine.set_option("guard_band", 2)
    engine.set_grid(lo, hi, count)
    engine.set_model(cfg["ds"], dtype="f64")
    for lean in (0, 0, 2, 2, 0):
        res = engine.sweep_safeopt(cfg["b"], want_masks=True, lean=lean)
        assert res["guard_passes"] >= 1
        _check_oracle(res, _masks(engine), ref)
    # (the profile reports the re-evaluation's pass, so whether these first passes had tiles to skip is seen with the band back on
    # its default -- a new plan: its first K1b sweep records, the next one skips)
    engine.set_option("guard_band", 1)
    for _ in range(3):
        engine.sweep_safeopt(cfg["b"], want_masks=True, lean=2)
    assert engine.profile()["k1_tiles_skipped"] > 0


def test_no_skip_where_every_tile_holds_a_safe_candidate(colpath):
    """A grid inside the safe set: no tile can be skipped (k1_tiles_skipped == 0) and the result is the oracle's."""
    engine = colpath
    cfg = synthetic.make_config("H", n=96)
    lo, hi = cfg["bound"][:, 0], cfg["bound"][:, 1]
    coarse = oracle.grid_points(lo, hi, [64, 64])
    cref = oracle.safeopt_sweep(coarse, cfg["ds"], cfg["b"])
    # a small box around the safe candidate with the largest lcb of the constraint
    mean, var = cref["mean"][:, 1], cref["var"][:, 1]
    c = coarse[int(np.argmax(mean - cfg["b"] * np.sqrt(np.maximum(var, 0.0))))]
    w = 0.002 * (hi - lo)
    lo2, hi2, count = c - w, c + w, [256, 128]
    ref = oracle.safeopt_sweep(oracle.grid_points(lo2, hi2, count), cfg["ds"], cfg["b"])
    assert ref["S"].all()
    skipped, lean2, lean0 = _sweeps(engine, cfg, lo2, hi2, count, cfg["b"])
    assert skipped == 0
    _same(lean2, lean0)
    _check_oracle(*lean2, ref)


def test_audit_checks_samples_on_skipped_tiles(colpath):
    """The standing audit (every sweep, 64 Ki samples) lands samples on skipped tiles: it counts them and finds the exact values inside
    the tiles' enclosures (no violation)."""
    engine = colpath
    cfg = synthetic.make_config("H", n=96)
    lo, hi, count = cfg["bound"][:, 0], cfg["bound"][:, 1], [256, 128]
    engine.set_option("guard_audit", 65536)
    try:
        skipped, lean2, lean0 = _sweeps(engine, cfg, lo, hi, count, cfg["b"])
        assert skipped > 0
        engine.set_option("guard_audit_scale_ppm", 1000000)           # (clears the counts)
        for _ in range(2):
            engine.sweep_safeopt(cfg["b"], want_masks=True, lean=2)
            engine.synchronize()
        p = engine.profile()
        assert p["guard_audit_samples"] >= 65536 and p["guard_audit_skipped"] > 0, p
        assert p["guard_audit_violations"] == 0, p
    finally:
        engine.set_option("guard_audit", 1024)


def test_skip_decisions_across_b(colpath):
    """The same plan swept at several b (guard band in force): as b grows, tiles near the boundary change between evaluated and
    skipped.  At every b the lean-2 sweep equals the lean-0 sweep bit for bit, and it never skips more tiles than hold no safe candidate."""
    engine = colpath
    cfg = synthetic.make_config("H", n=96)
    lo, hi, count = cfg["bound"][:, 0], cfg["bound"][:, 1], [256, 128]
    _sweeps(engine, cfg, lo, hi, count, cfg["b"])
    skips = {}
    for b in (1.0, 3.0, 4.0, 8.0, 3.0):
        res2 = engine.sweep_safeopt(b, want_masks=True, lean=2)
        skipped = engine.profile()["k1_tiles_skipped"]
        lean2 = (res2, _masks(engine))
        res0 = engine.sweep_safeopt(b, want_masks=True, lean=0)
        lean0 = (res0, _masks(engine))
        _same(lean2, lean0)
        assert res0["guard_band"] == 0
        unsafe = int((~lean0[1]["S"].reshape(count[1] // 64, 64, count[0] // 128, 128).any(axis=(1, 3))).sum())
        assert skipped <= unsafe, (b, skipped, unsafe)
        assert skips.setdefault(b, skipped) == skipped                # (the same b on the same plan: the same tiles)
    assert len(set(skips.values())) > 1, skips


def test_audit_after_a_skipping_sweep_and_a_new_plan(colpath):
    """A lean-2 sweep that skipped tiles, then a new grid (more tiles) and model swept by GoOSE (K1i, then K1b on the byte-mask path)
    and a trust-region sweep, all audited: the skip records of the earlier launch are not read again (guard_audit_skipped unchanged)
    and no violation is counted."""
    engine = colpath
    cfg = synthetic.make_config("H", n=96)
    lo, hi = cfg["bound"][:, 0], cfg["bound"][:, 1]
    engine.set_option("guard_audit", 65536)
    try:
        _sweeps(engine, cfg, lo, hi, [256, 128], cfg["b"])
        engine.sweep_safeopt(cfg["b"], want_masks=True, lean=2)
        assert engine.profile()["k1_tiles_skipped"] > 0
        engine.synchronize()
        p0 = engine.profile()
        assert p0["guard_audit_skipped"] > 0 and p0["guard_audit_violations"] == 0, p0
        engine.set_grid(lo, hi, [512, 256])
        engine.set_model(cfg["ds"], dtype="f64")
        engine.sweep_goose(cfg["b"])
        engine.sweep_goose(cfg["b"])
        engine.sweep_tr(cfg["b"], 0.5 * (lo + hi), float(np.max(hi - lo)))
        engine.synchronize()
        p1 = engine.profile()
        assert p1["guard_audit_samples"] > p0["guard_audit_samples"], (p0, p1)
        assert p1["guard_audit_skipped"] == p0["guard_audit_skipped"] and p1["guard_audit_violations"] == 0, p1
    finally:
        engine.set_option("guard_audit", 1024)
