"""GPU tests of the constraint tiles a lean-2 column-path sweep leaves unevaluated because the plan's enclosures prove them SAFE
(option k1_skip_safe; csrc/bilinear_post.inc.hpp: encl_safe, k_bl_sched_tiles1 classes 4 / 5, k_bpost csafe).  Such a tile gets every
S bit, no U bit, |S| = 8192 and bounds for its keys, and the set phase reads what the plan's recording sweep stored for it -- so masks,
counts, indices, u* and L[1] must equal a lean-0 sweep's and the oracle's bit for bit, the count of such tiles must equal the CPU
census (tests/skip_safe_cases.py; tests/test_skip_safe_cpu.py shows no cell is near a threshold), and whoever else writes the resident
posterior must make the next K1b sweep evaluate and record everything again.

The gradient class (a proved-safe tile that runs gradient phases): on the inside box every tile is proved safe and the gate always
keeps the tile with the grid's largest gradient sample, so that case runs it (tests/test_skip_safe_cpu.py asserts the premise); its
L[1] is compared with lean 0's and the oracle's like every other case's."""
import numpy as np
import pytest

import skip_safe_cases as cases

pytestmark = pytest.mark.gpu

CASES = [(cases.WHOLE, 1.0), (cases.WHOLE, 0.25), (cases.WHOLE, 3.0), (cases.INSIDE, None)]
# (the sweep, comparison and start-up helpers are tests/skip_safe_cases.py's: tests/test_gpu_history.py uses them too)
KEYS = cases.KEYS
_masks, _sweep, _same, _check_oracle, _census, _skips = cases.masks, cases.sweep, cases.same, cases.check_oracle, cases.census_safe, cases.skips
_colpath_options, _start, _fresh = cases.colpath_options, cases.start, cases.fresh


def _b(b):
    return cases.config()["b"] if b is None else b


@pytest.fixture
def colpath(engine):
    _colpath_options(engine)
    yield engine
    engine.set_option("fuse_classify", -1)
    engine.set_option("col_path", 1)
    engine.set_option("k1_skip_safe", 1)
    engine.set_option("k1_sched", 1)
    engine.set_option("bilinear", 1)
    engine.set_option("guard_audit", 1024)


@pytest.mark.parametrize("name,b", CASES)
def test_lean_levels_and_oracle(colpath, name, b):
    """K1i, K1b (records), lean 2, lean 0: lean 2 == lean 0 == the oracle; the proved-safe and proved-unsafe tile counts are the CPU
    census's, and the unsafe count does not depend on the option.  On the inside box every tile is proved safe (the constraint's launch
    has gradient tiles only), the objective still takes all four tiles (|S| = the grid, M and the minimiser the oracle's)."""
    eng, b = colpath, _b(b)
    ref = cases.reference(name, b)
    _start(eng, name, b)
    lean2 = _sweep(eng, b, 2)
    prof = eng.profile()
    assert prof["set_path"] == 1 and prof["posterior_kernel"] == 4
    safe, unsafe = _skips(eng)
    lean0 = _sweep(eng, b, 0)
    assert _skips(eng) == (0, 0)
    print(f"{name} b={b}: k1_tiles_skipped_safe {safe}, k1_tiles_skipped {unsafe}, census {_census(name, b)}")
    assert safe == _census(name, b)
    _same(lean2, lean0)
    _check_oracle(*lean2, ref)
    _same(lean2, _fresh(name, b))
    eng.set_option("k1_skip_safe", 0)
    off = _sweep(eng, b, 2)
    assert _skips(eng) == (0, unsafe)
    _same(off, lean0)
    if name == cases.INSIDE:
        assert safe == 4 and lean2[0]["count_S"] == ref["S"].size


def test_option_on_against_off(colpath):
    """k1_skip_safe 1 / 0 and k1_sched 1 / 0 on one engine (the unlisted launch takes the same decision in the kernel): results and
    all four masks identical, the same tiles skipped."""
    eng, name, b = colpath, cases.WHOLE, 1.0
    _start(eng, name, b)
    outs, unsafe = [], None
    for skip_safe in (1, 0, 1):
        for sched in (1, 0):
            eng.set_option("k1_skip_safe", skip_safe)
            eng.set_option("k1_sched", sched)
            outs.append(_sweep(eng, b, 2))
            unsafe = _skips(eng)[1] if unsafe is None else unsafe
            assert unsafe > 0 and _skips(eng) == (_census(name, b) if skip_safe else 0, unsafe), (skip_safe, sched, _skips(eng))
    for o in outs[1:]:
        _same(outs[0], o)
    _check_oracle(*outs[0], cases.reference(name, b))


def test_changing_b(colpath):
    """b walks 3.0 -> 1.0 -> 0.25 -> 3.0 on one plan: the classes change between sweeps (no proved-safe tile at 3.0, two below), every
    sweep equals a fresh engine's."""
    eng, name = colpath, cases.WHOLE
    _start(eng, name, 3.0)
    seen = []
    for b in (3.0, 1.0, 0.25, 3.0):
        out = _sweep(eng, b, 2)
        assert _skips(eng)[0] == _census(name, b), (b, _skips(eng))
        seen.append(_skips(eng)[0])
        _same(out, _fresh(name, b))
    assert seen == [0, 2, 2, 0]


def _foreign_k1g(eng, name, b):
    eng.set_option("bilinear", 0)
    eng.sweep_safeopt(b, want_masks=True)
    assert eng.profile()["posterior_kernel"] == 3
    eng.set_option("bilinear", 1)


def _foreign_posterior(eng, name, b):
    mean, var = eng.posterior()
    assert np.isfinite(mean).all() and np.isfinite(var).all()


def _foreign_roundtrip(eng, name, b):
    lo, hi, count = cases.grid(name)
    eng.set_model(cases.config()["ds"], dtype="f64")
    eng.set_grid(lo, hi, list(count))


@pytest.mark.parametrize("foreign", [_foreign_k1g, _foreign_posterior, _foreign_roundtrip])
def test_foreign_writers(colpath, foreign):
    """Somebody else writes the resident posterior behind a sweep that skipped proved-safe tiles -- a K1g sweep (`bilinear` off and on
    again), engine.posterior() (K1 in full, not on the column path), a set_model / set_grid round trip --: the first K1b sweep after
    it skips nothing of either kind (it evaluates, stores and records again), the one after skips what the census says, and every
    lean-2 sweep equals a fresh engine's bit for bit."""
    eng, name, b = colpath, cases.WHOLE, 1.0
    _start(eng, name, b)
    _same(_sweep(eng, b, 2), _fresh(name, b))
    assert _skips(eng)[0] == _census(name, b) and _skips(eng)[1] > 0
    foreign(eng, name, b)
    for _ in range(3):                       # (a new model's first sweep runs K1i: not the plan's)
        out = _sweep(eng, b, 2)
        if eng.profile()["posterior_kernel"] == 4:
            _same(out, _fresh(name, b))
            break
    assert eng.profile()["posterior_kernel"] == 4 and _skips(eng) == (0, 0), _skips(eng)
    _same(_sweep(eng, b, 2), _fresh(name, b))
    assert _skips(eng)[0] == _census(name, b) and _skips(eng)[1] > 0


@pytest.mark.parametrize("name,b", [(cases.WHOLE, 1.0), (cases.INSIDE, None)])
def test_audit_checks_samples_on_proved_safe_tiles(colpath, name, b):
    """The standing audit, 64 Ki samples every sweep: samples land on skipped tiles -- on the inside box every skipped tile is a
    proved-safe one --, their reference values lie in the enclosures widened by the band and their stored values inside the enclosures
    bit for bit: zero violations."""
    eng, b = colpath, _b(b)
    eng.set_option("guard_audit", 65536)
    _start(eng, name, b)
    eng.set_option("guard_audit_scale_ppm", 1000000)           # (clears the counts)
    for _ in range(2):
        eng.sweep_safeopt(b, want_masks=True, lean=2)
        eng.synchronize()
    safe, unsafe = _skips(eng)
    assert safe > 0 and (name != cases.INSIDE or unsafe == 0)
    p = eng.profile()
    assert p["guard_audit_samples"] >= 65536 and p["guard_audit_skipped"] > 0, p
    assert p["guard_audit_violations"] == 0, p
