"""sbo_sample_paths over its range: the committed cases of paths_oracle.CASES, the library's own posterior as a second reference, a
path as a function (chunks, a path alone and among others, permuted and duplicated pools, ties), repeated calls, read-only calls, an
fp32 model, changed models, every refusal, and the host class.

The edges the committed cases stand at, by the constants of csrc/paths.hip (the comment above paths_oracle.CASES has the list per
kernel; tests/test_sample_paths_cpu.py reads the constants from the source and holds the list to them): point tiles of 128 (m in {1,
127, 128, 129, 513}, a second tile for workgroup 0 at m = 131 073), K-slabs of 32 columns (F in {1, 31, 32, 33, 1024, 8192}, n in {1, 2,
31, 32, 33, 64, 65, 300}, F = n = 33), path blocks of 16 (S in {1, 15, 16, 17, 33, 64}), the strides of the solve (n = 1024 | 1025, 2048),
d = 1, 3, 6, 8 in padded lanes, q = 1 .. 4 with the first and the last output, both ends, both factor sources.

The reference is paths_oracle.paths_solve (np.linalg.solve on K + sn2 I), normalised units: (values - Y_mean) / Y_std is compared
absolutely at TOL64 = 1e-10, the indices exactly -- every committed case is sharp (no top-two gap below 1e-8,
tests/test_sample_paths_cpu.py), and the NumPy routes agree among themselves to 7.7e-13.

Largest deviations of the values seen on an MI355X over the committed cases: 2.5e-13 (n = 2048), then 1.8e-13 (n = 1024) and 1.5e-13
(n = 300, q = 4); every case below n = 300 stays under 1.2e-13.  The other tests of this file: 3.2e-13 on the fp32 model (n = 90),
below 9e-14 elsewhere; against posterior()'s mean 5.9e-14.  The halves of a pool, a permuted and duplicated pool and path 37 of 64
submitted alone returned bit-identical values."""
import ctypes as C

import numpy as np
import pytest

import safebo_amd
from safebo_amd import SweepEngine, _lib

import model_remove as mr
import paths_oracle as po
from paths_oracle import TOL64
from test_gpu_batch_select import _assert_same, _config_b, _pool, _snapshot
from test_gpu_expander_gain import _bo

pytestmark = pytest.mark.gpu

IDS = [po.case_id(c) for c in po.CASES]
T = 128                                                      # kPathTile (tests/test_sample_paths_cpu.py holds the source to it)


def _norm(ds, o, values):
    return (values - ds["Y_mean"][o]) / ds["Y_std"][o]


def _check(eng, ds, o, pts, draws, f, maximize, label):
    """One call with the values against the oracle's f [m, S] (normalised), and the lean call against the first."""
    S = draws[2].shape[0]
    got = eng.sample_paths(pts, S, o, draws=draws, maximize=bool(maximize), return_values=True)
    assert got["index"].dtype == np.int64 and got["index"].shape == got["value"].shape == (S,)
    assert got["values"].shape == (len(pts), S) and got["x"].shape == (S, pts.shape[1])
    err = float(np.max(np.abs(_norm(ds, o, got["values"]) - f)))
    print(label, "values", err)
    idx, _ = po.best(f, maximize)
    assert np.array_equal(got["index"], idx), (label, got["index"], idx)
    assert got["value"].tobytes() == got["values"][got["index"], np.arange(S)].tobytes(), label
    assert np.array_equal(got["x"], pts[idx])
    assert err < TOL64, (label, err)
    lean = eng.sample_paths(pts, S, o, draws=draws, maximize=bool(maximize))
    assert set(lean) == {"index", "x", "value"}
    assert lean["index"].tobytes() == got["index"].tobytes() and lean["value"].tobytes() == got["value"].tobytes(), label
    return got


def _sharp(f, maximize=0):
    gap = po.sharpness(f, maximize)
    assert gap > po.SHARP, gap
    return f


# ------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("i", range(len(po.CASES)), ids=IDS)
def test_every_committed_case_against_the_oracle(engine, i):
    c = po.CASES[i]
    ds, pts, draws, f = po.reference(i)
    engine.set_model(ds, use_invK=c["use_invK"])
    assert (engine.n, engine.d, engine.q) == (c["n"], c["d"], c["q"])
    _check(engine, ds, c["output"], pts, draws, f, c["maximize"], po.case_id(c))


# ------------------------------------------------------------------------------------------ 2. against the library itself
def test_a_path_with_zero_draws_is_the_librarys_posterior_mean(engine):
    """n = 40, 257 points, S = 3, zero weights and noise: every path equals posterior()'s mean at set_points(points) within TOL64
    (un-normalised by Y_std); the call after that leaves posterior() bit for bit."""
    ds, bound, _ = _config_b(40)
    pts = _pool(bound, 257, 2101)
    omega, phase, weights, noise = SweepEngine.path_draws(2, 40, 3, 1024, 2102)
    draws = (omega, phase, np.zeros_like(weights), np.zeros_like(noise))
    engine.set_model(ds)
    engine.set_points(pts)
    post0 = engine.posterior()
    for o in (0, 1):
        got = engine.sample_paths(pts, 3, o, draws=draws, return_values=True)
        err = float(np.max(np.abs(got["values"] - post0[0][:, o:o + 1]))) / ds["Y_std"][o]
        print("output", o, "against posterior()", err)
        assert err < TOL64, err
        assert got["index"].tolist() == [int(np.argmin(got["values"][:, 0]))] * 3
    for x, y in zip(post0, engine.posterior()):
        assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------ 3. a path is a function
def test_chunks_columns_permutations_and_ties(engine):
    """n = 40, 4 T + 1 = 513 points, F = 1024.  The same draws on the two halves of the pool, merged, are the whole call's values bit for
    bit.  Path 37 of 64 submitted alone agrees within TOL64 (whether the bits agree is printed: DESIGN.md section 20).  A permuted and
    a duplicated pool: identical rows hold identical bits.  The best row of a path copied to an earlier and to a later tile: the
    lowest index is returned."""
    ds, bound, _ = _config_b(40)
    pts = _pool(bound, 4 * T + 1, 2201)
    draws = SweepEngine.path_draws(2, 40, 64, 1024, 2202)
    f = _sharp(po.paths_solve(ds, 0, draws, pts))
    engine.set_model(ds)
    whole = _check(engine, ds, 0, pts, draws, f, 0, "whole")
    half = 2 * T
    a = engine.sample_paths(pts[:half], 64, 0, draws=draws, return_values=True)
    b = engine.sample_paths(pts[half:], 64, 0, draws=draws, return_values=True)
    assert np.vstack([a["values"], b["values"]]).tobytes() == whole["values"].tobytes()
    merged = np.where(b["value"] < a["value"], b["index"] + half, a["index"])
    assert np.array_equal(merged, whole["index"])
    # a path alone and as column 37 of 64
    one = tuple(x[37:38] if k >= 2 else x for k, x in enumerate(draws))
    alone = engine.sample_paths(pts, 1, 0, draws=one, return_values=True)
    err = float(np.max(np.abs(alone["values"][:, 0] - whole["values"][:, 37]))) / ds["Y_std"][0]
    print("path 37 alone against column 37 of 64:", err, "bit-identical:", alone["values"][:, 0].tobytes() == whole["values"][:, 37].tobytes())
    assert err < TOL64 and alone["index"][0] == whole["index"][37]
    # permuted and duplicated
    rng = np.random.default_rng(2203)
    perm = rng.permutation(2 * len(pts))
    src = perm % len(pts)
    dup = engine.sample_paths(np.vstack([pts, pts])[perm], 64, 0, draws=draws, return_values=True)
    assert dup["values"].tobytes() == whole["values"][src].tobytes()
    first = np.array([int(np.nonzero(src == r)[0][0]) for r in whole["index"]])          # (the lowest place of a path's best row)
    assert np.array_equal(dup["index"], first) and dup["value"].tobytes() == whole["value"].tobytes()
    # a tie over three tiles
    tie = pts.copy()
    r = int(whole["index"][5])
    tie[[r, 2 * T + 14]] = tie[[2 * T + 14, r]]              # (the best row of path 5 stands in tile 2)
    tie[T + 12] = tie[3 * T + 116] = tie[2 * T + 14]         # ... and in tiles 1 and 3
    got = engine.sample_paths(tie, 64, 0, draws=draws, return_values=True)
    v = got["values"][:, 5]
    assert v[T + 12].tobytes() == v[2 * T + 14].tobytes() == v[3 * T + 116].tobytes() == whole["value"][5].tobytes()
    assert got["index"][5] == T + 12 and got["value"][5].tobytes() == whole["value"][5].tobytes()
    top = engine.sample_paths(tie, 64, 0, draws=draws, maximize=True, return_values=True)
    assert top["values"].tobytes() == got["values"].tobytes()
    assert np.array_equal(top["index"], np.argmax(got["values"], axis=0))


def test_repeated_calls_return_the_same_bits(engine):
    ds, bound, _ = _config_b(90)
    pts = _pool(bound, 1000, 2301)
    engine.set_model(ds)
    a = engine.sample_paths(pts, 17, 1, features=333, seed=2302, return_values=True)
    for _ in range(2):
        b = engine.sample_paths(pts, 17, 1, features=333, seed=2302, return_values=True)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
    other = engine.sample_paths(pts, 17, 1, features=333, seed=2303, return_values=True)
    assert other["values"].tobytes() != a["values"].tobytes()


# ------------------------------------------------------------------------------------------ 4. read-only
def test_the_call_changes_nothing(engine):
    """n = 90: the posterior on a 64 x 72 grid (K1b and K1g) and a SafeOpt sweep with its masks are identical before and after a
    call; with the posterior and the masks of a sweep resident, a call leaves posterior() and the masks as they were."""
    ds, bound, cfg = _config_b(90)
    lo, hi, count, b = bound[:, 0], bound[:, 1], [64, 72], cfg["b"]
    pts = _pool(bound, 257, 2401)
    engine.set_model(ds)
    before = _snapshot(engine, lo, hi, count, b)
    post0 = engine.posterior()
    first = engine.sample_paths(pts, 16, 0, seed=2402, return_values=True)
    for x, y in zip(post0, engine.posterior()):
        assert x.tobytes() == y.tobytes()
    masks1 = [engine.mask(k) for k in ("S", "U", "M")] + [engine.mask("G", 1)]
    for x, y in zip(before["masks"], masks1):
        assert np.array_equal(x, y)
    _assert_same(before, _snapshot(engine, lo, hi, count, b))
    again = engine.sample_paths(pts, 16, 0, seed=2402, return_values=True)
    for k in first:
        assert first[k].tobytes() == again[k].tobytes(), k


# ------------------------------------------------------------------------------------------ 5. fp32
def test_an_fp32_model_keeps_the_fp64_bar(engine):
    ds, bound, _ = _config_b(90)
    pts = _pool(bound, 257, 2501)
    draws = SweepEngine.path_draws(2, 90, 16, 1024, 2502)
    f = _sharp(po.paths_solve(ds, 1, draws, pts))
    engine.set_model(ds, dtype="f32")
    try:
        got = _check(engine, ds, 1, pts, draws, f, 0, "f32")
        assert got["values"].dtype == np.float64
    finally:
        engine.set_model(ds, dtype="f64")


# ------------------------------------------------------------------------------------------ 6. changed models
def test_after_an_append_and_after_a_removal(engine):
    """n = 40 -> 41 by append_sample -> 40 by remove_sample(0): each against the oracle on the changed data.  An append followed by the
    removal of that row gives the first call's bits back."""
    ds, bound, cfg = _config_b(40)
    ds90 = cfg["ds"]
    pts = _pool(bound, 257, 2601)
    omega, phase, weights, noise = SweepEngine.path_draws(2, 41, 16, 1024, 2602)
    d40, d41 = (omega, phase, weights, np.ascontiguousarray(noise[:, :40])), (omega, phase, weights, noise)
    engine.set_model(ds)
    first = _check(engine, ds, 0, pts, d40, _sharp(po.paths_solve(ds, 0, d40, pts)), 0, "n = 40")
    engine.append_sample(ds90["X_norm"][40], ds90["Y_norm"][40])
    ds41 = mr.with_rows(ds, ds90["X_norm"][:41], ds90["Y_norm"][:41])
    _check(engine, ds41, 0, pts, d41, _sharp(po.paths_solve(ds41, 0, d41, pts)), 0, "appended")
    engine.remove_sample(40)
    back = engine.sample_paths(pts, 16, 0, draws=d40, return_values=True)
    for k in first:
        assert first[k].tobytes() == back[k].tobytes(), k
    engine.append_sample(ds90["X_norm"][40], ds90["Y_norm"][40])
    engine.remove_sample(0)
    ds40 = mr.without(ds41, 0)
    _check(engine, ds40, 0, pts, d40, _sharp(po.paths_solve(ds40, 0, d40, pts)), 0, "removed")


# ------------------------------------------------------------------------------------------ 7. refusals
STALE_INDEX, STALE_VALUE, STALE_FILL = 5, 2.0, 7.0


def _raw(eng, draws, pts, S, F, output=0, maximize=0, m=None, null=(), values=None, ctx=True, opts=True, result=True):
    """The C call itself: (status, result structure, values buffer), the outputs holding stale content that a refusal has to clear
    (the result) or to leave alone (the values).  ``null``: the names of the arrays passed as NULL."""
    arrays = dict(zip(("omega", "phase", "weights", "noise"), (np.ascontiguousarray(a, dtype=np.float64) for a in draws)))
    arrays["points"] = np.ascontiguousarray(pts, dtype=np.float64)
    ptr = lambda name: None if name in null else arrays[name].ctypes.data_as(C.c_void_p)
    res = _lib.PathsResult()
    for s in range(_lib.SBO_MAX_PATHS):
        res.index[s], res.value[s] = STALE_INDEX, STALE_VALUE
    o = _lib.PathsOpts(output, S, F, maximize)
    rc = eng._lib.sbo_sample_paths(eng._ctx if ctx else None, C.byref(o) if opts else None, ptr("omega"), ptr("phase"), ptr("weights"),
                                   ptr("noise"), len(arrays["points"]) if m is None else m, ptr("points"),
                                   None if values is None else values.ctypes.data_as(C.c_void_p), C.byref(res) if result else None)
    return rc, res, values


def _cleared(res):
    return list(res.index) == [-1] * _lib.SBO_MAX_PATHS and np.isnan(np.array(res.value)).all()


def test_a_call_without_a_model_is_refused():
    with safebo_amd.SweepEngine(0) as eng:
        draws = SweepEngine.path_draws(2, 4, 2, 8, 0)
        rc, res, values = _raw(eng, draws, np.zeros((3, 2)), 2, 8, values=np.full((3, 2), STALE_FILL))
        assert rc == _lib.SBO_E_NO_MODEL and _cleared(res) and (values == STALE_FILL).all()
        with pytest.raises(safebo_amd.SafeBOError) as ei:
            eng.sample_paths(np.zeros((3, 2)), 2, features=8)
        assert ei.value.code == _lib.SBO_E_NO_MODEL


def test_refused_calls_clear_the_result_and_leave_the_values_and_the_next_call_intact(engine):
    ds, bound, _ = _config_b(40)                              # q = 2
    pts = _pool(bound, 65, 2701)
    S, F = 3, 33
    draws = SweepEngine.path_draws(2, 40, S, F, 2702)
    engine.set_model(ds)
    want = engine.sample_paths(pts, S, 0, draws=draws, return_values=True)

    def spoiled(k, value):
        out = [a.copy() for a in draws]
        out[k].reshape(-1)[-1] = value
        return tuple(out)

    bad_pts = pts.copy()
    bad_pts[64, 1] = np.nan
    inf_pts = pts.copy()
    inf_pts[0, 0] = -np.inf
    bad = [dict(null=("omega",)), dict(null=("phase",)), dict(null=("weights",)), dict(null=("noise",)), dict(null=("points",)),
           dict(m=0), dict(m=-3), dict(m=_lib.SBO_PATHS_MAX_POINTS + 1), dict(S=0), dict(S=-1), dict(S=_lib.SBO_MAX_PATHS + 1),
           dict(F=0), dict(F=-2), dict(F=_lib.SBO_MAX_FEATURES + 1), dict(output=-1), dict(output=2), dict(maximize=2), dict(maximize=-1),
           dict(draws=spoiled(0, np.nan)), dict(draws=spoiled(1, np.inf)), dict(draws=spoiled(2, -np.inf)), dict(draws=spoiled(3, np.nan)),
           dict(pts=bad_pts), dict(pts=inf_pts), dict(ctx=False), dict(opts=False)]
    for kw in bad:
        args = dict(draws=draws, pts=pts, S=S, F=F)
        args.update(kw)
        rc, res, values = _raw(engine, values=np.full((65, S), STALE_FILL), **args)
        assert rc == _lib.SBO_E_INVALID and _cleared(res) and (values == STALE_FILL).all(), kw
    rc, _, values = _raw(engine, draws, pts, S, F, result=False, values=np.full((65, S), STALE_FILL))
    assert rc == _lib.SBO_E_INVALID and (values == STALE_FILL).all()
    # the values cap: 64 paths and 2^23 + 1 points are 8 bytes over it.  The refusal comes before anything is read or written, so the
    # points are a block of untouched zero pages and the values a small buffer; without values_out the same shape would be accepted
    m = _lib.SBO_PATHS_MAX_VALUES // (8 * _lib.SBO_MAX_PATHS) + 1
    assert m <= _lib.SBO_PATHS_MAX_POINTS
    many = np.zeros((m, 2))
    d64 = SweepEngine.path_draws(2, 40, _lib.SBO_MAX_PATHS, F, 2703)
    rc, res, values = _raw(engine, d64, many, _lib.SBO_MAX_PATHS, F, values=np.full(16, STALE_FILL))
    assert rc == _lib.SBO_E_UNSUPPORTED and _cleared(res) and (values == STALE_FILL).all()
    assert "SBO_PATHS_MAX_VALUES" in engine._lib.sbo_last_error().decode()
    del many
    rc, res, _ = _raw(engine, draws, pts, S, F)               # (values_out is optional)
    assert rc == _lib.SBO_OK and list(res.index[:S]) == want["index"].tolist() and list(res.index[S:]) == [-1] * (_lib.SBO_MAX_PATHS - S)
    assert np.array(res.value[:S]).tobytes() == want["value"].tobytes() and np.isnan(np.array(res.value[S:])).all()
    again = engine.sample_paths(pts, S, 0, draws=draws, return_values=True)
    for k in want:
        assert want[k].tobytes() == again[k].tobytes(), k


# ------------------------------------------------------------------------------------------ 8. host class
def test_thompson_of_the_host_class():
    """Benoit, 40 samples around (1.0, -0.6), b = 2, config B's 50 x 50 grid: Thompson(4, seed=3) proposes four members of the
    sweep's S, each the oracle's arg-min of its path over S; the same seed gives the same proposals, another seed other values."""
    m = _bo(40, (1.0, -0.6), 0.5, 2.0, (50, 50))
    ds, pts = m.inference_datasets, m._all_points()
    X, value = m.Thompson(4, seed=3)
    S = m.engine.mask("S")
    assert X.shape == (4, 2) and value.shape == (4,) and S.sum() > 4
    members = pts[np.nonzero(S)[0]]
    draws = SweepEngine.path_draws(2, ds["X_norm"].shape[0], 4, 1024, 3)
    f = _sharp(po.paths_solve(ds, 0, draws, members))
    idx, best = po.best(f, 0)
    assert np.array_equal(X, members[idx])
    for x in X:
        assert (members == x).all(axis=1).any()
    assert float(np.max(np.abs(_norm(ds, 0, value) - best))) < TOL64
    X2, value2 = m.Thompson(4, seed=3)
    assert X2.tobytes() == X.tobytes() and value2.tobytes() == value.tobytes()
    _, value3 = m.Thompson(4, seed=4)
    assert not np.array_equal(value3, value)
