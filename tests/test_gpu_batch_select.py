"""sbo_batch_select over its range: the committed cases of batch_oracle.CASES, the library's own append + posterior as a second
reference, ties and the independence of a point's value from the list it stands in, min_std and repeated picks, read-only and
reproducible calls, changed models, an fp32 model, every refusal, and the host class.

The edges the committed cases stand at, by the constants of csrc/batch.hip (the comment above batch_oracle.CASES has the list per
kernel; tests/test_batch_cpu.py reads the constants from the source and holds the list to them):
  small shapes      n in {1, 2, 20, 40, 63, 64, 65, 300}, m in {1, 8, 63, 64, 65, 257, 5000}, k in {1, 2, 8, 64} with k > m twice,
                    d in {1, 2, 4, 8}, q = 3 with outputs 0 and 2, 0 / 1 / 5 pending points, both factor sources;
  k_batch_v0        its three tiers P = 32 | 16 | 8 points per workgroup (n <= 512 | <= 1024 | <= SBO_MAX_N = 2048), row blocks of
                    4 * 1024 / P = 128 | 256 | 512 rows: n = 512, 1024, 2048 (the 128 KiB LDS ceiling of each tier) and n = 513, 1025
                    (the first n of a tier: a top block of one row), m = 16, 33, 257 (one workgroup, a last workgroup of one point);
  k_batch_pass      LDS chunks of kBatChunk = 512 augmented observations: na = n + n_pending + j from 508 to 523 and from exactly
                    512, three and five chunks at n = 1025 and 2048; m = 8192 * 256 + 513, the second trip of its grid-stride loop;
  k_batch_u         strides of 1024 columns and 16 rows: na from 1023 to 1030, and up to ld = SBO_MAX_N + SBO_MAX_BATCH = 2112;
  padded lanes      d = 3 in dpad 4, d = 6 in dpad 8 (next to d = 1 in dpad 2);
  changed models    an append that moves the model from P = 32 to P = 16 and the removal that moves it back, a block append
                    (sbo_model_append_batch) of the batch across n = 512.

The reference is batch_oracle.select_naive (the full matrix inverted at every step; at n = 2048 select_incremental, which
tests/test_batch_cpu.py ties to the definition by full inverses behind the last two picks), normalised units: std / Y_std and
var / Y_std^2 are compared absolutely at TOL64 = 1e-10, picks exactly -- every committed case has a top-two gap above 1e-8 at every
step (tests/test_batch_cpu.py), and the NumPy routes agree among themselves to 4.3e-13.

Largest deviations seen on an MI355X over the committed cases: std 2.1e-12 (n = 20, m = 8, k = 64: 56 repeated picks), then 8.4e-13
(n = 300, m = 5000, k = 64) and 4.5e-13 (n = 2048, m = 300, k = 59); var 3.1e-13 (n = 300, m = 5000, k = 64), then 2.4e-13 (n = 600,
d = 3) and 2.2e-13 (n = 1100, d = 6); n = 2048 has var 1.5e-13.  Every other test of this file stays below 1e-13 (DESIGN.md
section 17)."""
import ctypes as C

import numpy as np
import pytest

import safebo_amd
from safebo_amd import SafeOpt, _lib, synthetic

import batch_oracle as bo
import model_remove as mr
from batch_oracle import TOL64

pytestmark = pytest.mark.gpu

IDS = [bo.case_id(c) for c in bo.CASES]


def _errors(got, ref, ds, o):
    ys = float(ds["Y_std"][o])
    e_std = float(np.max(np.abs(got["std"] / ys - np.sqrt(np.maximum(0.0, ref["v_pick"]))))) if len(ref["index"]) else 0.0
    e_var = float(np.max(np.abs(got["var"] / ys ** 2 - np.maximum(0.0, ref["v"]))))
    return e_std, e_var


def _check(eng, ds, o, pool, k, pending, ref, label):
    got = eng.batch_select(pool, k, o, pending, return_var=True)
    assert got["index"].dtype == np.int64 and got["x"].shape == (len(got["index"]), pool.shape[1]) and got["var"].shape == (len(pool),)
    assert np.array_equal(got["index"], ref["index"]), (label, got["index"], ref["index"])
    assert np.array_equal(got["x"], pool[ref["index"]])
    e_std, e_var = _errors(got, ref, ds, o)
    print(label, "std", e_std, "var", e_var)
    assert e_std < TOL64 and e_var < TOL64, (label, e_std, e_var)
    return got


def _config_b(n=40):
    ds0 = synthetic.make_config("B", n=90, seed=5)
    ds = ds0["ds"] if n == 90 else mr.with_rows(ds0["ds"], ds0["ds"]["X_norm"][:n], ds0["ds"]["Y_norm"][:n])
    return ds, np.asarray(ds0["bound"], dtype=np.float64), ds0


def _config_b_sharp(n):
    """Config B's data at n rows (seed 5) with log_sn = -1, which keeps the oracle sharp from a few hundred rows on (the committed
    cases from n = 505 up)."""
    cfg = synthetic.make_config("B", n=n, seed=5)
    ds = synthetic.make_dataset(cfg["X"], cfg["Y"], synthetic.default_hypopt(2, 2, log_sn=-1.0))
    return ds, np.asarray(cfg["bound"], dtype=np.float64)


def _pool(bound, m, seed):
    return np.random.default_rng(seed).uniform(bound[:, 0], bound[:, 1], size=(m, bound.shape[0]))


def _raw(eng, pool, k, output=0, pending=None, n_pending=None, min_std=0.0, want_var=False, m=None):
    """The C call itself: (status, result structure, var or None)."""
    pool = None if pool is None else np.ascontiguousarray(pool, dtype=np.float64)
    pend = None if pending is None else np.ascontiguousarray(pending, dtype=np.float64)
    opts = _lib.BatchOpts(output, k, (0 if pend is None else len(pend)) if n_pending is None else n_pending, 0, min_std)
    res = _lib.BatchResult()
    res.n_selected, res.index[3], res.std[3] = 9, 4, 2.0            # (stale content a refusal has to clear)
    mm = (0 if pool is None else len(pool)) if m is None else m
    var = np.empty(max(mm, 1)) if want_var else None
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = eng._lib.sbo_batch_select(eng._ctx, C.byref(opts), mm, ptr(pool), ptr(pend), ptr(var), C.byref(res))
    return rc, res, var


def _cleared(res):
    return res.n_selected == 0 and list(res.index) == [-1] * _lib.SBO_MAX_BATCH and list(res.std) == [0.0] * _lib.SBO_MAX_BATCH


# ------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("i", range(len(bo.CASES)), ids=IDS)
def test_every_committed_case_against_the_naive_oracle(engine, i):
    c = bo.CASES[i]
    ds, pool, pending, ref = bo.reference(i)
    engine.set_model(ds, use_invK=c["use_invK"])
    assert (engine.n, engine.d, engine.q) == (c["n"], c["d"], c["q"])
    got = _check(engine, ds, c["output"], pool, c["k"], pending, ref, bo.case_id(c))
    assert len(got["index"]) == c["k"]
    if c["k"] > c["m"]:
        assert len(set(got["index"].tolist())) < c["k"]          # (a pool point is picked again)
    if i >= bo.FIRST_LARGE:                                      # (without var_out the conditioning behind the last pick is skipped)
        lean = engine.batch_select(pool, c["k"], c["output"], pending, return_var=False)
        assert "var" not in lean
        assert lean["index"].tobytes() == got["index"].tobytes() and lean["std"].tobytes() == got["std"].tobytes()


def test_a_lane_on_its_second_trip_and_a_tie_across_trips(engine):
    """The planted pool (batch_oracle.planted_pool): m = 8192 * 256 + 513, so the first 513 lanes of k_batch_pass see a second
    candidate of their own.  A copied row holds the bits of its original (the lane's second trip against its first), and with row
    17's far point also at row 17 + 8192 * 256 -- an exact tie inside one lane, across trips -- the batch is unchanged: the lower
    index is taken."""
    i = next(t for t, c in enumerate(bo.CASES) if c.get("pool") == "planted")
    c = bo.CASES[i]
    ds, pool, _, ref = bo.reference(i)
    M, o = bo.M_TRIP, c["output"]
    engine.set_model(ds, use_invK=c["use_invK"])
    got = _check(engine, ds, o, pool, c["k"], None, ref, "planted")
    assert got["index"].tolist() == list(bo.PLANTED)
    same = np.setdiff1d(np.arange(c["m"] - M), [p % M for p in bo.PLANTED])
    assert same.size == 510 and np.array_equal(pool[M + same], pool[same])
    assert got["var"][M + same].tobytes() == got["var"][same].tobytes()
    tie = pool.copy()
    tie[M + 17] = pool[17]
    t = engine.batch_select(tie, c["k"], o, None, return_var=True)
    assert 17 in t["index"].tolist() and M + 17 not in t["index"].tolist(), t["index"]
    # (a point's value does not depend on the list it stands in: the batch and every other row are what they were)
    assert np.array_equal(t["index"], got["index"]) and t["std"].tobytes() == got["std"].tobytes()
    assert t["var"][M + 17] == t["var"][17] and np.array_equal(np.delete(t["var"], M + 17), np.delete(got["var"], M + 17))


# ------------------------------------------------------------------------------------------ 2. against the library itself
@pytest.mark.parametrize("o", [0, 1])
def test_var_out_is_the_posterior_after_appending_the_picks(engine, o):
    """n = 40, m = 257, k = 4 with one pending point: after append_sample of the pending point and the picks (arbitrary y) the
    library's own posterior() at the pool has the variance of output o that var_out announced, within TOL64 normalised; then the
    rows leave again."""
    ds, bound, _ = _config_b(40)
    pool, pending = _pool(bound, 257, 201), _pool(bound, 1, 202)
    engine.set_model(ds)
    ref = bo.select_naive(ds, o, pool, 4, pending)
    assert ref["gaps"].min() > bo.GAP
    got = _check(engine, ds, o, pool, 4, pending, ref, "before")
    added = np.vstack([pending, got["x"]])
    try:
        for t, x in enumerate(added):
            engine.append_sample((x - ds["X_mean"]) / ds["X_std"], np.array([0.3 * t - 0.5, 1.0 - 0.2 * t]))
        engine.set_points(pool)
        _, var = engine.posterior()
    finally:
        while engine.n > 40:
            engine.remove_sample(engine.n - 1)
    err = float(np.max(np.abs(var[:, o] - got["var"]))) / float(ds["Y_std"][o]) ** 2
    print(o, err)
    assert err < TOL64, err
    _check(engine, ds, o, pool, 4, pending, ref, "after")      # (the rows have left again: the model is the one it was, to rounding)


@pytest.mark.parametrize("o", [0, 1])
def test_var_out_is_the_posterior_after_a_block_append_across_a_tier(engine, o):
    """The batched campaign (batch_select, then one block update for the results) at the first tier boundary of k_batch_v0:
    n = 509, m = 257, k = 8 with one pending point, log_sn = -1.  append_samples of the pending point and the eight picks (arbitrary
    y; sbo_model_append_batch) gives n = 518, and posterior() at the pool has the variance of output o that var_out announced,
    within TOL64 normalised; a call on the grown model (P = 16) agrees with the oracle on 518 rows; then the rows leave again."""
    ds, bound = _config_b_sharp(509)
    pool, pending = _pool(bound, 257, 211), _pool(bound, 1, 212)
    engine.set_model(ds)
    ref = bo.select_naive(ds, o, pool, 8, pending)
    assert ref["gaps"].min() > bo.GAP
    got = _check(engine, ds, o, pool, 8, pending, ref, "before")
    added = (np.vstack([pending, got["x"]]) - ds["X_mean"]) / ds["X_std"]
    y = np.column_stack([0.3 * np.arange(9) - 0.5, 1.0 - 0.2 * np.arange(9)])
    try:
        engine.append_samples(added, y)
        assert engine.n == 518
        engine.set_points(pool)
        _, var = engine.posterior()
        ds518 = mr.extended(ds, added, y)
        ref518 = bo.select_naive(ds518, o, pool, 2)
        assert ref518["gaps"].min() > bo.GAP
        _check(engine, ds518, o, pool, 2, None, ref518, "grown")
    finally:
        while engine.n > 509:
            engine.remove_sample(engine.n - 1)
    err = float(np.max(np.abs(var[:, o] - got["var"]))) / float(ds["Y_std"][o]) ** 2
    print(o, err)
    assert err < TOL64, err


# ------------------------------------------------------------------------------------------ 3. ties and order
def test_ties_permutations_embeddings_and_repeated_calls(engine):
    """n = 40, m = 257, k = 8.  A pool with every row twice: the lower index is picked and a row's copy holds the same bits.  A
    permuted pool: the same picks and the same bits per point.  The points embedded in a longer pool (copies at other offsets,
    three workgroups): the same bits at every copy.  Two calls: the same bits."""
    ds, bound, _ = _config_b(40)
    P = _pool(bound, 257, 301)
    engine.set_model(ds)
    ref = bo.select_naive(ds, 0, P, 8)
    assert ref["gaps"].min() > bo.GAP
    a = _check(engine, ds, 0, P, 8, None, ref, "plain")
    b = engine.batch_select(P, 8, 0, None, return_var=True)
    assert a["index"].tobytes() == b["index"].tobytes() and a["std"].tobytes() == b["std"].tobytes() and a["var"].tobytes() == b["var"].tobytes()
    dup = engine.batch_select(np.vstack([P, P]), 8, 0, None, return_var=True)
    assert np.array_equal(dup["index"], a["index"]) and dup["std"].tobytes() == a["std"].tobytes()
    assert dup["var"][:257].tobytes() == a["var"].tobytes() and dup["var"][257:].tobytes() == a["var"].tobytes()
    perm = np.random.default_rng(302).permutation(257)
    p = engine.batch_select(P[perm], 8, 0, None, return_var=True)
    assert np.array_equal(perm[p["index"]], a["index"]) and p["std"].tobytes() == a["std"].tobytes()
    assert p["var"].tobytes() == a["var"][perm].tobytes()
    long = np.vstack([P, P[3:], P[:77]])
    e = engine.batch_select(long, 8, 0, None, return_var=True)
    assert np.array_equal(e["index"], a["index"]) and e["std"].tobytes() == a["std"].tobytes()
    assert e["var"].tobytes() == np.concatenate([a["var"], a["var"][3:], a["var"][:77]]).tobytes()


# ------------------------------------------------------------------------------------------ 4. min_std and repeats
def test_a_one_point_pool_repeats_and_min_std_stops(engine):
    ds, bound, _ = _config_b(40)
    P = _pool(bound, 1, 401)
    engine.set_model(ds)
    ref = bo.follow(ds, 0, P, [0, 0, 0, 0])
    got = _check(engine, ds, 0, P, 4, None, ref, "one point")
    assert got["index"].tolist() == [0, 0, 0, 0] and np.all(np.diff(got["std"]) < 0.0) and got["std"][-1] > 0.0
    cut = 0.5 * (got["std"][0] + got["std"][1])
    rc, res, _ = _raw(engine, P, 4, min_std=cut)
    assert rc == _lib.SBO_OK and res.n_selected == 1 and res.index[0] == 0 and list(res.index[1:]) == [-1] * 63
    assert res.std[0] == got["std"][0] and list(res.std[1:]) == [0.0] * 63
    one = engine.batch_select(P, 4, 0, None, min_std=cut, return_var=True)
    assert one["index"].tolist() == [0] and one["x"].shape == (1, 2)
    assert abs(one["var"][0] - got["std"][1] ** 2) < TOL64 * float(ds["Y_std"][0]) ** 2     # (the one pick has been conditioned on)
    none = engine.batch_select(P, 4, 0, None, min_std=2.0 * got["std"][0])
    assert none["index"].shape == (0,) and none["x"].shape == (0, 2) and none["std"].shape == (0,)


# ------------------------------------------------------------------------------------------ 5. read-only
def _snapshot(eng, lo, hi, count, b):
    """What the resident model gives, bit for bit (tests/test_gpu_model_loo.py): the posterior on a fresh grid on K1b and on K1g, a
    full SafeOpt sweep and its masks."""
    out = {}
    try:
        for name, bl in (("K1b", 2), ("K1g", 0)):
            eng.set_option("bilinear", bl)
            eng.set_grid(lo, hi, count)
            eng.posterior_run()
            assert eng.profile()["posterior_kernel"] == mr.KERNEL[name], name
            out[name] = eng.posterior()
    finally:
        eng.set_option("bilinear", 1)
    eng.set_grid(lo, hi, count)
    eng.sweep_safeopt(b)
    out["sweep"] = eng.sweep_safeopt(b, want_masks=True)
    out["masks"] = [eng.mask(k) for k in ("S", "U", "M")] + [eng.mask("G", 1)]
    return out


def _assert_same(a, b):
    for name in ("K1b", "K1g"):
        for x, y in zip(a[name], b[name]):
            assert np.array_equal(x, y) and np.array_equal(x.view(np.uint64), y.view(np.uint64)), name
    for k, v in a["sweep"].items():
        assert np.array_equal(np.asarray(v), np.asarray(b["sweep"][k])), k
    for x, y in zip(a["masks"], b["masks"]):
        assert np.array_equal(x, y)


def test_the_call_changes_nothing(engine):
    """n = 90: the posterior on a 64 x 72 grid (K1b and K1g) and a SafeOpt sweep with its masks are identical before and after a
    call; with the posterior and the masks of a sweep resident, a call leaves posterior(), the masks and the next sweep as they were."""
    ds, bound, cfg = _config_b(90)
    lo, hi, count, b = bound[:, 0], bound[:, 1], [64, 72], cfg["b"]
    pool, pending = _pool(bound, 257, 501), _pool(bound, 1, 502)
    engine.set_model(ds)
    before = _snapshot(engine, lo, hi, count, b)
    post0 = engine.posterior()
    first = engine.batch_select(pool, 8, 0, pending, return_var=True)
    post1 = engine.posterior()
    for x, y in zip(post0, post1):
        assert x.tobytes() == y.tobytes()
    masks1 = [engine.mask(k) for k in ("S", "U", "M")] + [engine.mask("G", 1)]
    for x, y in zip(before["masks"], masks1):
        assert np.array_equal(x, y)
    _assert_same(before, _snapshot(engine, lo, hi, count, b))
    second = engine.batch_select(pool, 8, 0, pending, return_var=True)
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), k


# ------------------------------------------------------------------------------------------ 6. changed models
def test_after_an_append_and_after_a_removal(engine):
    """n = 40: after an append_sample (the resident factor has grown: leading dimension > n) and after a remove_sample(0) the call
    agrees with the oracle on the rows the model then holds."""
    ds, bound, cfg = _config_b(40)
    ds90 = cfg["ds"]
    pool = _pool(bound, 257, 601)
    engine.set_model(ds)
    engine.append_sample(ds90["X_norm"][40], ds90["Y_norm"][40])
    ds41 = mr.with_rows(ds, ds90["X_norm"][:41], ds90["Y_norm"][:41])
    ref = bo.select_naive(ds41, 1, pool, 4)
    assert ref["gaps"].min() > bo.GAP
    _check(engine, ds41, 1, pool, 4, None, ref, "appended")
    engine.remove_sample(0)
    ds40 = mr.without(ds41, 0)
    ref = bo.select_naive(ds40, 0, pool, 4, pool[:2] + 0.01)
    assert ref["gaps"].min() > bo.GAP
    _check(engine, ds40, 0, pool, 4, pool[:2] + 0.01, ref, "removed")


def test_an_append_across_a_tier_of_v0_and_back(engine):
    """n = 512 (P = 32, four full blocks of 128 rows), m = 257, k = 4; append_sample of one more row of config B gives n = 513: the
    P = 16 tier, blocks of 256 rows and a top block of one row, on a factor an append has grown -- compared with the oracle on 513
    rows.  remove_sample(512) takes the last row away again, which leaves every other row of the factor as it is: the call gives
    the bits of the first one."""
    ds513, bound = _config_b_sharp(513)
    ds512 = mr.with_rows(ds513, ds513["X_norm"][:512], ds513["Y_norm"][:512])
    pool = _pool(bound, 257, 611)
    engine.set_model(ds512)
    ref = bo.select_naive(ds512, 0, pool, 4)
    assert ref["gaps"].min() > bo.GAP
    first = _check(engine, ds512, 0, pool, 4, None, ref, "n = 512")
    engine.append_sample(ds513["X_norm"][512], ds513["Y_norm"][512])
    try:
        assert engine.n == 513
        ref = bo.select_naive(ds513, 0, pool, 4)
        assert ref["gaps"].min() > bo.GAP
        _check(engine, ds513, 0, pool, 4, None, ref, "n = 513")
    finally:
        engine.remove_sample(512)
    again = engine.batch_select(pool, 4, 0, None, return_var=True)
    for key in first:
        assert first[key].tobytes() == again[key].tobytes(), key


# ------------------------------------------------------------------------------------------ 7. fp32
def test_an_fp32_model_keeps_the_fp64_bar(engine):
    """Config B at n = 90 as an fp32 model: the factor the call reads is built in fp64 for every model dtype and the call uploads
    the fp64 observations itself, so picks, std and var meet TOL64."""
    ds, bound, _ = _config_b(90)
    pool, pending = _pool(bound, 257, 701), _pool(bound, 1, 702)
    ref = bo.select_naive(ds, 0, pool, 8, pending)
    assert ref["gaps"].min() > bo.GAP
    engine.set_model(ds, dtype="f32")
    try:
        got = _check(engine, ds, 0, pool, 8, pending, ref, "f32")
        assert got["std"].dtype == np.float64 and got["var"].dtype == np.float64
    finally:
        engine.set_model(ds, dtype="f64")


# ------------------------------------------------------------------------------------------ 8. refusals
def test_a_call_without_a_model_is_refused():
    with safebo_amd.SweepEngine(0) as eng:
        rc, res, _ = _raw(eng, np.zeros((3, 2)), 1)
        assert rc == _lib.SBO_E_NO_MODEL and _cleared(res)
        with pytest.raises(safebo_amd.SafeBOError) as ei:
            eng.batch_select(np.zeros((3, 2)), 1)
        assert ei.value.code == _lib.SBO_E_NO_MODEL


def test_refused_calls_clear_the_result_and_leave_the_next_one_intact(engine):
    ds, bound, _ = _config_b(40)
    pool, pending = _pool(bound, 65, 801), _pool(bound, 2, 802)
    engine.set_model(ds)
    want = engine.batch_select(pool, 4, 0, pending, return_var=True)
    nan_pool, inf_pend = pool.copy(), pending.copy()
    nan_pool[64, 1], inf_pend[1, 0] = np.nan, np.inf
    bad = [dict(pool=None, k=1, m=3), dict(pool=pool, k=1, m=0), dict(pool=pool, k=1, m=-5), dict(pool=pool, k=1, output=-1),
           dict(pool=pool, k=1, output=2), dict(pool=pool, k=0), dict(pool=pool, k=-3), dict(pool=pool, k=65),
           dict(pool=pool, k=1, n_pending=-1), dict(pool=pool, k=1, n_pending=2), dict(pool=pool, k=63, pending=pending),
           dict(pool=pool, k=1, pending=np.zeros((64, 2))), dict(pool=nan_pool, k=1), dict(pool=pool, k=1, pending=inf_pend),
           dict(pool=pool, k=1, min_std=-1e-300), dict(pool=pool, k=1, min_std=float("nan")), dict(pool=pool, k=1, min_std=float("inf"))]
    for kw in bad:
        rc, res, _ = _raw(engine, **kw)
        assert rc == _lib.SBO_E_INVALID and _cleared(res), kw
    opts = _lib.BatchOpts(0, 1, 0, 0, 0.0)
    res = _lib.BatchResult()
    p = pool.ctypes.data_as(C.c_void_p)
    assert engine._lib.sbo_batch_select(None, C.byref(opts), 65, p, None, None, C.byref(res)) == _lib.SBO_E_INVALID and _cleared(res)
    assert engine._lib.sbo_batch_select(engine._ctx, None, 65, p, None, None, C.byref(res)) == _lib.SBO_E_INVALID and _cleared(res)
    assert engine._lib.sbo_batch_select(engine._ctx, C.byref(opts), 65, p, None, None, None) == _lib.SBO_E_INVALID
    with pytest.raises(ValueError):
        engine.batch_select(nan_pool, 1)
    again = engine.batch_select(pool, 4, 0, pending, return_var=True)
    for k in want:
        assert want[k].tobytes() == again[k].tobytes(), k
    # k + n_pending == SBO_MAX_BATCH is served
    rc, res, _ = _raw(engine, pool, 62, pending=pending)
    assert rc == _lib.SBO_OK and res.n_selected == 62


def test_a_conditioning_step_with_s_not_positive_is_refused(engine):
    """A caller's inverse that is positive definite but not the model's -- 10 I -- gives k_z . u = 10 |k_z|^2 >= 10 sf2^2 > sf2 + sn2 at
    an observation z: conditioning on it has s < 0, the call is SBO_E_INVALID and the result cleared; the model itself is untouched."""
    ds, bound, _ = _config_b(40)
    wrong = dict(ds)
    wrong["invKopt"] = [10.0 * np.eye(40), 10.0 * np.eye(40)]
    pool = _pool(bound, 65, 901)
    z = ds["X_norm"][:1] * ds["X_std"] + ds["X_mean"]
    engine.set_model(wrong)
    rc, res, _ = _raw(engine, pool, 2, pending=z, want_var=True)
    assert rc == _lib.SBO_E_INVALID and _cleared(res)
    assert "s <= 0" in engine._lib.sbo_last_error().decode()
    with pytest.raises(ValueError):
        engine.batch_select(pool, 2, 0, z)
    engine.set_model(ds)
    ref = bo.select_naive(ds, 0, pool, 2, z)
    _check(engine, ds, 0, pool, 2, z, ref, "after a refusal")


# ------------------------------------------------------------------------------------------ 9. host class
def test_batch_of_the_host_class():
    m = mr.init_bo(SafeOpt.BO, n=12)
    res = m.sweep()
    X1, s1 = m.Batch(1)
    want = max(res["minimizer_std"], res["expander_std"])
    assert X1.shape == (1, 2) and s1.shape == (1,) and abs(s1[0] - want) <= 1e-9 * want, (s1, want)
    masks = m.masks()
    member = masks["M"].reshape(-1) | masks["G1"].reshape(-1)
    pts = m._all_points()
    X4, s4 = m.Batch(4)
    assert X4.shape == (4, 2) and s4.shape == (4,) and np.all(np.diff(s4) <= 0.0) and np.array_equal(X4[0], X1[0])
    for x in X4:
        hit = np.nonzero(np.all(pts == x, axis=1))[0]
        assert hit.size == 1 and member[hit[0]], x
    Xp, sp = m.Batch(4, pending=X4[:1])
    assert Xp.shape == (4, 2) and not np.array_equal(Xp, X4) and sp[0] < s4[0]
    # (conditioning on a pending point is the step a pick takes: the batch goes on where Batch(4) stood after its first pick)
    assert np.array_equal(Xp[:3], X4[1:]) and np.array_equal(sp[:3], s4[1:])
