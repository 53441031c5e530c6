"""sbo_expander_gain over its range: the committed cases of expander_oracle.CASES, the library's own append + posterior as a second
reference, repeated calls, duplicated and permuted lists, read-only calls, an fp32 model, changed models, every refusal, and the
host class.

The edges the committed cases stand at, by the constants of csrc/expander.hip (the comment above expander_oracle.CASES has the list
per kernel; tests/test_expander_gain_cpu.py reads the constants from the source and holds the list to them): tiles of 64 x 64 pairs
(ms, mt in {1, 63, 64, 65, 257}), K-slabs of 32 observations (n = 32 | 33, 64 | 65), target splits (five on one source; a second
target tile per workgroup at ms = 257, mt = 13121), the stage-1 tiers (n = 512 | 513, 1024 | 1025, 2048), d = 1, 3, 6 in padded lanes,
q = 2, 3, 4 with the full and a one-bit mask, b = 0, 2, 3, both factor sources.

The reference is expander_oracle.gain_naive (per source and constraint the full (n + 1) x (n + 1) matrix inverted; at n = 2048
gain_rank1, which tests/test_expander_gain_cpu.py ties to the definition on two sources), normalised units: margin is compared
absolutely at TOL64 = 1e-10, count and witness exactly -- every committed case is sharp (no |z| and no top-two gap below 1e-8,
tests/test_expander_gain_cpu.py), and the NumPy routes agree among themselves to 2.0e-11.

Largest deviations of margin seen on an MI355X over the committed cases: 5.9e-12 (n = 300, q = 4, one-bit mask), then 2.5e-12
(n = 1025, d = 3) and 1.1e-12 (n = 2048); every other case and every other test of this file stays below 5e-13.  Duplicated and
permuted sources and permuted targets returned bit-identical margins."""
import ctypes as C

import numpy as np
import pytest

import oracle
import safebo_amd
from safebo_amd import SafeOpt, _lib, synthetic

import expander_oracle as eo
import model_remove as mr
from expander_oracle import TOL64
from test_gpu_batch_select import _assert_same, _config_b, _config_b_sharp, _pool, _snapshot

pytestmark = pytest.mark.gpu

IDS = [eo.case_id(c) for c in eo.CASES]


def _check(eng, b, S, T, ref, label, constraints=None):
    got = eng.expander_gain(S, T, b, constraints, return_margin=True)
    assert got["count"].dtype == np.int64 and got["witness"].dtype == np.int64 and got["expander"].dtype == bool
    assert got["count"].shape == got["margin"].shape == got["witness"].shape == (len(S),)
    err = float(np.max(np.abs(got["margin"] - ref["margin"])))
    print(label, "margin", err)
    assert np.array_equal(got["count"], ref["count"]), (label, got["count"], ref["count"])
    assert np.array_equal(got["witness"], ref["witness"]), (label, got["witness"], ref["witness"])
    assert np.array_equal(got["expander"], ref["count"] > 0)
    assert err < TOL64, (label, err)
    return got


def _sharp(ref):
    zmin, gap = eo.sharpness(ref)
    assert zmin > eo.SHARP and gap > eo.SHARP, (zmin, gap)
    return ref


def _same_bits(a, b):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def _raw(eng, sources, targets, b=3.0, mask=0, ms=None, mt=None, want=True):
    """The C call itself: (status, count, margin, witness), the outputs holding stale content a refusal has to clear."""
    src = None if sources is None else np.ascontiguousarray(sources, dtype=np.float64)
    tgt = None if targets is None else np.ascontiguousarray(targets, dtype=np.float64)
    ms = (0 if src is None else len(src)) if ms is None else ms
    mt = (0 if tgt is None else len(tgt)) if mt is None else mt
    size = max(ms, 1)
    count, margin, witness = np.full(size, 7, dtype=np.int64), np.full(size, 2.0), np.full(size, 5, dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    opts = _lib.ExpanderOpts(b, mask, 0)
    rc = eng._lib.sbo_expander_gain(eng._ctx, C.byref(opts), ms, ptr(src), mt, ptr(tgt), ptr(count), ptr(margin) if want else None,
                                    ptr(witness) if want else None)
    return rc, count, margin, witness


def _cleared(count, margin, witness, ms):
    return count[:ms].tolist() == [0] * ms and np.isnan(margin[:ms]).all() and witness[:ms].tolist() == [-1] * ms


# ------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("i", range(len(eo.CASES)), ids=IDS)
def test_every_committed_case_against_the_oracle(engine, i):
    c = eo.CASES[i]
    ds, S, T, ref = eo.reference(i)
    engine.set_model(ds, use_invK=c["use_invK"])
    assert (engine.n, engine.d, engine.q) == (c["n"], c["d"], c["q"])
    cons = None if c["mask"] == 0 else eo.constraints_of(c["q"], c["mask"])
    got = _check(engine, c["b"], S, T, ref, eo.case_id(c), cons)
    lean = engine.expander_gain(S, T, c["b"], cons)
    assert set(lean) == {"count", "expander"} and lean["count"].tobytes() == got["count"].tobytes()
    if c.get("mixed"):
        assert (got["count"] == 0).any() and got["expander"].any()


# ------------------------------------------------------------------------------------------ 2. against the library itself
def test_the_count_is_the_posterior_after_appending_the_optimistic_row(engine):
    """n = 40, four sources, 257 targets, b = 3: for each source g the row (g, ucb_1(g)) is appended with append_sample (the objective's
    value is arbitrary), posterior() at the targets gives the raw lcb_1, and the number of targets with lcb_1 >= 0 is the count the
    call announced; the row leaves again, and behind the removals the call returns the bits it returned before."""
    ds, bound, _ = _config_b(40)
    S, T, b = _pool(bound, 4, 1101), _pool(bound, 257, 1102), 3.0
    ref = _sharp(eo.gain_naive(ds, b, S, T))
    engine.set_model(ds)
    first = _check(engine, b, S, T, ref, "before")
    engine.set_points(S)
    mean, var = engine.posterior()
    ucb = (mean[:, 1] - ds["Y_mean"][1]) / ds["Y_std"][1] + b * np.sqrt(var[:, 1]) / ds["Y_std"][1]
    counts = []
    for g in range(len(S)):
        engine.append_sample((S[g] - ds["X_mean"]) / ds["X_std"], np.array([0.25, ucb[g]]))
        try:
            engine.set_points(T)
            m1, v1 = engine.posterior()
        finally:
            engine.remove_sample(40)
        counts.append(int(np.sum(m1[:, 1] - b * np.sqrt(v1[:, 1]) >= 0.0)))
    assert counts == first["count"].tolist(), (counts, first["count"])
    _same_bits(first, engine.expander_gain(S, T, b, return_margin=True))


# ------------------------------------------------------------------------------------------ 3. order and repetition
def test_repeated_calls_duplicated_and_permuted_lists(engine):
    """n = 40, q = 2, 70 sources and 257 targets.  Two calls: the same bits.  Every source twice, then permuted: each source keeps its
    count and witness, its margin within TOL64 (the bits are compared and the outcome printed: DESIGN.md section 19).  Permuted
    targets: the counts stay, the witnesses map through the permutation."""
    ds, bound, _ = _config_b(40)
    S, T, b = _pool(bound, 70, 1201), _pool(bound, 257, 1202), 3.0
    ref = _sharp(eo.gain_naive(ds, b, S, T))
    engine.set_model(ds)
    a = _check(engine, b, S, T, ref, "plain")
    _same_bits(a, engine.expander_gain(S, T, b, return_margin=True))
    rng = np.random.default_rng(1203)
    perm = rng.permutation(140)
    dup = engine.expander_gain(np.vstack([S, S])[perm], T, b, return_margin=True)
    src = perm % 70
    assert np.array_equal(dup["count"], a["count"][src]) and np.array_equal(dup["witness"], a["witness"][src])
    assert float(np.max(np.abs(dup["margin"] - a["margin"][src]))) < TOL64
    print("duplicated and permuted sources: margins bit-identical:", dup["margin"].tobytes() == a["margin"][src].tobytes())
    tp = rng.permutation(257)
    p = engine.expander_gain(S, T[tp], b, return_margin=True)
    assert np.array_equal(p["count"], a["count"]) and np.array_equal(tp[p["witness"]], a["witness"])
    assert float(np.max(np.abs(p["margin"] - a["margin"]))) < TOL64
    print("permuted targets: margins bit-identical:", p["margin"].tobytes() == a["margin"].tobytes())


# ------------------------------------------------------------------------------------------ 4. read-only
def test_the_call_changes_nothing(engine):
    """n = 90: the posterior on a 64 x 72 grid (K1b and K1g) and a SafeOpt sweep with its masks are identical before and after a
    call; with the posterior and the masks of a sweep resident, a call leaves posterior() and the masks as they were."""
    ds, bound, cfg = _config_b(90)
    lo, hi, count, b = bound[:, 0], bound[:, 1], [64, 72], cfg["b"]
    S, T = _pool(bound, 65, 1301), _pool(bound, 257, 1302)
    engine.set_model(ds)
    before = _snapshot(engine, lo, hi, count, b)
    post0 = engine.posterior()
    first = engine.expander_gain(S, T, b, return_margin=True)
    for x, y in zip(post0, engine.posterior()):
        assert x.tobytes() == y.tobytes()
    masks1 = [engine.mask(k) for k in ("S", "U", "M")] + [engine.mask("G", 1)]
    for x, y in zip(before["masks"], masks1):
        assert np.array_equal(x, y)
    _assert_same(before, _snapshot(engine, lo, hi, count, b))
    _same_bits(first, engine.expander_gain(S, T, b, return_margin=True))


# ------------------------------------------------------------------------------------------ 5. fp32
def test_an_fp32_model_keeps_the_fp64_bar(engine):
    ds, bound, _ = _config_b(90)
    S, T, b = _pool(bound, 65, 1401), _pool(bound, 257, 1402), 3.0
    ref = _sharp(eo.gain_naive(ds, b, S, T))
    engine.set_model(ds, dtype="f32")
    try:
        got = _check(engine, b, S, T, ref, "f32")
        assert got["margin"].dtype == np.float64
    finally:
        engine.set_model(ds, dtype="f64")


# ------------------------------------------------------------------------------------------ 6. changed models
def test_after_an_append_and_after_a_removal(engine):
    ds, bound, cfg = _config_b(40)
    ds90 = cfg["ds"]
    S, T, b = _pool(bound, 65, 1501), _pool(bound, 257, 1502), 3.0
    engine.set_model(ds)
    engine.append_sample(ds90["X_norm"][40], ds90["Y_norm"][40])
    ds41 = mr.with_rows(ds, ds90["X_norm"][:41], ds90["Y_norm"][:41])
    _check(engine, b, S, T, _sharp(eo.gain_naive(ds41, b, S, T)), "appended")
    engine.remove_sample(0)
    ds40 = mr.without(ds41, 0)
    _check(engine, b, S, T, _sharp(eo.gain_naive(ds40, b, S, T)), "removed")


def test_a_block_append_across_a_tier_of_stage_1(engine):
    """n = 509 (P = 32), log_sn = -1; append_samples of nine rows gives n = 518: the P = 16 tier on a factor a block append has grown,
    compared with the oracle on 518 rows; the rows leave again one by one."""
    ds518, bound = _config_b_sharp(518)
    ds509 = mr.with_rows(ds518, ds518["X_norm"][:509], ds518["Y_norm"][:509])
    S, T, b = _pool(bound, 3, 1601), _pool(bound, 65, 1602), 3.0
    engine.set_model(ds509)
    _check(engine, b, S, T, _sharp(eo.gain_naive(ds509, b, S, T)), "n = 509")
    engine.append_samples(ds518["X_norm"][509:], ds518["Y_norm"][509:])
    try:
        assert engine.n == 518
        _check(engine, b, S, T, _sharp(eo.gain_naive(ds518, b, S, T)), "n = 518")
    finally:
        while engine.n > 509:
            engine.remove_sample(engine.n - 1)


# ------------------------------------------------------------------------------------------ 7. refusals
def test_a_call_without_a_model_is_refused():
    with safebo_amd.SweepEngine(0) as eng:
        rc, count, margin, witness = _raw(eng, np.zeros((3, 2)), np.zeros((2, 2)))
        assert rc == _lib.SBO_E_NO_MODEL and _cleared(count, margin, witness, 3)
        with pytest.raises(safebo_amd.SafeBOError) as ei:
            eng.expander_gain(np.zeros((3, 2)), np.zeros((2, 2)), 3.0)
        assert ei.value.code == _lib.SBO_E_NO_MODEL


def test_refused_calls_clear_the_outputs_and_leave_the_next_one_intact(engine):
    ds, bound, _ = _config_b(40)
    S, T = _pool(bound, 5, 1701), _pool(bound, 65, 1702)
    engine.set_model(ds)                                     # q = 2: bit 1 is the only constraint
    want = engine.expander_gain(S, T, 3.0, return_margin=True)
    nan_S, inf_T = S.copy(), T.copy()
    nan_S[4, 1], inf_T[64, 0] = np.nan, np.inf
    bad = [dict(sources=None, targets=T, ms=5), dict(sources=S, targets=None, mt=65), dict(sources=S, targets=T, mt=0),
           dict(sources=S, targets=T, mt=-3), dict(sources=S, targets=T, b=-1e-300), dict(sources=S, targets=T, b=float("nan")),
           dict(sources=S, targets=T, b=float("inf")), dict(sources=S, targets=T, mask=1), dict(sources=S, targets=T, mask=3),
           dict(sources=S, targets=T, mask=4), dict(sources=S, targets=T, mask=1 << 31), dict(sources=nan_S, targets=T),
           dict(sources=S, targets=inf_T)]
    for kw in bad:
        rc, count, margin, witness = _raw(engine, **kw)
        assert rc == _lib.SBO_E_INVALID and _cleared(count, margin, witness, 5), kw
    for kw in (dict(sources=S, targets=T, ms=0), dict(sources=S, targets=T, ms=-2)):
        assert _raw(engine, **kw)[0] == _lib.SBO_E_INVALID
    many = np.zeros((_lib.SBO_EXPANDER_MAX_POINTS + 1, 2))
    rc, count, margin, witness = _raw(engine, S, many)
    assert rc == _lib.SBO_E_UNSUPPORTED and _cleared(count, margin, witness, 5)
    rc, count, margin, witness = _raw(engine, many, T)
    assert rc == _lib.SBO_E_UNSUPPORTED and _cleared(count, margin, witness, len(many))
    opts = _lib.ExpanderOpts(3.0, 0, 0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    count = np.full(5, 7, dtype=np.int64)
    assert engine._lib.sbo_expander_gain(None, C.byref(opts), 5, p(S), 65, p(T), p(count), None, None) == _lib.SBO_E_INVALID
    assert count.tolist() == [0] * 5
    assert engine._lib.sbo_expander_gain(engine._ctx, None, 5, p(S), 65, p(T), p(count), None, None) == _lib.SBO_E_INVALID
    assert engine._lib.sbo_expander_gain(engine._ctx, C.byref(opts), 5, p(S), 65, p(T), None, None, None) == _lib.SBO_E_INVALID
    rc, count, _, _ = _raw(engine, S, T, want=False)         # (margin and witness are optional)
    assert rc == _lib.SBO_OK and np.array_equal(count, want["count"])
    _same_bits(want, engine.expander_gain(S, T, 3.0, return_margin=True))


def test_a_model_without_constraints_and_a_source_with_s_not_positive(engine):
    """q = 1 has nothing to certify: SBO_E_INVALID.  A caller's inverse that is positive definite but not the model's -- 10 I -- gives
    v(g) = sf2 - 10 |k_g|^2 < -sn2 at an observation g: s <= 0, SBO_E_INVALID with cleared outputs; the model itself is untouched."""
    ds, bound, _ = _config_b(40)
    T = _pool(bound, 65, 1801)
    one = {k: (v[:, :1] if k in ("Y_norm", "hypopt") else v[:1] if k in ("Y_mean", "Y_std", "invKopt") else v) for k, v in ds.items()}
    engine.set_model(one)
    rc, count, margin, witness = _raw(engine, T[:3], T)
    assert rc == _lib.SBO_E_INVALID and _cleared(count, margin, witness, 3)
    wrong = dict(ds)
    wrong["invKopt"] = [10.0 * np.eye(40), 10.0 * np.eye(40)]
    g = ds["X_norm"][:1] * ds["X_std"] + ds["X_mean"]
    engine.set_model(wrong)
    rc, count, margin, witness = _raw(engine, np.vstack([T[:2], g]), T)
    assert rc == _lib.SBO_E_INVALID and _cleared(count, margin, witness, 3)
    assert "s = v + sn2 <= 0" in engine._lib.sbo_last_error().decode()
    with pytest.raises(ValueError):
        engine.expander_gain(g, T, 3.0)
    engine.set_model(ds)
    _check(engine, 3.0, T[:3], T, eo.gain_naive(ds, 3.0, T[:3], T), "after a refusal")


# ------------------------------------------------------------------------------------------ 8. host class
def _bo(n, centre, radius, b, grid, **kw):
    m = SafeOpt.BO([mr.benoit_f, mr.benoit_g], mr.BOUND, b, grid=grid, **kw)
    X, Y = m.Data_sampling(n, np.array(centre), radius)
    m.fixed_hyper = synthetic.default_hypopt(2, 2)
    m.GP_initialization(X, Y, "RBF", multi_hyper=5, var_out=True)
    return m


def test_expander_of_the_host_class():
    """Benoit, 40 samples around (1.0, -0.6), b = 2, a 32 x 28 grid: eight members of S are more uncertain than the minimiser; by the
    oracle every one of them certifies a candidate outside S, so Expander() returns the most uncertain one, with a witness outside S.
    The default constructor's Expander() is the sweep's, unchanged.  With 12 samples around (1.4, -0.8) no member of S is more
    uncertain than the minimiser: the answer of an empty G."""
    args = (40, (1.0, -0.6), 0.5, 2.0, (32, 28))
    m = _bo(*args, expanders="hallucinated", expander_sources=64)
    ds, pts = m.inference_datasets, m._all_points()
    ref = oracle.safeopt_sweep(pts, ds, 2.0)
    std = np.sqrt(ref["var"][:, 0])
    cand = np.nonzero(ref["S"] & (std > ref["minimizer_std"]))[0]
    order = cand[np.argsort(-std[cand], kind="stable")][:64]
    outside = np.nonzero(~ref["S"])[0]
    assert order.size == 8 and np.min(np.abs(np.diff(std[order]))) > 1e-6
    gain = _sharp(eo.gain_naive(ds, 2.0, pts[order], pts[outside]))
    hit = np.nonzero(gain["count"] > 0)[0]
    assert hit.size == 8
    x, s = m.Expander()
    assert np.array_equal(x, pts[order[hit[0]]]) and abs(s - std[order[hit[0]]]) <= 1e-9 * s, (x, s)
    xw, c, Lc = m.expander_witness
    assert c is None and Lc is None and np.array_equal(xw, pts[outside[gain["witness"][hit[0]]]])
    few = _bo(*args, expanders="hallucinated", expander_sources=1)
    x1, s1 = few.Expander()
    assert np.array_equal(x1, x) and s1 == s
    plain = _bo(*args)
    res = plain.sweep()
    xp, sp = plain.Expander()
    assert np.array_equal(xp, res["expander_x"]) and sp == res["expander_std"] and plain.expander_witness is None
    none = _bo(12, (1.4, -0.8), 0.3, 3.0, (20, 20), expanders="hallucinated")
    x0, s0 = none.Expander()
    assert np.array_equal(x0, np.zeros(2)) and s0 == 0.0 and none.expander_witness is None
