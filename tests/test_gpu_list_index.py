"""Spatial index of explicit candidate lists (option list_index, csrc/sets_index.inc.hpp): expander sets and GoOSE's coverage search
on scattered lists must come out identical to the exhaustive evaluation, and lists above the exhaustive cap (2^21) now sweep."""
import numpy as np
import pytest

import oracle
from safebo_amd import GoOSE, SafeOpt, synthetic

pytestmark = pytest.mark.gpu


def _problem(d, q=2, n=64, seed=0, log_ell=0.3, offset=0.0):
    """Points ~ U(-1, 1)^d; objective + q - 1 constraints g_c(x) = 0.8 - 3 ||x - s_c||^2 / d + offset >= 0 (s_c: shifted centres)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, size=(n, d))
    cols = [np.sin(2.0 * X).sum(1) + 0.3 * X[:, 0]]
    for c in range(1, q):
        s = np.zeros(d)
        s[0] = 0.25 * (c - 1)
        cols.append(0.8 - 3.0 * ((X - s) ** 2).sum(1) / d + offset)
    hyp = synthetic.default_hypopt(d, q, log_ell=log_ell, log_sn=-3.0)
    return synthetic.make_dataset(X, np.stack(cols, axis=1), hyp)


def _sweep_all(engine, b, quirk, q, goose):
    res = engine.sweep_safeopt(b, quirk_L_index=quirk, want_masks=True)
    out = {"res": res, "S": engine.mask("S"), "U": engine.mask("U"), "M": engine.mask("M"),
           "G": [engine.mask("G", c) for c in range(1, q)], "prof": engine.profile()}
    if goose:
        out["goose"] = engine.sweep_goose(b, quirk_L_index=quirk, want_masks=True)
        out["O"] = [engine.mask("O", c) for c in range(1, q)]
    return out


def _index_vs_exhaustive(engine, pts, ds, b, quirk=True, goose=True):
    q = ds["Y_norm"].shape[1]
    engine.set_model(ds, dtype="f64")
    engine.set_points(pts)
    got = {}
    try:
        for li in (1, 0):
            engine.set_option("list_index", li)
            got[li] = _sweep_all(engine, b, quirk, q, goose)
    finally:
        engine.set_option("list_index", -1)
    a, e = got[1], got[0]
    for k in ("S", "U", "M"):
        assert np.array_equal(a[k], e[k]), k
    for c in range(q - 1):
        assert np.array_equal(a["G"][c], e["G"][c]), c
    for k in ("minimizer_index", "expander_index", "count_S", "count_U", "count_M", "expander_best_c"):
        assert a["res"][k] == e["res"][k], k
    assert list(a["res"]["count_G"]) == list(e["res"]["count_G"])
    assert list(a["res"]["expander_index_c"]) == list(e["res"]["expander_index_c"])
    assert a["prof"]["list_index_leaf_pairs"] + a["prof"]["list_index_nodes_skipped"] > 0 or a["res"]["count_U"] == 0 \
        or a["res"]["count_S"] == 0
    assert e["prof"]["list_index_leaf_pairs"] == 0
    if q == 2:
        assert e["res"]["n_exact_rechecks"] == e["res"]["count_S"]
    if goose:
        for c in range(q - 1):
            assert np.array_equal(a["O"][c], e["O"][c]), c
        for k in ("safe_min_index", "target_index", "explore_index", "target_best_c", "count_S", "count_U"):
            assert a["goose"][k] == e["goose"][k], k
        assert list(a["goose"]["count_O"]) == list(e["goose"]["count_O"])
        assert list(a["goose"]["target_index_c"]) == list(e["goose"]["target_index_c"])
    return a


@pytest.mark.parametrize("d", [3, 6])
def test_index_equals_exhaustive_scattered(engine, d):
    pts = np.random.default_rng(10 + d).uniform(-1.0, 1.0, size=(40000, d))
    a = _index_vs_exhaustive(engine, pts, _problem(d), 2.0)
    assert a["res"]["count_S"] > 100 and a["res"]["count_U"] > 100 and a["res"]["count_G"][0] > 0
    # one constraint: U is exactly everything outside S (no candidate sits on lcb = 0)
    assert np.array_equal(a["U"], ~a["S"])


@pytest.mark.parametrize("quirk", [True, False])
def test_index_equals_exhaustive_wo_three_outputs(engine, quirk):
    cfg = synthetic.make_config("C", n=64)
    pts = np.random.default_rng(3).uniform(cfg["bound"][:, 0], cfg["bound"][:, 1], size=(30000, 2))
    a = _index_vs_exhaustive(engine, pts, cfg["ds"], cfg["b"], quirk=quirk)
    assert a["res"]["count_S"] > 0


@pytest.mark.parametrize("quirk", [True, False])
def test_index_equals_exhaustive_two_constraints_4d(engine, quirk):
    pts = np.random.default_rng(5).uniform(-1.0, 1.0, size=(30000, 4))
    a = _index_vs_exhaustive(engine, pts, _problem(4, q=3), 2.0, quirk=quirk)
    assert a["res"]["count_S"] > 0 and a["res"]["count_U"] > 0


def test_index_equals_exhaustive_d8(engine):
    pts = np.random.default_rng(8).uniform(-1.0, 1.0, size=(20000, 8))
    a = _index_vs_exhaustive(engine, pts, _problem(8, log_ell=0.6), 2.0)
    assert a["res"]["count_S"] > 0 and a["res"]["count_U"] > 0


def test_index_duplicate_points(engine):
    base = np.random.default_rng(11).uniform(-1.0, 1.0, size=(6000, 3))
    pts = np.repeat(base, 4, axis=0)[np.random.default_rng(12).permutation(24000)]
    a = _index_vs_exhaustive(engine, pts, _problem(3), 2.0)
    assert a["res"]["count_S"] > 0 and a["res"]["count_U"] > 0


def test_index_one_leaf(engine):
    pts = np.random.default_rng(13).uniform(-1.0, 1.0, size=(200, 3))
    a = _index_vs_exhaustive(engine, pts, _problem(3), 2.0)
    assert a["res"]["count_S"] > 0 and a["res"]["count_U"] > 0


def test_index_fp32_points(engine):
    pts = np.random.default_rng(14).uniform(-1.0, 1.0, size=(30000, 5)).astype(np.float32)
    _index_vs_exhaustive(engine, pts, _problem(5), 2.0)


def test_index_empty_U(engine):
    # the constraint is far above zero everywhere: every candidate safe, U empty, no expander
    pts = np.random.default_rng(15).uniform(-1.0, 1.0, size=(20000, 3))
    a = _index_vs_exhaustive(engine, pts, _problem(3, offset=50.0, log_ell=1.0), 2.0)
    assert a["res"]["count_U"] == 0 and a["res"]["count_S"] == 20000 and a["res"]["count_G"][0] == 0


def test_index_guard_band_option(engine):
    engine.set_option("guard_band", 2)
    try:
        pts = np.random.default_rng(16).uniform(-1.0, 1.0, size=(20000, 3))
        _index_vs_exhaustive(engine, pts, _problem(3), 2.0)
    finally:
        engine.set_option("guard_band", 1)


def test_list_above_the_cap_equals_the_grid_transform(engine):
    """A 2048 x 1100 grid (2 252 800 points, above the exhaustive cap) handed over as a shuffled explicit list: the default
    option sweeps it on the index (before it: SBO_E_UNSUPPORTED), with the grid transform's masks and counts; indices come from
    the unshuffled list (ties go to the lowest index)."""
    cfg = synthetic.make_config("B", n=48)
    lo, hi = cfg["bound"][:, 0], cfg["bound"][:, 1]
    count = [2048, 1100]
    engine.set_model(cfg["ds"])
    engine.set_grid(lo, hi, count)
    ref = engine.sweep_safeopt(cfg["b"], want_masks=True)
    rm = {k: engine.mask(k) for k in ("S", "U", "M")}
    rm["G"] = engine.mask("G", 1)
    pts = oracle.grid_points(lo, hi, count)
    perm = np.random.default_rng(17).permutation(pts.shape[0])
    engine.set_points(pts[perm])
    res = engine.sweep_safeopt(cfg["b"], want_masks=True)
    prof = engine.profile()
    assert prof["list_index_build_ms"] > 0 and prof["list_index_leaf_pairs"] > 0
    for k in ("S", "U", "M"):
        got = np.empty_like(rm[k])
        got[perm] = engine.mask(k)
        assert np.array_equal(got, rm[k]), k
    got = np.empty_like(rm["G"])
    got[perm] = engine.mask("G", 1)
    assert np.array_equal(got, rm["G"]) and rm["G"].any()
    for k in ("count_S", "count_U", "count_M"):
        assert res[k] == ref[k], k
    assert list(res["count_G"]) == list(ref["count_G"])
    engine.set_points(pts)
    res = engine.sweep_safeopt(cfg["b"])
    for k in ("minimizer_index", "expander_index", "count_S", "count_M"):
        assert res[k] == ref[k], k
    # option 0 keeps today's refusal above the cap
    engine.set_option("list_index", 0)
    try:
        with pytest.raises(RuntimeError):
            engine.sweep_safeopt(cfg["b"])
    finally:
        engine.set_option("list_index", -1)


def test_large_6d_list_agrees_with_the_reference_predicate(engine):
    """4 * 2^20 scattered points in 6-D with a constraint, fp64, n = 256, default option: 512 sampled safe candidates (half in G,
    half not) against the reference predicate in NumPy over every U point, on the device's own posterior."""
    d, N = 6, 4 << 20
    ds = _problem(d, n=256)
    pts = np.random.default_rng(18).uniform(-1.0, 1.0, size=(N, d))
    engine.set_model(ds, dtype="f64")
    engine.set_points(pts)
    b = 2.0
    res = engine.sweep_safeopt(b, want_masks=True)
    S, U, G = engine.mask("S"), engine.mask("U"), engine.mask("G", 1)
    mean, var = engine.posterior()
    lcb, ucb = oracle.bounds(mean, var, b)
    L = float(res["L"][1])
    assert res["count_S"] > 0 and res["count_U"] > 0
    rng = np.random.default_rng(19)
    inG, outG = np.flatnonzero(S & G), np.flatnonzero(S & ~G)
    assert inG.size >= 16 and outG.size >= 16, (inG.size, outG.size)
    sample = np.concatenate([rng.choice(inG, min(256, inG.size), replace=False), rng.choice(outG, min(256, outG.size), replace=False)])
    XU = pts[U]
    for g in sample:
        ss = None
        for a in range(d):
            df = (pts[g, a] - XU[:, a]) + 1e-8
            ss = df * df if ss is None else ss + df * df
        want = bool(np.any(ucb[g, 1] - L * np.sqrt(ss) >= 0.0))
        assert want == bool(G[g]), g


def _benoit_f(u, noise=0):
    return u[0] ** 2 + u[1] ** 2 + u[0] * u[1]


def _benoit_g(u, noise=0):
    return -(1. - u[0] + u[1] ** 2 + 2. * u[1])


@pytest.mark.parametrize("cls", ["SafeOpt", "GoOSE"])
def test_classes_take_scattered_candidates(cls):
    """SafeOpt.BO / GoOSE.BO with candidates=: the class methods return rows of the list, equal to the engine-level sweep."""
    bound = np.array([[-.6, 1.5], [-1., 1.]])
    pts = np.random.default_rng(20).uniform(bound[:, 0], bound[:, 1], size=(30000, 2))
    B = SafeOpt.BO if cls == "SafeOpt" else GoOSE.BO
    m = B([_benoit_f, _benoit_g], bound, 2.0, candidates=pts, list_index=1)
    X, Y = m.Data_sampling(20, np.array([1.4, -.8]), 0.3)
    m.fixed_hyper = synthetic.default_hypopt(2, 2)
    m.GP_initialization(X, Y, "RBF", multi_hyper=5, var_out=True)
    try:
        if cls == "SafeOpt":
            x, std = m.Minimizer()
            ex, estd = m.Expander()
            masks = m.masks()
            ref = m.engine.sweep_safeopt(2.0, quirk_L_index=True)
            assert np.array_equal(x, pts[ref["minimizer_index"]]) and std == ref["minimizer_std"]
            assert ref["expander_index"] >= 0 and np.array_equal(ex, pts[ref["expander_index"]]) and estd == ref["expander_std"]
            assert masks["S"].shape == (30000,) and int(masks["S"].sum()) == ref["count_S"]
            assert int(masks["G1"].sum()) == int(ref["count_G"][0])
        else:
            t, tl = m.Target()
            xe = m.explore_safeset(t)
            ref = m.engine.sweep_goose(2.0, quirk_L_index=True)
            assert ref["target_index"] >= 0 and np.array_equal(t, pts[ref["target_index"]]) and tl == ref["target_lcb"]
            assert np.array_equal(xe, pts[ref["explore_index"]])
    finally:
        m.engine.close()
