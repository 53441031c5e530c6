"""sbo_posterior_joint over its range: the committed cases of joint_oracle.CASES, the library's own posterior and sample paths as second
references, position independence, repeated and read-only calls, an fp32 model, changed models, every refusal, and the host class.

The edges the committed cases stand at, by the constants of csrc/joint.hip (the comment above joint_oracle.CASES has the list per
kernel; tests/test_posterior_joint_cpu.py reads the constants from the source and holds the list to them): tiles and panels of 64 (m
in {1, 2, 63, 64, 65, 129, 257, 513}, the cap 2048), K-slabs of 32 (n in {1, 31, 32, 33, 300, 1025, 2048}), draw blocks of 16 (S in {0,
1, 16, 17, 64}), d = 1, 3, 8 in padded lanes, q = 1 .. 4 with the first and the last output, both ends, both kinds of covariance, both
factor sources, jitter 0 (with noise), 1e-8, 1e-6, 1e-4.

Mean and covariance are compared with joint_oracle.joint_solve (np.linalg.solve on K + sn2 I) in normalised units at TOL64 = 1e-10.
The draws of a weakly regularised factor are not comparable entry by entry across routes -- with a jitter of 1e-6 the oracle's own
routes differ by up to 1.5e-10 --, so the factor is tested by its defining properties (lower, positive diagonal, |chol chol^T - (cov +
Y_std^2 jitter sf2 I)| <= 2 (m + 1) 2^-53 max diag: the textbook backward-error bound of Cholesky, derived and not measured) and the
draws against the returned factor (1e-12 (1 + |value|)); on the noise = 1 cases the draws are also held to the oracle's at TOL64 with
equal indices.  Every figure is printed before it is asserted.

Largest figures seen on an MI355X over the committed cases: mean 3.5e-13 and cov 2.1e-13 (both n = 300, q = 4; every other case under
7.3e-14); the backward error between 0 (m = 1, 2) and 18.2 units of 2^-53 max diag at m = 2048, where the bound allows 4098; draws
against mean + chol z 3.8e-15; draws against the oracle 1.0e-11 (n = 300, m = 257, jitter 1e-8), 1.2e-12 at the cap.  The other
tests of this file: 2.2e-12 on the fp32 model (draws against the oracle, n = 90), below 6.5e-14 against posterior() (DESIGN.md
section 21)."""
import ctypes as C

import numpy as np
import pytest

import safebo_amd
from safebo_amd import SweepEngine, _lib

import batch_oracle as bo
import joint_oracle as jo
import model_remove as mr
from joint_oracle import TOL64
from test_gpu_batch_select import _assert_same, _config_b, _pool, _snapshot
from test_gpu_expander_gain import _bo

pytestmark = pytest.mark.gpu

IDS = [jo.case_id(c) for c in jo.CASES]
U = 2.0 ** -53


def _factor_checks(got, ds, o, jitter, label):
    """The returned factor by its defining properties, against the returned covariance."""
    cov, chol = got["cov"], got["chol"]
    m = len(cov)
    ys = float(ds["Y_std"][o])
    sf2 = bo.params(ds, o)[1]
    assert not np.triu(chol, 1).any(), label
    assert (np.diag(chol) > 0.0).all(), label
    A = cov + (ys * ys) * (jitter * sf2) * np.eye(m)
    back = float(np.max(np.abs(chol @ chol.T - A)))
    bound = 2.0 * (m + 1) * U * float(np.max(np.diag(A)))
    print(label, "backward error", back, "bound", bound, "in units of 2^-53 max diag", back / (U * float(np.max(np.diag(A)))))
    rel = np.diag(chol) ** 2 / np.diag(A)
    row = got["pivot_row"]
    print(label, "pivot_min", got["pivot_min"], "row", row, "from the factor", float(rel.min()), int(np.argmin(rel)))
    assert back <= bound, (label, back, bound)
    assert 0 <= row < m and rel[row] <= rel.min() * (1.0 + 1e-12), (label, row, int(np.argmin(rel)))
    assert abs(got["pivot_min"] - rel[row]) <= 1e-12 * rel[row], (label, got["pivot_min"], rel[row])


def _check(eng, ds, c, pts, z, ref, label):
    """One call with every array against the oracle and against itself, and the lean call against the first."""
    o, S, m = c["output"], c["S"], len(pts)
    ys, ym = float(ds["Y_std"][o]), float(ds["Y_mean"][o])
    sn2 = bo.params(ds, o)[2]
    kw = dict(output=o, z=z, noise=bool(c["noise"]), jitter=c["jitter"], maximize=bool(c["maximize"]))
    got = eng.posterior_joint(pts, return_cov=True, return_chol=True, return_draws=True, **kw)
    assert got["mean"].shape == (m,) and got["cov"].shape == got["chol"].shape == (m, m) and got["draws"].shape == (m, S)
    e_mean = float(np.max(np.abs((got["mean"] - ym) / ys - ref["mean"])))
    e_cov = float(np.max(np.abs(got["cov"] / (ys * ys) - (ref["C"] + (sn2 if c["noise"] else 0.0) * np.eye(m)))))
    print(label, "mean", e_mean, "cov", e_cov)
    assert got["cov"].tobytes() == np.ascontiguousarray(got["cov"].T).tobytes(), label
    _factor_checks(got, ds, o, c["jitter"], label)
    lean = eng.posterior_joint(pts, return_cov=False, **kw)
    assert lean["mean"].tobytes() == got["mean"].tobytes()
    assert lean["pivot_row"] == got["pivot_row"] and np.float64(lean["pivot_min"]).tobytes() == np.float64(got["pivot_min"]).tobytes() \
        if S else (lean["pivot_row"] == -1 and np.isnan(lean["pivot_min"]))
    if S:
        assert got["index"].dtype == np.int64 and got["index"].shape == got["value"].shape == (S,) and got["x"].shape == (S, pts.shape[1])
        own = got["mean"][:, None] + got["chol"] @ z.T
        e_own = float(np.max(np.abs(got["draws"] - own) / (1.0 + np.abs(own))))
        print(label, "draws against mean + chol z", e_own)
        idx, _ = jo.best(got["draws"], c["maximize"])
        assert np.array_equal(got["index"], idx), (label, got["index"], idx)
        assert got["value"].tobytes() == got["draws"][got["index"], np.arange(S)].tobytes(), label
        assert np.array_equal(got["x"], pts[idx])
        assert lean["index"].tobytes() == got["index"].tobytes() and lean["value"].tobytes() == got["value"].tobytes(), label
        assert e_own <= 1e-12, (label, e_own)
        if c["noise"]:
            e_ref = float(np.max(np.abs((got["draws"] - ym) / ys - ref["draws"])))
            print(label, "draws against the oracle", e_ref)
            assert np.array_equal(got["index"], jo.best(ref["draws"], c["maximize"])[0]), label
            assert e_ref < TOL64, (label, e_ref)
    else:
        assert "index" not in got and "value" not in got
    assert e_mean < TOL64 and e_cov < TOL64, (label, e_mean, e_cov)
    return got


# ------------------------------------------------------------------------------------------ 1 - 4. the committed cases
@pytest.mark.parametrize("i", range(len(jo.CASES)), ids=IDS)
def test_every_committed_case(engine, i):
    c = jo.CASES[i]
    ds, pts, z, ref = jo.reference(i)
    engine.set_model(ds, use_invK=c["use_invK"])
    assert (engine.n, engine.d, engine.q) == (c["n"], c["d"], c["q"])
    _check(engine, ds, c, pts, z, ref, jo.case_id(c))


# ------------------------------------------------------------------------------------------ 5. the library as second reference
def test_against_posterior_and_sample_paths(engine):
    """n = 40, 257 points: diag(cov) and mean against set_points + posterior() within TOL64; with z = 0 every draw is the mean bit for
    bit; sample_paths with zero weights and noise gives the mean within TOL64."""
    ds, bound, _ = _config_b(40)
    pts = _pool(bound, 257, 3101)
    engine.set_model(ds)
    engine.set_points(pts)
    mean0, var0 = engine.posterior()
    omega, phase, weights, noise = SweepEngine.path_draws(2, 40, 3, 64, 3102)
    for o in (0, 1):
        ys = float(ds["Y_std"][o])
        got = engine.posterior_joint(pts, o, z=np.zeros((3, 257)), return_draws=True)
        e_mean = float(np.max(np.abs(got["mean"] - mean0[:, o]))) / ys
        e_var = float(np.max(np.abs(np.diag(got["cov"]) - var0[:, o]))) / (ys * ys)
        print("output", o, "against posterior(): mean", e_mean, "variance", e_var)
        for s in range(3):
            assert got["draws"][:, s].tobytes() == got["mean"].tobytes()
        assert got["index"].tolist() == [int(np.argmin(got["mean"]))] * 3
        paths = engine.sample_paths(pts, 3, o, draws=(omega, phase, np.zeros_like(weights), np.zeros_like(noise)), return_values=True)
        e_path = float(np.max(np.abs(paths["values"] - got["mean"][:, None]))) / ys
        print("output", o, "sample_paths with zero draws against mean", e_path)
        assert e_mean < TOL64 and e_var < TOL64 and e_path < TOL64
    for x, y in zip((mean0, var0), engine.posterior()):
        assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------ 6. position independence
def test_entries_follow_their_points_and_leading_blocks_stand(engine):
    """The 129-point case (n = 64, d = 8, q = 4).  A permuted and duplicated pool with noise = 1: every entry of cov holds the bits of
    its two points.  The first 65 points alone: cov and chol are the leading blocks of the longer call's, bit for bit.  A repeated
    call returns the same bits."""
    i = [k for k, c in enumerate(jo.CASES) if c["m"] == 129][0]
    c = jo.CASES[i]
    ds, pts, z, _ = jo.reference(i)
    o = c["output"]
    engine.set_model(ds, use_invK=c["use_invK"])
    whole = engine.posterior_joint(pts, o, z=z, jitter=1e-6, return_chol=True, return_draws=True)
    again = engine.posterior_joint(pts, o, z=z, jitter=1e-6, return_chol=True, return_draws=True)
    for k in whole:
        assert np.asarray(whole[k]).tobytes() == np.asarray(again[k]).tobytes(), k
    head = engine.posterior_joint(pts[:65], o, jitter=1e-6, return_chol=True)
    assert head["cov"].tobytes() == np.ascontiguousarray(whole["cov"][:65, :65]).tobytes()
    assert head["chol"].tobytes() == np.ascontiguousarray(whole["chol"][:65, :65]).tobytes()
    assert head["mean"].tobytes() == whole["mean"][:65].tobytes()
    noisy = engine.posterior_joint(pts, o, noise=True, jitter=0.0, return_chol=True)
    rng = np.random.default_rng(3201)
    perm = rng.permutation(2 * len(pts))
    src = perm % len(pts)
    dup = engine.posterior_joint(np.vstack([pts, pts])[perm], o, noise=True, jitter=0.0)
    want = noisy["cov"][np.ix_(src, src)]
    same = src[:, None] == src[None, :]
    off = ~np.eye(len(src), dtype=bool)
    # (a point and its copy are two observations: between them stands the covariance of f, without sn2; everywhere else the bits follow)
    plain = engine.posterior_joint(pts, o, noise=False)["cov"][np.ix_(src, src)]
    want = np.where(same & off, plain, want)
    assert dup["cov"].tobytes() == np.ascontiguousarray(want).tobytes()
    assert dup["mean"].tobytes() == noisy["mean"][src].tobytes()


# ------------------------------------------------------------------------------------------ 7. read-only
def _profile_equal(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in a)


def test_the_call_changes_nothing(engine):
    """n = 90: the posterior on a 64 x 72 grid (K1b and K1g) and a SafeOpt sweep with its masks are identical before and after a
    call; with the posterior and the masks of a sweep resident, a call leaves posterior(), the masks and profile() as they were."""
    ds, bound, cfg = _config_b(90)
    lo, hi, count, b = bound[:, 0], bound[:, 1], [64, 72], cfg["b"]
    pts = _pool(bound, 257, 3301)
    engine.set_model(ds)
    before = _snapshot(engine, lo, hi, count, b)
    post0, prof0 = engine.posterior(), engine.profile()
    first = engine.posterior_joint(pts, 0, 16, 3302, return_chol=True, return_draws=True)
    assert _profile_equal(prof0, engine.profile())
    for x, y in zip(post0, engine.posterior()):
        assert x.tobytes() == y.tobytes()
    masks1 = [engine.mask(k) for k in ("S", "U", "M")] + [engine.mask("G", 1)]
    for x, y in zip(before["masks"], masks1):
        assert np.array_equal(x, y)
    _assert_same(before, _snapshot(engine, lo, hi, count, b))
    again = engine.posterior_joint(pts, 0, 16, 3302, return_chol=True, return_draws=True)
    for k in first:
        assert np.asarray(first[k]).tobytes() == np.asarray(again[k]).tobytes(), k


# ------------------------------------------------------------------------------------------ 8. models
def _case(ds, o, pts, z, noise, jitter):
    c = dict(output=o, S=0 if z is None else len(z), noise=int(noise), jitter=jitter, maximize=0)
    return c, jo.joint_solve(ds, o, pts, z, noise, jitter)


def test_an_fp32_model_keeps_the_fp64_bar(engine):
    ds, bound, _ = _config_b(90)
    pts = _pool(bound, 129, 3401)
    z = SweepEngine.joint_draws(129, 16, 3402)
    c, ref = _case(ds, 1, pts, z, True, 1e-6)
    engine.set_model(ds, dtype="f32")
    try:
        got = _check(engine, ds, c, pts, z, ref, "f32")
        assert got["cov"].dtype == np.float64
    finally:
        engine.set_model(ds, dtype="f64")


def test_after_an_append_and_after_a_removal(engine):
    """n = 40 -> 41 by append_sample -> 40 by remove_sample(0): each against the oracle on the changed data.  An append followed by the
    removal of that row gives the first call's bits back."""
    ds, bound, cfg = _config_b(40)
    ds90 = cfg["ds"]
    pts = _pool(bound, 129, 3501)
    z = SweepEngine.joint_draws(129, 16, 3502)
    engine.set_model(ds)
    c, ref = _case(ds, 0, pts, z, True, 1e-6)
    first = _check(engine, ds, c, pts, z, ref, "n = 40")
    engine.append_sample(ds90["X_norm"][40], ds90["Y_norm"][40])
    ds41 = mr.with_rows(ds, ds90["X_norm"][:41], ds90["Y_norm"][:41])
    _check(engine, ds41, c, pts, z, _case(ds41, 0, pts, z, True, 1e-6)[1], "appended")
    engine.remove_sample(40)
    back = engine.posterior_joint(pts, 0, z=z, noise=True, jitter=1e-6, return_chol=True, return_draws=True)
    for k in first:
        assert np.asarray(first[k]).tobytes() == np.asarray(back[k]).tobytes(), k
    engine.append_sample(ds90["X_norm"][40], ds90["Y_norm"][40])
    engine.remove_sample(0)
    ds40 = mr.without(ds41, 0)
    _check(engine, ds40, c, pts, z, _case(ds40, 0, pts, z, True, 1e-6)[1], "removed")


# ------------------------------------------------------------------------------------------ 9. refusals
STALE_INDEX, STALE_VALUE, STALE_FILL = 5, 2.0, 7.0


def _raw(eng, pts, z=None, S=None, output=0, noise=0, maximize=0, jitter=1e-6, m=None, null=(), ctx=True, opts=True, result=True, chol=True):
    """The C call itself: (status, result structure, the four output arrays), the outputs holding stale content that a refusal has to
    clear (the result) or to leave alone (the arrays).  ``null``: the names of the inputs passed as NULL; ``chol``: whether chol_out is passed."""
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    z = None if z is None else np.ascontiguousarray(z, dtype=np.float64)
    S = (0 if z is None else len(z)) if S is None else S
    mm = len(pts) if m is None else m
    room = min(max(mm, 1), 64)                                # (a refused call writes nothing: small blocks do for any m)
    outs = [np.full(room, STALE_FILL), np.full((room, room), STALE_FILL), np.full((room, room), STALE_FILL),
            np.full((room, max(S, 1)), STALE_FILL)]
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    res = _lib.JointResult()
    for s in range(_lib.SBO_MAX_PATHS):
        res.index[s], res.value[s] = STALE_INDEX, STALE_VALUE
    res.pivot_min, res.pivot_row = STALE_VALUE, STALE_INDEX
    o = _lib.JointOpts(output, S, noise, maximize, jitter)
    rc = eng._lib.sbo_posterior_joint(eng._ctx if ctx else None, C.byref(o) if opts else None, mm, None if "points" in null else ptr(pts),
                                      None if "z" in null else ptr(z), *[ptr(a) if chol or k != 2 else None for k, a in enumerate(outs)],
                                      C.byref(res) if result else None)
    return rc, res, outs


def _cleared(res):
    return list(res.index) == [-1] * _lib.SBO_MAX_PATHS and np.isnan(np.array(res.value)).all() and np.isnan(res.pivot_min) \
        and res.pivot_row == -1


def _untouched(outs):
    return all((a == STALE_FILL).all() for a in outs)


def test_a_call_without_a_model_is_refused():
    with safebo_amd.SweepEngine(0) as eng:
        rc, res, outs = _raw(eng, np.zeros((3, 2)), np.zeros((2, 3)))
        assert rc == _lib.SBO_E_NO_MODEL and _cleared(res) and _untouched(outs)
        with pytest.raises(safebo_amd.SafeBOError) as ei:
            eng.posterior_joint(np.zeros((3, 2)))
        assert ei.value.code == _lib.SBO_E_NO_MODEL


def test_refused_calls_clear_the_result_and_write_no_array_and_leave_the_next_call_intact(engine):
    ds, bound, _ = _config_b(40)                              # q = 2
    pts = _pool(bound, 33, 3601)
    z = SweepEngine.joint_draws(33, 3, 3602)
    engine.set_model(ds)
    want = engine.posterior_joint(pts, 0, z=z, return_chol=True, return_draws=True)
    bad_pts = pts.copy()
    bad_pts[32, 1] = np.nan
    bad_z = z.copy()
    bad_z[2, 32] = np.inf
    bad = [dict(null=("points",)), dict(null=("z",)), dict(z=None, S=3), dict(S=0), dict(m=0), dict(m=-3), dict(output=-1), dict(output=2),
           dict(S=-1), dict(S=_lib.SBO_MAX_PATHS + 1), dict(noise=2), dict(noise=-1), dict(maximize=2), dict(jitter=-1e-9),
           dict(jitter=np.nan), dict(jitter=np.inf), dict(pts=bad_pts), dict(z=bad_z), dict(ctx=False), dict(opts=False)]
    for kw in bad:
        args = dict(pts=pts, z=z)
        args.update(kw)
        rc, res, outs = _raw(engine, **args)
        assert rc == _lib.SBO_E_INVALID and _cleared(res) and _untouched(outs), kw
    rc, _, outs = _raw(engine, pts, z, result=False)
    assert rc == _lib.SBO_E_INVALID and _untouched(outs)
    # the cap: the refusal comes before anything is read or written, so the points are a block of untouched zero pages
    rc, res, outs = _raw(engine, np.zeros((_lib.SBO_JOINT_MAX_POINTS + 1, 2)))
    assert rc == _lib.SBO_E_UNSUPPORTED and _cleared(res) and _untouched(outs)
    assert "SBO_JOINT_MAX_POINTS" in engine._lib.sbo_last_error().decode()
    with pytest.raises(ValueError, match="SBO_JOINT_MAX_POINTS"):
        engine.posterior_joint(np.zeros((_lib.SBO_JOINT_MAX_POINTS + 1, 2)))
    # a duplicated point without jitter and noise: its second row has a zero pivot
    # (nine scattered points: every other pivot is far above the threshold.  With a jitter the Schur complement of the pair is
    # [[s + j, s], [s, s + j]], whose second pivot j (2 s + j) / (s + j) is at most 2 j)
    twice, z9 = pts[:9].copy(), np.ascontiguousarray(z[:, :9])
    twice[5] = twice[2]
    rc, res, outs = _raw(engine, twice, z9, jitter=0.0)
    message = engine._lib.sbo_last_error().decode()
    print(message)
    assert rc == _lib.SBO_E_INVALID and _cleared(res) and _untouched(outs)
    assert "row 5" in message and "jitter" in message and "noise" in message
    with pytest.raises(ValueError, match="row 5"):
        engine.posterior_joint(twice, 0, z=z9, jitter=0.0)
    ok = engine.posterior_joint(twice, 0, z=z9, jitter=1e-8, return_chol=True)
    jit = float(ds["Y_std"][0]) ** 2 * 1e-8 * bo.params(ds, 0)[1]
    rel5 = ok["chol"][5, 5] ** 2 / (ok["cov"][5, 5] + jit)
    print("the duplicate's pivot with jitter 1e-8:", rel5, "bound", 2.0 * jit / (ok["cov"][5, 5] + jit), "pivot_min", ok["pivot_min"], ok["pivot_row"])
    assert ok["pivot_row"] == 5 and 0.0 < rel5 <= 2.1 * jit / (ok["cov"][5, 5] + jit)
    rc, res, outs = _raw(engine, twice, None, jitter=0.0, chol=False)         # (no factor is needed: nothing to refuse)
    assert rc == _lib.SBO_OK and res.pivot_row == -1 and np.isnan(res.pivot_min)
    assert (outs[2] == STALE_FILL).all() and not (outs[0] == STALE_FILL).any() and outs[1][:9, :9].tobytes() != np.full((9, 9), STALE_FILL).tobytes()
    rc, res, _ = _raw(engine, pts, z)
    assert rc == _lib.SBO_OK and list(res.index[:3]) == want["index"].tolist() and list(res.index[3:]) == [-1] * (_lib.SBO_MAX_PATHS - 3)
    assert np.array(res.value[:3]).tobytes() == want["value"].tobytes() and np.isnan(np.array(res.value[3:])).all()
    assert res.pivot_row == want["pivot_row"] and res.pivot_min == want["pivot_min"]
    again = engine.posterior_joint(pts, 0, z=z, return_chol=True, return_draws=True)
    for k in want:
        assert np.asarray(want[k]).tobytes() == np.asarray(again[k]).tobytes(), k


# ------------------------------------------------------------------------------------------ 10. host class
def test_exact_thompson_of_the_host_class():
    """Benoit, 40 samples around (1.0, -0.6), b = 2, a 40 x 40 grid (at most 1600 members of S): Thompson(3, exact=True) proposes three
    members of the sweep's S, each the arg-min of its exact draw over S with the draw's minimum as its value; Thompson(3) without the
    keyword gives what it gave before the exact call."""
    m = _bo(40, (1.0, -0.6), 0.5, 2.0, (40, 40))
    ds, pts = m.inference_datasets, m._all_points()
    X0, value0 = m.Thompson(3)
    X, value = m.Thompson(3, exact=True)
    S = m.engine.mask("S")
    members = pts[np.nonzero(S)[0]]
    assert X.shape == (3, 2) and value.shape == (3,) and 3 < len(members) <= _lib.SBO_JOINT_MAX_POINTS
    for x in X:
        assert (members == x).all(axis=1).any()
    full = m.engine.posterior_joint(members, 0, 3, 0, return_draws=True, return_chol=True)
    assert value.tobytes() == full["draws"].min(axis=0).tobytes()
    assert np.array_equal(X, members[np.argmin(full["draws"], axis=0)])
    own = full["mean"][:, None] + full["chol"] @ SweepEngine.joint_draws(len(members), 3, 0).T
    assert float(np.max(np.abs(full["draws"] - own) / (1.0 + np.abs(own)))) <= 1e-12
    ref = jo.joint_solve(ds, 0, members, None, False, 1e-6)
    assert float(np.max(np.abs((full["mean"] - ds["Y_mean"][0]) / ds["Y_std"][0] - ref["mean"]))) < TOL64
    X1, value1 = m.Thompson(3)
    assert X1.tobytes() == X0.tobytes() and value1.tobytes() == value0.tobytes()
