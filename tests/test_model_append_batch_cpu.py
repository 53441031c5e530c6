"""CPU side of sbo_model_append_batch: the NumPy statement of the block update against the inverse of K over all rows and against k
one-row updates, the sharpness of every committed case, the ABI, and the host state of GP.add_samples -- with a stub in the engine's
place (the device call itself is checked under the gpu marker, tests/test_gpu_model_append_batch.py)."""
import ctypes as C

import numpy as np
import pytest

import oracle
from safebo_amd import SafeOpt, _lib, synthetic
from safebo_amd.GP_Safe import LazyInvK

import model_append_batch as mb
from model_remove import init_bo


def _routes(case):
    """Both NumPy routes of a case, every output: (ds of all rows, [(M_block, alpha_block, M_rows, alpha_rows, pivots)])."""
    ds, xn, yn, full = mb.case_data(case)
    out = []
    for o in range(case[3]):
        M, alpha = mb.start_state(ds, o)
        B, Z, rho = mb.block_inputs(ds, xn, yn, o)
        N, a2, piv = mb.append_block_update(M, alpha, B, Z, rho)
        out.append((N, a2) + mb.append_rows_update(M, alpha, B, Z, rho) + (piv,))
    return full, out


@pytest.mark.parametrize("case", mb.CASES, ids=mb.case_id)
def test_every_committed_case_is_sharp(case):
    """The condition the GPU tests rest on: at 500 random points of the box the posterior of the NumPy block route is within
    SHARP = 1e-11 (normalised; a tenth of the fp64 bar) of oracle.gp_inference on the model rebuilt from all rows, and the block
    route agrees with k one-row updates -- in the posterior within SHARP as well, and in M and alpha within 1e-9 relative (both are
    backward-stable routes to the one lower factor with positive diagonal; their difference is a few cond(K) eps, and cond(K) <=
    n sf2 / sn2 < 1e5 on this list).  A case that fails is replaced, not loosened."""
    n0, k, d, q = case[:4]
    full, routes = _routes(case)
    b = mb.box(d)
    pts = np.random.default_rng(1).uniform(b[:, 0], b[:, 1], size=(500, d))
    om, ov = oracle.gp_inference(pts, full)
    gm, gv = mb.posterior_from(full, [r[0] for r in routes], [r[1] for r in routes], pts)
    sm, sv = mb.posterior_from(full, [r[2] for r in routes], [r[3] for r in routes], pts)
    ys = full["Y_std"]
    assert mb.nerr(gm, om, ys, 1) < mb.SHARP and mb.nerr(gv, ov, ys, 2) < mb.SHARP, (mb.nerr(gm, om, ys, 1), mb.nerr(gv, ov, ys, 2))
    assert mb.nerr(gm, sm, ys, 1) < mb.SHARP and mb.nerr(gv, sv, ys, 2) < mb.SHARP
    for N, a2, N2, a3, piv in routes:
        assert piv.shape == (k,) and np.all(piv > 0.0)
        assert np.max(np.abs(N - N2)) < 1e-9 * np.max(np.abs(N)) and np.max(np.abs(a2 - a3)) < 1e-9 * (1.0 + np.max(np.abs(a2)))


@pytest.mark.parametrize("case", [c for c in mb.CASES if c[0] + c[1] <= 130], ids=mb.case_id)
def test_block_update_gives_the_inverse_over_all_rows(case):
    """N from the block update is lower triangular with a positive diagonal, keeps the old factor in its first n rows, N^T N K = I
    for K over all n + k rows at the 1e-9 of tests/test_host_classes.py, and alpha' = inv(K) times the right-hand side."""
    n0, k, d, q = case[:4]
    full, routes = _routes(case)
    for o, (N, a2, _, _, _) in enumerate(routes):
        assert N.shape == (n0 + k, n0 + k) and a2.shape == (n0 + k,)
        assert np.array_equal(np.triu(N, 1), np.zeros_like(N)) and np.all(np.diag(N) > 0.0)
        ell, sf2, sn2 = mb.hyper(full, o)
        K = oracle.cov_mat(full["X_norm"], full["X_norm"], ell, sf2) + sn2 * np.eye(n0 + k)
        assert np.allclose((N.T @ N) @ K, np.eye(n0 + k), atol=1e-9)
        want = full["invKopt"][o] @ (full["Y_norm"][:, o] - oracle.mean_prior(full)[o])
        assert np.max(np.abs(a2 - want)) < 1e-9 * (1.0 + np.max(np.abs(want)))


def test_a_block_of_one_is_the_single_append_formula():
    ds, xn, yn, _ = mb.case_data((20, 1, 2, 2, -2.0, "invK"))
    for o in range(2):
        M, alpha = mb.start_state(ds, o)
        B, Z, rho = mb.block_inputs(ds, xn, yn, o)
        N, a2, _ = mb.append_block_update(M, alpha, B, Z, rho)
        u = M.T @ (M @ B[:, 0])
        s = Z[0, 0] - B[:, 0] @ u
        assert np.allclose(N[20, :20], -u / np.sqrt(s), rtol=1e-13, atol=0) and N[20, 20] == pytest.approx(1.0 / np.sqrt(s), rel=1e-14)
        assert a2[20] == pytest.approx((rho[0] - B[:, 0] @ alpha) / s, rel=1e-12)


def test_refusal_model_margins():
    """The margins the GPU refusal tests use: with x_iso at position 0, 3, 7 of k = 8 and 63 of k = 64, output 1's Schur pivot at that
    position is far below zero (about -2.9) while every pivot before it is >= 0.02, and output 0 accepts the whole block."""
    ds = mb.refusal_model()
    for k, pos in ((8, 0), (8, 3), (8, 7), (64, 63)):
        xn, yn = mb.refusal_block(ds, k, pos)
        p0, p1 = mb.block_pivots(ds, xn, yn, 0), mb.block_pivots(ds, xn, yn, 1)
        assert p0.shape == (k,) and np.all(p0 >= 0.02), (k, pos, p0.min())
        assert p1.shape == (pos + 1,) and p1[pos] < -2.0 and np.all(p1[:pos] >= 0.02), (k, pos, p1)


# ---------------------------------------------------------------------------------------------- ABI
def test_the_library_exports_and_binds_the_symbol():
    raw = C.CDLL(_lib.library_path())
    assert hasattr(raw, "sbo_model_append_batch")
    entry = [s for s in _lib.SYMBOLS if s[0] == "sbo_model_append_batch"]
    assert len(entry) == 1 and entry[0][1] is C.c_int and len(entry[0][2]) == 4
    assert _lib.SBO_MAX_APPEND == 64
    lib = _lib.load()
    x = np.zeros(2)
    assert lib.sbo_model_append_batch(None, 1, x.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p)) == _lib.SBO_E_INVALID
    with pytest.raises(ValueError):
        _lib.check(lib.sbo_model_append_batch(None, 1, None, None))


# ---------------------------------------------------------------------------------------------- host classes
class _NoDevice:
    """In the engine's place: records the calls (the device side is not under test here)."""

    def __init__(self):
        self.calls = []

    def append_samples(self, xn, yn):
        self.calls.append(("block", xn.copy(), yn.copy()))

    def append_sample(self, xn, yn):
        self.calls.append(("append", xn.copy(), yn.copy()))

    def remove_sample(self, index):
        self.calls.append(("remove", index))

    def model_loo(self, b, Y_norm):
        self.calls.append(("loo",))
        n, q = Y_norm.shape
        z = np.zeros(q)
        return {"resid": np.zeros((n, q)), "var": np.ones((n, q)), "z": np.zeros((n, q)), "logdet": z, "lpd": z, "z_max": z,
                "z_argmax": z.astype(np.int64), "outside": z.astype(np.int64), "nll": z}


def _stubbed(n):
    m = init_bo(SafeOpt.BO, n=n)
    m._engine = _NoDevice()
    m._uploaded_version = m._model_version
    return m


def _K(m, i):
    d, n = m.nx_dim, m.X_norm.shape[0]
    return m.Cov_mat("RBF", m.X_norm, m.X_norm, np.exp(2 * m.hypopt[:d, i]), np.exp(2 * m.hypopt[d, i])) \
        + (np.exp(2 * m.hypopt[d + 1, i]) + np.finfo(np.float32).eps) * np.eye(n)


def _rows(m, k, seed=5):
    rng = np.random.default_rng(seed)
    X = np.array([1.4, -0.8]) + 0.25 * rng.uniform(-1, 1, size=(k, 2))
    return X, np.array([m.calculate_plant_outputs(x) for x in X])


def test_add_samples_host_state_is_the_block_bordered_inverse():
    m = _stubbed(10)
    X0, Y0, v0 = m.X.copy(), m.Y.copy(), m._model_version
    consts = [np.array(m.inference_datasets[k]) for k in ("X_mean", "X_std", "Y_mean", "Y_std", "hypopt")]
    X, Y = _rows(m, 5)
    m.add_samples(X, Y)
    assert [c[0] for c in m._engine.calls] == ["block"]
    assert np.allclose(m._engine.calls[0][1], (X - m.X_mean) / m.X_std) and np.allclose(m._engine.calls[0][2], (Y - m.Y_mean) / m.Y_std)
    assert m._model_version == v0 + 1 and m._uploaded_version == m._model_version and m._cand_token is None
    assert m.n_point == 15 and np.array_equal(m.X, np.vstack([X0, X])) and np.array_equal(m.Y, np.vstack([Y0, Y]))
    ds = m.inference_datasets
    assert np.array_equal(ds["X_norm"], (m.X - m.X_mean) / m.X_std) and np.array_equal(ds["Y_norm"], (m.Y - m.Y_mean) / m.Y_std)
    for k, was in zip(("X_mean", "X_std", "Y_mean", "Y_std", "hypopt"), consts):
        assert np.array_equal(np.array(ds[k]), was), k
    for i in range(2):
        assert ds["invKopt"][i].shape == (15, 15)
        assert np.allclose(ds["invKopt"][i] @ _K(m, i), np.eye(15), atol=1e-9)


def test_add_samples_equals_add_sample_row_by_row():
    a, b = _stubbed(10), _stubbed(10)
    X, Y = _rows(a, 4)
    a.add_samples(X, Y)
    for x, y in zip(X, Y):
        b.add_sample(x, y, incremental=True)
    assert np.array_equal(a.X_norm, b.X_norm) and np.array_equal(a.Y_norm, b.Y_norm)
    for i in range(2):
        assert np.allclose(a.invKopt[i], b.invKopt[i], rtol=1e-9, atol=1e-9 * np.max(np.abs(b.invKopt[i])))


def test_blocks_above_the_limit_are_split():
    m = _stubbed(10)
    X, Y = _rows(m, 2 * _lib.SBO_MAX_APPEND + 6)
    v0 = m._model_version
    m.add_samples(X, Y)
    assert [(c[0], c[1].shape[0]) for c in m._engine.calls] == [("block", 64), ("block", 64), ("block", 6)]
    assert np.allclose(np.vstack([c[1] for c in m._engine.calls]), (X - m.X_mean) / m.X_std)
    assert m.n_point == 10 + 134 and m._model_version == v0 + 1 and m._uploaded_version == m._model_version
    for i in range(2):
        assert np.allclose(m.inference_datasets["invKopt"][i] @ _K(m, i), np.eye(144), atol=1e-9)


def test_incremental_false_refits_once():
    m = _stubbed(10)
    fits = []
    real = m.determine_hyperparameters
    m.determine_hyperparameters = lambda Xn, Yn: (fits.append(Xn.shape[0]), real(Xn, Yn))[1]
    X, Y = _rows(m, 3)
    v0 = m._model_version
    m.add_samples(X, Y, incremental=False)
    assert fits == [13] and m._engine.calls == [] and m.n_point == 13
    assert m._model_version == v0 + 1 and m._uploaded_version != m._model_version
    assert np.allclose(m.X_norm.mean(axis=0), 0.0, atol=1e-12)              # (re-normalised over all rows)


def test_window_removes_the_right_count():
    m = _stubbed(12)
    X, Y = _rows(m, 3)
    third = m.X[3].copy()
    m.add_samples(X[:2], Y[:2], window=14)
    assert [c[0] for c in m._engine.calls] == ["block"] and m.n_point == 14
    m._engine.calls.clear()
    X2, Y2 = _rows(m, 3, seed=9)
    m.add_samples(X2, Y2, window=14)
    assert [c[0] for c in m._engine.calls] == ["remove"] * 3 + ["block"] and all(c == ("remove", 0) for c in m._engine.calls[:3])
    assert m.n_point == 14 and np.array_equal(m.X[0], third) and np.array_equal(m.X[-3:], X2)
    for i in range(2):
        assert np.allclose(m.inference_datasets["invKopt"][i] @ _K(m, i), np.eye(14), atol=1e-9)


def test_refit_when_is_asked_once_after_the_block():
    m = _stubbed(10)
    seen = []
    X, Y = _rows(m, 4)
    m.add_samples(X, Y, refit_when=lambda loo: (seen.append(loo["mean"].shape), False)[1])
    assert seen == [(14, 2)] and [c[0] for c in m._engine.calls] == ["block", "loo"]
    fits = []
    real = m.determine_hyperparameters
    m.determine_hyperparameters = lambda Xn, Yn: (fits.append(Xn.shape[0]), real(Xn, Yn))[1]
    m.add_samples(*_rows(m, 2, seed=8), refit_when=lambda loo: True)
    assert fits == [16] and m._uploaded_version != m._model_version


def test_an_unread_lazy_inverse_stays_lazy_over_the_new_rows():
    m = _stubbed(10)
    hyp, Xn = m.hypopt, m.X_norm
    m.invKopt = LazyInvK(lambda i: m._invK(Xn, hyp, i), 2)
    assert m.invKopt[0].shape == (10, 10) and not m.invKopt.materialised
    m.add_samples(*_rows(m, 3))
    assert isinstance(m.invKopt, LazyInvK) and not m.invKopt.materialised and m.invKopt._items[1] is None
    assert m.inference_datasets["invKopt"] is m.invKopt
    for i in range(2):
        assert np.allclose(m.invKopt[i] @ _K(m, i), np.eye(13), atol=1e-9)


@pytest.mark.parametrize("bad", ["x_shape", "y_shape", "rows", "k0", "x_nan", "y_inf", "window_le_k", "window_not_incremental",
                                 "refit_not_incremental", "refit_not_callable"])
def test_value_errors_touch_nothing(bad):
    m = _stubbed(8)
    X, Y = _rows(m, 3)
    kw = {}
    if bad == "x_shape":
        X = X[:, :1]
    elif bad == "y_shape":
        Y = Y[:, 0]
    elif bad == "rows":
        Y = Y[:2]
    elif bad == "k0":
        X, Y = X[:0], Y[:0]
    elif bad == "x_nan":
        X[1, 0] = np.nan
    elif bad == "y_inf":
        Y[2, 1] = np.inf
    elif bad == "window_le_k":
        kw = dict(window=3)
    elif bad == "window_not_incremental":
        kw = dict(incremental=False, window=10)
    elif bad == "refit_not_incremental":
        kw = dict(incremental=False, refit_when=lambda loo: False)
    else:
        kw = dict(refit_when=3)
    v0 = m._model_version
    with pytest.raises(ValueError):
        m.add_samples(X, Y, **kw)
    assert m._engine.calls == [] and m.n_point == 8 and m.X.shape == (8, 2) and m._model_version == v0


def test_engine_append_samples_checks_before_the_call():
    """SweepEngine.append_samples raises for shapes, k = 0, k > SBO_MAX_APPEND and non-finite values before the library is called."""
    import safebo_amd

    class _Lib:
        def sbo_model_append_batch(self, *a):
            raise AssertionError("the library must not be reached")
    eng = object.__new__(safebo_amd.SweepEngine)
    eng._lib, eng._ctx, eng.n, eng.d, eng.q, eng._obs = _Lib(), None, 5, 2, 2, (np.zeros((5, 2)), None, None)
    ok = np.zeros((3, 2))
    for X, Y in ((np.zeros((3, 3)), ok), (ok, np.zeros((3, 1))), (ok, np.zeros((2, 2))), (np.zeros(2), np.zeros(2)),
                 (np.zeros((0, 2)), np.zeros((0, 2))), (np.zeros((65, 2)), np.zeros((65, 2))),
                 (np.array([[0.0, np.nan]] * 3), ok), (ok, np.array([[np.inf, 0.0]] * 3))):
        with pytest.raises(ValueError):
            eng.append_samples(X, Y)
    assert eng.n == 5
    eng._ctx = None                               # (nothing to close)
