"""sbo_nll_grad_batch and sbo_fit_local on the device: GP_Classic's NLL gradient and multistart fit (models/GP_Classic.py:168-240)
against the NumPy restatement of tests/nll_grad_oracle.py and SciPy SLSQP."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
from safebo_amd import _lib
from nll_grad_oracle import FLOAT32_EPS, classic_bounds, classic_starts, grad_scale, nll_grad, slsqp_fit

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nll_population.npz")
SHAPES = [(4, 2), (20, 2), (45, 2), (128, 4), (300, 3)]


def _member(n, d):
    fx = np.load(FIXTURE)
    return fx[f"X_{n}_{d}"], fx[f"y_{n}_{d}"], fx[f"H_{n}_{d}"]


def benoit_f(u):
    return u[0] ** 2 + u[1] ** 2 + u[0] * u[1]


def benoit_g(u):
    return -(1. - u[0] + u[1] ** 2 + 2. * u[1])


def _normalise(X, Y):
    return (X - X.mean(0)) / X.std(0), (Y - Y.mean(0)) / Y.std(0)


def benoit_data(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 2))
    X = np.array([1.1, -0.8]) + 0.5 * rng.uniform(size=(n, 1)) * u / np.linalg.norm(u, axis=1, keepdims=True)
    Y = np.stack([[benoit_f(x), benoit_g(x)] for x in X])
    return _normalise(X, Y)


def wo_data(engine, n, seed=3):
    rng = np.random.default_rng(seed)
    U = np.column_stack([rng.uniform(4.0, 7.0, n), rng.uniform(70.0, 100.0, n)])
    return _normalise(U, engine.plant_wo(U))


@pytest.mark.parametrize("n,d", SHAPES)
def test_nll_is_nll_batch_bit_for_bit(engine, n, d):
    X, y, H = _member(n, d)
    nll, grad = engine.nll_grad_batch(X, y, H)
    ref = engine.nll_batch(X, y, H)
    assert np.array_equal(nll.view(np.uint64), ref.view(np.uint64))
    assert grad.shape == H.shape


@pytest.mark.parametrize("n,d", SHAPES)
def test_gradient_matches_oracle(engine, n, d):
    X, y, H = _member(n, d)
    nll, grad = engine.nll_grad_batch(X, y, H)
    checked = 0
    for p, h in enumerate(H):
        f, g = nll_grad(h, X, y)
        if not np.isfinite(f):
            assert nll[p] == np.inf and np.all(np.isnan(grad[p]))
            continue
        scale = grad_scale(h, X, y)
        assert np.all(np.abs(grad[p] - g) <= 1e-8 * scale + 1e-300), (p, grad[p], g, scale)
        checked += 1
    assert checked >= 35


def test_failed_factors_give_inf_and_nan(engine):
    X, y, _ = _member(20, 2)
    X = np.vstack([X, X[:1]])                            # a repeated input: K is singular up to the jitter
    y = np.append(y, y[0])
    H = np.array([[np.nan, 0.0, 0.0, -1.0],             # no pivot survives a NaN
                  [0.0, 0.0, 30.0, -300.0],             # sf2 = e^60 and sn2 underflows: the jitter is lost in rounding
                  [0.0, 0.0, 0.0, -1.0]])
    nll, grad = engine.nll_grad_batch(X, y, H)
    ref = engine.nll_batch(X, y, H)
    assert np.array_equal(nll.view(np.uint64), ref.view(np.uint64))
    assert nll[0] == np.inf and np.all(np.isnan(grad[0]))
    assert np.all(np.isnan(grad[1])) if nll[1] == np.inf else np.all(np.isfinite(grad[1]))
    assert np.isfinite(nll[2]) and np.all(np.isfinite(grad[2]))


def test_repeated_calls_are_identical(engine):
    X, y, H = _member(128, 4)
    a = engine.nll_grad_batch(X, y, H)
    b = engine.nll_grad_batch(X, y, H)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
    assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    Xn, Yn = benoit_data(14, 0)
    starts = classic_starts(2, 10)
    r1 = engine.fit_local(Xn, Yn, classic_bounds(2), starts)
    r2 = engine.fit_local(Xn, Yn, classic_bounds(2), starts)
    for k in r1:
        assert np.array_equal(r1[k], r2[k]), k


def _check_per_start(engine, Xn, Yn, bounds, starts, res, maxiter):
    q, P = res["nll"].shape
    lo, hi = bounds[:, 0], bounds[:, 1]
    for o in range(q):
        f_start = engine.nll_batch(Xn, Yn[:, o], np.clip(starts, lo, hi))      # the device objective at the clipped starts
        for s in range(P):
            st = res["status"][o, s]
            f0 = f_start[s]
            if st == _lib.SBO_FIT_NOT_PD:
                assert not np.isfinite(f0) and res["nll"][o, s] == np.inf
                continue
            x = res["x"][o, s]
            assert np.all(x >= lo) and np.all(x <= hi)
            assert res["nll"][o, s] <= f0
            # the host's NLL at the result: optima sit at the noise floor sn2 = e^-16, where cond(K) reaches 1e9 - 1e10 and two
            # factorisations of the same K differ by cond(K) eps relative
            assert res["nll"][o, s] == pytest.approx(oracle.negative_loglikelihood(x, Xn, Yn[:, o]), rel=1e-5, abs=1e-5)
            assert st in (_lib.SBO_FIT_FTOL, _lib.SBO_FIT_GTOL, _lib.SBO_FIT_MAXITER, _lib.SBO_FIT_LINESEARCH)
            if st == _lib.SBO_FIT_GTOL:
                assert res["pgnorm"][o, s] <= 1e-8
            if st == _lib.SBO_FIT_MAXITER:
                assert res["iters"][o, s] == maxiter
            else:
                assert res["iters"][o, s] <= maxiter
            assert res["evals"][o, s] >= res["iters"][o, s] + 1
        b = int(np.argmin(res["nll"][o]))
        assert res["best_nll"][o] == res["nll"][o, b] and np.array_equal(res["best_x"][o], res["x"][o, b])


@pytest.mark.parametrize("maxiter", [0, 3, 10000])
def test_fit_local_per_start_contract(engine, maxiter):
    Xn, Yn = benoit_data(12, 1)
    starts = classic_starts(2, 10)
    starts[0] = [9.0, -9.0, 0.5, -1.0]                   # outside the box: clipped first
    res = engine.fit_local(Xn, Yn, classic_bounds(2), starts, maxiter=maxiter)
    _check_per_start(engine, Xn, Yn, classic_bounds(2), starts, res, maxiter)
    if maxiter == 0:
        assert np.all(res["iters"] == 0)


def test_fit_local_batches_outputs_bit_for_bit(engine):
    Xn, Yn = wo_data(engine, 64)
    starts = classic_starts(2, 10)
    B = classic_bounds(2)
    res = engine.fit_local(Xn, Yn, B, starts)
    for o in range(Yn.shape[1]):
        one = engine.fit_local(Xn, Yn[:, o:o + 1], B, starts)
        for k in ("x", "nll", "iters", "evals", "pgnorm", "status", "best_x", "best_nll"):
            assert np.array_equal(one[k][0], res[k][o]), (o, k)


CASES = [("benoit", n) for n in (4, 8, 12, 16, 20)] + [("wo", 64), ("wo", 256)]


@pytest.mark.parametrize("kind,n", CASES)
def test_fit_local_reaches_slsqp(engine, kind, n):
    Xn, Yn = benoit_data(n, n) if kind == "benoit" else wo_data(engine, n)
    B = classic_bounds(2)
    starts = classic_starts(2, 10)
    res = engine.fit_local(Xn, Yn, B, starts)
    _check_per_start(engine, Xn, Yn, B, starts, res, 10000)
    for o in range(Yn.shape[1]):
        _, f_ref, _, _ = slsqp_fit(Xn, Yn[:, o], starts, B)
        assert res["best_nll"][o] <= f_ref + 1e-4 * max(1.0, abs(f_ref)), (kind, n, o, res["best_nll"][o], f_ref)


def test_argument_errors(engine):
    X, y, H = _member(20, 2)
    lib = _lib.load()
    ctx = engine._ctx
    p = lambda a: a.ctypes.data_as(C.c_void_p)        # noqa: E731
    nll, grad = np.empty(len(H)), np.empty(H.shape)
    assert lib.sbo_nll_grad_batch(None, 20, 2, p(X), p(y), len(H), p(H), p(nll), p(grad)) == _lib.SBO_E_INVALID
    assert lib.sbo_nll_grad_batch(ctx, 20, 2, None, p(y), len(H), p(H), p(nll), p(grad)) == _lib.SBO_E_INVALID
    assert lib.sbo_nll_grad_batch(ctx, 20, 2, p(X), p(y), 0, p(H), p(nll), p(grad)) == _lib.SBO_E_INVALID
    assert lib.sbo_nll_grad_batch(ctx, 20, 9, p(X), p(y), len(H), p(H), p(nll), p(grad)) == _lib.SBO_E_INVALID
    assert lib.sbo_nll_grad_batch(ctx, 4096, 2, p(X), p(y), len(H), p(H), p(nll), p(grad)) == _lib.SBO_E_INVALID
    assert lib.sbo_nll_grad_batch(ctx, 20, 2, p(X), p(y), len(H), p(H), p(nll), None) == _lib.SBO_E_INVALID
    Y = np.ascontiguousarray(np.column_stack([y, y]))
    B = classic_bounds(2)
    lo, hi = np.ascontiguousarray(B[:, 0]), np.ascontiguousarray(B[:, 1])
    S = classic_starts(2, 4)
    bx, bf = np.empty((2, 4)), np.empty(2)
    args = [ctx, 20, 2, 2, p(X), p(Y), 4, p(S), p(lo), p(hi), 100, 1e-7, 1e-8, p(bx), p(bf), None, None, None, None, None, None]
    assert lib.sbo_fit_local(*args) == _lib.SBO_OK
    for i, bad in [(0, None), (4, None), (7, None), (13, None), (3, 0), (3, 9), (6, 0), (10, -1), (11, -1.0), (12, float("nan"))]:
        a = list(args)
        a[i] = bad
        assert lib.sbo_fit_local(*a) == _lib.SBO_E_INVALID, i
    a = list(args)
    a[8], a[9] = p(hi), p(lo)                            # lo > hi
    assert lib.sbo_fit_local(*a) == _lib.SBO_E_INVALID
    with pytest.raises(ValueError):
        engine.fit_local(X, Y, B[:-1], S)
    with pytest.raises(ValueError):
        engine.nll_grad_batch(X, y, H[:, :-1])
