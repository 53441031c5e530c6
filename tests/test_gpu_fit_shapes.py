"""The hyper-parameter fit kernels over their whole shape range: sbo_nll_batch / sbo_nll_grad_batch at d = 1, 5, 8 across the
workgroup-size switch (n = 96) and up to the LDS limits, sbo_fit_de against its bit-exact host twin (tests/de_twin.py), and
sbo_fit_local at new shapes with many outputs."""
import time

import numpy as np
import pytest

import de_twin
import oracle
import safebo_amd
from nll_grad_oracle import grad_scale, nll_grad, slsqp_fit
from safebo_amd import _lib
from test_gpu_fit_local import _check_per_start     # (the per-start contract of the existing fit_local tests)

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
NLL_LDS_N8, GRAD_LDS_N8 = 1920, 1600        # n (d + 2) 8 B <= 150 KiB and n (d + 4) 8 B <= 150 KiB at d = 8


def _data(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    y = np.sin(X @ rng.uniform(0.3, 1.0, d)) + 0.05 * rng.standard_normal(n)
    y = (y - y.mean()) / (y.std() if n > 1 else 1.0)
    return np.ascontiguousarray(X), np.ascontiguousarray(y)


def _population(d, n_floor, n_well, seed, non_pd=True):
    """Members near the noise floor (sn2 = e^-16 + 1e-8), well-conditioned ones (sn2 ~ 0.1 .. 0.5, long-ish length scales), and
    one member with sf2 = exp(800) = inf: no Cholesky factor."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n_floor):
        rows.append(np.concatenate([rng.uniform(-0.5, 0.8, d), [rng.uniform(-0.3, 0.3), -8.0]]))
    for _ in range(n_well):
        rows.append(np.concatenate([rng.uniform(0.0, 1.0, d), [rng.uniform(-0.3, 0.3), rng.uniform(-1.2, -0.35)]]))
    if non_pd:
        rows.append(np.concatenate([np.zeros(d), [400.0, -1.0]]))
    return np.array(rows)


def _K(h, X):
    n, d = X.shape
    W, sf2, sn2 = np.exp(2 * h[:d]), np.exp(2 * h[d]), np.exp(2 * h[d + 1])
    return oracle.cov_mat(X, X, W, sf2) + (sn2 + 1e-8) * np.eye(n)


def _nll_longdouble(h, X, y):
    """NLL from an extended-precision Cholesky of the fp64 K (the reference's expression, no 1/2, no constant)."""
    K = _K(h, X)
    K = ((K + K.T) * 0.5).astype(np.longdouble)
    n = K.shape[0]
    L = np.zeros_like(K)
    for j in range(n):
        v = K[j:, j] - L[j:, :j] @ L[j, :j]
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    z = np.zeros(n, dtype=np.longdouble)
    yl = y.astype(np.longdouble)
    for j in range(n):
        z[j] = (yl[j] - L[j, :j] @ z[:j]) / L[j, j]
    return float(z @ z + 2 * np.sum(np.log(np.diag(L))))


SHAPES = [(n, d) for d in (1, 5, 8) for n in (1, 2, 63, 64, 65, 95, 96, 97, 700)]
_WORST = {"ratio": 0.0}


@pytest.mark.parametrize("n,d", SHAPES)
def test_nll_and_gradient_over_the_shape_range(engine, n, d):
    """Every shape: NLL of nll_grad_batch bit for bit nll_batch's; non-PD member inf with NaN gradient; well-conditioned members
    (cond K <= 1e6) against the NumPy NLL and gradient; noise-floor members (n <= 300) against an extended-precision Cholesky
    within a small multiple of n cond(K) eps."""
    X, y = _data(n, d, 1000 * d + n)
    big = n >= 500
    H = _population(d, 1 if big else 2, 1 if big else 2, n + d)
    t0 = time.perf_counter()
    nll = engine.nll_batch(X, y, H)
    nll2, grad = engine.nll_grad_batch(X, y, H)
    print(f"n={n} d={d} P={len(H)}: {time.perf_counter() - t0:.3f} s")
    assert np.array_equal(nll.view(np.uint64), nll2.view(np.uint64))
    assert nll[-1] == np.inf and np.all(np.isnan(grad[-1]))
    for p, h in enumerate(H[:-1]):
        K = _K(h, X)
        cond = float(np.linalg.cond(K))
        assert np.isfinite(nll[p]), (p, h)
        if cond <= 1e6:
            ref = oracle.negative_loglikelihood(h, X, y)
            assert abs(nll[p] - ref) <= 1e-9 * max(1.0, abs(ref)), (p, nll[p], ref, cond)
            f, g = nll_grad(h, X, y)
            scale = grad_scale(h, X, y)
            assert np.all(np.abs(grad[p] - g) <= 1e-8 * scale + 1e-300), (p, grad[p], g, scale)
        elif n <= 300:
            ref = _nll_longdouble(h, X, y)
            ratio = abs(nll[p] - ref) / max(1.0, abs(ref)) / (n * cond * EPS)
            _WORST["ratio"] = max(_WORST["ratio"], ratio)
            print(f"  member {p}: cond {cond:.2e}, |err| / (n cond eps) = {ratio:.2e} (worst so far {_WORST['ratio']:.2e})")
            assert ratio < 4.0, (p, nll[p], ref, cond)
            assert np.all(np.isfinite(grad[p]))


@pytest.mark.parametrize("d", range(1, 9))
def test_lds_limits_are_refused_cleanly(engine, d):
    """One row past each kernel's LDS budget (or past SBO_MAX_N) is refused before any allocation or launch."""
    n_nll = min(_lib.SBO_MAX_N, (150 * 1024) // (8 * (d + 2)))
    n_grad = min(_lib.SBO_MAX_N, (150 * 1024) // (8 * (d + 4)))
    h = np.zeros((1, d + 2))
    for n_max, calls in ((n_nll, ("nll",)), (n_grad, ("grad", "local"))):
        X = np.zeros((n_max + 1, d))
        y = np.zeros(n_max + 1)
        want = safebo_amd.SafeBOError if n_max < _lib.SBO_MAX_N else ValueError
        for call in calls:
            with pytest.raises(want) as ei:
                if call == "nll":
                    engine.nll_batch(X, y, h)
                elif call == "grad":
                    engine.nll_grad_batch(X, y, h)
                else:
                    engine.fit_local(X, y[:, None], np.array([[-1.0, 1.0]] * (d + 2)), h, maxiter=0)
            if want is safebo_amd.SafeBOError:
                assert ei.value.code == _lib.SBO_E_UNSUPPORTED, (d, call)


def test_nll_at_its_lds_limit(engine):
    """d = 8: n = 1920 is the largest NLL the LDS staging holds -- accepted and correct; n = 1921 refused (UNSUPPORTED)."""
    d = 8
    X, y = _data(NLL_LDS_N8 + 1, d, 5)
    h = np.concatenate([np.full(d, 1.0), [0.0, -0.5]])[None, :]
    with pytest.raises(safebo_amd.SafeBOError) as ei:
        engine.nll_batch(X, y, h)
    assert ei.value.code == _lib.SBO_E_UNSUPPORTED
    X, y = X[:NLL_LDS_N8], y[:NLL_LDS_N8]
    t0 = time.perf_counter()
    nll = engine.nll_batch(X, y, h)
    print(f"nll_batch n={NLL_LDS_N8} d=8 P=1: {time.perf_counter() - t0:.2f} s")
    ref = oracle.negative_loglikelihood(h[0], X, y)
    assert np.linalg.cond(_K(h[0], X)) < 1e6
    assert abs(nll[0] - ref) <= 1e-9 * abs(ref), (nll[0], ref)


def test_gradient_and_local_fit_at_their_lds_limit(engine):
    """d = 8: n = 1600 is the largest gradient / fit_local the LDS holds -- accepted and correct; n = 1601 refused."""
    d, n = 8, GRAD_LDS_N8
    X, y = _data(n + 1, d, 6)
    h = np.concatenate([np.full(d, 1.0), [0.0, -0.5]])[None, :]
    B = np.array([[-1.0, 2.0]] * (d + 1) + [[-3.0, 0.0]])
    for call in (lambda: engine.nll_grad_batch(X, y, h), lambda: engine.fit_local(X, y[:, None], B, h, maxiter=0)):
        with pytest.raises(safebo_amd.SafeBOError) as ei:
            call()
        assert ei.value.code == _lib.SBO_E_UNSUPPORTED
    X, y = X[:n], y[:n]
    t0 = time.perf_counter()
    nll, grad = engine.nll_grad_batch(X, y, h)
    t1 = time.perf_counter()
    res = engine.fit_local(X, y[:, None], B, h, maxiter=0)
    print(f"nll_grad_batch n={n} d=8 P=1: {t1 - t0:.2f} s; fit_local maxiter 0: {time.perf_counter() - t1:.2f} s")
    f, g = nll_grad(h[0], X, y)
    assert abs(nll[0] - f) <= 1e-9 * abs(f)
    assert np.all(np.abs(grad[0] - g) <= 1e-8 * grad_scale(h[0], X, y) + 1e-300), (grad[0], g)
    assert res["status"][0, 0] == _lib.SBO_FIT_MAXITER and res["iters"][0, 0] == 0 and res["evals"][0, 0] == 1
    assert np.array_equal(res["nll"][0, 0:1].view(np.uint64), nll.view(np.uint64)) and np.array_equal(res["x"][0, 0], h[0])


# ---------------------------------------------------------------------------------------------- device DE vs its twin
DE_CASES = [(1, 1, 4), (14, 2, 20), (97, 5, 4), (40, 8, 33)]


def _de_problem(n, d, P, seed, inf_box=False):
    X, y = _data(n, d, seed)
    B = np.array([[-1.5, 1.5]] * d + [[-1.0, 1.0], [-6.0, -0.5]])
    if inf_box:
        B[d] = [-1.0, 400.0]                 # sf2 = exp(2 h) overflows above h ~ 354.9: those members have no factor
    rng = np.random.default_rng(seed + 1)
    pop = rng.uniform(B[:, 0], B[:, 1], size=(P, d + 2))
    if inf_box:
        pop[0] = B[:, 1]                     # the corner: energy inf from the start
    return X, y, B, pop


@pytest.mark.parametrize("n,d,P", DE_CASES)
@pytest.mark.parametrize("maxiter", [0, 1, 7, 8, 9, 40])
@pytest.mark.parametrize("tol", [0.0, 1e3])
def test_device_de_equals_its_host_twin_bit_for_bit(engine, n, d, P, maxiter, tol):
    """sbo_fit_de against tests/de_twin.py with the device's own NLL (nll_batch) as the energy: best_x, best_energy and the
    generation count identical.  tol = 0 runs every generation; tol = 1e3 stops at the first check (gen 8 or the last)."""
    X, y, B, pop = _de_problem(n, d, P, 31 * n + d)
    seed = 0x5EED0000 + n * 100 + d
    bx, be, bg = engine.fit_de(X, y, B, pop, seed=seed, maxiter=maxiter, tol=tol)
    tx, te, tg = de_twin.fit_de(lambda p: engine.nll_batch(X, y, p), B, pop, seed, maxiter, tol)
    assert bg == tg, (bg, tg)
    assert tg == maxiter if tol == 0 else (tg == maxiter or tg % 8 == 0)
    assert np.array_equal(np.float64(be).view(np.uint64), np.float64(te).view(np.uint64)), (be, te)
    assert np.array_equal(bx.view(np.uint64), tx.view(np.uint64)), (bx, tx)


@pytest.mark.parametrize("maxiter", [9, 24])
def test_device_de_with_infinite_energies_equals_its_twin(engine, maxiter):
    """A box whose corner has no Cholesky factor: energies hold inf (no convergence check can pass while they do), the redraws
    land in the overflowing range -- still the twin's result bit for bit."""
    n, d, P = 14, 2, 20
    X, y, B, pop = _de_problem(n, d, P, 77, inf_box=True)
    assert engine.nll_batch(X, y, pop[:1])[0] == np.inf
    seed = 2 ** 64 - 3
    bx, be, bg = engine.fit_de(X, y, B, pop, seed=seed, maxiter=maxiter, tol=1e6)
    energies = []

    def energy(p):
        e = engine.nll_batch(X, y, p)
        energies.append(e)
        return e

    tx, te, tg = de_twin.fit_de(energy, B, pop, seed, maxiter, 1e6)
    assert any(np.isinf(e).any() for e in energies[1:]), "no trial without a factor"
    assert bg == tg and np.float64(be).view(np.uint64) == np.float64(te).view(np.uint64) and np.array_equal(bx.view(np.uint64), tx.view(np.uint64))


# ---------------------------------------------------------------------------------------------- fit_local at new shapes
def many_outputs_problem(n, d):
    """(X, Y [n, SBO_MAX_Q], box, 33 starts, maxiter) of test_fit_local_many_outputs_across_the_workgroup_switch."""
    q, P, maxiter = _lib.SBO_MAX_Q, 33, 12
    X, _ = _data(n, d, 400 + n + d)
    rng = np.random.default_rng(n * d)
    Y = np.column_stack([np.sin(X @ rng.uniform(0.2, 1.0, d) + o) for o in range(q)])
    Y = (Y - Y.mean(0)) / Y.std(0)
    B = np.array([[-2.0, 2.0]] * (d + 1) + [[-8.0, -2.0]])
    return X, Y, B, rng.uniform(B[:, 0], B[:, 1], size=(P, d + 2)), maxiter


def slsqp_problem(n, d):
    """(X, y, box, 3 starts) of test_fit_local_reaches_slsqp_at_new_shapes."""
    X, y = _data(n, d, 900 + n + d)
    B = np.array([[-2.0, 2.0]] * (d + 1) + [[-8.0, -2.0]])
    return X, y, B, np.random.default_rng(d).uniform(B[:, 0], B[:, 1], size=(3, d + 2))


@pytest.mark.parametrize("d", [1, 5, 8])
@pytest.mark.parametrize("n", [95, 96, 97])
def test_fit_local_many_outputs_across_the_workgroup_switch(engine, n, d):
    """q = SBO_MAX_Q outputs x 33 starts = 264 workgroups (more than the CUs): the per-start contract of every (output, start)."""
    X, Y, B, starts, maxiter = many_outputs_problem(n, d)
    q, P = Y.shape[1], len(starts)
    t0 = time.perf_counter()
    res = engine.fit_local(X, Y, B, starts, maxiter=maxiter)
    print(f"fit_local n={n} d={d} q={q} P={P} maxiter={maxiter}: {time.perf_counter() - t0:.2f} s")
    _check_per_start(engine, X, Y, B, starts, res, maxiter)


@pytest.mark.parametrize("n,d", [(97, 1), (96, 5), (95, 8)])
def test_fit_local_reaches_slsqp_at_new_shapes(engine, n, d):
    """From the same few starts the device fit is no worse than SciPy SLSQP with the analytic gradient."""
    X, y, B, starts = slsqp_problem(n, d)
    t0 = time.perf_counter()
    res = engine.fit_local(X, y[:, None], B, starts)
    print(f"fit_local n={n} d={d} P=3 to convergence: {time.perf_counter() - t0:.2f} s")
    _check_per_start(engine, X, y[:, None], B, starts, res, 10000)
    _, f_ref, _, _ = slsqp_fit(X, y, starts, B)
    assert res["best_nll"][0] <= f_ref + 1e-4 * max(1.0, abs(f_ref)), (res["best_nll"][0], f_ref)
