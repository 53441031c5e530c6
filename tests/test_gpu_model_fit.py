"""sbo_fit_de_batch and sbo_model_fit on the device: the batched DE against q single searches and the host
twin, the polish contract against SciPy L-BFGS-B, the built model against sbo_model_set's and the oracle, repeatability, isolation
of a failed call, the host classes in ``fit_on_device = "model"`` and the host-wait count."""
import os

import numpy as np
import pytest
from scipy.optimize import minimize
from scipy.stats import qmc

import de_twin
import oracle
import robust_oracle
import safebo_amd
from safebo_amd import SafeOpt, StableOpt, _lib
from safebo_amd.GP_Safe import GP, LazyInvK
from test_gpu_fit_local import benoit_data, benoit_f, benoit_g, wo_data

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SAFE_BOX = np.array([[-1.5, 1.5]] * 3 + [[-5.0, -2.0]])          # GP_Safe's box at d = 2 (models/GP_Safe.py:205)
BOUND = np.array([[-.6, 1.5], [-1., 1.]])


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _lhs(box, P, seed):
    return qmc.scale(qmc.LatinHypercube(box.shape[0], seed=seed).random(P), box[:, 0], box[:, 1])


# ---- 1. batched DE = q single DEs ----------------------------------------------------------------------------------------------
def _de_data(n, d, q, seed):
    """q outputs of different roughness and noise over the same inputs: their searches converge at different generations."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    cols = []
    for o in range(q):
        w = rng.uniform(0.3, 1.0, d) * (1.0 + o)
        cols.append(np.sin(X @ w + o) + (0.02 + 0.1 * o) * rng.standard_normal(n))
    Y = np.column_stack(cols)
    Y = (Y - Y.mean(0)) / Y.std(0)
    box = np.array([[-1.5, 1.5]] * d + [[-1.0, 1.0], [-6.0, -0.5]])
    return np.ascontiguousarray(X), np.ascontiguousarray(Y), box


# (n, d, q, P, maxiter): n = 95 / 96 / 97 cross the workgroup-size switch; maxiter 20 and 43 end off the 8-generation cadence
BATCH_CASES = [(14, 2, 3, 20, 40), (95, 1, 2, 12, 20), (96, 6, 8, 16, 43), (97, 2, 3, 20, 40), (128, 2, 2, 24, 24)]


def _mixed_tol(engine, X, Y, box, pop, seeds, maxiter):
    """The largest tolerance of a fixed geometric ladder at which some outputs stop by convergence and others by the limit."""
    for tol in np.geomspace(1.0, 1e-8, 65):
        gens = engine.fit_de_batch(X, Y, box, pop, seeds, maxiter=maxiter, tol=float(tol))[2]
        if np.any(gens < maxiter) and np.any(gens == maxiter):
            return float(tol)
    return None


@pytest.mark.parametrize("n,d,q,P,maxiter", BATCH_CASES)
def test_batched_de_equals_single_searches_bit_for_bit(engine, n, d, q, P, maxiter):
    X, Y, box = _de_data(n, d, q, 7 * n + d)
    pop = np.random.default_rng(n + q).uniform(box[:, 0], box[:, 1], size=(P, d + 2))
    seeds = [0xD15EA5E + 1000 * n + 17 * o for o in range(q)]
    tol = _mixed_tol(engine, X, Y, box, pop, seeds, maxiter)
    assert tol is not None, "no tolerance of the ladder stops some outputs by convergence and others by the limit"
    bx, be, bg = engine.fit_de_batch(X, Y, box, pop, seeds, maxiter=maxiter, tol=tol)
    print(f"n={n} d={d} q={q} P={P} maxiter={maxiter} tol={tol:.3g}: generations {bg.tolist()}")
    assert np.any(bg < maxiter) and np.any(bg == maxiter)
    assert np.all((bg == maxiter) | (bg % 8 == 0))
    for o in range(q):
        sx, se, sg = engine.fit_de(X, Y[:, o], box, pop, seed=seeds[o], maxiter=maxiter, tol=tol)
        assert sg == bg[o], (o, sg, bg[o])
        assert np.array_equal(_bits(se), _bits(be[o])), (o, se, be[o])
        assert np.array_equal(_bits(sx), _bits(bx[o])), (o, sx, bx[o])


@pytest.mark.parametrize("tol", [0.0, 1e3])
def test_batched_de_single_output_and_limits(engine, tol):
    """q = 1 (one output cannot stop both ways in one call: tol = 0 runs to the limit, tol = 1e3 stops at the first check), and
    maxiter = 0 / 1 / 8 / 9 around the cadence."""
    X, Y, box = _de_data(40, 2, 1, 5)
    pop = np.random.default_rng(9).uniform(box[:, 0], box[:, 1], size=(16, 4))
    for maxiter in (0, 1, 8, 9, 30):
        bx, be, bg = engine.fit_de_batch(X, Y, box, pop, [77], maxiter=maxiter, tol=tol)
        sx, se, sg = engine.fit_de(X, Y[:, 0], box, pop, seed=77, maxiter=maxiter, tol=tol)
        assert bg[0] == sg and (sg == maxiter if tol == 0.0 else sg == min(maxiter, 8))
        assert np.array_equal(_bits(se), _bits(be[0])) and np.array_equal(_bits(sx), _bits(bx[0]))


def test_batched_de_output_equals_the_host_twin(engine):
    n, d, q, P, maxiter = 14, 2, 3, 20, 40
    X, Y, box = _de_data(n, d, q, 7 * n + d)
    pop = np.random.default_rng(n + q).uniform(box[:, 0], box[:, 1], size=(P, d + 2))
    seeds = [2 ** 64 - 5, 12345, 99]
    tol = _mixed_tol(engine, X, Y, box, pop, seeds, maxiter)
    assert tol is not None
    bx, be, bg = engine.fit_de_batch(X, Y, box, pop, seeds, maxiter=maxiter, tol=tol)
    o = int(np.argmin(bg))                                # an output that converged while others went on
    assert bg[o] < maxiter
    tx, te, tg = de_twin.fit_de(lambda p: engine.nll_batch(X, Y[:, o], p), box, pop, seeds[o], maxiter, tol)
    assert tg == bg[o] and np.array_equal(_bits(te), _bits(be[o])) and np.array_equal(_bits(tx), _bits(bx[o]))


# ---- 2. the polish contract ----------------------------------------------------------------------------------------------------
def _norm_ds(Xn, Yn):
    """A dataset whose normalised data are (Xn, Yn) themselves (mean 0, std 1)."""
    d, q = Xn.shape[1], Yn.shape[1]
    return {"X_mean": np.zeros(d), "X_std": np.ones(d), "Y_mean": np.zeros(q), "Y_std": np.ones(q),
            "X_norm": np.ascontiguousarray(Xn), "Y_norm": np.ascontiguousarray(Yn)}


def _host_gp(n, d):
    m = GP([lambda u, noise=0: 0.0])
    m.kernel, m.nx_dim, m.n_point = "RBF", d, n
    return m


POLISH_CASES = [("benoit", n) for n in (4, 8, 12, 16, 20)] + [("wo", 64), ("wo", 256)]


@pytest.mark.parametrize("kind,n", POLISH_CASES)
def test_polish_contract_and_host_lbfgsb(engine, kind, n):
    """report.nll <= report.de_nll, hypopt inside the box, nll_batch at hypopt == report.nll exactly, polish = 0 returns the batched
    DE's best; and from the same DE best SciPy L-BFGS-B on the host objective (the "de" mode's polish) reaches f_s with
    nll <= f_s + 1e-4 max(1, |f_s|)."""
    Xn, Yn = benoit_data(n, n) if kind == "benoit" else wo_data(engine, n)
    q, D = Yn.shape[1], 4
    P, maxiter, seed = 15 * D, 48, 11
    pop = _lhs(SAFE_BOX, P, seed)
    ds = _norm_ds(Xn, Yn)
    seeds = [seed + o for o in range(q)]
    bx, be, bg = engine.fit_de_batch(Xn, Yn, SAFE_BOX, pop, seeds, maxiter=maxiter, tol=0.01)
    r0 = engine.model_fit(ds, SAFE_BOX, pop, seed=seed, maxiter=maxiter, tol=0.01, polish=False)
    assert np.array_equal(_bits(r0["hypopt"].T), _bits(bx)) and np.array_equal(_bits(r0["nll"]), _bits(be))
    assert np.array_equal(_bits(r0["de_nll"]), _bits(be)) and np.array_equal(r0["generations"], bg)
    assert np.all(r0["polished"] == 0) and np.all(r0["polish_status"] == -1) and np.all(r0["polish_evals"] == 0)
    r = engine.model_fit(ds, SAFE_BOX, pop, seed=seed, maxiter=maxiter, tol=0.01)
    assert engine.n == n and engine.d == 2 and engine.q == q
    assert np.array_equal(_bits(r["de_nll"]), _bits(be)) and np.array_equal(r["generations"], bg)
    H = r["hypopt"]
    assert np.all(H >= SAFE_BOX[:, :1]) and np.all(H <= SAFE_BOX[:, 1:])
    host = _host_gp(n, 2)
    for o in range(q):
        assert r["nll"][o] <= r["de_nll"][o]
        assert r["polished"][o] == int(r["nll"][o] < r["de_nll"][o])
        if not r["polished"][o]:
            assert np.array_equal(_bits(H[:, o]), _bits(bx[o]))
        assert 0 <= r["polish_status"][o] <= _lib.SBO_FIT_NOT_PD and r["polish_evals"][o] >= 1
        assert np.array_equal(_bits(engine.nll_batch(Xn, Yn[:, o], H[:, o][None, :])), _bits(r["nll"][o:o + 1]))
        res = minimize(host.negative_loglikelihood, bx[o], args=(Xn, Yn[:, o:o + 1]), method="L-BFGS-B", bounds=SAFE_BOX)
        f_s = min(float(res.fun), float(be[o]))            # the "de" mode keeps the DE's best unless the polish is lower
        print(f"{kind} n={n} output {o}: DE {be[o]:.10g} device {r['nll'][o]:.10g} L-BFGS-B {f_s:.10g} "
              f"(status {r['polish_status'][o]}, evals {r['polish_evals'][o]})")
        assert r["nll"][o] <= f_s + 1e-4 * max(1.0, abs(f_s)), (kind, n, o, r["nll"][o], f_s)


# ---- 3. the built model is sbo_model_set's -------------------------------------------------------------------------------------
def _noisy_benoit(n, seed):
    """Benoit observations with measurement noise (the fitted noise level then stays well above the floor of the box, so that
    inverting K on the host -- what the oracle does -- is accurate to the parity bar of tests/test_gpu_parity.py)."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 2))
    X = np.array([1.4, -0.8]) + 0.3 * rng.uniform(size=(n, 1)) ** 0.5 * u / np.linalg.norm(u, axis=1, keepdims=True)
    Y = np.stack([[benoit_f(x), benoit_g(x)] for x in X]) + 0.05 * rng.standard_normal((n, 2))
    return X, Y


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("zero_prior", [False, True])
def test_built_model_is_model_sets_and_matches_the_oracle(engine, zero_prior):
    X, Y = _noisy_benoit(24, 3)
    X_norm, Y_norm, X_mean, X_std, Y_mean, Y_std = oracle.data_normalization(X, Y)
    ds = {"X_mean": X_mean, "X_std": X_std, "Y_mean": Y_mean, "Y_std": Y_std, "X_norm": X_norm, "Y_norm": Y_norm}
    mp = np.zeros(2) if zero_prior else None
    lo, hi, count, b = BOUND[:, 0], BOUND[:, 1], [96, 64], 3.0
    pts = np.random.default_rng(4).uniform(lo, hi, size=(500, 2))

    def run(build):
        engine.set_grid(lo, hi, count)
        build()
        res = engine.sweep_safeopt(b, want_masks=True)
        masks = {k: engine.mask(k) for k in ("S", "U", "M")}
        masks["G1"] = engine.mask("G", 1)
        grid_post = engine.posterior()
        engine.set_points(pts)
        return res, masks, grid_post, engine.posterior()

    out = {}
    a = run(lambda: out.update(engine.model_fit(ds, SAFE_BOX, _lhs(SAFE_BOX, 60, 2), seed=2, maxiter=48, mean_prior=mp)))
    full = dict(ds, hypopt=out["hypopt"])
    bb = run(lambda: engine.set_model(full, use_invK=False, mean_prior=mp))
    assert _same(a[0], bb[0]), (a[0], bb[0])
    assert _same(a[1], bb[1])
    for (m1, v1), (m2, v2) in ((a[2], bb[2]), (a[3], bb[3])):
        assert np.array_equal(_bits(m1), _bits(m2)) and np.array_equal(_bits(v1), _bits(v2))
    # against the oracle with invK inverted on the host from hypopt_out (the tolerance of test_posterior_fp64_grid[use_invK=False])
    ods = oracle.make_inference_dataset(X, Y, out["hypopt"])
    assert np.array_equal(ods["X_norm"], X_norm) and np.array_equal(ods["Y_norm"], Y_norm)
    om, ov = robust_oracle.gp_inference_prior(pts, ods, mp) if zero_prior else oracle.gp_inference(pts, ods)
    mean, var = a[3]
    em = float(np.max(np.abs(mean - om) / np.maximum(1.0, Y_std)))
    ev = float(np.max(np.abs(var - ov) / np.maximum(1.0, Y_std) ** 2))
    print(f"zero_prior={zero_prior}: hypopt {out['hypopt'].T.tolist()}, |mean - oracle| {em:.3g}, |var - oracle| {ev:.3g}")
    assert em < 1e-10 and ev < 1e-10, (em, ev)


# ---- 4. repeatability and isolation --------------------------------------------------------------------------------------------
def test_repeatable_and_a_failed_call_leaves_the_model(engine):
    Xn, Yn = wo_data(engine, 45)
    ds = _norm_ds(Xn, Yn)
    pop = _lhs(SAFE_BOX, 60, 1)
    pts = np.random.default_rng(0).uniform(-1.5, 1.5, size=(300, 2))
    r1 = engine.model_fit(ds, SAFE_BOX, pop, seed=3, maxiter=30)
    engine.set_points(pts)
    b1 = [engine.bounds(2.0, o, k) for o in range(3) for k in ("lcb", "ucb")]
    r2 = engine.model_fit(ds, SAFE_BOX, pop, seed=3, maxiter=30)
    engine.set_points(pts)
    b2 = [engine.bounds(2.0, o, k) for o in range(3) for k in ("lcb", "ucb")]
    for k in ("hypopt", "nll", "de_nll", "generations", "polish_status", "polish_evals", "polished", "host_syncs"):
        assert np.array_equal(r1[k], r2[k]), k
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(b1, b2))

    def still_the_same_model():
        engine.set_points(pts)                            # (drops the resident posterior: the bounds are evaluated again)
        b3 = [engine.bounds(2.0, o, k) for o in range(3) for k in ("lcb", "ucb")]
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(b1, b3))
        assert engine.n == 45 and engine.q == 3

    with pytest.raises(ValueError):                       # P < 4
        engine.model_fit(ds, SAFE_BOX, pop[:3], seed=3, maxiter=30)
    still_the_same_model()
    with pytest.raises(ValueError):                       # lo > hi
        engine.model_fit(ds, SAFE_BOX[:, ::-1], pop, seed=3, maxiter=30)
    still_the_same_model()
    with pytest.raises(ValueError, match="no kernel with name"):
        engine.model_fit(ds, SAFE_BOX, pop, seed=3, maxiter=30, kernel="Matern")
    still_the_same_model()
    with pytest.raises(ValueError):                       # maxiter < 0
        engine.model_fit(ds, SAFE_BOX, pop, seed=3, maxiter=-1)
    still_the_same_model()
    big = _norm_ds(np.zeros((1700, 8)), np.zeros((1700, 1)))      # 8 (n d + 4 n) bytes of LDS > 150 KiB: refused before any launch
    with pytest.raises(safebo_amd.SafeBOError) as ei:
        engine.model_fit(big, np.array([[-1.0, 1.0]] * 10), np.zeros((8, 10)), maxiter=1)
    assert ei.value.code == _lib.SBO_E_UNSUPPORTED
    still_the_same_model()
    bad = _norm_ds(Xn, Yn.copy())
    bad["Y_norm"][7, 1] = np.nan                          # every member of output 1 has a NaN likelihood
    with pytest.raises(ValueError, match="output 1"):
        engine.model_fit(bad, SAFE_BOX, pop, seed=3, maxiter=9)
    still_the_same_model()
    lib, p = _lib.load(), (lambda a: a.ctypes.data)
    one = np.ones(3)
    assert lib.sbo_model_fit(engine._ctx, 0, b"RBF", 45, 2, 3, p(one), p(one), p(one), p(one), p(ds["X_norm"]), p(ds["Y_norm"]), None,
                             None, p(pop), p(np.empty((4, 3))), None) == _lib.SBO_E_INVALID          # opts == NULL
    still_the_same_model()


# ---- 5. the host classes -------------------------------------------------------------------------------------------------------
DE_OPTS = {"seed": 5, "maxiter": 40, "tol": 1e-4}


def _check_fit_against_the_de_twin(m, twin, noise_lo):
    d = m.nx_dim
    assert np.all(m.hypopt[:d + 1] >= -1.5) and np.all(m.hypopt[:d + 1] <= 1.5)
    assert np.all(m.hypopt[d + 1] >= noise_lo) and np.all(m.hypopt[d + 1] <= -2.0)
    assert np.array_equal(m.X_norm, twin.X_norm) and np.array_equal(m.Y_norm, twin.Y_norm)
    for i in range(m.ny_dim):
        f_de = twin.negative_loglikelihood(twin.hypopt[:, i], twin.X_norm, twin.Y_norm[:, i:i + 1])
        f_model = twin.negative_loglikelihood(m.hypopt[:, i], twin.X_norm, twin.Y_norm[:, i:i + 1])
        print(f"  output {i}: NLL model {f_model:.10g}, de {f_de:.10g}")
        assert f_model <= f_de + 1e-3 * max(1.0, abs(f_de)), (i, f_model, f_de)


def test_safeopt_class_in_model_mode(engine):
    def make(mode):
        m = SafeOpt.BO([lambda u, noise=0: benoit_f(u), lambda u, noise=0: benoit_g(u)], BOUND, 3.0, grid=(64, 48))
        m._engine = engine                                 # the suite's one context
        m.fit_on_device, m.de_options = mode, dict(DE_OPTS)
        return m

    m, twin = make("model"), make("de")
    X, Y = m.Data_sampling(14, np.array([1.4, -.8]), 0.3)
    x_new = np.array([1.3, -0.7])
    y_new = m.calculate_plant_outputs(x_new)
    twin.GP_initialization(X, Y, "RBF", multi_hyper=5)
    m.GP_initialization(X, Y, "RBF", multi_hyper=5)
    assert isinstance(m.inference_datasets["invKopt"], LazyInvK) and m._uploaded_version == m._model_version
    _check_fit_against_the_de_twin(m, twin, -5.0)
    first = m.sweep()
    twin.add_sample(x_new, y_new)
    m.add_sample(x_new, y_new)
    _check_fit_against_the_de_twin(m, twin, -5.0)
    assert m._uploaded_version == m._model_version         # the sweep below uploads nothing
    res = m.sweep()
    assert res is not first and not m.invKopt.materialised
    engine.set_model(m.inference_datasets, use_invK=False)
    engine.set_grid(BOUND[:, 0], BOUND[:, 1], m.grid)
    ref = engine.sweep_safeopt(m.b, quirk_L_index=m.reference_quirk_L_index)
    assert _same(res, ref), (res, ref)
    # a dataset with the unread lazy invKopt handed back to GP_inference goes up without it; reading it gives the host expression
    x = np.array([[1.2, -0.6], [1.0, -0.5]])
    mean, var = m.GP_inference(x, dict(m.inference_datasets))
    engine.set_points(x)
    m2, v2 = engine.posterior()                            # (the model of set_model(..., use_invK=False) above)
    assert not m.invKopt.materialised and np.array_equal(_bits(mean), _bits(m2)) and np.array_equal(_bits(var), _bits(v2))
    assert np.array_equal(m.inference_datasets["invKopt"][1], m._invK(m.X_norm, m.hypopt, 1))


def test_stableopt_class_in_model_mode(engine):
    z = np.load(os.path.join(HERE, "golden", "stableopt", "w_shape.npz"))
    plants = [lambda x, noise=0: (float(robust_oracle.w_shape(x[0], x[1])), 0.0)]

    def make(mode):
        bo = StableOpt.BO(plants, np.array([[-1.0, 2.0]]), np.array([[2.0, 4.0]]), 2.0, grid=(301,), grid_d=(201,))
        bo._engine = engine
        bo.fit_on_device, bo.de_options = mode, dict(DE_OPTS)
        return bo

    m, twin = make("model"), make("de")
    X, Y = z["sampled_x"].astype(np.float64), z["sampled_output"].astype(np.float64)
    x_new, y_new = z["observed_x"][0].astype(np.float64), z["observed_output"][0].astype(np.float64)
    twin.GP_initialization(X, Y, "RBF", multi_hyper=1)
    m.GP_initialization(X, Y, "RBF", multi_hyper=1)
    assert m._uploaded_version == m._model_version
    _check_fit_against_the_de_twin(m, twin, -8.0)
    m.robust_sweep(m.ucb)
    twin.add_sample(x_new, y_new)
    m.add_sample(x_new, y_new)
    _check_fit_against_the_de_twin(m, twin, -8.0)
    assert m._uploaded_version == m._model_version
    res = m.robust_sweep(m.ucb)
    assert not m.invKopt.materialised
    engine.set_model(m.inference_datasets, use_invK=False, mean_prior=np.zeros(m.ny_dim))
    engine.set_grid([-1.0, 2.0], [2.0, 4.0], [301, 201])
    ref = engine.sweep_robust(2.0, 1, "ucb")
    assert _same(res, ref), (res, ref)


# ---- 6. host waits do not grow with q ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maxiter", [8, 21])
def test_host_waits_do_not_grow_with_q(engine, maxiter):
    Xn, Yn = wo_data(engine, 45)
    pop = _lhs(SAFE_BOX, 60, 1)
    syncs = []
    for q in (1, 3):
        r = engine.model_fit(_norm_ds(Xn, Yn[:, :q]), SAFE_BOX, pop, seed=1, maxiter=maxiter, tol=0.0, atol=0.0)
        assert np.array_equal(r["generations"], np.full(q, maxiter))
        syncs.append(r["host_syncs"])
    checks = len([g for g in range(maxiter) if (g & 7) == 7 or g + 1 == maxiter])
    assert syncs[0] == syncs[1] == checks + 1, (syncs, checks)
