"""sbo_mean_grad and sbo_lipschitz on the device against oracle.mean_grad and the NumPy / SciPy twin
(tests/lipschitz_oracle.py): values, independence of the list, the bound's contract on four configs, edge cases and refusals,
read-only behaviour, the two tiers of the solver, and the host classes' ``lipschitz="box"``."""
import ctypes as C

import numpy as np
import pytest

import oracle
import lipschitz_oracle as lo_
import model_remove as mr
import refine_sets_oracle as rs
import safebo_amd
from safebo_amd import GoOSE, SafeOpt, _lib, synthetic

pytestmark = pytest.mark.gpu

RTOL = 1e-9          # per output, of the largest |grad_o| over the test's points: what the suite holds L to against the same oracle


def _config_b(n):
    """Config B's data as tests/test_gpu_model_loo.py makes it: -> (ds, use_invK)."""
    if n < 3:
        ds0 = synthetic.make_config("B", n=90, seed=5)["ds"]
        return mr.with_rows(ds0, ds0["X_norm"][:n], ds0["Y_norm"][:n]), True
    cfg = synthetic.make_config("B", n=n, seed=5)
    if n < 300:
        return cfg["ds"], True
    return synthetic.make_dataset(cfg["X"], cfg["Y"], synthetic.default_hypopt(2, 2, log_sn=-1.0)), False


def _box_points(lo, hi, count, seed):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(lo, hi, size=(count, len(lo)))
    pts[0] = lo
    if count > 1:
        pts[-1] = hi
    return pts


def _check_grad(engine, ds, pts, tag):
    got, inf = engine.mean_grad(pts, infnorm=True)
    want = oracle.mean_grad(pts, ds)
    assert got.shape == want.shape
    for o in range(want.shape[1]):
        scale = np.max(np.abs(want[:, o, :]))
        dev = np.max(np.abs(got[:, o, :] - want[:, o, :]))
        print(f"{tag} output {o}: max |dgrad| {dev:.3e} of max |grad| {scale:.3e}")
        assert dev <= RTOL * scale, (tag, o, dev, scale)
    assert np.array_equal(inf, np.max(np.abs(got), axis=2))
    return got


B_LO, B_HI = np.array([-0.6, -1.0]), np.array([1.5, 1.0])


# ------------------------------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 300, 2048])
def test_mean_grad_over_n(engine, n):
    ds, use_invK = _config_b(n)
    engine.set_model(ds, use_invK=use_invK)
    _check_grad(engine, ds, _box_points(B_LO, B_HI, 300, 100 + n), f"n {n}")


@pytest.mark.parametrize("d", [1, 3, 6, 8])
def test_mean_grad_over_d(engine, d):
    rng = np.random.default_rng(200 + d)
    X = rng.uniform(-1.0, 1.0, size=(40, d))
    Y = np.column_stack([np.sum(np.sin(2.0 * X), axis=1), np.sum(X * X, axis=1) - 0.5 * X[:, 0]])
    ds = synthetic.make_dataset(X, Y, synthetic.default_hypopt(d, 2))
    engine.set_model(ds)
    _check_grad(engine, ds, _box_points(-np.ones(d), np.ones(d), 300, 210 + d), f"d {d}")


@pytest.mark.parametrize("q", [1, 3, 8])
def test_mean_grad_over_q(engine, q):
    rng = np.random.default_rng(300 + q)
    X = rng.uniform(B_LO, B_HI, size=(40, 2))
    cols = [synthetic.benoit(X)] + [np.sin((1.0 + 0.3 * k) * X[:, 0]) - np.cos(0.7 * k * X[:, 1]) for k in range(6)]
    Y = np.column_stack(cols)[:, :q]
    hyp = synthetic.default_hypopt(2, q)
    for o in range(q):
        hyp[:, o] = synthetic.default_hypopt(2, 1, log_ell=-0.3 - 0.1 * o, log_sf=0.05 * o, log_sn=-2.0 + 0.1 * o)[:, 0]
    hyp[1, :] += 0.2                                           # (another length-scale on axis 1)
    ds = synthetic.make_dataset(X, Y, hyp)
    engine.set_model(ds)
    _check_grad(engine, ds, _box_points(B_LO, B_HI, 300, 310 + q), f"q {q}")


@pytest.mark.parametrize("n_points", [1, 255, 257, 100_000])
def test_mean_grad_over_list_lengths(engine, n_points):
    cfg = synthetic.make_config("A")
    engine.set_model(cfg["ds"])
    _check_grad(engine, cfg["ds"], _box_points(B_LO, B_HI, n_points, 400 + n_points % 7), f"N {n_points}")


def test_mean_grad_with_a_zero_prior_mean(engine):
    """GP_Robust's prior (mean_prior = 0 for every output).  The oracle's prior is -2 Y_mean / Y_std: with Y_mean = 0 it is zero, and
    Y_mean enters the gradient nowhere else."""
    ds = synthetic.make_config("B", n=64)["ds"]
    engine.set_model(ds, mean_prior=np.zeros(2))
    _check_grad(engine, dict(ds, Y_mean=np.zeros(2)), _box_points(B_LO, B_HI, 300, 500), "zero prior")
    engine.set_model(ds)
    _check_grad(engine, ds, _box_points(B_LO, B_HI, 300, 500), "default prior")


def benoit_f(u, noise=0):
    return u[0] ** 2 + u[1] ** 2 + u[0] * u[1]


def benoit_g(u, noise=0):
    return -(1. - u[0] + u[1] ** 2 + 2. * u[1])


def _mirror(cls, n=12, grid=(50, 50), b=3.0, **kw):
    """As tests/test_host_classes.py::_init."""
    m = cls([benoit_f, benoit_g], np.stack([B_LO, B_HI], axis=1), b, grid=grid, **kw)
    X, Y = m.Data_sampling(n, np.array([1.4, -.8]), 0.3)
    m.fixed_hyper = synthetic.default_hypopt(2, 2)
    m.GP_initialization(X, Y, "RBF", multi_hyper=5, var_out=True)
    return m


def test_mean_grad_after_append_and_remove():
    """A factor an append has grown and one a removal has swapped, against the oracle on the host dataset the mirror keeps."""
    m = _mirror(SafeOpt.BO)
    pts = _box_points(B_LO, B_HI, 300, 600)
    rng = np.random.default_rng(601)
    for _ in range(3):
        x = np.array([1.4, -.8]) + rng.uniform(-0.25, 0.25, size=2)
        m.add_sample(x, m.calculate_plant_outputs(x), incremental=True)
    assert m.engine.n == 15
    got = _check_grad(m.engine, m.inference_datasets, pts, "appended")
    assert np.array_equal(got, m.mean_grad(pts))
    m.remove_sample(2)
    m.remove_sample(0)
    assert m.engine.n == 13
    _check_grad(m.engine, m.inference_datasets, pts, "removed")
    seeds = m.engine.lipschitz_seeds(B_LO, B_HI)
    assert np.array_equal(seeds, lo_.default_seeds(m.inference_datasets, B_LO, B_HI))    # (the engine followed the appends and removals)
    m.engine.close()


# ------------------------------------------------------------------------------------------ 2. independence
def test_mean_grad_does_not_depend_on_the_list(engine):
    cfg = synthetic.make_config("A")
    engine.set_model(cfg["ds"])
    pts = _box_points(B_LO, B_HI, 100_000, 700)
    x = np.array([0.3217, -0.4481])
    alone, alone_inf = engine.mean_grad(x, infnorm=True)
    for pos in (0, 7, 99_999):
        lst = pts.copy()
        lst[pos] = x
        g, inf = engine.mean_grad(lst, infnorm=True)
        assert g[pos].tobytes() == alone[0].tobytes() and inf[pos].tobytes() == alone_inf[0].tobytes(), pos
        g2, inf2 = engine.mean_grad(lst, infnorm=True)
        assert g2.tobytes() == g.tobytes() and inf2.tobytes() == inf.tobytes()
        assert np.array_equal(inf, np.max(np.abs(g), axis=2))


# ------------------------------------------------------------------------------------------ 3. the bound
@pytest.mark.parametrize("name", ["A", "B64", "C64", "D128"])
def test_lipschitz_contract(engine, name):
    """Default seeds, top = 4, every output.  The fine-grid maximum is taken twice.  With the device's own evaluator (``mean_grad`` on
    the same fine grid) L >= it holds exactly, no tolerance: both sides are one arithmetic.  Against the oracle's fine-grid maximum
    the comparison carries the 1e-9 relative that this file holds the device's values to against the same oracle: where the
    maximum sits on a seed (config B, n = 64, output 1: the box corner (-0.6, -1), which is a default seed and a fine-grid point) both
    sides are the value at one and the same point in two arithmetics -- device 5.8676871146897, oracle 5.867687114689717, 3 ulp apart
    -- and an exact >= between them would test the rounding of two formulas of the kernel distance, not the solver."""
    c = lo_.case(name)
    ds, lo, hi = c["ds"], c["lo"], c["hi"]
    engine.set_model(ds)
    d, q = engine.d, engine.q
    out = engine.lipschitz(lo, hi, top=4)
    seeds = engine.lipschitz_seeds(lo, hi)
    assert np.array_equal(seeds, lo_.default_seeds(ds, lo, hi))
    _, sinf = engine.mean_grad(seeds, infnorm=True)
    fine_dev = np.max(engine.mean_grad(oracle.grid_points(lo, hi, [lo_.CASES[name][2]] * d), infnorm=True)[1], axis=0)
    assert np.all(np.abs(fine_dev - c["fine"]) <= RTOL * c["fine"])
    print(f"{name}: fine grid on the device {fine_dev}")
    print(f"{name}: L {out['L']} L_seed {out['L_seed']} twin {c['twin']['L']} fine {c['fine']} evaluations {out['evaluations']} "
          f"problems {out['problems']} converged {out['converged']}")
    assert out["seeds_used"] == seeds.shape[0] and out["problems"] == q * d * 2 * 4
    assert out["problems"] <= out["evaluations"] <= 200 * out["problems"] and 0 <= out["converged"] <= out["problems"]
    for o in range(q):
        x = out["x"][o]
        assert np.all(x >= lo) and np.all(x <= hi)
        assert out["L"][o] >= out["L_seed"][o]
        assert out["L_seed"][o].tobytes() == np.max(sinf[:, o]).tobytes()
        g, inf = engine.mean_grad(x, infnorm=True)
        assert out["L"][o].tobytes() == inf[0, o].tobytes()
        assert out["sign"][o] in (1, -1) and out["sign"][o] * g[0, o, out["axis"][o]] == out["L"][o]
        assert out["L"][o] >= fine_dev[o], (name, o, out["L"][o], fine_dev[o])
        assert out["L"][o] >= c["fine"][o] * (1.0 - RTOL), (name, o, out["L"][o], c["fine"][o])
        assert out["L"][o] >= c["twin"]["L"][o] * (1.0 - 1e-9), (name, o, out["L"][o], c["twin"]["L"][o])
    again = engine.lipschitz(lo, hi, top=4)
    for k in out:
        assert np.asarray(out[k]).tobytes() == np.asarray(again[k]).tobytes(), k


# ------------------------------------------------------------------------------------------ 4. edge cases and refusals
@pytest.fixture
def model_a(engine):
    c = lo_.case("A")
    engine.set_model(c["ds"])
    return c


def _attained(engine, out, outputs):
    for o in outputs:
        _, inf = engine.mean_grad(out["x"][o], infnorm=True)
        assert out["L"][o].tobytes() == inf[0, o].tobytes() and out["L"][o] >= out["L_seed"][o]


def test_one_seed(engine, model_a):
    out = engine.lipschitz(model_a["lo"], model_a["hi"], seeds=np.array([0.5, 0.0]))
    assert out["seeds_used"] == 1 and out["problems"] == 2 * 2 * 2     # (one seed per (output, axis, sign), whatever `top`)
    _, inf = engine.mean_grad(np.array([0.5, 0.0]), infnorm=True)
    assert out["L_seed"].tobytes() == inf[0].tobytes()
    _attained(engine, out, range(2))


def test_coarse_grid_seeds_rise(engine, model_a):
    """The 9 x 8 grid of A: the grid's L is 13 % / 3 % below the box's (twin), so L must rise above L_seed."""
    lo, hi = model_a["lo"], model_a["hi"]
    seeds = oracle.grid_points(lo, hi, [9, 8])
    out = engine.lipschitz(lo, hi, seeds=seeds)
    twin = lo_.box_L(model_a["ds"], lo, hi, seeds=seeds, top=4)
    print(f"9 x 8: L {out['L']} L_seed {out['L_seed']} twin {twin['L']}")
    _attained(engine, out, range(2))
    for o in range(2):
        assert out["L"][o] > out["L_seed"][o]
        assert out["L"][o] >= twin["L"][o] * (1.0 - 1e-9)


def test_degenerate_axis_is_held(engine, model_a):
    lo, hi = np.array([-0.6, 0.3]), np.array([1.5, 0.3])
    out = engine.lipschitz(lo, hi)
    assert out["problems"] == 2 * 1 * 2 * 4
    assert np.all(out["x"][:, 1] == 0.3) and np.all((out["x"][:, 0] >= lo[0]) & (out["x"][:, 0] <= hi[0]))
    _attained(engine, out, range(2))
    # (problems run for the axes of span > 0 only: along the line the component g_0 is maximised, g_1 is sampled at seeds and finals)
    line = np.stack([np.linspace(lo[0], hi[0], 2001), np.full(2001, 0.3)], axis=1)
    assert np.all(out["L"] >= np.max(np.abs(oracle.mean_grad(line, model_a["ds"])[:, :, 0]), axis=0) * (1.0 - RTOL))


def test_seeds_outside_the_box_are_skipped(engine, model_a):
    lo, hi = model_a["lo"], model_a["hi"]
    inside = oracle.grid_points(lo, hi, [9, 8])
    bad = np.array([[1.6, 0.0], [0.0, -1.5], [np.nan, 0.0], [0.0, np.inf], [-0.7, 1.1]])
    mixed = np.vstack([bad[:2], inside[:30], bad[2:4], inside[30:], bad[4:]])
    want, out = engine.lipschitz(lo, hi, seeds=inside), engine.lipschitz(lo, hi, seeds=mixed)
    assert out["seeds_used"] == 72 and want["seeds_used"] == 72
    for k in want:
        assert np.asarray(out[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    with pytest.raises(ValueError):
        engine.lipschitz(lo, hi, seeds=bad)


def test_output_mask_and_max_eval(engine, model_a):
    lo, hi = model_a["lo"], model_a["hi"]
    full = engine.lipschitz(lo, hi)
    one = engine.lipschitz(lo, hi, outputs=[1])
    assert one["L"][0] == 0.0 and one["L_seed"][0] == 0.0 and np.all(one["x"][0] == 0.0) and one["problems"] == full["problems"] // 2
    assert one["L"][1].tobytes() == full["L"][1].tobytes() and np.array_equal(one["x"][1], full["x"][1])
    short = engine.lipschitz(lo, hi, max_eval=1)
    assert short["converged"] == 0 and short["evaluations"] == short["problems"]
    assert np.all(short["L"] >= short["L_seed"]) and short["L_seed"].tobytes() == full["L_seed"].tobytes()
    _attained(engine, short, range(2))


def test_refusals(engine, model_a):
    lib = _lib.load()
    lo, hi = model_a["lo"], model_a["hi"]
    seeds = np.ascontiguousarray(oracle.grid_points(lo, hi, [3, 3]))
    sp = seeds.ctypes.data_as(C.c_void_p)
    grad, inf = np.empty((9, 2, 2)), np.empty((9, 2))
    gp, ip = grad.ctypes.data_as(C.c_void_p), inf.ctypes.data_as(C.c_void_p)

    def opts(**kw):
        o = _lib.LipschitzOpts()
        for a in range(2):
            o.lo[a], o.hi[a] = lo[a], hi[a]
        for k, v in kw.items():
            if k in ("lo", "hi"):
                for a in range(2):
                    getattr(o, k)[a] = v[a]
            else:
                setattr(o, k, v)
        return o

    res = _lib.LipschitzResult()
    ctx, INV = engine._ctx, _lib.SBO_E_INVALID
    assert lib.sbo_mean_grad(None, 9, sp, gp, ip) == INV
    assert lib.sbo_mean_grad(ctx, 9, None, gp, ip) == INV
    assert lib.sbo_mean_grad(ctx, 9, sp, None, None) == INV
    assert lib.sbo_mean_grad(ctx, 0, sp, gp, ip) == INV and lib.sbo_mean_grad(ctx, -3, sp, gp, ip) == INV
    assert lib.sbo_mean_grad(ctx, 9, sp, gp, None) == _lib.SBO_OK and lib.sbo_mean_grad(ctx, 9, sp, None, ip) == _lib.SBO_OK
    assert np.array_equal(inf, np.max(np.abs(grad), axis=2))
    good = opts()
    assert lib.sbo_lipschitz(None, C.byref(good), 9, sp, C.byref(res)) == INV
    assert lib.sbo_lipschitz(ctx, None, 9, sp, C.byref(res)) == INV
    assert lib.sbo_lipschitz(ctx, C.byref(good), 9, None, C.byref(res)) == INV
    assert lib.sbo_lipschitz(ctx, C.byref(good), 9, sp, None) == INV
    assert lib.sbo_lipschitz(ctx, C.byref(good), 0, sp, C.byref(res)) == INV
    for bad in (opts(top=17), opts(max_eval=2001), opts(lo=[1.6, -1.0]), opts(hi=[np.inf, 1.0]), opts(lo=[np.nan, -1.0]),
                opts(output_mask=4), opts(output_mask=1 | 8), opts(tol=float("nan"))):
        assert lib.sbo_lipschitz(ctx, C.byref(bad), 9, sp, C.byref(res)) == INV
    assert lib.sbo_lipschitz(ctx, C.byref(opts(top=16, max_eval=2000, output_mask=3)), 9, sp, C.byref(res)) == _lib.SBO_OK
    assert res.problems == 2 * 2 * 2 * 9            # (nine seeds: fewer than top = 16)


def test_fp32_model_and_no_model(engine):
    ds = lo_.case("A")["ds"]
    engine.set_model(ds, dtype="f32")
    for call in (lambda: engine.mean_grad(np.zeros((1, 2))), lambda: engine.lipschitz(B_LO, B_HI, seeds=np.zeros((1, 2)))):
        with pytest.raises(safebo_amd.SafeBOError) as e:
            call()
        assert e.value.code == _lib.SBO_E_UNSUPPORTED
    engine.set_model(ds)
    fresh = safebo_amd.SweepEngine(0)
    try:
        lib, z = _lib.load(), np.zeros((1, 2))
        o, res = _lib.LipschitzOpts(), _lib.LipschitzResult()
        g = np.empty((1, 1, 2))
        zp = z.ctypes.data_as(C.c_void_p)
        assert lib.sbo_mean_grad(fresh._ctx, 1, zp, g.ctypes.data_as(C.c_void_p), None) == _lib.SBO_E_NO_MODEL
        assert lib.sbo_lipschitz(fresh._ctx, C.byref(o), 1, zp, C.byref(res)) == _lib.SBO_E_NO_MODEL
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------ 5. read-only
def test_both_calls_leave_everything_resident_alone(engine, model_a):
    lo, hi = model_a["lo"], model_a["hi"]
    engine.set_grid(lo, hi, [64, 48])

    def snapshot():
        res = engine.sweep_safeopt(3.0, want_masks=True)
        masks = [engine.mask(k).tobytes() for k in ("S", "U", "M")] + [engine.mask("G", 1).tobytes()]
        mean, var = engine.posterior()
        return res, masks, mean.tobytes(), var.tobytes()

    s0 = engine.profile()["guard_audit_samples"]
    before = snapshot()
    s1 = engine.profile()["guard_audit_samples"]
    engine.mean_grad(_box_points(lo, hi, 1000, 800))
    engine.lipschitz(lo, hi)
    assert engine.profile()["guard_audit_samples"] == s1
    assert engine.n_local == 64 * 48
    after = snapshot()
    s2 = engine.profile()["guard_audit_samples"]
    assert s1 >= s0 and s2 >= s1                             # (advanced by the sweeps alone)
    for k in before[0]:
        assert np.asarray(before[0][k]).tobytes() == np.asarray(after[0][k]).tobytes(), k
    assert before[1:] == after[1:]


# ------------------------------------------------------------------------------------------ 6. tiers
@pytest.mark.parametrize("n", [64, 300])
def test_streamed_solver_equals_the_lds_tier(engine, n):
    ds, use_invK = _config_b(n)
    engine.set_model(ds, use_invK=use_invK)
    lds = engine.lipschitz(B_LO, B_HI)
    engine.set_option("lipschitz_lds", 0)
    try:
        streamed = engine.lipschitz(B_LO, B_HI)
    finally:
        engine.set_option("lipschitz_lds", 1)
    for k in lds:
        assert np.asarray(lds[k]).tobytes() == np.asarray(streamed[k]).tobytes(), k
    lib = _lib.load()
    for v in (-1, 2):
        assert lib.sbo_set_option(engine._ctx, b"lipschitz_lds", C.c_int64(v)) == _lib.SBO_E_INVALID
        assert lib.sbo_last_error().decode() == "lipschitz_lds must be 0 (stream X_norm and alpha) or 1 (LDS when they fit)"


# ------------------------------------------------------------------------------------------ 7. mirrors
def _link_holds(m, x, xp, c, L):
    P = rs.problem(m.inference_datasets, m.b, B_LO, B_HI, "var", maximize=True, link=(c, L), pair=True)
    return rs.feasible(P, np.concatenate([x, xp]))[1] >= -1e-9


def test_mirrors_default_is_the_grid():
    a, b = _mirror(SafeOpt.BO), _mirror(SafeOpt.BO, lipschitz="grid")
    try:
        assert a.lipschitz == "grid"
        for i in range(2):
            assert a.maximize_infnorm_mean_grad(i) == float(a.sweep()["L"][i]) == b.maximize_infnorm_mean_grad(i)
        xa, sa = a.Expander(refine=True)
        xb, sb = b.Expander(refine=True)
        assert np.array_equal(xa, xb) and sa == sb
        assert (a.expander_witness is None) == (b.expander_witness is None)
        if a.expander_witness is not None:
            assert a.expander_witness[2] == float(a.sweep()["L"][1]) == b.expander_witness[2]
            assert np.array_equal(a.expander_witness[0], b.expander_witness[0])
        assert a._box_L_cache is None                        # (the default never asks for the box value)
        with pytest.raises(ValueError):
            SafeOpt.BO([benoit_f, benoit_g], np.stack([B_LO, B_HI], axis=1), 3.0, lipschitz="cube")
    finally:
        a.engine.close()
        b.engine.close()


@pytest.mark.parametrize("cls", [SafeOpt.BO, GoOSE.BO])
def test_mirrors_box(cls):
    m = _mirror(cls, lipschitz="box")
    try:
        for i in range(2):
            grid_L = float(m.sweep()["L"][i])
            box_L = float(m.engine.lipschitz(B_LO, B_HI)["L"][i])
            v = m.maximize_infnorm_mean_grad(i)
            print(f"{cls.__module__} output {i}: grid L {grid_L} box L {box_L}")
            assert v >= grid_L and v == max(grid_L, box_L)
            assert m.maximize_infnorm_mean_grad(i, lipschitz="grid") == grid_L
        L1 = m.maximize_infnorm_mean_grad(1)
        if cls is SafeOpt.BO:
            grid_x, grid_std = m.Expander(refine=False)
            x, std = m.Expander(refine=True)
            wit = m.expander_witness
            if wit is None:                                  # (the seed pair no longer satisfies the link: the grid value stays)
                assert np.array_equal(x, grid_x) and std == grid_std
            else:
                assert wit[2] == L1 and wit[1] == 1 and _link_holds(m, x, wit[0], 1, L1)
        else:
            wit = None
            assert m.goose_sweep()["target_index"] < 0       # (no optimistic point on this model's grid: nothing to refine;
            assert np.isinf(m.Target(refine=True)[1])        #  the fixture below has some)
        print(f"{cls.__module__}: witness {'kept the grid value' if wit is None else 'refined'}")
        version = m._box_L_cache[0]
        xn = np.array([1.3, -0.7])
        m.add_sample(xn, m.calculate_plant_outputs(xn), incremental=True)
        v = m.maximize_infnorm_mean_grad(1)
        assert m._box_L_cache[0] == m._model_version != version
        assert v == max(float(m.sweep()["L"][1]), float(m.engine.lipschitz(B_LO, B_HI)["L"][1]))
        assert m.engine.n == 13
    finally:
        m.engine.close()


def test_goose_target_carries_the_box_L():
    """GoOSE.BO.Target(refine=True) with ``lipschitz="box"`` on the committed fixture whose 50 x 50 grid has optimistic points
    (tests/test_gpu_refine_sets.py::_init_fixture): the witness carries max(grid L, box L) and the pair satisfies the link with it."""
    import os
    name = "benoit_n20_50x50"
    z = np.load(os.path.join(rs.GOLDEN, name + ".npz"))
    lo, hi = z["bound"][:, 0].copy(), z["bound"][:, 1].copy()

    def make(**kw):
        m = GoOSE.BO([benoit_f, benoit_g], z["bound"], float(z["b"]), grid=tuple(rs.GRIDS[name]), **kw)
        m.fixed_hyper = z["hypopt"]
        m.GP_initialization(z["X"], z["Y"], "RBF", multi_hyper=5, var_out=True)
        return m

    g, m = make(), make(lipschitz="box")
    try:
        grid_x, grid_lcb = m.Target(refine=False)
        assert np.all(np.isfinite(grid_x))
        ref_x, ref_lcb = g.Target(refine=True)               # (the default: the grid's L)
        if g.target_witness is not None:
            assert g.target_witness[2] == float(g.goose_sweep()["L"][1])
        x, lcb = m.Target(refine=True)
        L1 = max(float(m.goose_sweep()["L"][1]), float(m.engine.lipschitz(lo, hi)["L"][1]))
        assert L1 >= float(g.goose_sweep()["L"][1])
        wit = m.target_witness
        print(f"GoOSE fixture: grid L {float(m.goose_sweep()['L'][1])} box {L1}: {'kept the grid value' if wit is None else 'refined'}")
        if wit is None:
            assert np.array_equal(x, grid_x) and lcb == grid_lcb
        else:
            assert wit[2] == L1 and wit[1] == 1
            P = rs.problem(m.inference_datasets, m.b, lo, hi, "lcb", at="xp", link=(1, L1), pair=True)
            assert rs.feasible(P, np.concatenate([wit[0], x]))[1] >= -1e-9
    finally:
        g.engine.close()
        m.engine.close()
