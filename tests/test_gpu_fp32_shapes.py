"""The fp32 posterior kernels over their shape range (run with -m gpu): K1g<float> (separable tables, grids), K1<float> (generic,
explicit lists and ragged shards) and K1c<float> (generic chunked) against the fp64 NumPy oracle, BASELINE hyper-parameters
(log sigma_n = -2, log ell = -0.5, log sigma_f = 0), both factor modes.  Bar: TOL32 = 1e-4 of tests/test_gpu_parity.py, in its
normalised units (mean / max(1, Y_std), var / max(1, Y_std)^2).  Every case asserts which kernel ran (sbo_profile.posterior_kernel)
and records its error; the worst per kernel is printed (-s / -rA) and kept in profiles/fp32_band_checks.md.
"""
import numpy as np
import pytest

import oracle
from safebo_amd import synthetic

pytestmark = pytest.mark.gpu
TOL32 = 1e-4
K1, K1C, K1G = 1, 2, 3
WORST = {}                       # kernel -> [worst mean error, worst var error] over the cases run so far


def _dataset(d, q, n, seed):
    """The construction of tests/test_gpu_parity.py::test_posterior_fp64_scattered_points_any_dimension at BASELINE."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, size=(n, d))
    Y = np.stack([np.sin(X.sum(1) * (i + 1)) + 0.5 * X[:, 0] for i in range(q)], axis=1)
    return synthetic.make_dataset(X, Y, synthetic.default_hypopt(d, q)), np.full(d, -1.3), np.full(d, 1.3)


def _check(engine, ds, pts, kernel, what):
    mean, var = engine.posterior()
    assert engine.profile()["posterior_kernel"] == kernel, (what, engine.profile()["posterior_kernel"])
    assert mean.dtype == np.float32 and var.dtype == np.float32
    om, ov = oracle.gp_inference(np.asarray(pts, dtype=np.float64), ds)
    assert mean.shape == om.shape and var.shape == ov.shape
    ys = np.maximum(1.0, ds["Y_std"])
    em = float(np.max(np.abs(mean - om) / ys)) if mean.size else 0.0
    ev = float(np.max(np.abs(var - ov) / ys ** 2)) if var.size else 0.0
    w = WORST.setdefault(kernel, [0.0, 0.0])
    w[0], w[1] = max(w[0], em), max(w[1], ev)
    print(f"fp32 kernel {kernel} {what}: |d mean| {em:.3e} |d var| {ev:.3e}   worst so far {w[0]:.3e} {w[1]:.3e}")
    assert np.isfinite(mean).all() and np.isfinite(var).all(), what
    assert em < TOL32 and ev < TOL32, (what, em, ev)
    return mean, var


# d = len(count) in 1 .. 6, q in 1 .. 3, n on both sides of the 16-padding, counts with ragged 16-position strips and 4-line tiles
GRID_CASES = [
    ([37], 2, 1), ([37], 33, 3), ([33, 5], 15, 2), ([17, 3], 16, 3), ([1, 9], 17, 1), ([70, 33], 100, 2), ([70, 33], 300, 3),
    ([13, 11, 10], 33, 3), ([13, 11, 10], 15, 1), ([9, 8, 7, 6], 300, 2), ([9, 8, 7, 6], 16, 1), ([6, 5, 4, 5, 4], 17, 1),
    ([6, 5, 4, 5, 4], 100, 2), ([4, 3, 4, 3, 4, 3], 100, 3), ([4, 3, 4, 3, 4, 3], 2, 2),
]


@pytest.mark.parametrize("count,n,q", GRID_CASES, ids=["x".join(map(str, c)) + f"-n{n}-q{q}" for c, n, q in GRID_CASES])
@pytest.mark.parametrize("use_invK", [True, False])
def test_fp32_table_kernel_on_grids(engine, count, n, q, use_invK):
    d = len(count)
    named = {(2, 2): "B", (2, 3): "C", (4, 2): "D"}.get((d, q))       # the synthetic configs where they fit
    if named:
        cfg = synthetic.make_config(named, n=n)
        ds, lo, hi = cfg["ds"], cfg["bound"][:, 0], cfg["bound"][:, 1]
    else:
        ds, lo, hi = _dataset(d, q, n, 500 + 10 * d + q)
    engine.set_model(ds, dtype="f32", use_invK=use_invK)
    engine.set_grid(lo, hi, count)
    _check(engine, ds, oracle.grid_points(lo, hi, count), K1G, f"grid {count} n={n} q={q} invK={use_invK}")


@pytest.mark.parametrize("use_invK", [True, False])
def test_fp32_shards_of_a_grid(engine, use_invK):
    """The ranges of tests/test_gpu_parity.py::test_shard_ranges_reproduce_the_whole_grid_bitwise on an fp32 model: whole-line shards run
    K1g and reproduce the whole grid bit for bit, ragged ones run the generic kernel and meet the oracle; a one-candidate and an empty
    shard."""
    cfg = synthetic.make_config("B", n=128)
    lo, hi, count = cfg["bound"][:, 0], cfg["bound"][:, 1], [64, 50]
    pts = oracle.grid_points(lo, hi, count)
    engine.set_model(cfg["ds"], dtype="f32", use_invK=use_invK)
    engine.set_grid(lo, hi, count)
    m, v = _check(engine, cfg["ds"], pts, K1G, f"whole 64x50 invK={use_invK}")
    for first, nloc in [(0, 64), (0, 640), (640, 2560), (3136, 64), (64 * 7, 64 * 3)]:
        engine.set_grid(lo, hi, count, first=first, n_local=nloc)
        ms, vs = engine.posterior()
        assert engine.profile()["posterior_kernel"] == K1G
        assert ms.dtype == np.float32 and np.array_equal(ms, m[first:first + nloc]) and np.array_equal(vs, v[first:first + nloc]), (first, nloc)
    for first, nloc in [(0, 1), (0, 1000), (1000, 2200), (3199, 1), (37, 64)]:
        engine.set_grid(lo, hi, count, first=first, n_local=nloc)
        _check(engine, cfg["ds"], pts[first:first + nloc], K1, f"ragged shard ({first}, {nloc}) invK={use_invK}")
    engine.set_grid(lo, hi, count, first=5, n_local=0)
    ms, vs = engine.posterior()
    assert ms.shape == (0, 2) and vs.shape == (0, 2) and ms.dtype == np.float32


@pytest.mark.parametrize("d,q,n", [(1, 1, 9), (3, 2, 40), (5, 3, 64), (6, 1, 200), (8, 2, 33)])
@pytest.mark.parametrize("use_invK", [True, False])
def test_fp32_generic_kernel_on_lists(engine, d, q, n, use_invK):
    """Explicit lists of 1, 63, 65 and 777 points, handed over as float64 and as float32; the oracle evaluates the points the device
    received (the float32 ones widened)."""
    ds, lo, hi = _dataset(d, q, n, 100 + d)
    allpts = np.random.default_rng(200 + d).uniform(lo, hi, size=(777, d))
    engine.set_model(ds, dtype="f32", use_invK=use_invK)
    for N in (1, 63, 65, 777):
        for ptype in (np.float64, np.float32):
            pts = np.ascontiguousarray(allpts[:N].astype(ptype))
            engine.set_points(pts)
            _check(engine, ds, pts.astype(np.float64), K1, f"list d={d} q={q} n={n} N={N} {np.dtype(ptype).name} invK={use_invK}")


@pytest.mark.parametrize("cfg_name,n", [("B", 33), ("H", 300), ("H", 512)])
@pytest.mark.parametrize("use_invK", [True, False])
def test_fp32_chunked_generic_kernel(engine, cfg_name, n, use_invK):
    cfg = synthetic.make_config(cfg_name, n=n)
    pts = np.random.default_rng(n).uniform(cfg["bound"][:, 0], cfg["bound"][:, 1], size=(1500, 2))
    engine.set_option("posterior_path", 2)
    try:
        engine.set_model(cfg["ds"], dtype="f32", use_invK=use_invK)
        engine.set_points(pts)
        _check(engine, cfg["ds"], pts, K1C, f"chunked n={n} N=1500 invK={use_invK}")
    finally:
        engine.set_option("posterior_path", 0)
