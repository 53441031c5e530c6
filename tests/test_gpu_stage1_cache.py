"""Stage 1 of the GEMM posterior once per K1b plan, and the minimiser in two launches (M part ahead of the join, G part behind it).

The plan keeps stage 1's images (BilinearPlan::bt_ready): a resident model swept again does not rebuild them.  Whatever one engine did
before -- sweeps at another b, a K1i launch of a new model, another grid, another model, an append, `bilinear` toggled --, its sweeps
and its posterior must be those of a fresh engine brought to the same model, grid and options and nothing else.  Both engines run the
same kernels on the same operands, so every float is compared bit for bit.  The grid is one of whole 64 x 128 tiles with the column
path forced on (col_path 2, fuse_classify 1), the path the lean-2 benchmark sweep takes."""
import numpy as np
import pytest

import history_walk as hw
from safebo_amd import synthetic

pytestmark = pytest.mark.gpu

OPTS = {"fuse_classify": 1, "col_path": 2}
B1, B2 = 3.0, 2.4


def _bits(v):
    a = np.asarray(v)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, ref, label):
    assert sorted(got) == sorted(ref), label
    for k in ref:
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), (label, k, got[k], ref[k])


def _dataset(problem):
    cfg_name, n = hw.PROBLEMS[problem]
    return synthetic.make_config(cfg_name, n=n)["ds"]


def _appends(problem, count):
    """`count` normalised samples of the problem's plant, fixed by the problem alone."""
    cfg_name, n = hw.PROBLEMS[problem]
    cfg = synthetic.make_config(cfg_name, n=n)
    rng = np.random.default_rng(77)
    out = []
    for _ in range(count):
        x = rng.uniform(cfg["bound"][:, 0], cfg["bound"][:, 1])
        y = synthetic.benoit(x[None])[0]
        out.append(((x - cfg["ds"]["X_mean"]) / cfg["ds"]["X_std"], (y - cfg["ds"]["Y_mean"]) / cfg["ds"]["Y_std"]))
    return out


def _set_grid(eng, grid):
    bound = synthetic.make_config("H", n=96)["bound"]
    eng.set_grid(bound[:, 0], bound[:, 1], hw.ALL_GRIDS[grid])


def _probe(eng, label):
    """Two full sweeps (a new model's first runs K1i, the second builds K1b's plan and records its enclosures: from here on both engines
    are on the same plan state), then lean-2 sweeps at two values of b and back, then a full sweep and the posterior."""
    out = {}
    kernels = []
    for i in range(2):
        eng.sweep_safeopt(B1, want_masks=True)
        kernels.append(int(eng.profile()["posterior_kernel"]))
    for i, b in enumerate((B1, B2, B1)):
        out[f"lean2_{i}"] = eng.sweep_safeopt(b, want_masks=True, lean=2)
        prof = eng.profile()
        kernels.append(int(prof["posterior_kernel"]))
        out[f"lean2_{i}"]["tiles_skipped"] = int(prof["k1_tiles_skipped"])
        out[f"lean2_{i}"]["set_path"] = int(prof["set_path"])
        for k in ("S", "U", "M"):
            out[f"lean2_{i}"]["mask_" + k] = eng.mask(k)
        out[f"lean2_{i}"]["mask_G"] = eng.mask("G", 1)
    out["full"] = eng.sweep_safeopt(B2, want_masks=True)
    kernels.append(int(eng.profile()["posterior_kernel"]))
    mean, var = eng.posterior()
    out["posterior"] = {"mean": mean, "var": var}
    return out, kernels


def _check(engine, state, label):
    """`state`: (grid, problem, appended samples, bilinear) -- what a fresh engine is given."""
    import safebo_amd
    grid, problem, n_app, bilinear = state
    got, kernels = _probe(engine, label)
    with safebo_amd.SweepEngine(0) as fresh:
        fresh.set_option("guard_audit_every", 1)
        for k, v in OPTS.items():
            fresh.set_option(k, v)
        fresh.set_option("bilinear", bilinear)
        _set_grid(fresh, grid)
        fresh.set_model(_dataset(problem))
        for xn, yn in _appends(problem, n_app):
            fresh.append_sample(xn, yn)
        ref, rkernels = _probe(fresh, label)
        fresh.synchronize()
        assert fresh.profile()["guard_audit_violations"] == 0
    # (the first sweep of each probe may differ -- K1i on a new model, K1b on a resident one --; the compared ones may not)
    assert kernels[1:] == rkernels[1:], (label, kernels, rkernels)
    for part in ref:
        _same(got[part], ref[part], f"{label}: {part}")
    return kernels


def test_stage1_images_follow_the_plan(engine):
    for k, v in OPTS.items():
        engine.set_option(k, v)
    try:
        _set_grid(engine, "t256x128")
        engine.set_model(_dataset("H"))
        k = _check(engine, ("t256x128", "H", 0, 1), "new model")
        assert k[0] == 6 and k[1:] == [4] * 5, k            # K1i, then the plan: built once, five launches on it
        # the same plan again, straight into sweeps at another b (stage 1 does not run: the images are the plan's)
        k = _check(engine, ("t256x128", "H", 0, 1), "resident model")
        assert k == [4] * 6, k
        # a model change (its first sweep is a K1i launch, whose images go into the same buffer) and back
        engine.set_model(_dataset("B"))
        k = _check(engine, ("t256x128", "B", 0, 1), "model B")
        assert k[0] == 6, k
        engine.set_model(_dataset("H"))
        _check(engine, ("t256x128", "H", 0, 1), "model H again")
        # a grid change and back
        _set_grid(engine, "t128x64")
        _check(engine, ("t128x64", "H", 0, 1), "smaller grid")
        _set_grid(engine, "t256x128")
        _check(engine, ("t256x128", "H", 0, 1), "grid back")
        # an append under a live K1b plan
        for n_app, (xn, yn) in enumerate(_appends("H", 2), 1):
            engine.append_sample(xn, yn)
            _check(engine, ("t256x128", "H", n_app, 1), f"append {n_app}")
        # bilinear 1 -> 0 -> 1 and 1 -> 2 between sweeps
        for value in (0, 1, 2, 1):
            engine.set_option("bilinear", value)
            k = _check(engine, ("t256x128", "H", 2, value), f"bilinear {value}")
            assert k[-1] == (3 if value == 0 else 4), (value, k)
    finally:
        engine.set_option("bilinear", 1)
        for k, v in hw.DEFAULTS.items():
            engine.set_option(k, v)


def _three_sweeps(engine, ds):
    """A model's first sweep (K1i) and two on K1b's plan, all lean 2 with masks: results, kernels and set paths."""
    engine.set_model(ds)
    out = []
    for b in (B1, B2, B1):
        res = engine.sweep_safeopt(b, want_masks=True, lean=2)
        prof = engine.profile()
        res["kernel"], res["set_path"] = int(prof["posterior_kernel"]), int(prof["set_path"])
        res["tiles_skipped"] = int(prof["k1_tiles_skipped"])
        for k in ("S", "U", "M"):
            res["mask_" + k] = engine.mask(k)
        res["mask_G"] = engine.mask("G", 1)
        out.append(res)
    return out


def test_minimiser_split_is_the_same_on_one_stream_and_on_two(engine):
    """col_overlap 1 (M part beside the expander chain, G part behind the join) against 0 (one stream, in order), and K1i's deferred
    gradient launch (grad_defer) against the gate in front of the posterior on a model's first sweep: every index, count, u*, L key
    and guard count equal, bit for bit."""
    for k, v in OPTS.items():
        engine.set_option(k, v)
    try:
        _set_grid(engine, "t256x128")
        ds = _dataset("H")
        runs = {}
        for overlap, defer in ((1, 1), (0, 1), (1, 0), (0, 0)):
            engine.set_option("col_overlap", overlap)
            engine.set_option("grad_defer", defer)
            runs[(overlap, defer)] = _three_sweeps(engine, ds)
        ref = runs[(1, 1)]
        assert [r["kernel"] for r in ref] == [6, 4, 4] and all(r["set_path"] == 1 for r in ref), [(r["kernel"], r["set_path"]) for r in ref]
        assert ref[2]["tiles_skipped"] > 0, "the third sweep runs on recorded enclosures"
        for key, run in runs.items():
            for i, (got, want) in enumerate(zip(run, ref)):
                _same(got, want, f"col_overlap, grad_defer = {key}, sweep {i}")
    finally:
        engine.set_option("col_overlap", 1)
        engine.set_option("grad_defer", 1)
        for k, v in hw.DEFAULTS.items():
            engine.set_option(k, v)
