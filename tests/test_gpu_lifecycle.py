"""A context's whole life, three times over, beside the session's: everything that allocates lazily is reached (the fp64 twin of an
fp32 model, the column path, a K1i and a K1b plan, the standing audit, sbo_refine, the robust sweep), then the context is closed with
all of it live: the twin, and the audit of the round's last sweep, which nothing has collected.  Every round must give the first
round's results bit for bit (a fresh context carries nothing over), and the session's engine must repeat, bit for bit, a sweep it
took before the rounds (a teardown disturbs no other context)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle  # noqa: E402
import safebo_amd  # noqa: E402
from safebo_amd import synthetic  # noqa: E402
from test_gpu_robust import make_model  # noqa: E402

pytestmark = pytest.mark.gpu


def _flat(res):
    """A result dict as one list of arrays (order of the keys), for exact comparison."""
    return [np.atleast_1d(np.asarray(res[k])) for k in sorted(res) if not isinstance(res[k], dict)]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _round():
    out = []
    small = synthetic.make_config("B", n=16)
    big = synthetic.make_config("B", n=64)
    lo, hi = big["bound"][:, 0], big["bound"][:, 1]
    assert small["ds"]["X_norm"].shape == (16, 2) and small["ds"]["Y_norm"].shape[1] == 2
    with safebo_amd.SweepEngine(0) as eng:
        eng.set_option("guard_audit_every", 1)
        # an fp32 model on an explicit list: the twin is built, and the sweep's recheck re-evaluates candidates on it
        pts = lo + (hi - lo) * np.random.default_rng(5).uniform(size=(512, 2))
        eng.set_points(pts)
        eng.set_model(small["ds"], dtype="f32")
        out += _flat(eng.sweep_safeopt(small["b"], want_masks=True))
        rechecks = eng.profile()["fp64_rechecks"]
        print(f"lifecycle: fp64 rechecks of the fp32 sweep {rechecks} / 512")
        assert rechecks > 0
        out += [eng.mask(k) for k in ("S", "U", "M")]
        # the robust sweep at the smallest shape of test_gpu_robust.py
        ds, rlo, rhi = make_model(2, 1, 25, 5)
        eng.set_model(ds, mean_prior=np.zeros(1))
        eng.set_grid(rlo, rhi, [37, 23])
        out += _flat(eng.sweep_robust(2.0, 1, "ucb"))
        out += list(eng.robust_arrays())
        # an fp64 model on a grid of whole tiles, column path forced: K1i on the first sweep, K1b's plan from the second on, an audit
        # behind every posterior launch
        eng.set_option("col_path", 2)
        eng.set_option("fuse_classify", 1)                   # (auto asks for the fused classification from four workgroups per CU on)
        eng.set_grid(lo, hi, [128, 128])
        eng.set_model(big["ds"], dtype="f64")
        out += _flat(eng.sweep_safeopt(big["b"], lean=2))
        kernels = [eng.profile()["posterior_kernel"]]
        assert eng.profile()["set_path"] == 1
        out += _flat(eng.sweep_goose(big["b"], want_masks=True))
        kernels.append(eng.profile()["posterior_kernel"])
        assert kernels == [6, 4], kernels
        out += list(eng.posterior())
        seeds = oracle.grid_points(lo, hi, [3, 3])
        r = eng.refine(big["b"], seeds, lo=lo, hi=hi)
        out += [r["x"], r["value"], r["status"]]
        # the last call before the context goes: a sweep on K1b's plan whose audit, enqueued on its own stream behind the posterior,
        # nothing has collected -- the sweep waits for the main stream only, and no profile is read behind it
        out += _flat(eng.sweep_goose(big["b"]))
    return out


def test_three_lives_beside_the_session_engine(engine):
    cfg = synthetic.make_config("B", n=64)
    lo, hi = cfg["bound"][:, 0], cfg["bound"][:, 1]
    engine.set_grid(lo, hi, [128, 128])
    engine.set_model(cfg["ds"], dtype="f64")
    engine.sweep_safeopt(cfg["b"])                             # (K1i; the sweep that is repeated runs on K1b's plan)
    before = _flat(engine.sweep_safeopt(cfg["b"], want_masks=True)) + [engine.mask(k) for k in ("S", "U", "M")] + list(engine.posterior())
    first = _round()
    for _ in range(2):
        assert _same(_round(), first)
    after = _flat(engine.sweep_safeopt(cfg["b"], want_masks=True)) + [engine.mask(k) for k in ("S", "U", "M")] + list(engine.posterior())
    assert _same(after, before)
