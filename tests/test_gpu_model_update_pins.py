"""sbo_model_append, sbo_model_append_batch and sbo_model_remove leave the resident model they left before they became three requests
to one driver (csrc/api.hip: model_update_run; csrc/model.hip: the stage functions and model_update_commit; sbo::ResidentFactor):
tests/golden/model_updates/record_before_one_driver.npz holds what the commit named in its ``commit`` entry gave on an MI355X for the
cases listed here (tests/golden/model_updates/record.py writes it).  The history walk compares an engine with fresh engines of the same
commit and cannot see a change that moves both; here everything is compared for equality across the commit, floats bit for bit (the
device code is the same).  After every step of a case:

  the posterior (mean, var) on a 70 x 65 grid with bilinear = 0 (K1g) and on the default path (K1b / K1i: both axes >= 64), and on a
  300-point list, with the kernel the profile names (models with d != 2: the list only);
  model_loo's arrays and summary;
  one sweep_safeopt result with its masks, and the profile's host_syncs;
  after a refused call the status code and the whole sbo_last_error text, and the same observables, which must equal those before it.

Arrays of more than 16 values are pinned as their SHA-256 digest.

Cases, each the smallest shape at which its path can still go wrong:

  append_*    two single appends from n0 = 1, 15, 16 (the npad step at 16): the first grows a tight factor, the second finds room;
              q = 1, 2, 3 and d = 1, 2, 8 (the three dpad instances); both model sources
  block_*     (n0, k) = (1, 1), (15, 2), (16, 8), (16, 9), (17, 63), (63, 64): k = 8 / 9 is the kp padding step, 63 / 64 the last wave
              column; block_five: five blocks of 64 from n = 90 (the growth copy of a factor that is not tight: capacity 384 crossed)
  remove_*    index 0, middle and last at n = 2, 17, 65 on a tight factor, followed by a second removal (the spare pair in both
              directions); remove_grown_*: the same behind an append
  mixed_*     append, block of 8, remove(0), append, remove(last): library factor at n0 = 20; caller's invK at n0 = 100 on a resident
              grid (chol_async: factor_sync has a chain to wait for); fp32 with its fp64 twin at n0 = 20; fp32 with a stale twin (an
              fp32 model, an fp64 one, then an fp32 one under fp64_recheck = 0: the twin takes no part)
  refuse_*    tests/model_append_batch.py's isolated row (a pivot far below zero on output 1) in the single and the block form, a
              non-finite value in either, k = 0 and k = 65, a removal from n = 1, an index out of range
  capacity    one n = 2048 model: the single append and a block of one at n = SBO_MAX_N, then a removal and a block of two
  no_model    the three calls on a fresh context
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from safebo_amd import _lib as L, synthetic  # noqa: E402

import model_append_batch as mb  # noqa: E402
from test_gpu_recheck_pins import unpack  # noqa: E402  (pack / unpack: the fixture's form)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(HERE, "golden", "model_updates", "record_before_one_driver.npz")
COUNT = [70, 65]
DIGEST_ABOVE = 16
LOO_KEYS = ("resid", "var", "logdet", "lpd", "z_max", "z_argmax", "outside")
MIXED = (("append", 0), ("block", 1, 9), ("remove", 0), ("append", 9), ("remove", -1))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _raw(eng, step, xn, yn):
    """The ABI call itself (the host class refuses some of these arguments on its own): (status, sbo_last_error)."""
    kind = step[0]
    if kind == "append":
        rc = eng._lib.sbo_model_append(eng._ctx, _ptr(xn), _ptr(yn))
    elif kind == "block":
        rc = eng._lib.sbo_model_append_batch(eng._ctx, int(step[1]), _ptr(xn), _ptr(yn))
    else:
        rc = eng._lib.sbo_model_remove(eng._ctx, int(step[1]))
    return {"status": rc, "error": np.frombuffer(eng._lib.sbo_last_error(), dtype=np.uint8) if rc else np.zeros(0, dtype=np.uint8)}


def _observe(eng, box, b):
    """What the resident model gives."""
    lo, hi = box[:, 0], box[:, 1]
    d = box.shape[0]
    pts = np.random.default_rng(300).uniform(lo, hi, size=(300, d))
    out = {"n": eng.n}

    def post(tag):
        mean, var = eng.posterior()
        out[tag + "_mean"], out[tag + "_var"], out[tag + "_kernel"] = mean, var, eng.profile()["posterior_kernel"]
    if d == 2:
        try:
            eng.set_option("bilinear", 0)
            eng.set_grid(lo, hi, COUNT)
            post("grid_bilinear0")
        finally:
            eng.set_option("bilinear", 1)
        eng.set_grid(lo, hi, COUNT)
        post("grid_default")
    eng.set_points(pts)
    post("list")
    loo = eng.model_loo(3.0)
    for k in LOO_KEYS:
        out["loo_" + k] = loo[k]
    if d == 2:
        eng.set_grid(lo, hi, COUNT)
    try:
        res = eng.sweep_safeopt(b, want_masks=True)
        out["sweep_empty"] = 0
    except L.EmptySafeSetError:                                  # (a model of a row or two may have no safe candidate: that is pinned)
        out["sweep_empty"] = 1
    else:
        out.update({"sweep_" + k: v for k, v in res.items()})
        for k in "SUM":
            out["mask_" + k] = np.packbits(eng.mask(k))
        for c in range(1, eng.q):
            out[f"mask_G{c}"] = np.packbits(eng.mask("G", c))
    out["profile_host_syncs"] = eng.profile()["host_syncs"]
    return out


def _same(a, b):
    return a.keys() == b.keys() and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def _run(eng, ds, box, b, rows, steps, dtype="f64", use_invK=True, grid_first=False, before=None):
    """set_model(ds), then the steps, the observables behind each (``grid_first``: the grid is resident before the model, and the
    first step follows set_model at once: nothing has waited for the deferred factor chain of a caller's invK).  A step is ("append", row), ("block", first row, end row),
    ("remove", index) -- through the host class, which must succeed -- or ("refuse", the raw step, x, y)."""
    Xn, Yn = rows
    out = {}
    if grid_first:
        eng.set_grid(box[:, 0], box[:, 1], COUNT)
    if before:
        before()
    eng.set_model(ds if use_invK else {k: v for k, v in ds.items() if k != "invKopt"}, dtype=dtype, use_invK=use_invK)
    if not grid_first:
        out["step0_set"] = last = _observe(eng, box, b)
    for i, step in enumerate(steps, 1):
        name = f"step{i}_{step[0]}"
        if step[0] == "refuse":
            n = eng.n
            out[name + "_call"] = _raw(eng, step[1], np.ascontiguousarray(step[2], dtype=np.float64), np.ascontiguousarray(step[3], dtype=np.float64))
            assert out[name + "_call"]["status"] != 0 and eng.n == n, (name, out[name + "_call"]["status"])
            got = _observe(eng, box, b)
            assert _same(got, last), name
        else:
            if step[0] == "append":
                eng.append_sample(Xn[step[1]], Yn[step[1]])
            elif step[0] == "block":
                eng.append_samples(Xn[step[1]:step[2]], Yn[step[1]:step[2]])
            else:
                eng.remove_sample(step[1] if step[1] >= 0 else eng.n + step[1])
            got = _observe(eng, box, b)
        out[name] = last = got
    return out


def _data(n0, k, d, q, log_sn=-2.0):
    ds, xn, yn, _ = mb.case_data((n0, k, d, q, log_sn, ""))
    return ds, mb.box(d), (xn, yn)


def _append(n0, d, q, use_invK):
    def run(eng):
        ds, box, rows = _data(n0, 2, d, q)
        return _run(eng, ds, box, 3.0, rows, [("append", 0), ("append", 1)], use_invK=use_invK)
    return run


def _block(n0, k, d, q, use_invK):
    def run(eng):
        ds, box, rows = _data(n0, k, d, q)
        return _run(eng, ds, box, 3.0, rows, [("block", 0, k)], use_invK=use_invK)
    return run


def _block_five(eng):
    ds, box, rows = _data(90, 320, 2, 2, log_sn=-1.0)
    return _run(eng, ds, box, 3.0, rows, [("block", 64 * i, 64 * i + 64) for i in range(5)], use_invK=False)


def _remove(n, index, grown):
    def run(eng):
        ds, box, rows = _data(n, 1, 2, 2)
        steps = ([("append", 0)] if grown else []) + [("remove", index)] + ([("remove", 0 if index else -1)] if n + grown > 2 else [])
        return _run(eng, ds, box, 3.0, rows, steps, use_invK=bool(index))
    return run


def _mixed(n0, dtype="f64", use_invK=False, stale_twin=False):
    def run(eng):
        ds, box, rows = _data(n0, 10, 2, 2)

        def before():
            eng.set_model(ds, dtype="f32")                       # (its fp64 twin is built)
            eng.set_model(ds)                                    # (not that twin's model)
            eng.set_option("fp64_recheck", 0)
        try:
            return _run(eng, ds, box, 3.0, rows, MIXED, dtype=dtype, use_invK=use_invK, grid_first=use_invK, before=before if stale_twin else None)
        finally:
            eng.set_option("fp64_recheck", 1)
    return run


def _refusals(eng):
    ds = mb.refusal_model()
    box = np.array([[-2.0, 2.0], [-2.0, 2.0]])
    x_iso, y_ok = ds["X_norm"][-1], np.array([0.1, 0.2])
    xb, yb = mb.refusal_block(ds, 8, 3)
    assert mb.block_pivots(ds, x_iso[None], y_ok[None], 1)[0] < -2.0 and mb.block_pivots(ds, xb, yb, 1)[-1] < -1.0
    xv = xb.copy()
    xv[3] = 0.5 * xv[2]                                          # (the same block without the isolated row: accepted)
    x_nan, y_inf = xb.copy(), yb.copy()
    x_nan[5, 1], y_inf[7, 0] = np.nan, np.inf
    big = np.zeros((65, 2))
    steps = [("refuse", ("append",), x_iso, y_ok), ("refuse", ("block", 8), xb, yb),
             ("refuse", ("append",), np.array([np.nan, 0.0]), y_ok), ("refuse", ("append",), x_iso, np.array([0.1, np.inf])),
             ("refuse", ("block", 8), x_nan, yb), ("refuse", ("block", 8), xb, y_inf),
             ("refuse", ("block", 0), big, big), ("refuse", ("block", 65), big, big),
             ("refuse", ("remove", -1), big, big), ("refuse", ("remove", 64), big, big),
             ("block", 0, 8), ("refuse", ("remove", 72), big, big)]
    return _run(eng, ds, box, 2.0, (xv, yb), steps)


def _refuse_last_row(eng):
    ds, box, rows = _data(2, 1, 2, 2)
    z = np.zeros(2)
    return _run(eng, ds, box, 3.0, rows, [("remove", 1), ("refuse", ("remove", 0), z, z), ("append", 0)], use_invK=False)


def _capacity(eng):
    n = L.SBO_MAX_N
    X = np.random.default_rng(2048).uniform(mb.box(2)[:, 0], mb.box(2)[:, 1], size=(n + 2, 2))
    Xn, Yn, X_mean, X_std, Y_mean, Y_std = synthetic.data_normalization(X, synthetic.benoit(X))
    ds = {"X_mean": X_mean, "X_std": X_std, "Y_mean": Y_mean, "Y_std": Y_std, "X_norm": Xn[:n], "Y_norm": Yn[:n],
          "hypopt": synthetic.default_hypopt(2, 2, log_sn=-1.0)}
    rows = (Xn[n:], Yn[n:])
    steps = [("refuse", ("append",), rows[0][0], rows[1][0]), ("refuse", ("block", 1), rows[0][:1], rows[1][:1]), ("remove", 1000),
             ("refuse", ("block", 2), rows[0], rows[1]), ("append", 0), ("refuse", ("append",), rows[0][1], rows[1][1])]
    return _run(eng, ds, mb.box(2), 3.0, rows, steps, use_invK=False)


def _no_model(eng):
    import safebo_amd
    z = np.zeros((2, 2))
    with safebo_amd.SweepEngine(0) as fresh:
        return {f"call_{'_'.join(map(str, s))}": _raw(fresh, s, z, z) for s in (("append",), ("block", 2), ("remove", 0))}


CASES = {
    "append_n1_d2_q2_invK": _append(1, 2, 2, True),
    "append_n15_d1_q1_K": _append(15, 1, 1, False),
    "append_n16_d8_q3_invK": _append(16, 8, 3, True),
    "append_n15_d2_q3_K": _append(15, 2, 3, False),
    "append_n16_d2_q1_K": _append(16, 2, 1, False),
    "block_n1_k1": _block(1, 1, 2, 2, True),
    "block_n15_k2_d1": _block(15, 2, 1, 2, False),
    "block_n16_k8_q3": _block(16, 8, 2, 3, True),
    "block_n16_k9": _block(16, 9, 2, 2, False),
    "block_n17_k63_d8": _block(17, 63, 8, 2, True),
    "block_n63_k64": _block(63, 64, 2, 2, False),
    "block_five": _block_five,
    **{f"remove_n{n}_{name}": _remove(n, index, 0) for n in (2, 17, 65) for name, index in (("first", 0), ("middle", n // 2), ("last", n - 1))
       if not (n == 2 and name == "middle")},
    **{f"remove_grown_n{n}_{name}": _remove(n, index, 1) for n in (2, 17, 65) for name, index in (("first", 0), ("middle", n // 2), ("last", n))
       if not (n == 2 and name == "middle")},
    "mixed_K_n20": _mixed(20),
    "mixed_invK_async_n100": _mixed(100, use_invK=True),
    "mixed_f32_twin_n20": _mixed(20, dtype="f32"),
    "mixed_f32_stale_twin_n20": _mixed(20, dtype="f32", stale_twin=True),
    "refuse_isolated_row": _refusals,
    "refuse_last_row": _refuse_last_row,
    "capacity": _capacity,
    "no_model": _no_model,
}


def arrays(case, results):
    """{"case/step/key": array}: float64 as uint64 bit patterns, float32 as their bit patterns in int64, everything else int64 / uint8;
    above DIGEST_ABOVE values the SHA-256 digest of those bytes."""
    flat = {}
    for step, res in results.items():
        for k, v in res.items():
            a = np.ascontiguousarray(v)
            if a.dtype == np.float64:
                a = a.view(np.uint64)
            elif a.dtype == np.float32:
                a = a.view(np.uint32).astype(np.int64)
            elif a.dtype != np.uint8:
                assert a.dtype.kind in "iub", (case, step, k, a.dtype)
                a = a.astype(np.int64)
            a = a.reshape(-1)
            if a.size > DIGEST_ABOVE:
                a = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
            flat[f"{case}/{step}/{k}"] = a
    return flat


def check_case(name, got):
    """what makes a case worth pinning: the grid posteriors of an fp64 model of 16 < n <= 512 rows came from K1g and from K1b / K1i, and
    its sweep found a safe set"""
    for step, v in got.items():
        if "grid_default_kernel" in v and 16 < v["n"] <= 512 and v["grid_default_mean"].dtype == np.float64:
            assert v["grid_bilinear0_kernel"] == mb.KERNEL["K1g"], (name, step, v["grid_bilinear0_kernel"])
            assert v["grid_default_kernel"] in (4, 6), (name, step, v["grid_default_kernel"])
            assert v["sweep_empty"] == 0 and v["sweep_count_S"] > 0, (name, step)


@pytest.mark.parametrize("name", list(CASES))
def test_model_updates_leave_what_they_left_before_the_one_driver(engine, name):
    got = CASES[name](engine)
    check_case(name, got)
    flat = arrays(name, got)
    z = unpack(np.load(FIXTURE))
    bad = []
    for key, a in flat.items():
        want = z[key]
        same = a.dtype == want.dtype and np.array_equal(a, want)
        if a.size <= 8 or not same:
            print(f"{key}: {a.tolist() if a.size <= 8 else 'digest'} {'==' if same else '!= ' + str(want.tolist() if want.size <= 8 else 'digest')}")
        if not same:
            bad.append(key)
    assert not bad, bad
    recorded = {k for k in z if k.split("/")[0] == name}
    assert recorded == set(flat), recorded ^ set(flat)
