"""CPU side of sbo_batch_select: the two NumPy routes to the greedy batch under hallucinated observations agree (the identity the
device recursion rests on), every committed case of the GPU test has a top-two gap above batch_oracle.GAP at every step (the condition
under which the device's picks must equal the oracle's exactly), the symbol, its structures and SBO_MAX_BATCH are what
include/safebo.h declares, and the argument checks of SweepEngine.batch_select and BO.Batch fire before anything touches the device
(the device call itself is checked under the gpu marker, tests/test_gpu_batch_select.py).

Agreement of the routes, measured over the committed cases (normalised units): picks identical everywhere; variances of the picks
within 2.3e-13 and of the pool after the last conditioning within 4.3e-13 (both at n = 300, m = 5000, k = 64; the other cases stay
below 2e-13; printed per case by the test, the assertion is TOL64 = 1e-10).  Smallest top-two gap of a case: 1.8e-7 (same case)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from safebo_amd import SafeOpt, SweepEngine, _lib

import batch_oracle as bo
import model_remove as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [bo.case_id(c) for c in bo.CASES]


@pytest.mark.parametrize("i", range(len(bo.CASES)), ids=IDS)
def test_the_two_routes_agree_and_the_case_is_sharp(i):
    c = bo.CASES[i]
    ds, pool, pending, a = bo.reference(i)
    b = bo.select_incremental(ds, c["output"], pool, c["k"], pending)
    assert a["index"].shape == (c["k"],) and np.array_equal(a["index"], b["index"]), (a["index"], b["index"])
    err_p, err_v = float(np.max(np.abs(a["v_pick"] - b["v_pick"]))), float(np.max(np.abs(a["v"] - b["v"])))
    print(bo.case_id(c), "routes", err_p, err_v, "min gap", a["gaps"].min(), b["gaps"].min())
    assert err_p < bo.TOL64 and err_v < bo.TOL64, (err_p, err_v)
    assert a["gaps"].min() > bo.GAP and b["gaps"].min() > bo.GAP, (a["gaps"], b["gaps"])
    assert np.all(np.diff(a["v_pick"]) <= 1e-12)             # (greedy on a shrinking variance: the picks' values do not grow)


def test_the_case_list_covers_every_edge():
    col = lambda key: {c[key] for c in bo.CASES}
    assert col("n") >= {1, 2, 63, 64, 65, 300} and col("m") >= {1, 63, 64, 65, 257, 5000}
    assert col("k") == {1, 2, 8, 64} and col("d") == {1, 2, 4, 8} and col("n_pending") == {0, 1, 5}
    assert {(c["q"], c["output"]) for c in bo.CASES} >= {(3, 0), (3, 2)}
    assert col("use_invK") == {True, False} and any(c["k"] > c["m"] for c in bo.CASES)


def test_follow_and_min_std():
    """follow() along the naive picks reproduces them; min_std between the second and the first std stops after one pick; a pending
    point equal to the first pick changes the batch."""
    i = 4                                                    # (n = 65, m = 257, k = 8, no pending points)
    c = bo.CASES[i]
    assert c["k"] >= 3 and c["n_pending"] == 0
    ds, pool, pending, a = bo.reference(i)
    f = bo.follow(ds, c["output"], pool, a["index"], pending)
    assert np.array_equal(f["v_pick"], a["v_pick"]) and np.array_equal(f["v"], a["v"])
    cut = 0.5 * (a["std"][0] + a["std"][1])
    s = bo.select_naive(ds, c["output"], pool, c["k"], pending, min_std=cut)
    assert list(s["index"]) == [a["index"][0]]
    p = bo.select_naive(ds, c["output"], pool, c["k"] - 1, pool[a["index"][:1]])
    assert np.array_equal(p["index"], a["index"][1:])        # (the first pick as a pending point: the rest of the batch follows)


def test_symbol_structures_and_limit_match_the_header(tmp_path):
    text = open(os.path.join(ROOT, "include", "safebo.h")).read()
    assert int(re.search(r"#define\s+SBO_MAX_BATCH\s+(\d+)", text).group(1)) == _lib.SBO_MAX_BATCH == 64
    assert "sbo_batch_select" in {n for n, _, _ in _lib.SYMBOLS}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safebo.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d\\n", '
                   'sizeof(sbo_batch_opts), offsetof(sbo_batch_opts, min_std), sizeof(sbo_batch_result), offsetof(sbo_batch_result, index), '
                   'offsetof(sbo_batch_result, std), SBO_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.BatchOpts), _lib.BatchOpts.min_std.offset, C.sizeof(_lib.BatchResult), _lib.BatchResult.index.offset,
                   _lib.BatchResult.std.offset, 3]
    lib = _lib.load()
    assert lib.sbo_batch_select(None, None, 1, None, None, None, None) == _lib.SBO_E_INVALID
    res = _lib.BatchResult()
    res.n_selected, res.index[0] = 7, 5
    assert lib.sbo_batch_select(None, None, 1, None, None, None, C.byref(res)) == _lib.SBO_E_INVALID
    assert res.n_selected == 0 and list(res.index) == [-1] * 64 and list(res.std) == [0.0] * 64


def _bare_engine(d=2, q=2):
    """An engine object without a context: every call that reached the library would fail on it."""
    eng = SweepEngine.__new__(SweepEngine)
    eng._ctx, eng._lib, eng.d, eng.q = None, None, d, q
    return eng


@pytest.mark.parametrize("kwargs", [
    dict(points=np.zeros((4, 3)), k=1), dict(points=np.zeros((0, 2)), k=1), dict(points=np.zeros((2, 2, 2)), k=1),
    dict(points=np.zeros((4, 2)), k=0), dict(points=np.zeros((4, 2)), k=65), dict(points=np.zeros((4, 2)), k=1.5),
    dict(points=np.zeros((4, 2)), k=True), dict(points=np.zeros((4, 2)), k=1, output=2), dict(points=np.zeros((4, 2)), k=1, output=-1),
    dict(points=np.zeros((4, 2)), k=1, pending=np.zeros((2, 3))), dict(points=np.zeros((4, 2)), k=60, pending=np.zeros((5, 2))),
    dict(points=np.zeros((4, 2)), k=1, min_std=-1.0), dict(points=np.zeros((4, 2)), k=1, min_std=float("nan")),
    dict(points=np.zeros((4, 2)), k=1, min_std=float("inf")), dict(points=np.array([[0.0, np.nan]]), k=1),
    dict(points=np.zeros((4, 2)), k=1, pending=np.array([[np.inf, 0.0]])),
])
def test_batch_select_checks_its_arguments_on_the_host(kwargs):
    with pytest.raises(ValueError):
        _bare_engine().batch_select(**kwargs)


def test_accepted_arguments_come_back_in_library_form():
    pts, k, o, pend, ms = SweepEngine.batch_arguments(2, 2, [0.5, 1.0], np.int64(3), 1, [[1.0, 2.0]], 0)
    assert pts.shape == (1, 2) and pts.dtype == np.float64 and (k, o, ms) == (3, 1, 0.0) and pend.shape == (1, 2)
    assert SweepEngine.batch_arguments(2, 2, np.zeros((3, 2)), 64, 0, np.zeros((0, 2)), 0.5)[3] is None
    assert SweepEngine.batch_arguments(0, 0, np.zeros((3, 5)), 1, 4, None, 0.0)[0].shape == (3, 5)     # (no model: the library answers)


@pytest.mark.parametrize("kwargs", [dict(k=0), dict(k=65), dict(k=2.0), dict(k=2, pending=np.zeros((1, 3))), dict(k=2, min_std=-0.1),
                                    dict(k=2, min_std=float("nan")), dict(k=40, pending=np.zeros((30, 2)))])
def test_batch_checks_its_arguments_before_the_device(kwargs):
    """BO.Batch refuses bad arguments before it sweeps (the instance holds no model and never creates an engine here)."""
    m = SafeOpt.BO([mr.benoit_f, mr.benoit_g], mr.BOUND, 3.0, grid=(20, 20))
    with pytest.raises(ValueError):
        m.Batch(**kwargs)
    assert "GP-BUCB" in SafeOpt.BO.Batch.__doc__ and "lowest flat index" in SafeOpt.BO.Batch.__doc__
    assert "not reference behaviour" in SafeOpt.BO.Batch.__doc__
