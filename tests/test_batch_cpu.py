"""CPU side of sbo_batch_select: the two NumPy routes to the greedy batch under hallucinated observations agree (the identity the
device recursion rests on), every committed case of the GPU test has a top-two gap above batch_oracle.GAP at every step (the condition
under which the device's picks must equal the oracle's exactly), the symbol, its structures and SBO_MAX_BATCH are what
include/safebo.h declares, and the argument checks of SweepEngine.batch_select and BO.Batch fire before anything touches the device
(the device call itself is checked under the gpu marker, tests/test_gpu_batch_select.py).

Agreement of the routes, measured over the committed cases (normalised units): picks identical everywhere; variances of the picks
within 2.3e-13 and of the pool after the last conditioning within 4.3e-13 (both at n = 300, m = 5000, k = 64; the other cases stay
below 2e-13; printed per case by the test, the assertion is TOL64 = 1e-10).  Smallest top-two gap of a case: 1.8e-7 (same case).
The cases from n = 505 up (batch_oracle.FIRST_LARGE): picks identical on both routes; variances of the picks within 1.8e-13 and of
the pool within 3.3e-13 (both at n = 600, d = 3; n = 1100, d = 6: 2.9e-13; the d = 2 cases stay below 1.8e-13); at n = 2048, k = 59,
where the recursion is the reference, it differs from one full 2112 x 2112 inverse behind all picks by 1.8e-13 and from one behind
all but the last by 7.2e-14 at the last pick, which is the arg-max there.  Smallest top-two gaps: 2.2e-6 (n = 2048), 2.2e-5
(n = 1020), 1.4e-4 (n = 505); the planted large-m pool: 2.3e-2, its batch the four planted rows.

The case list is held to the constants of csrc/batch.hip and csrc/whiten.hpp, read from the source (test_the_case_list_covers_every_edge)."""
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
    assert a["index"].shape == (c["k"],)
    if c.get("oracle") == "incremental":
        # the reference is the recursion itself: the definition enters through one full inverse behind all picks (the final v)
        # and one behind all but the last (the last pick is the arg-max there, with its value and its gap)
        picks = a["index"]
        last = bo.variance_after(ds, c["output"], pool, picks[:-1], pending)
        assert int(np.argmax(last)) == picks[-1] and bo._gap(last) > bo.GAP, (int(np.argmax(last)), picks[-1], bo._gap(last))
        err_p = abs(float(last[picks[-1]] - a["v_pick"][-1]))
        err_v = float(np.max(np.abs(bo.variance_after(ds, c["output"], pool, picks, pending) - a["v"])))
        gaps = a["gaps"]
    else:
        b = bo.select_incremental(ds, c["output"], pool, c["k"], pending)
        assert np.array_equal(a["index"], b["index"]), (a["index"], b["index"])
        err_p, err_v = float(np.max(np.abs(a["v_pick"] - b["v_pick"]))), float(np.max(np.abs(a["v"] - b["v"])))
        gaps = np.minimum(a["gaps"], b["gaps"])
    print(bo.case_id(c), "routes", err_p, err_v, "min gap", gaps.min())
    assert err_p < bo.TOL64 and err_v < bo.TOL64, (err_p, err_v)
    assert gaps.min() > bo.GAP, gaps
    assert np.all(np.diff(a["v_pick"]) <= 1e-12)             # (greedy on a shrinking variance: the picks' values do not grow)
    if c.get("pool") == "planted":
        assert a["index"].tolist() == list(bo.PLANTED)       # (the batch is the four planted rows, on both sides of the trip boundary)
        assert c["m"] - bo.M_TRIP == 513
        same =np.setdiff1d(np.arange(513), [p % bo.M_TRIP for p in bo.PLANTED])
        assert same.size == 510 and np.array_equal(pool[bo.M_TRIP + same], pool[same])


def _constant(text, pattern, what):
    hit = re.search(pattern, text)
    assert hit, f"csrc/batch.hip or csrc/whiten.hpp no longer states {what} in the form this test reads: revisit batch_oracle.CASES and the pattern"
    return [int(g) for g in hit.groups()]


def test_the_case_list_covers_every_edge():
    col = lambda key: {c[key] for c in bo.CASES}
    assert col("n") >= {1, 2, 63, 64, 65, 300, 505, 512, 513, 600, 1020, 1024, 1025, 1100, 2048}
    assert col("m") >= {1, 16, 33, 63, 64, 65, 257, 300, 1000, 5000, 2097152 + 513}
    assert col("k") >= {1, 2, 4, 8, 16, 59, 64} and col("d") == {1, 2, 3, 4, 6, 8} and col("n_pending") == {0, 1, 3, 5}
    assert {(c["q"], c["output"]) for c in bo.CASES} >= {(3, 0), (3, 2)}
    assert col("use_invK") == {True, False} and any(c["k"] > c["m"] for c in bo.CASES)
    new = bo.CASES[bo.FIRST_LARGE:]
    assert len(new) == 10 and {c["use_invK"] for c in new} == {True, False} and len(col("seed")) == len(bo.CASES)
    # the constants of the kernels, from the source: a case at each of them
    text = open(os.path.join(ROOT, "safe-bayesian-optimization_amd", "csrc", "batch.hip")).read()
    shared = open(os.path.join(ROOT, "safe-bayesian-optimization_amd", "csrc", "whiten.hpp")).read()     # whiten_tile, factor_*_mv
    const = lambda name, src=text: _constant(src, r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", name)[0]
    chunk, threads, rows, v0threads = const("kBatChunk"), const("kBatThreads"), const("kWhitenRows", shared), const("kWhitenThreads", shared)
    assert const("kFactorMvThreads", shared) == v0threads      # (k_batch_u's strides)
    assert re.search(r"__launch_bounds__\(kWhitenThreads\)\s*void\s+k_batch_v0", text) and "const int P = whiten_tier(n);" in text
    assert re.search(r"__launch_bounds__\(kFactorMvThreads\)\s*void\s+k_batch_u", text)
    cap = _constant(text, r"const\s+int\s+nb\s*=[^;]*\(m\s*\+\s*kBatThreads\s*-\s*1\)\s*/\s*kBatThreads\s*,\s*(\d+)\s*\)\s*;",
                    "the workgroup cap of k_batch_pass")[0]
    t1, p1, t2, p2, p3 = _constant(shared, r"int\s+whiten_tier\(int\s+n\)\s*\{\s*return\s+n\s*<=\s*(\d+)\s*\?\s*(\d+)\s*:\s*n\s*<=\s*(\d+)\s*\?\s*(\d+)\s*:\s*(\d+)\s*;",
                                   "the tiers of whiten_tile")
    max_n = int(re.search(r"#define\s+SBO_MAX_N\s+(\d+)", open(os.path.join(ROOT, "include", "safebo.h")).read()).group(1))
    assert (chunk, threads, rows, v0threads, cap, max_n) == (512, 256, 4, 1024, 8192, _lib.SBO_MAX_N) and cap * threads == bo.M_TRIP
    assert (t1, p1, t2, p2, p3) == (512, 32, 1024, 16, 8)
    assert [8 * t * p for t, p in ((t1, p1), (t2, p2), (max_n, p3))] == [128 * 1024] * 3          # (each tier ends at the LDS ceiling)
    for t in (t1, t2):
        assert {t, t + 1} <= col("n"), t
    assert max_n in col("n")
    for p in (p2, p3):                                       # (a top block of one row in the tiers with more than one block)
        rb = rows * v0threads // p
        assert any(c["n"] % rb == 1 and c["n"] > rb and (p2 if c["n"] <= t2 else p3) == p and c["n"] > t1 for c in bo.CASES), p
    assert any(c["n"] == t1 and c["n"] % (rows * v0threads // p1) == 0 for c in bo.CASES)
    na = lambda c: (c["n"] + c["n_pending"], c["n"] + c["n_pending"] + c["k"])
    for edge in (chunk, v0threads):
        assert any(na(c)[0] < edge < na(c)[1] for c in bo.CASES), edge
    assert any(na(c)[0] == chunk for c in bo.CASES) and any(na(c)[0] == v0threads for c in bo.CASES)
    assert any(na(c)[1] == max_n + _lib.SBO_MAX_BATCH for c in bo.CASES)
    assert any(c["m"] > cap * threads for c in bo.CASES) and any(c["m"] % p for p in (p1, p2, p3) for c in new)
    assert {c["d"] for c in new} >= {3, 6}


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
