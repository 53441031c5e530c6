"""CPU side of sbo_sample_paths: the two NumPy routes to a sample path agree and every committed case of the GPU test is sharp by the
oracle alone (every path's top-two gap above paths_oracle.SHARP = 1e-8: the condition under which the device's indices must equal the
oracle's exactly); the definition is the posterior's (the paths' mean and variance are the posterior's, and a path with zero draws is
the posterior mean); the symbol, its structures and its caps are what include/safebo.h declares; the argument checks of
SweepEngine.sample_paths fire before anything touches the device; chunks merge as one call would answer (the C call stubbed; the
device call itself is checked under the gpu marker, tests/test_gpu_sample_paths.py); SafeOpt.BO.Thompson hands over the members of S.

Agreement of the routes over the committed cases (normalised units, every value): within 7.7e-13 (n = 300, q = 4), then 3.9e-13
(n = 1025) and 3.4e-13 (n = 2048); the assertion is TOL64 / 10 = 1e-11.  Smallest top-two gap of a case: 7.9e-5 (n = 2, d = 1).
Statistics of 4096 paths on F = 4096 features (n = 20, 8 points, three seeds, both outputs): the mean deviates by at most 3.3 standard
errors, the variance by at most 4.5 - 6.4 % (without the noise term 52 - 58 %, with the scale sqrt(sf2 / F) 47 - 52 %; the bound is 25 %).

The case list is held to the constants of csrc/paths.hip, csrc/slab_tiles.hpp and csrc/internal.hpp, read from the source (test_the_case_list_covers_every_edge)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from safebo_amd import SafeOpt, SweepEngine, _lib

import batch_oracle as bo
import model_remove as mr
import paths_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [po.case_id(c) for c in po.CASES]


@pytest.mark.parametrize("i", range(len(po.CASES)), ids=IDS)
def test_the_two_routes_agree_and_the_case_is_sharp(i):
    c = po.CASES[i]
    ds, pts, draws, f = po.reference(i)
    assert f.shape == (c["m"], c["S"]) and pts.shape == (c["m"], c["d"]) and ds["X_norm"].shape == (c["n"], c["d"])
    assert ds["Y_norm"].shape[1] == c["q"]
    err = float(np.max(np.abs(f - po.paths_invK(ds, c["output"], draws, pts))))
    gap = po.sharpness(f, c["maximize"])
    print(po.case_id(c), "routes", err, "min gap", gap)
    assert err < po.TOL64 / 10, err
    assert gap > po.SHARP, gap


def _constant(text, name):
    hit = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert hit, f"csrc/paths.hip, csrc/slab_tiles.hpp or csrc/whiten.hpp no longer states {name} in the form this test reads: revisit paths_oracle.CASES and the pattern"
    return int(hit.group(1))


def test_the_case_list_covers_every_edge():
    col = lambda key: {c[key] for c in po.CASES}
    text = open(os.path.join(ROOT, "safe-bayesian-optimization_amd", "csrc", "paths.hip")).read()
    tiles = open(os.path.join(ROOT, "safe-bayesian-optimization_amd", "csrc", "slab_tiles.hpp")).read()    # the slab and the 128-row tile
    common = open(os.path.join(ROOT, "safe-bayesian-optimization_amd", "csrc", "internal.hpp")).read()     # spad_of, with_spad
    tile, slab, grid = _constant(text, "kPathTile"), _constant(tiles, "kSlabK"), _constant(text, "kPathGridTiles")
    assert (tile, slab, grid) == (128, 32, 1024) and _constant(tiles, "kTile128") == tile and "kPathTile == kTile128" in text
    assert "k0 += kSlabK" in text and "tile128_step(lds, g," in text                     # (k_path_main walks its K axis in these slabs)
    assert "A.Spad = spad_of(S);" in text and "with_spad(A.Spad," in text and \
        re.search(r"int\s+spad_of\(int\s+S\)\s*\{\s*return\s+S\s*<=\s*16\s*\?\s*16\s*:\s*S\s*<=\s*32\s*\?\s*32\s*:\s*64\s*;", common), \
        "csrc/paths.hip no longer pads the paths in the form this test reads: revisit paths_oracle.CASES"
    assert re.search(r"nwg\s*=\s*\(int\)std::min<long long>\(ntiles,\s*kPathGridTiles\)\s*;", text), \
        "csrc/paths.hip no longer bounds its grid in the form this test reads: revisit paths_oracle.CASES"
    shared = open(os.path.join(ROOT, "safe-bayesian-optimization_amd", "csrc", "whiten.hpp")).read()     # factor_lower_mv, factor_upper_mv
    assert re.search(r"__launch_bounds__\(1024\)\s*void\s+k_path_solve", text) and text.count("j += 1024") == 1 and \
        _constant(shared, "kFactorMvThreads") == 1024 and shared.count("j += kFactorMvThreads") == 1 and \
        shared.count("i += kFactorMvThreads / 64") == 1 and "static_assert(kFactorMvThreads == 1024" in text, \
        "k_path_solve no longer walks in strides of 1024: revisit the n of paths_oracle.CASES"
    header = open(os.path.join(ROOT, "include", "safebo.h")).read()
    max_n = int(re.search(r"#define\s+SBO_MAX_N\s+(\d+)", header).group(1))
    assert max_n == _lib.SBO_MAX_N
    # the issue's shapes
    assert col("m") >= {1, tile - 1, tile, tile + 1, 4 * tile + 1}
    assert any(-(-c["m"] // tile) > grid for c in po.CASES)                             # a workgroup with a second tile
    assert col("F") >= {1, slab - 1, slab, slab + 1, 1024, _lib.SBO_MAX_FEATURES}
    assert col("n") >= {1, 2, slab - 1, slab, slab + 1, 2 * slab, 2 * slab + 1, 300, 1024, 1025, max_n}
    assert any(c["F"] == slab + 1 and c["n"] == slab + 1 for c in po.CASES)
    assert col("S") >= {1, 15, 16, 17, 33, _lib.SBO_MAX_PATHS}
    assert col("d") == {1, 2, 3, 6, 8} and col("q") == {1, 2, 3, 4}
    for q in (2, 3, 4):
        assert any(c["q"] == q and c["output"] == q - 1 for c in po.CASES), q
    assert any(c["q"] == 4 and c["output"] == 0 for c in po.CASES)
    assert col("maximize") == {0, 1} and col("use_invK") == {True, False} and len(col("seed")) == len(po.CASES)
    big = [c for c in po.CASES if c["n"] == max_n]
    assert len(big) == 1 and big[0]["m"] <= 65 and big[0]["S"] == 16 and big[0]["F"] == 1024 and big[0]["log_sn"] == -1.0


# ------------------------------------------------------------------------------------------ the definition is the posterior's
def _small():
    ds, pts, _ = bo.make_case(dict(n=20, m=8, d=2, q=2, seed=81, n_pending=0, output=0))
    return ds, pts


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("o", [0, 1])
def test_mean_and_variance_of_many_paths_are_the_posteriors(seed, o):
    """n = 20 (config B, seed 5, default hyper-parameters), 8 pool points, F = 4096, 4096 paths.  E weights = E noise = 0, so the
    paths' mean is the posterior mean for any omega: within 5 standard errors at every point.  Their variance is the posterior's up
    to the O(1 / sqrt(F)) error of the feature kernel: within 25 %.  The bound tells the definition from its neighbours: without the
    noise term, and with the scale sqrt(sf2 / F), the deviation is far beyond it."""
    ds, pts = _small()
    N, F = 4096, 4096
    draws = SweepEngine.path_draws(2, 20, N, F, seed)
    mean, var = po.posterior(ds, o, pts)
    assert np.min(var) > 1e-4
    f = po.paths_solve(ds, o, draws, pts)
    z = np.abs(f.mean(axis=1) - mean) / np.sqrt(f.var(axis=1, ddof=1) / N)
    dev = np.abs(f.var(axis=1, ddof=1) / var - 1.0)
    no_noise = np.abs(po.paths_solve(ds, o, draws, pts, use_noise=False).var(axis=1, ddof=1) / var - 1.0)
    half = np.abs(po.paths_solve(ds, o, draws, pts, scale=np.sqrt(0.5)).var(axis=1, ddof=1) / var - 1.0)
    print("seed", seed, "output", o, "mean: standard errors", float(z.max()), "variance: deviation", float(dev.min()), float(dev.max()),
          "without noise", float(no_noise.max()), "scale sqrt(sf2 / F)", float(half.max()))
    assert z.max() < 5.0, z
    assert dev.max() < 0.25, dev
    assert no_noise.max() > 0.25 and half.max() > 0.25


@pytest.mark.parametrize("o", [0, 1])
def test_a_path_with_zero_draws_is_the_posterior_mean(o):
    ds, pts = _small()
    omega, phase, weights, noise = SweepEngine.path_draws(2, 20, 3, 64, 5)
    draws = (omega, phase, np.zeros_like(weights), np.zeros_like(noise))
    mean = (oracle.gp_inference(pts, ds)[0][:, o] - ds["Y_mean"][o]) / ds["Y_std"][o]
    for route in (po.paths_solve, po.paths_invK):
        f = route(ds, o, draws, pts)
        assert float(np.max(np.abs(f - mean[:, None]))) < 1e-12


# ------------------------------------------------------------------------------------------ the ABI
def test_symbol_structures_and_caps_match_the_header(tmp_path):
    text = open(os.path.join(ROOT, "include", "safebo.h")).read()
    assert int(re.search(r"#define\s+SBO_MAX_PATHS\s+(\d+)", text).group(1)) == _lib.SBO_MAX_PATHS == 64
    assert int(re.search(r"#define\s+SBO_MAX_FEATURES\s+(\d+)", text).group(1)) == _lib.SBO_MAX_FEATURES == 8192
    assert int(re.search(r"#define\s+SBO_PATHS_MAX_POINTS\s+(\d+)", text).group(1)) == _lib.SBO_PATHS_MAX_POINTS == 1 << 24
    assert int(re.search(r"#define\s+SBO_PATHS_MAX_VALUES\s+(\d+)ULL", text).group(1)) == _lib.SBO_PATHS_MAX_VALUES == 1 << 32
    assert re.search(r"\bint\s+sbo_sample_paths\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "sbo_sample_paths" in {n for n, _, _ in _lib.SYMBOLS}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safebo.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %d\\n", '
                   'sizeof(sbo_paths_opts), offsetof(sbo_paths_opts, n_features), offsetof(sbo_paths_opts, maximize), '
                   'sizeof(sbo_paths_result), offsetof(sbo_paths_result, index), offsetof(sbo_paths_result, value), SBO_ABI_VERSION); '
                   'return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.PathsOpts), _lib.PathsOpts.n_features.offset, _lib.PathsOpts.maximize.offset, C.sizeof(_lib.PathsResult),
                   _lib.PathsResult.index.offset, _lib.PathsResult.value.offset, 3]
    assert C.sizeof(_lib.PathsOpts) == 16 and C.sizeof(_lib.PathsResult) == 16 * _lib.SBO_MAX_PATHS
    lib = _lib.load()
    assert hasattr(C.CDLL(_lib.library_path()), "sbo_sample_paths")
    assert lib.sbo_sample_paths(None, None, None, None, None, None, 1, None, None, None) == _lib.SBO_E_INVALID
    res = _lib.PathsResult()
    for s in range(_lib.SBO_MAX_PATHS):
        res.index[s], res.value[s] = 5, 2.0
    assert lib.sbo_sample_paths(None, None, None, None, None, None, 1, None, None, C.byref(res)) == _lib.SBO_E_INVALID
    assert list(res.index) == [-1] * _lib.SBO_MAX_PATHS and np.isnan(np.array(res.value)).all()


# ------------------------------------------------------------------------------------------ the host's checks
def test_path_draws_are_reproducible_in_the_documented_order():
    d, n, S, F, seed = 3, 7, 5, 11, 42
    omega, phase, weights, noise = SweepEngine.path_draws(d, n, S, F, seed)
    assert omega.shape == (F, d) and phase.shape == (F,) and weights.shape == (S, F) and noise.shape == (S, n)
    assert all(a.dtype == np.float64 for a in (omega, phase, weights, noise))
    rng = np.random.default_rng(seed)
    want = (rng.standard_normal((F, d)), rng.uniform(0.0, 2.0 * np.pi, F), rng.standard_normal((S, F)), rng.standard_normal((S, n)))
    for a, b in zip((omega, phase, weights, noise), want):
        assert a.tobytes() == b.tobytes()
    assert phase.min() >= 0.0 and phase.max() < 2.0 * np.pi
    again = SweepEngine.path_draws(d, n, S, F, seed)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, want))
    assert SweepEngine.path_draws(d, n, S, F, seed + 1)[2].tobytes() != weights.tobytes()
    assert SweepEngine.path_draws(2, 4, 1)[0].shape == (1024, 2)                      # (the default number of features)


def _bare_engine(d=2, q=3, n=4):
    """An engine object without a context: every call that reached the library would fail on it."""
    eng = SweepEngine.__new__(SweepEngine)
    eng._ctx, eng._lib, eng.d, eng.q, eng.n = None, None, d, q, n
    return eng


Z2 = np.zeros((4, 2))


def _draws(F=8, d=2, S=2, n=4):
    return SweepEngine.path_draws(d, n, S, F, 0)


def _with(i, a, S=2):
    dr = list(_draws(S=S))
    dr[i] = a
    return tuple(dr)


@pytest.mark.parametrize("kwargs", [
    dict(points=np.zeros((4, 3)), n_paths=2), dict(points=np.zeros((0, 2)), n_paths=2), dict(points=np.zeros((2, 2, 2)), n_paths=2),
    dict(points=np.array([[0.0, np.nan]]), n_paths=2), dict(points=np.array([[np.inf, 0.0]]), n_paths=2),
    dict(points=Z2, n_paths=0), dict(points=Z2, n_paths=65), dict(points=Z2, n_paths=2.0), dict(points=Z2, n_paths=True),
    dict(points=Z2, n_paths=2, output=3), dict(points=Z2, n_paths=2, output=-1), dict(points=Z2, n_paths=2, output=1.0),
    dict(points=Z2, n_paths=2, features=0), dict(points=Z2, n_paths=2, features=8193), dict(points=Z2, n_paths=2, features=64.0),
    dict(points=Z2, n_paths=2, seed=-1), dict(points=Z2, n_paths=2, seed=0.5), dict(points=Z2, n_paths=2, maximize=2),
    dict(points=Z2, n_paths=2, maximize="yes"), dict(points=Z2, n_paths=2, maximize=None),
    dict(points=Z2, n_paths=2, draws=_draws()[:3]), dict(points=Z2, n_paths=2, draws=np.zeros(4)),
    dict(points=Z2, n_paths=2, draws=_draws(d=3)), dict(points=Z2, n_paths=2, draws=_draws(S=3)),
    dict(points=Z2, n_paths=2, draws=_draws(n=5)), dict(points=Z2, n_paths=2, draws=_with(0, np.zeros((0, 2)))),
    dict(points=Z2, n_paths=2, draws=_with(1, np.zeros(7))), dict(points=Z2, n_paths=2, draws=_with(1, np.zeros((8, 1)))),
    dict(points=Z2, n_paths=2, draws=_with(2, np.zeros((2, 7)))), dict(points=Z2, n_paths=2, draws=_with(3, np.zeros(4))),
    dict(points=Z2, n_paths=2, draws=_with(0, np.full((8, 2), np.nan))), dict(points=Z2, n_paths=2, draws=_with(1, np.full(8, np.inf))),
    dict(points=Z2, n_paths=2, draws=_with(2, np.full((2, 8), np.nan))), dict(points=Z2, n_paths=2, draws=_with(3, np.full((2, 4), -np.inf))),
    dict(points=Z2, n_paths=2, draws=_draws(F=8193)),
])
def test_sample_paths_checks_its_arguments_on_the_host(kwargs):
    with pytest.raises(ValueError):
        _bare_engine().sample_paths(**kwargs)
    with pytest.raises(ValueError):
        SweepEngine.path_arguments(2, 3, 4, **kwargs)


def test_accepted_arguments_come_back_in_library_form():
    pts, S, o, F, seed, mx, draws = SweepEngine.path_arguments(2, 3, 4, [0.5, 1.0], np.int64(2), 2, 64, 7, True)
    assert pts.shape == (1, 2) and pts.dtype == np.float64 and (S, o, F, seed, mx) == (2, 2, 64, 7, 1) and draws is None
    given = tuple(np.asarray(a, dtype=np.float32) for a in _draws(F=9))
    out = SweepEngine.path_arguments(2, 3, 4, Z2, 2, draws=given, features=1024)
    assert out[3] == 9 and out[5] == 0 and all(a.dtype == np.float64 and a.flags["C_CONTIGUOUS"] for a in out[6])
    assert SweepEngine.path_arguments(0, 0, 0, np.zeros((3, 5)), 1, 6)[2] == 6         # (no model: the library answers)


# ------------------------------------------------------------------------------------------ chunks
def _stub(table, calls):
    """_paths_call answered from a table f [m, S]: the rows are recognised by their first coordinate."""
    def call(self, opts, draws, pts, want_values):
        rows = pts[:, 0].astype(int)
        calls.append(rows.tolist())
        z = table[rows]
        S = z.shape[1]
        assert (int(opts.n_paths), draws[2].shape[0]) == (S, S)
        key = np.where(np.isnan(z), -np.inf, z if opts.maximize else -z)
        some = ~np.isnan(z).all(axis=0)
        idx = np.where(some, np.argmax(key, axis=0), -1).astype(np.int64)
        val = np.where(some, z[np.maximum(idx, 0), np.arange(S)], np.nan)
        return idx, val, (z.copy() if want_values else None)
    return call


@pytest.mark.parametrize("maximize", [False, True])
def test_chunks_merge_as_one_call(monkeypatch, maximize):
    """SweepEngine.sample_paths with the C call stubbed by a table f [m, S]: chunks of 5 points (one path's best value sits in two
    chunks -- the lower global index wins --, one path has NaN in a whole chunk, one everywhere, one its best in the last, short chunk)
    give the indices, values and value table of the unchunked call, with the same draws in every call."""
    rng = np.random.default_rng(9)
    m, S = 23, 5
    f = rng.standard_normal((m, S))
    top = 9.0 if maximize else -9.0
    f[3, 1] = f[17, 1] = top                                 # a tie across chunks
    f[5:10, 2] = np.nan                                      # a chunk without a value
    f[:, 3] = np.nan                                         # no value at all
    f[20, 4] = 1.25 * top                                    # the best in the last, short chunk
    pts = np.column_stack([np.arange(m, dtype=np.float64), np.zeros(m)])
    seen = []

    def remember(self, opts, draws, p, want):
        seen.append(draws)
        return _stub(f, calls)(self, opts, draws, p, want)

    calls = []
    monkeypatch.setattr(SweepEngine, "_paths_call", remember)
    eng = _bare_engine(q=2)
    whole = eng.sample_paths(pts, S, maximize=maximize, features=8, seed=4, return_values=True)
    assert calls == [list(range(m))]
    monkeypatch.setattr(SweepEngine, "_paths_chunk", 5)
    calls.clear()
    got = eng.sample_paths(pts, S, maximize=maximize, features=8, seed=4, return_values=True)
    assert calls == [list(range(lo, min(lo + 5, m))) for lo in range(0, m, 5)]
    pick = np.nanargmax if maximize else np.nanargmin
    assert got["index"].tolist() == whole["index"].tolist() == [int(pick(f[:, 0])), 3, int(pick(f[:, 2])), -1, 20]
    assert np.array_equal(got["value"], whole["value"], equal_nan=True) and np.array_equal(got["values"], f, equal_nan=True)
    assert np.array_equal(got["x"][[0, 1, 2, 4]], pts[got["index"][[0, 1, 2, 4]]]) and np.isnan(got["x"][3]).all()
    want = SweepEngine.path_draws(2, 4, S, 8, 4)
    for dr in seen:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(dr, want))
    lean = eng.sample_paths(pts, S, maximize=maximize, features=8, seed=4)
    assert set(lean) == {"index", "x", "value"} and lean["index"].tolist() == got["index"].tolist()


def test_the_values_cap_shrinks_the_chunk(monkeypatch):
    """A value table of 64 paths is 512 bytes a point: under a cap of 4096 bytes the points go in chunks of 8 where the values are
    asked for, and in one call where they are not."""
    sizes = []

    def call(self, opts, draws, pts, want):
        sizes.append(len(pts))
        S = int(opts.n_paths)
        return np.zeros(S, dtype=np.int64), np.zeros(S), (np.zeros((len(pts), S)) if want else None)

    monkeypatch.setattr(SweepEngine, "_paths_call", call)
    monkeypatch.setattr(SweepEngine, "_paths_values", 4096)
    eng = _bare_engine(q=2)
    eng.sample_paths(np.zeros((20, 2)), 64, features=8, return_values=True)
    assert sizes == [8, 8, 4]
    sizes.clear()
    eng.sample_paths(np.zeros((20, 2)), 64, features=8)
    assert sizes == [20]
    assert SweepEngine._paths_chunk == _lib.SBO_PATHS_MAX_POINTS


# ------------------------------------------------------------------------------------------ the host class
class _FakeEngine:
    def __init__(self, S):
        self.S, self.calls = S, []

    def mask(self, which, c=0):
        assert which == "S"
        return self.S

    def sample_paths(self, points, n_paths, output=0, features=1024, seed=0, **kw):
        self.calls.append(dict(points=np.array(points), n_paths=n_paths, output=output, features=features, seed=seed, **kw))
        idx = np.arange(n_paths) % len(points)
        return {"index": idx, "x": np.asarray(points)[idx], "value": np.arange(n_paths, dtype=np.float64)}


def test_thompson_hands_over_the_members_of_S_in_ascending_order(monkeypatch):
    m = SafeOpt.BO([mr.benoit_f, mr.benoit_g], mr.BOUND, 3.0, grid=(6, 5))
    S = np.zeros(30, dtype=bool)
    S[[28, 3, 17, 4]] = True
    fake = _FakeEngine(S)
    swept = []
    monkeypatch.setattr(m, "_engine", fake)                  # (the ``engine`` property hands out what is there)
    monkeypatch.setattr(m, "sweep", lambda want_masks=False: swept.append(want_masks))
    X, value = m.Thompson(3, seed=11, features=256)
    assert swept == [True] and len(fake.calls) == 1
    call = fake.calls[0]
    assert np.array_equal(call["points"], m._all_points()[[3, 4, 17, 28]])
    assert (call["n_paths"], call["output"], call["features"], call["seed"]) == (3, 0, 256, 11)
    assert X.shape == (3, 2) and np.array_equal(X, m._all_points()[[3, 4, 17]]) and value.tolist() == [0.0, 1.0, 2.0]
    fake.S = np.zeros(30, dtype=bool)
    X0, v0 = m.Thompson(2)
    assert X0.shape == (0, 2) and v0.shape == (0,) and len(fake.calls) == 1
    for bad in (dict(k=0), dict(k=65), dict(k=2.0), dict(k=2, features=0), dict(k=2, seed=-1)):
        with pytest.raises(ValueError):
            m.Thompson(**bad)
    assert "not reference behaviour" in SafeOpt.BO.Thompson.__doc__
