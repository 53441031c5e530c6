"""What sbo_posterior_joint rests on that needs no device: the three NumPy routes of joint_oracle agree and every committed case with
draws is sharp; the committed cases cover the edges of csrc/joint.hip's constants; the covariance is positive semi-definite; exact
draws have the posterior's mean and covariance; the ABI structures match the header; SweepEngine.joint_arguments refuses bad
arguments before anything touches the device; SafeOpt.BO.Thompson(exact=True) hands posterior_joint the pool Thompson() hands
sample_paths (the C call stubbed) and refuses a safe set above the cap."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from safebo_amd import SafeOpt, SweepEngine, _lib

import batch_oracle as bo
import joint_oracle as jo
import model_remove as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [jo.case_id(c) for c in jo.CASES]


# ------------------------------------------------------------------------------------------ 1 - 4. the routes and the cases
@pytest.mark.parametrize("i", range(len(jo.CASES)), ids=IDS)
def test_the_routes_agree_the_covariance_is_psd_and_the_case_is_sharp(i):
    c = jo.CASES[i]
    ds, pts, z, ref = jo.reference(i)
    assert pts.shape == (c["m"], c["d"]) and ds["X_norm"].shape == (c["n"], c["d"]) and ds["Y_norm"].shape[1] == c["q"]
    assert ref["draws"].shape == (c["m"], c["S"]) and (z is None) == (c["S"] == 0)
    sf2 = bo.params(ds, c["output"])[1]
    e_mean = e_cov = e_draws = 0.0
    for route in (jo.joint_invK, jo.joint_white):
        other = route(ds, c["output"], pts, z, c["noise"], c["jitter"])
        e_mean = max(e_mean, float(np.max(np.abs(other["mean"] - ref["mean"]))))
        e_cov = max(e_cov, float(np.max(np.abs(other["C"] - ref["C"]))))
        if c["S"]:
            e_draws = max(e_draws, float(np.max(np.abs(other["draws"] - ref["draws"]))))
    low = float(np.linalg.eigvalsh(ref["C"])[0])
    gap = jo.sharpness(ref["draws"], c["maximize"]) if c["S"] else float("inf")
    print(jo.case_id(c), "routes: mean", e_mean, "C", e_cov, "draws", e_draws, "smallest eigenvalue / sf2", low / sf2, "min gap", gap)
    assert e_mean < 1e-11 and e_cov < 1e-11, (e_mean, e_cov)
    if c["noise"] and c["S"]:
        assert e_draws < jo.TOL64 / 4, e_draws
    assert low >= -1e-12 * sf2, low
    assert gap > jo.SHARP, gap


def _constant(text, name):
    hit = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert hit, f"the source no longer states {name} in the form this test reads: revisit joint_oracle.CASES and the pattern"
    return int(hit.group(1))


def test_the_case_list_covers_every_edge():
    col = lambda key: {c[key] for c in jo.CASES}
    text = open(os.path.join(ROOT, "safe-bayesian-optimization_amd", "csrc", "joint.hip")).read()
    shared = open(os.path.join(ROOT, "safe-bayesian-optimization_amd", "csrc", "slab_tiles.hpp")).read()   # the slab and the two tiles
    common = open(os.path.join(ROOT, "safe-bayesian-optimization_amd", "csrc", "internal.hpp")).read()     # spad_of, with_spad
    tile, draw, slab = _constant(text, "kJointTile"), _constant(text, "kJointDrawTile"), _constant(shared, "kSlabK")
    assert (tile, draw, slab) == (64, 128, 32) and _constant(shared, "kTile128") == draw and "kJointDrawTile == kTile128" in text
    assert "A.Spad = spad_of(S);" in text and "with_spad(A.Spad," in text and \
        re.search(r"int\s+spad_of\(int\s+S\)\s*\{\s*return\s+S\s*<=\s*16\s*\?\s*16\s*:\s*S\s*<=\s*32\s*\?\s*32\s*:\s*64\s*;", common), \
        "csrc/joint.hip no longer pads the draws in the form this test reads: revisit joint_oracle.CASES"
    header = open(os.path.join(ROOT, "include", "safebo.h")).read()
    max_n = int(re.search(r"#define\s+SBO_MAX_N\s+(\d+)", header).group(1))
    cap = int(re.search(r"#define\s+SBO_JOINT_MAX_POINTS\s+(\d+)", header).group(1))
    assert max_n == _lib.SBO_MAX_N and cap == _lib.SBO_JOINT_MAX_POINTS == 2048
    assert col("m") >= {1, 2, tile - 1, tile, tile + 1, 2 * tile + 1, 4 * tile + 1, 8 * tile + 1, cap}
    assert col("n") >= {1, slab - 1, slab, slab + 1, 300, 1025, max_n}
    assert col("S") >= {0, 1, 16, 17, _lib.SBO_MAX_PATHS}
    assert col("d") == {1, 2, 3, 8} and col("q") == {1, 2, 3, 4}
    for q in (2, 3, 4):
        assert any(c["q"] == q and c["output"] == q - 1 for c in jo.CASES), q
    assert any(c["q"] == 4 and c["output"] == 0 for c in jo.CASES)
    assert col("maximize") == {0, 1} and col("noise") == {0, 1} and col("use_invK") == {True, False} and len(col("seed")) == len(jo.CASES)
    assert col("jitter") == {0.0, 1e-8, 1e-6, 1e-4} and all(c["noise"] == 1 for c in jo.CASES if c["jitter"] == 0.0)
    big = [c for c in jo.CASES if c["n"] == max_n]
    assert len(big) == 1 and big[0]["m"] == 65 and big[0]["log_sn"] == -1.0
    at_cap = [c for c in jo.CASES if c["m"] == cap]
    assert len(at_cap) == 1 and at_cap[0]["n"] == 64


# ------------------------------------------------------------------------------------------ 5. statistics
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("o", [0, 1])
def test_exact_draws_have_the_posteriors_mean_and_covariance(seed, o):
    """n = 20 (config B, seed 5, default hyper-parameters), 8 pool points, 4096 exact draws: the sample mean within 4 standard errors
    of mu at every point, the sample covariance within 4 standard errors of C entry by entry -- for normal draws the variance of an
    entry of the sample covariance is (C_ii C_jj + C_ij^2) / (N - 1) (Wishart)."""
    ds, pts, _ = bo.make_case(dict(n=20, m=8, d=2, q=2, seed=81, n_pending=0, output=0))
    N = 4096
    ref = jo.joint_solve(ds, o, pts, SweepEngine.joint_draws(8, N, seed), False, 0.0)
    f, mu, Cm = ref["draws"], ref["mean"], ref["C"]
    assert np.min(np.diag(Cm)) > 1e-4
    zm = np.abs(f.mean(axis=1) - mu) / np.sqrt(np.diag(Cm) / N)
    zc = np.abs(np.cov(f) - Cm) / np.sqrt((np.outer(np.diag(Cm), np.diag(Cm)) + Cm * Cm) / (N - 1))
    print("seed", seed, "output", o, "mean: standard errors", float(zm.max()), "covariance: standard errors", float(zc.max()))
    assert zm.max() < 4.0, zm
    assert zc.max() < 4.0, zc


# ------------------------------------------------------------------------------------------ 6. the ABI
def test_symbol_structures_and_caps_match_the_header(tmp_path):
    text = open(os.path.join(ROOT, "include", "safebo.h")).read()
    assert int(re.search(r"#define\s+SBO_JOINT_MAX_POINTS\s+(\d+)", text).group(1)) == _lib.SBO_JOINT_MAX_POINTS == 2048
    assert re.search(r"\bint\s+sbo_posterior_joint\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "sbo_posterior_joint" in {n for n, _, _ in _lib.SYMBOLS}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safebo.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", '
                   'sizeof(sbo_joint_opts), offsetof(sbo_joint_opts, n_draws), offsetof(sbo_joint_opts, noise), '
                   'offsetof(sbo_joint_opts, maximize), offsetof(sbo_joint_opts, jitter), sizeof(sbo_joint_result), '
                   'offsetof(sbo_joint_result, value), offsetof(sbo_joint_result, pivot_min), offsetof(sbo_joint_result, pivot_row), '
                   'SBO_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.JointOpts), _lib.JointOpts.n_draws.offset, _lib.JointOpts.noise.offset, _lib.JointOpts.maximize.offset,
                   _lib.JointOpts.jitter.offset, C.sizeof(_lib.JointResult), _lib.JointResult.value.offset, _lib.JointResult.pivot_min.offset,
                   _lib.JointResult.pivot_row.offset, 3]
    assert C.sizeof(_lib.JointOpts) == 24 and C.sizeof(_lib.JointResult) == 16 * _lib.SBO_MAX_PATHS + 16
    lib = _lib.load()
    assert hasattr(C.CDLL(_lib.library_path()), "sbo_posterior_joint")
    res = _lib.JointResult()
    for s in range(_lib.SBO_MAX_PATHS):
        res.index[s], res.value[s] = 5, 2.0
    res.pivot_min, res.pivot_row = 2.0, 5
    assert lib.sbo_posterior_joint(None, None, 1, None, None, None, None, None, None, None) == _lib.SBO_E_INVALID
    assert lib.sbo_posterior_joint(None, None, 1, None, None, None, None, None, None, C.byref(res)) == _lib.SBO_E_INVALID
    assert list(res.index) == [-1] * _lib.SBO_MAX_PATHS and np.isnan(np.array(res.value)).all()
    assert np.isnan(res.pivot_min) and res.pivot_row == -1


# ------------------------------------------------------------------------------------------ 7. the host's checks
def test_joint_draws_are_reproducible():
    z = SweepEngine.joint_draws(5, 3, 7)
    assert z.shape == (3, 5) and z.dtype == np.float64
    assert np.array_equal(z, np.random.default_rng(7).standard_normal((3, 5)))
    assert SweepEngine.joint_draws(5, 0, 7).shape == (0, 5)


GOOD = dict(d=2, q=2, points=np.zeros((4, 2)), output=0, n_draws=2, seed=0, z=None, noise=False, jitter=1e-6, maximize=False)


@pytest.mark.parametrize("kwargs", [
    dict(points=np.zeros((4, 3))), dict(points=np.zeros((0, 2))), dict(points=np.zeros((2, 2, 2))),
    dict(points=np.zeros((_lib.SBO_JOINT_MAX_POINTS + 1, 2))), dict(points=np.array([[0.0, np.nan]])), dict(points=np.array([[np.inf, 0.0]])),
    dict(output=-1), dict(output=2), dict(output=1.0), dict(output=True), dict(n_draws=-1), dict(n_draws=_lib.SBO_MAX_PATHS + 1),
    dict(n_draws=2.0), dict(seed=-1), dict(seed=0.5), dict(noise=2), dict(noise="yes"), dict(maximize=2), dict(maximize=None),
    dict(jitter=-1e-9), dict(jitter=np.nan), dict(jitter=np.inf), dict(jitter="small"), dict(jitter=True),
    dict(z=np.zeros((2, 5))), dict(z=np.zeros((0, 4))), dict(z=np.zeros((_lib.SBO_MAX_PATHS + 1, 4))), dict(z=np.full((2, 4), np.nan)),
    dict(z=np.zeros((2, 2, 4))),
], ids=lambda kw: "-".join(kw))
def test_joint_arguments_refuses(kwargs):
    args = dict(GOOD)
    args.update(kwargs)
    with pytest.raises(ValueError):
        SweepEngine.joint_arguments(**args)


def test_accepted_arguments_come_back_in_library_form():
    pts, output, S, seed, z, noise, jitter, maximize = SweepEngine.joint_arguments(2, 3, [[1, 2], [3, 4]], np.int64(2), 0, 5, None, True, 0,
                                                                                   np.bool_(False))
    assert pts.dtype == np.float64 and pts.flags.c_contiguous and pts.shape == (2, 2)
    assert (output, S, seed, z, noise, jitter, maximize) == (2, 0, 5, None, 1, 0.0, 0)
    assert type(output) is int and type(jitter) is float
    zz = np.asfortranarray(np.ones((3, 2), dtype=np.float32))
    _, _, S, _, z, _, _, _ = SweepEngine.joint_arguments(0, 0, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0][:2], 7, 1, 0, zz[:, :1])
    assert S == 3 and z.dtype == np.float64 and z.flags.c_contiguous and z.shape == (3, 1)
    cap = SweepEngine.joint_arguments(2, 2, np.zeros((_lib.SBO_JOINT_MAX_POINTS, 2)))[0]
    assert cap.shape[0] == _lib.SBO_JOINT_MAX_POINTS
    with pytest.raises(ValueError, match="SBO_JOINT_MAX_POINTS"):
        SweepEngine.joint_arguments(2, 2, np.zeros((_lib.SBO_JOINT_MAX_POINTS + 1, 2)))


# ------------------------------------------------------------------------------------------ 8, 9. the host class
class _FakeEngine:
    def __init__(self, S):
        self.S, self.paths, self.joint = S, [], []

    def mask(self, which, c=0):
        assert which == "S"
        return self.S

    def sample_paths(self, points, n_paths, output=0, features=1024, seed=0, **kw):
        self.paths.append(dict(points=np.array(points), k=n_paths, output=output, features=features, seed=seed, **kw))
        idx = np.arange(n_paths) % len(points)
        return {"index": idx, "x": np.asarray(points)[idx], "value": np.arange(n_paths, dtype=np.float64)}

    def posterior_joint(self, points, output=0, n_draws=0, seed=0, **kw):
        SweepEngine.joint_arguments(np.asarray(points).shape[1], 2, points, output, n_draws, seed)      # (what the real method checks first)
        self.joint.append(dict(points=np.array(points), k=n_draws, output=output, seed=seed, **kw))
        idx = (np.arange(n_draws) + 1) % len(points)
        return {"mean": np.zeros(len(points)), "index": idx, "x": np.asarray(points)[idx], "value": -np.arange(n_draws, dtype=np.float64),
                "pivot_min": 1.0, "pivot_row": 0}


def _host(monkeypatch, grid, members):
    m = SafeOpt.BO([mr.benoit_f, mr.benoit_g], mr.BOUND, 3.0, grid=grid)
    S = np.zeros(grid[0] * grid[1], dtype=bool)
    S[members] = True
    fake = _FakeEngine(S)
    swept = []
    monkeypatch.setattr(m, "_engine", fake)                  # (the ``engine`` property hands out what is there)
    monkeypatch.setattr(m, "sweep", lambda want_masks=False: swept.append(want_masks))
    return m, fake, swept


def test_exact_thompson_hands_over_the_pool_thompson_hands_to_sample_paths(monkeypatch):
    m, fake, swept = _host(monkeypatch, (6, 5), [28, 3, 17, 4])
    Xp, vp = m.Thompson(3, seed=11, features=256)
    X, value = m.Thompson(3, seed=11, features=256, exact=True)
    assert swept == [True, True] and len(fake.paths) == 1 and len(fake.joint) == 1
    call = fake.joint[0]
    assert np.array_equal(call["points"], fake.paths[0]["points"]) and np.array_equal(call["points"], m._all_points()[[3, 4, 17, 28]])
    assert (call["k"], call["output"], call["seed"]) == (3, 0, 11) and "features" not in call
    assert not any(call.get(k) for k in ("return_cov", "return_chol", "return_draws"))
    assert X.shape == (3, 2) and np.array_equal(X, m._all_points()[[4, 17, 28]]) and value.tolist() == [0.0, -1.0, -2.0]
    assert np.array_equal(Xp, m._all_points()[[3, 4, 17]]) and vp.tolist() == [0.0, 1.0, 2.0]
    # the keyword goes last and its default is today's call
    import inspect
    params = list(inspect.signature(SafeOpt.BO.Thompson).parameters.values())
    assert [p.name for p in params] == ["self", "k", "seed", "features", "exact"] and params[-1].default is False
    m.Thompson(3, 11, 256)
    assert len(fake.paths) == 2 and len(fake.joint) == 1
    fake.S = np.zeros(30, dtype=bool)
    X0, v0 = m.Thompson(2, exact=True)
    assert X0.shape == (0, 2) and v0.shape == (0,) and len(fake.joint) == 1
    for bad in (dict(k=0), dict(k=65), dict(k=2.0), dict(k=2, seed=-1)):
        with pytest.raises(ValueError):
            m.Thompson(exact=True, **bad)
    assert "not reference behaviour" in SafeOpt.BO.Thompson.__doc__ and "SBO_JOINT_MAX_POINTS" in SafeOpt.BO.Thompson.__doc__


def test_exact_thompson_raises_above_the_cap(monkeypatch):
    cap = _lib.SBO_JOINT_MAX_POINTS
    m, fake, _ = _host(monkeypatch, (64, 33), np.arange(cap + 1))
    with pytest.raises(ValueError, match=f"SBO_JOINT_MAX_POINTS = {cap}"):
        m.Thompson(2, exact=True)
    assert fake.joint == [] and fake.paths == []              # (no silent fallback to the paths)
    X, _ = m.Thompson(2)                                      # (the paths take the same pool)
    assert len(fake.paths) == 1 and len(fake.paths[0]["points"]) == cap + 1 and X.shape == (2, 2)
    fake.S[cap] = False
    m.Thompson(2, exact=True)
    assert len(fake.joint) == 1 and len(fake.joint[0]["points"]) == cap
