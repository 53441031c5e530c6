"""NumPy statements of sbo_sample_paths and the committed case list of its GPU test.

A sample path by pathwise conditioning (Matheron's rule), normalised units, output o, u(p) = xn(p) / sqrt(ell):
  phi_f(p) = sqrt(2 sf2 / F) cos(omega_f . u(p) + phase_f),  prior_s(p) = sum_f weights[s][f] phi_f(p),
  r_s[j] = (Y_norm[j][o] - mp) - prior_s(X_j) - sqrt(sn2) noise[s][j],  c_s = inv(K + sn2 I) r_s,
  f_s(p) = mp + prior_s(p) + sum_j k(X_j, p) c_s[j].
Two routes to f [m, S]:
  paths_solve  np.linalg.solve on K + sn2 I built from the hyper-parameters: the definition;
  paths_invK   the same formulas on the caller's inverse ds["invKopt"].
A case is sharp when every path's top-two gap at the end ``maximize`` selects exceeds SHARP: then the device's indices must equal the
oracle's exactly (tests/test_sample_paths_cpu.py holds every committed case to that)."""
import functools

import numpy as np

import oracle
from safebo_amd import SweepEngine

import batch_oracle as bo
import expander_oracle as eo

TOL64 = eo.TOL64                      # 1e-10 normalised: the project's fp64 bar
SHARP = eo.SHARP                      # 1e-8: top-two gaps above which indices are compared exactly


def _features(U, omega, phase, sf2):
    """phi [rows of U, F]."""
    return np.sqrt(2.0 * sf2 / omega.shape[0]) * np.cos(U @ omega.T + phase)


def _paths(ds, o, draws, points, solve, use_noise=True, scale=None):
    omega, phase, weights, noise = (np.asarray(a, dtype=np.float64) for a in draws)
    ell, sf2, sn2 = bo.params(ds, o)
    mp = float(oracle.mean_prior(ds)[o])
    Xn, P = np.asarray(ds["X_norm"], dtype=np.float64), bo.normalise(ds, points)
    rs = 1.0 / np.sqrt(ell)
    phi_X, phi_P = _features(Xn * rs, omega, phase, sf2), _features(P * rs, omega, phase, sf2)
    if scale is not None:                                    # (a wrong feature scale, for the test that the bound tells it apart)
        phi_X, phi_P = phi_X * scale, phi_P * scale
    R = (np.asarray(ds["Y_norm"][:, o], dtype=np.float64) - mp)[:, None] - phi_X @ weights.T
    if use_noise:
        R = R - np.sqrt(sn2) * noise.T
    return mp + phi_P @ weights.T + oracle.cov_mat(Xn, P, ell, sf2).T @ solve(R, Xn, ell, sf2, sn2)


def paths_solve(ds, o, draws, points, **kw):
    """f [m, S] by the definition: a linear solve on K + sn2 I built from the hyper-parameters."""
    return _paths(ds, o, draws, points,
                  lambda R, Xn, ell, sf2, sn2: np.linalg.solve(oracle.cov_mat(Xn, Xn, ell, sf2) + sn2 * np.eye(Xn.shape[0]), R), **kw)


def paths_invK(ds, o, draws, points, **kw):
    """f [m, S] on the caller's inverse."""
    return _paths(ds, o, draws, points, lambda R, *_: np.asarray(ds["invKopt"][o], dtype=np.float64) @ R, **kw)


def posterior(ds, o, points):
    """(mean [m], variance [m]) of output o in normalised units, on the caller's inverse (the formulas of oracle.gp_inference; the
    variance is not clipped)."""
    ell, sf2, _ = bo.params(ds, o)
    mp = float(oracle.mean_prior(ds)[o])
    Xn, invK = np.asarray(ds["X_norm"], dtype=np.float64), np.asarray(ds["invKopt"][o], dtype=np.float64)
    kx = oracle.cov_mat(Xn, bo.normalise(ds, points), ell, sf2)
    return mp + kx.T @ (invK @ (np.asarray(ds["Y_norm"][:, o], dtype=np.float64) - mp)), sf2 - np.sum(kx * (invK @ kx), axis=0)


def best(values, maximize):
    """(index [S], value [S]) of every path: the arg-min (``maximize``: arg-max) over the points, lowest index on a tie."""
    idx = np.argmax(values, axis=0) if maximize else np.argmin(values, axis=0)
    return idx.astype(np.int64), values[idx, np.arange(values.shape[1])]


def sharpness(values, maximize):
    """The smallest top-two gap over the paths at the end ``maximize`` selects (inf with one point)."""
    if values.shape[0] < 2:
        return float("inf")
    v = np.sort(-values if maximize else values, axis=0)
    return float(np.min(v[1] - v[0]))


# ---- the committed cases of tests/test_gpu_sample_paths.py ---------------------------------------------------------------------------
# (n, m, F, S, d, q, output, maximize, use_invK, seed), each edge once, not the product.  By the constants of csrc/paths.hip and
# csrc/slab_tiles.hpp (kSlabK)
# (tests/test_sample_paths_cpu.py reads them from the source and holds this list to them):
#   k_path_main    point tiles of kPathTile = 128: m in {1, 127, 128, 129, 513}; min(tiles, kPathGridTiles = 1024) workgroups walk the
#                  tiles: m = 131 073 gives workgroup 0 a second tile of one point; the K axis in slabs of kSlabK = 32, the features
#                  rounded up to a slab, then the observations: F in {1, 31, 32, 33, 1024, 8192}, n in {1, 2, 31, 32, 33, 64, 65, 300};
#                  F = 33 with n = 33: both kinds of column end in a slab that holds one of them; paths in blocks of 16, instantiated
#                  for 16 | 32 | 64: S in {1, 15, 16, 17, 33, 64};
#   k_path_solve   no tiers: 1024 threads, a wave per row and a thread per column in strides of 1024 -- n = 1024 | 1025 (a second
#                  column for thread 0) and n = SBO_MAX_N = 2048;
#   padded lanes   d = 1 in dpad 2, d = 3 in dpad 4, d = 6 and 8 in dpad 8;
#   outputs        q in {1, 2, 3, 4} with the first and the last output; both values of maximize; both factor sources.
# ``log_sn``: the noise of every output (-1 keeps the two routes together at these n, as in tests/batch_oracle.py).
CASES = [
    dict(n=1, m=1, F=1, S=1, d=2, q=2, output=0, maximize=0, use_invK=True, seed=61),
    dict(n=2, m=127, F=31, S=15, d=1, q=2, output=1, maximize=1, use_invK=False, seed=62),
    dict(n=31, m=128, F=32, S=16, d=2, q=1, output=0, maximize=0, use_invK=True, seed=63),
    dict(n=32, m=129, F=33, S=17, d=3, q=3, output=2, maximize=1, use_invK=False, seed=64),
    dict(n=33, m=513, F=33, S=33, d=6, q=4, output=3, maximize=0, use_invK=True, seed=65),
    dict(n=64, m=65, F=1024, S=64, d=8, q=3, output=0, maximize=1, use_invK=False, seed=66),
    dict(n=65, m=257, F=8192, S=3, d=2, q=2, output=0, maximize=0, use_invK=True, seed=67),
    dict(n=300, m=257, F=1024, S=64, d=2, q=4, output=0, maximize=0, use_invK=False, seed=68),
    dict(n=40, m=257, F=1024, S=64, d=2, q=2, output=1, maximize=1, use_invK=True, seed=69),
    dict(n=2, m=131073, F=32, S=1, d=2, q=2, output=0, maximize=0, use_invK=True, seed=70),
    dict(n=1024, m=65, F=1024, S=16, d=2, q=2, output=0, maximize=0, use_invK=True, seed=71, log_sn=-1.0),
    dict(n=1025, m=33, F=1024, S=16, d=2, q=2, output=1, maximize=1, use_invK=False, seed=72, log_sn=-1.0),
    dict(n=2048, m=65, F=1024, S=16, d=2, q=2, output=0, maximize=0, use_invK=False, seed=73, log_sn=-1.0),
]


def case_id(c):
    return "n{n}-m{m}-F{F}-S{S}-d{d}-q{q}-o{output}-{end}-{src}".format(end="max" if c["maximize"] else "min",
                                                                         src="invK" if c["use_invK"] else "hyper", **c)


def make_case(c):
    """(ds, points [m, d], draws) of a case: batch_oracle.make_case's data, a uniform pool in its box, and the draws of
    SweepEngine.path_draws under the case's seed."""
    ds, pool, _ = bo.make_case(dict(n=c["n"], m=c["m"], d=c["d"], q=c["q"], seed=c["seed"], n_pending=0, output=0,
                                    **({"log_sn": c["log_sn"]} if "log_sn" in c else {})))
    return ds, pool, SweepEngine.path_draws(c["d"], c["n"], c["S"], c["F"], c["seed"])


@functools.lru_cache(maxsize=None)
def reference(i):
    """Case i and its reference, computed once per process: (ds, points, draws, f [m, S] by paths_solve, normalised units)."""
    c = CASES[i]
    ds, pool, draws = make_case(c)
    f = paths_solve(ds, c["output"], draws, pool)
    f.setflags(write=False)
    return ds, pool, draws, f
