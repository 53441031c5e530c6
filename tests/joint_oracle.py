"""NumPy statements of sbo_posterior_joint and the committed case list of its GPU test.

The posterior of a point list as a multivariate normal, normalised units, output o:
  mu = mp + k(P, X) inv(K + sn2 I) (y - mp),   C = k(P, P) - k(P, X) inv(K + sn2 I) k(X, P),
  A = C + (noise sn2 + jitter sf2) I = L L^T,   f_s = mu + L z_s.
Three routes, each giving {"mean" [m], "C" [m, m], "L" [m, m], "draws" [m, S]}:
  joint_solve  np.linalg.solve on K + sn2 I built from the hyper-parameters: the definition;
  joint_invK   the same formulas on the caller's inverse ds["invKopt"];
  joint_white  through the Cholesky factor of K + sn2 I (t_p = inv(Lk) k(X, p), C = Kpp - T^T T), as the device goes.
C is symmetrised ((C + C^T) / 2) before it is factored: np.linalg.cholesky reads one triangle only.  A case is sharp when every draw's
top-two gap at the end ``maximize`` selects exceeds SHARP: then the device's indices must equal the oracle's exactly
(tests/test_posterior_joint_cpu.py holds every committed case with draws to that)."""
import functools

import numpy as np

import oracle
from safebo_amd import SweepEngine

import batch_oracle as bo
import expander_oracle as eo
import paths_oracle as po

TOL64 = eo.TOL64                      # 1e-10 normalised: the project's fp64 bar
SHARP = eo.SHARP                      # 1e-8: top-two gaps above which indices are compared exactly
best, sharpness = po.best, po.sharpness


def _parts(ds, o, points):
    ell, sf2, sn2 = bo.params(ds, o)
    mp = float(oracle.mean_prior(ds)[o])
    Xn, P = np.asarray(ds["X_norm"], dtype=np.float64), bo.normalise(ds, points)
    r = np.asarray(ds["Y_norm"][:, o], dtype=np.float64) - mp
    return ell, sf2, sn2, mp, Xn, P, r, oracle.cov_mat(Xn, P, ell, sf2), oracle.cov_mat(P, P, ell, sf2)


def _finish(mu, C, sf2, sn2, z, noise, jitter):
    C = 0.5 * (C + C.T)
    m = C.shape[0]
    L = np.linalg.cholesky(C + (sn2 * bool(noise) + jitter * sf2) * np.eye(m))
    z = np.zeros((0, m)) if z is None else np.asarray(z, dtype=np.float64).reshape(-1, m)
    return {"mean": mu, "C": C, "L": L, "draws": mu[:, None] + L @ z.T}


def joint_solve(ds, o, points, z=None, noise=False, jitter=0.0):
    """By the definition: linear solves on K + sn2 I built from the hyper-parameters."""
    ell, sf2, sn2, mp, Xn, P, r, kx, Kpp = _parts(ds, o, points)
    K = oracle.cov_mat(Xn, Xn, ell, sf2) + sn2 * np.eye(Xn.shape[0])
    sol = np.linalg.solve(K, np.column_stack([kx, r]))
    return _finish(mp + kx.T @ sol[:, -1], Kpp - kx.T @ sol[:, :-1], sf2, sn2, z, noise, jitter)


def joint_invK(ds, o, points, z=None, noise=False, jitter=0.0):
    """On the caller's inverse."""
    _, sf2, sn2, mp, _, _, r, kx, Kpp = _parts(ds, o, points)
    invK = np.asarray(ds["invKopt"][o], dtype=np.float64)
    return _finish(mp + kx.T @ (invK @ r), Kpp - kx.T @ (invK @ kx), sf2, sn2, z, noise, jitter)


def joint_white(ds, o, points, z=None, noise=False, jitter=0.0):
    """Through the Cholesky factor of K + sn2 I: the whitened vectors t_p, C = Kpp - T^T T, mu = mp + T^T w."""
    ell, sf2, sn2, mp, Xn, P, r, kx, Kpp = _parts(ds, o, points)
    Lk = np.linalg.cholesky(oracle.cov_mat(Xn, Xn, ell, sf2) + sn2 * np.eye(Xn.shape[0]))
    tw = np.linalg.solve(Lk, np.column_stack([kx, r]))
    T, w = tw[:, :-1], tw[:, -1]
    return _finish(mp + T.T @ w, Kpp - T.T @ T, sf2, sn2, z, noise, jitter)


ROUTES = (joint_solve, joint_invK, joint_white)


# ---- the committed cases of tests/test_gpu_posterior_joint.py ------------------------------------------------------------------------
# (n, m, S, d, q, output, maximize, noise, jitter, use_invK, seed), each edge once, not the product.  By the constants of
# csrc/joint.hip and csrc/slab_tiles.hpp (kSlabK) (tests/test_posterior_joint_cpu.py reads them from the source and holds this list to them):
#   k_joint_cov / _diag / _panel / _update   tiles and panels of kJointTile = 64: m in {1, 2, 63, 64, 65, 129, 257, 513} and the cap
#                  SBO_JOINT_MAX_POINTS = 2048 (with n = 64); the K axis of the covariance in slabs of kSlabK = 32 over n: n in {1, 31,
#                  32, 33, 300, 1025} and SBO_MAX_N = 2048 (with m = 65);
#   k_joint_draw   tiles of kJointDrawTile = 128 points; draws in blocks of 16, instantiated for 16 | 32 | 64: S in {0, 1, 16, 17, 64};
#   padded lanes   d = 1 in dpad 2, d = 3 in dpad 4, d = 8 in dpad 8;
#   outputs        q in {1, 2, 3, 4} with the first and the last output; both values of maximize and of noise; both factor sources;
#   jitter         0 with noise = 1, and 1e-8, 1e-6, 1e-4.
# ``log_sn``: the noise of every output (-1 keeps the routes together at these n, as in tests/batch_oracle.py).
CASES = [
    dict(n=1, m=1, S=1, d=2, q=2, output=0, maximize=0, noise=1, jitter=0.0, use_invK=True, seed=81),
    dict(n=31, m=2, S=16, d=1, q=2, output=1, maximize=1, noise=0, jitter=1e-6, use_invK=False, seed=82),
    dict(n=32, m=63, S=17, d=2, q=1, output=0, maximize=0, noise=0, jitter=1e-4, use_invK=True, seed=83),
    dict(n=33, m=64, S=64, d=3, q=3, output=2, maximize=1, noise=1, jitter=0.0, use_invK=False, seed=84),
    dict(n=40, m=65, S=0, d=2, q=2, output=1, maximize=0, noise=0, jitter=1e-6, use_invK=True, seed=85),
    dict(n=64, m=129, S=16, d=8, q=4, output=3, maximize=0, noise=0, jitter=1e-6, use_invK=False, seed=86),
    dict(n=300, m=257, S=64, d=2, q=4, output=0, maximize=1, noise=1, jitter=1e-8, use_invK=True, seed=87),
    dict(n=40, m=513, S=17, d=2, q=2, output=0, maximize=0, noise=0, jitter=1e-8, use_invK=False, seed=88),
    dict(n=1025, m=65, S=16, d=2, q=2, output=1, maximize=1, noise=1, jitter=1e-6, use_invK=True, seed=89, log_sn=-1.0),
    dict(n=2048, m=65, S=16, d=2, q=2, output=0, maximize=0, noise=1, jitter=0.0, use_invK=False, seed=90, log_sn=-1.0),
    dict(n=64, m=2048, S=64, d=2, q=2, output=0, maximize=0, noise=1, jitter=1e-6, use_invK=True, seed=91),
]


def case_id(c):
    return "n{n}-m{m}-S{S}-d{d}-q{q}-o{output}-{end}-{kind}-j{jitter:g}-{src}".format(
        end="max" if c["maximize"] else "min", kind="y" if c["noise"] else "f", src="invK" if c["use_invK"] else "hyper", **c)


def make_case(c):
    """(ds, points [m, d], z [S, m] or None) of a case: batch_oracle.make_case's data, a uniform pool in its box, and the draws of
    SweepEngine.joint_draws under the case's seed."""
    ds, pool, _ = bo.make_case(dict(n=c["n"], m=c["m"], d=c["d"], q=c["q"], seed=c["seed"], n_pending=0, output=0,
                                    **({"log_sn": c["log_sn"]} if "log_sn" in c else {})))
    return ds, pool, (SweepEngine.joint_draws(c["m"], c["S"], c["seed"]) if c["S"] else None)


@functools.lru_cache(maxsize=None)
def reference(i):
    """Case i and its reference, computed once per process: (ds, points, z, joint_solve's result, normalised units)."""
    c = CASES[i]
    ds, pool, z = make_case(c)
    ref = joint_solve(ds, c["output"], pool, z, c["noise"], c["jitter"])
    for a in ref.values():
        a.setflags(write=False)
    if z is not None:
        z.setflags(write=False)
    return ds, pool, z, ref
