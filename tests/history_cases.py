"""Models of the directed sequences of tests/test_gpu_history.py that need a construction: two fp32 models A and B of one shape whose
fp64 twins cannot be mistaken for one another.  CPU only (NumPy); tests/test_history_walk_cpu.py asserts what is claimed here.

B starts from 64 Benoit observations on [-2, 2]^2 under the default hyper-parameters; its constraint data Y_norm[:, 1] are then moved
(the posterior mean is linear in them: the least-norm solution of one small system) so that the fp64 lcb_1 of K candidates of the
64 x 66 grid, spread along the boundary of the safe set, lies DELTA (normalised) from zero, each on the side it was on.  DELTA = 1e-8 is
a hundred times the project's fp64 bar (1e-10: the fp64 twin and the NumPy oracle decide these candidates alike) and far below what an
fp32 posterior resolves (a mean of order one carries 6e-8 of rounding per operation, the measured band is never under 1e-4): the fp32
posterior decides each of them by its rounding, the fp64 posterior does not.  A is B with the same K candidates moved MARGIN = 2e-2 to
the same sides (and another objective): its fp64 posterior decides every one of them as B's fp64 posterior does -- so wherever B's
fp32 masks differ from B's fp64 masks on these candidates, A's fp64 posterior contradicts the fp32 one."""
import functools

import numpy as np

import oracle
from safebo_amd import synthetic

LO, HI, COUNT, B_CONF = np.array([-2.0, -2.0]), np.array([2.0, 2.0]), [64, 66], 2.0
K, DELTA, MARGIN = 16, 1e-8, 2e-2


def _weights(ds, pts, o):
    """w [N, n] with mean_norm = mp + w (Y_norm[:, o] - mp) at pts, as oracle.gp_inference forms it."""
    d = ds["X_norm"].shape[1]
    hyper = ds["hypopt"][:, o]
    k = oracle.calc_cov_mat(ds["X_norm"], (pts - ds["X_mean"]) / ds["X_std"], np.exp(2 * hyper[:d]), np.exp(2 * hyper[d]))
    return np.matmul(k.T, ds["invKopt"][o])


def _lcb1(ds, pts):
    mean, var = oracle.gp_inference(pts, ds)
    return (mean[:, 1] - B_CONF * np.sqrt(var[:, 1])) / max(1.0, float(ds["Y_std"][1]))


def _moved(ds, pts, target):
    """ds with Y_norm[:, 1] moved by the least-norm step that puts the normalised lcb_1 at pts on `target` (two corrections)."""
    out = dict(ds)
    w = _weights(ds, pts, 1) * float(ds["Y_std"][1]) / max(1.0, float(ds["Y_std"][1]))
    for _ in range(3):
        step = np.linalg.lstsq(w, target - _lcb1(out, pts), rcond=None)[0]
        Y = np.array(out["Y_norm"])
        Y[:, 1] += step
        out["Y_norm"] = Y
    return out


@functools.lru_cache(maxsize=1)
def twin_models():
    """dict: A, B (datasets of equal n, d, q, X and hyper-parameters), pts, picked [K] candidate indices, side [K] (+1 / -1)."""
    rng = np.random.default_rng(11)
    X = rng.uniform(-2.0, 2.0, size=(64, 2))
    base = synthetic.make_dataset(X, synthetic.benoit(X), synthetic.default_hypopt(2, 2))
    pts = oracle.grid_points(LO, HI, COUNT)
    lcb = _lcb1(base, pts)
    picked = []
    for j in np.argsort(np.abs(lcb)):                   # nearest the threshold first, no two within four grid steps of each other
        ij = np.array([j % COUNT[0], j // COUNT[0]])
        if all(np.max(np.abs(ij - np.array([p % COUNT[0], p // COUNT[0]]))) >= 4 for p in picked):
            picked.append(int(j))
        if len(picked) == K:
            break
    picked = np.array(picked)
    side = np.where(lcb[picked] >= 0, 1.0, -1.0)
    B = _moved(base, pts[picked], side * DELTA)
    A = _moved(base, pts[picked], side * MARGIN)
    YA = np.array(A["Y_norm"])
    YA[:, 0] = 0.5 * YA[:, 0] + 0.3 * np.sin(3.0 * X[:, 0])
    A["Y_norm"] = YA
    return {"A": A, "B": B, "pts": pts, "picked": picked, "side": side}
