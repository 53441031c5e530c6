"""Constructions that put exact ties and on-threshold candidates in front of the sweep reductions (tests/test_gpu_ties.py), and
the NumPy statements of what they promise (tests/test_tie_cases_cpu.py).  No device code: everything here runs on the CPU.

Every index a sweep returns comes out of an arg-reduction whose rule is "ties go to the lowest flat index" (np.argmax / np.argmin
order, models/SafeOpt.py:119-122, models/GoOSE.py:110-119).  Random models never tie; these do:

* mirror model   -- every observation on the hyper-plane x_last = 0 and a grid whose last (slowest) axis is bitwise symmetric
                    about 0: a kernel that evaluates each candidate with one operation sequence gives (i, j) and (i, count-1-j)
                    bitwise-equal mean and variance, in different tiles, workgroups and -- sharded -- ranks.
* duplicate list -- an explicit list with a block of points repeated at scattered positions.
* cell centres   -- explore_safeset targets with four / two / one nearest grid points.
* on-sphere TR   -- lattice points at distance exactly r from the trust region's centre.
* fp32 near-tie  -- two distances that differ in fp64 and collide when rounded to fp32.
"""
import numpy as np

import oracle

MIRROR_HYP = (-0.7, 0.3, 0.0, -4.0)          # log ell (every axis but the mirrored one), log ell (mirrored axis), log sf, log sn


# ---------------------------------------------------------------------------------------------------------------- mirror model
def mirror_model(q=2, n=24, seed=3, d=2, axis=None, same_constraints=False):
    """``inference_datasets`` dict of a d-input model of q outputs whose observations all have x[axis] = 0 (default: the last
    axis).  X_mean[axis] = 0 and X_std[axis] = 1 are set by hand (``oracle.data_normalization`` would divide by a zero std), so
    X_norm[:, axis] = 0 and the normalised candidate coordinate on that axis is the coordinate itself: +x and -x are bitwise
    mirror images.  ``same_constraints``: every constraint output carries the data and hyper-parameters of constraint 1, so
    G_1 == G_2 == .. and their winners are one candidate."""
    axis = d - 1 if axis is None else axis
    rng = np.random.default_rng(seed)
    free = [a for a in range(d) if a != axis]
    X = np.zeros((n, d))
    X[:, free[0]] = rng.uniform(-1, 1, n)
    x0 = X[:, free[0]]
    cols = [np.sin(3 * x0), 0.6 - x0 ** 2]
    noise = 0.01 * rng.standard_normal((n, 2))
    for a in free[1:]:                                       # (further free axes: drawn after the 2-D model's numbers)
        X[:, a] = rng.uniform(-1, 1, n)
        cols[0] = cols[0] + 0.4 * X[:, a]
        cols[1] = cols[1] - 0.3 * X[:, a] ** 2
    Y2 = np.stack(cols, axis=1) + noise
    extra = []
    for c in range(2, q):
        extra.append(Y2[:, 1] if same_constraints else 0.9 - 0.7 * (x0 - 0.1 * c) ** 2 + 0.01 * rng.standard_normal(n))
    Y = np.concatenate([Y2[:, :min(q, 2)]] + [e[:, None] for e in extra], axis=1)
    hyp1 = np.array([MIRROR_HYP[1] if a == axis else MIRROR_HYP[0] for a in range(d)] + [MIRROR_HYP[2], MIRROR_HYP[3]])
    hyp = np.tile(hyp1[:, None], (1, q))
    X_mean, X_std = X.mean(axis=0), X.std(axis=0)
    X_mean[axis], X_std[axis] = 0.0, 1.0
    Y_mean, Y_std = Y.mean(axis=0), Y.std(axis=0)
    X_norm = (X - X_mean) / X_std
    assert not X_norm[:, axis].any()
    return {"X_mean": X_mean, "X_std": X_std, "Y_mean": Y_mean, "Y_std": Y_std, "X_norm": X_norm, "Y_norm": (Y - Y_mean) / Y_std,
            "invKopt": oracle.build_invK(X_norm, hyp), "hypopt": hyp}


# name -> (lo, hi, count); the mirrored axis is the last one.  Dyadic steps: every coordinate is exact, +x and -x bitwise mirrors.
MIRROR_GRIDS = {
    "small": ([-1.0, -1.0], [1.0, 1.0], [65, 33]),                       # byte-mask path, a centre row (steps 2^-5 and 2^-4)
    "even": ([-1.0, -31 / 32], [1.0, 31 / 32], [65, 32]),                # no centre row: every candidate has a partner
    "tiles": ([-1.0, -63 / 64], [-1.0 + 127 / 64, 63 / 64], [128, 64]),  # two 128 x 64-row column-path tile rows' worth: one tile
    "wide": ([-1.0, -127 / 128], [-1.0 + 1023 / 512, 127 / 128], [1024, 128]),    # passes every size gate of the large-grid set phase
    "planes33": ([-1.0, -1.0], [-1.0 + 63 / 32, 1.0], [64, 33]),         # 33 planes: uneven shards on 2 and 3 ranks
    "column": ([-1.0, -1023 / 1024], [-1.0 + 1023 / 512, 1023 / 1024], [1024, 1024]),   # 1024 on both axes, whole column-path tiles
    "cube_k1t": ([-1.0, -1.0, -255 / 256], [-1.0 + 127 / 64, -1.0 + 127 / 64, 255 / 256], [128, 128, 256]),   # 2^22 candidates: K1t
    "cube_small": ([-1.0, -1.0, -15 / 16], [1.0, 1.0, 15 / 16], [17, 9, 16]),
}


def mirror_grid(name):
    lo, hi, count = MIRROR_GRIDS[name]
    return np.array(lo), np.array(hi), list(count)


def mirror_partner(index, count):
    """Flat index of the candidate mirrored in the last axis."""
    index = np.asarray(index, dtype=np.int64)
    plane = int(np.prod(count[:-1]))
    j = index // plane
    return (count[-1] - 1 - j) * plane + index % plane


def symmetrise(mean, var, count):
    """What a per-candidate kernel returns on a mirror model: the lower half of the last axis copied onto the upper half (the
    NumPy oracle's own posterior is symmetric to ~1e-16 only -- BLAS sums the two halves in different orders)."""
    q = mean.shape[1]
    shape = (count[-1], int(np.prod(count[:-1])), q)
    M, V = mean.reshape(shape).copy(), var.reshape(shape).copy()
    h = count[-1] // 2
    M[count[-1] - h:] = M[:h][::-1]
    V[count[-1] - h:] = V[:h][::-1]
    return M.reshape(-1, q), V.reshape(-1, q)


def tied(values, mask, winner):
    """Flat indices inside ``mask`` that hold ``values[winner]`` bitwise."""
    values = np.asarray(values)
    return np.flatnonzero(np.asarray(mask, dtype=bool) & (values == values[winner]))


def plane_shards(count, world):
    """[first plane, end plane) per rank of the sharded grid: the library's split of the slowest axis into whole hyper-planes,
    rank r starting at plane  planes * r // world  (``sbo_candidates_grid_sharded``)."""
    planes = int(count[-1])
    return [(planes * r // world, planes * (r + 1) // world) for r in range(world)]


def rank_of(index, count, world):
    plane = int(np.prod(count[:-1]))
    j = int(index) // plane
    for r, (a, b) in enumerate(plane_shards(count, world)):
        if a <= j < b:
            return r
    raise ValueError(index)


# ------------------------------------------------------------------------------------------------------------- duplicate lists
def duplicate_list(lo, hi, m=700, copies=3, seed=5, dtype=np.float64):
    """(points [copies * m, d], origin [copies * m]): ``m`` uniform points, the whole block repeated ``copies`` times, each repeat
    in its own fixed-seed order, so the repeats of a point sit at scattered positions.  Calling the middle segment the original,
    every point -- the winner of any reduction included -- has one duplicate at a lower and one at a higher index.
    origin[p] = the base point position p holds.  ``dtype`` float32: the points are rounded first, then repeated."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    base = rng.uniform(lo, hi, size=(m, lo.shape[0])).astype(dtype)
    origin = np.concatenate([rng.permutation(m) for _ in range(copies)])
    return np.ascontiguousarray(base[origin]), origin


# ------------------------------------------------------------------------------------------------------- cell-centre targets
CELL_LO, CELL_HI, CELL_COUNT = np.array([0.0, 0.0]), np.array([1.0, 1.0]), [33, 17]      # steps 2^-5 and 2^-4


def cell_targets():
    """(lo, hi, count, targets): name -> (target [2], flat indices of the equidistant nearest grid points, lowest first)."""
    lo, hi, count = CELL_LO, CELL_HI, CELL_COUNT
    hx, hy = 1.0 / 32, 1.0 / 16
    i, j = 11, 6
    cnt0 = count[0]
    t = {
        "centre": (np.array([(i + 0.5) * hx, (j + 0.5) * hy]), [j * cnt0 + i, j * cnt0 + i + 1, (j + 1) * cnt0 + i, (j + 1) * cnt0 + i + 1]),
        "edge_x": (np.array([(i + 0.5) * hx, j * hy]), [j * cnt0 + i, j * cnt0 + i + 1]),
        "edge_y": (np.array([i * hx, (j + 0.5) * hy]), [j * cnt0 + i, (j + 1) * cnt0 + i]),
        "point": (np.array([i * hx, j * hy]), [j * cnt0 + i]),
    }
    return lo, hi, count, t


def flat_model(n=12, seed=9, d=2):
    """One output (q = 1): no constraint, S is every candidate."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, size=(n, d))
    Y = np.sin(2 * X.sum(axis=1))[:, None]
    hyp = np.array([[-0.5]] * d + [[0.0], [-3.0]])
    return oracle.make_inference_dataset(X, Y, hyp)


def corner_model(n=30, seed=4):
    """q = 2 on the cell grid: the constraint is  x0 - (11 + 1/4) / 32  (noise-free, tight length scales, b = 0 reads the mean), so
    grid column 11 is unsafe and column 12 safe: the lowest-index corners of the 'centre' target's cell are not in S."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, size=(n, 2))
    Y = np.stack([np.sin(3 * X[:, 0]) + X[:, 1], X[:, 0] - 11.25 / 32], axis=1)
    hyp = np.array([[0.3, 0.3], [0.3, 0.3], [0.5, 0.5], [-5.0, -5.0]])
    return oracle.make_inference_dataset(X, Y, hyp)


def nearest_in(points, mask, target):
    """np.argmin of the fp64 Euclidean distance over ``mask`` (models/GoOSE.py:116-119) and the distances."""
    d = np.sqrt(((np.asarray(points, dtype=np.float64) - target) ** 2).sum(axis=1))
    return int(np.argmin(np.where(mask, d, np.inf))), d


# ------------------------------------------------------------------------------------------------------ on-sphere trust region
SPHERE_H = 2.0 ** -5
SPHERE_OFFSETS = [(5, 0), (-5, 0), (0, 5), (0, -5), (3, 4), (3, -4), (-3, 4), (-3, -4), (4, 3), (4, -3), (-4, 3), (-4, -3)]


def sphere_case():
    """(lo, hi, count, x_0, r, r_below, on_sphere flat indices): a 33 x 33 lattice of spacing h = 2^-5, x_0 its centre point,
    r = 5 h.  The twelve Pythagorean lattice points are at distance exactly r; r_below = nextafter(r, 0) excludes exactly those."""
    h = SPHERE_H
    count = [33, 33]
    lo, hi = np.array([0.0, 0.0]), np.array([32 * h, 32 * h])
    c = 16
    x0 = np.array([c * h, c * h])
    on = sorted((c + dj) * count[0] + (c + di) for di, dj in SPHERE_OFFSETS)
    return lo, hi, count, x0, 5 * h, float(np.nextafter(5 * h, 0.0)), on


# ------------------------------------------------------------------------------------------------------------ fp32 near-tie
def near_tie_list(m=3000, seed=8):
    """(points [m + 2, 2], target, near index, far index): the two points (1, 0) at index 0 and (0.99999999, 0) at the LAST index are
    at fp64 distances 1.0 and 0.99999999 from the target (0, 0); rounded to fp32 both are 1.0f.  Every other point is at distance
    >= 1.5.  The nearer point has the higher index: a reduction on fp32 distances returns index 0."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, m)
    rad = rng.uniform(1.5, 2.0, m)
    far = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    pts = np.concatenate([[[1.0, 0.0]], far, [[0.99999999, 0.0]]])
    return pts, np.zeros(2), pts.shape[0] - 1, 0


def near_tie_grid():
    """(lo, hi, count, target, near index, far index) -- a grid with the same collision: 5 x 3 points, axis 0 = 0, 2, .., 8, axis 1
    = 0, 1, 2, target (3 + 2^-30, 1): the grid points (2, 1) and (4, 1) are at distances 1 + 2^-30 and 1 - 2^-30, which are both
    1.0f in fp32 (eps 2^-23).  The nearer one, (4, 1), has the higher index."""
    lo, hi, count = np.array([0.0, 0.0]), np.array([8.0, 2.0]), [5, 3]
    t = np.array([3.0 + 2.0 ** -30, 1.0])
    return lo, hi, count, t, 1 * 5 + 2, 1 * 5 + 1


def robust_mirror_grid(axis):
    """(lo, hi, count) of the joint grid for the robust sweep of ``mirror_model(axis=axis)``: axis 0 the control, axis 1 the
    disturbance.  axis = 1: the disturbance is mirrored (the worst disturbance ties); axis = 0: the control is (the robust control
    ties), over a disturbance range the constraint 0.6 - d^2 stays positive on."""
    if axis == 1:
        return np.array([-1.0, -1.0]), np.array([1.0, 1.0]), [65, 33]
    return np.array([-31 / 32, -0.5]), np.array([31 / 32, 0.5]), [32, 65]


def near_tie_goose(n=120, seed=6, m=1200):
    """(ds, b, points, target index, near index, far index) for a full GoOSE sweep: ``near_tie_list`` with its target (0, 0)
    inserted in the middle of the list.  The constraint 1 - 1.2 exp(-|x|^2 / 0.18) is negative at the origin only, so the origin
    is the one unsafe candidate, the one member of O_1 and therefore the sweep's target; the explore step then chooses between
    the two colliding safe points."""
    pts, _, _, _ = near_tie_list(m=m)
    mid = pts.shape[0] // 2
    pts = np.concatenate([pts[:mid], [[0.0, 0.0]], pts[mid:]])
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.uniform(-2.2, 2.2, size=(n - 1, 2)), [[0.0, 0.0]]])
    r2 = (X ** 2).sum(axis=1)
    Y = np.stack([0.3 * X[:, 0] + 0.1 * r2, 1.0 - 1.2 * np.exp(-r2 / 0.18)], axis=1)
    hyp = np.array([[-0.9, -0.9], [-0.9, -0.9], [0.0, 0.0], [-4.0, -4.0]])
    return oracle.make_inference_dataset(X, Y, hyp), 1.0, pts, mid, pts.shape[0] - 1, 0
