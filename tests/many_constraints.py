"""Models with three to seven constraints on which EVERY constraint shapes the sets -- shared by tests/test_many_constraints_cpu.py
(the oracle alone: the preconditions) and tests/test_gpu_many_constraints.py (the device against the oracle).

Discs with shifted centres do not serve (``disc_model``, kept as the counter-example the CPU test rejects): U asks for every
constraint violated, so with many constraints it lies far from S and the G_c / O_c come out empty.  A fan of half-planes does:

    X ~ U(-1, 1)^d, objective sin(2 X).sum(1) + 0.3 X[:, 0]
    constraint c = 1 .. q-1:  g_c(x) = amp_c (t_c - x . u_c) + 0.15 sin(3 x[c % d] + c)
        theta_c = 0.5 ((c-1) / max(1, q-2) - 0.5), u_c = (cos theta_c, sin theta_c, 0, ..)
        t_c = 0.25 + 0.05 ((3c) % 4), amp_c = 0.6 + 0.2 ((3c) % 5)

``order`` permutes the constraint columns (the hyper-parameters stay with the column position), which is what moves the winner of
the host-side tie rules (expander_best_c, target_best_c) away from constraint 1."""
import functools

import numpy as np

import oracle
import robust_oracle
from safebo_amd import synthetic

B = 3.0


def hyper_parameters(d, q):
    hyp = synthetic.default_hypopt(d, q, log_ell=0.3, log_sn=-2.0)
    hyp[:d] += 0.2 * np.arange(q)[None, :] / q
    return hyp


def fan_outputs(X, q, order=None):
    """The q noise-free outputs of the fan at the rows of X [N, d]: [N, q]."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    d = X.shape[1]
    cols = []
    for c in range(1, q):
        theta = 0.5 * ((c - 1) / max(1, q - 2) - 0.5)
        u = np.zeros(d)
        u[0], u[1 % d] = np.cos(theta), (np.sin(theta) if d > 1 else 0.0)
        t, amp = 0.25 + 0.05 * ((3 * c) % 4), 0.6 + 0.2 * ((3 * c) % 5)
        cols.append(amp * (t - X @ u) + 0.15 * np.sin(3.0 * X[:, c % d] + c))
    if order is not None:
        assert sorted(order) == list(range(1, q))
        cols = [cols[c - 1] for c in order]
    return np.stack([np.sin(2.0 * X).sum(1) + 0.3 * X[:, 0]] + cols, axis=1)


def fan_inputs(d, n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(n, d))


def fan_model(q, d=2, n=40, seed=0, order=None):
    X = fan_inputs(d, n, seed)
    return synthetic.make_dataset(X, fan_outputs(X, q, order), hyper_parameters(d, q))


def disc_model(q, d=2, n=40, seed=0):
    """The obvious construction that does NOT work: constraint c is a disc of radius 0.8 whose centre sits on a circle of radius
    0.4 (every G_c and O_c comes out empty on the 40 x 36 grid, for q = 4, 5 and 8)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, size=(n, d))
    cols = []
    for c in range(1, q):
        a = 2.0 * np.pi * (c - 1) / (q - 1)
        ctr = np.zeros(d)
        ctr[0], ctr[1 % d] = 0.4 * np.cos(a), 0.4 * np.sin(a)
        cols.append(0.64 - np.sum((X - ctr) ** 2, axis=1))
    Y = np.stack([np.sin(2.0 * X).sum(1) + 0.3 * X[:, 0]] + cols, axis=1)
    return synthetic.make_dataset(X, Y, hyper_parameters(d, q))


# name -> q, d, n, seed, order, count.  The GPU file sweeps every one of them; the CPU file checks every one of them.
CASES = {
    "q4": dict(q=4, d=2, n=40, seed=0, order=None, count=[40, 36]),
    "q5": dict(q=5, d=2, n=40, seed=0, order=None, count=[40, 36]),
    "q8": dict(q=8, d=2, n=40, seed=3, order=None, count=[40, 36]),
    "q5_perm": dict(q=5, d=2, n=40, seed=0, order=[2, 3, 1, 4], count=[40, 36]),
    "q8_perm": dict(q=8, d=2, n=40, seed=0, order=[5, 1, 2, 3, 4, 6, 7], count=[40, 36]),
    "q4_gemm": dict(q=4, d=2, n=40, seed=0, order=None, count=[72, 70]),
    "q5_gemm": dict(q=5, d=2, n=40, seed=0, order=None, count=[72, 70]),
    "q8_gemm": dict(q=8, d=2, n=40, seed=3, order=None, count=[72, 70]),
    "q5_ranks": dict(q=5, d=2, n=40, seed=0, order=None, count=[40, 37]),      # 37 lines: uneven shards on 2 and on 3 ranks
    "q8_ranks": dict(q=8, d=2, n=40, seed=3, order=None, count=[40, 37]),
    "q4_3d": dict(q=4, d=3, n=60, seed=0, order=None, count=[13, 11, 10]),
    "q5_3d": dict(q=5, d=3, n=60, seed=0, order=None, count=[13, 11, 10]),
    "q8_3d": dict(q=8, d=3, n=60, seed=0, order=None, count=[13, 11, 10]),
}
# trust-region balls (centre, radius) per dimension: they must cut through S (0 < |T| < |S|, checked on the CPU)
TR_BALL = {2: (np.array([-0.3, 0.1]), 0.5), 3: (np.array([-0.3, 0.1, 0.0]), 0.7)}
# a caller's own target for explore_safeset: outside the safe set, off the grid
EXPLORE_TARGET = {2: np.array([0.83, -0.41]), 3: np.array([0.83, -0.41, 0.2])}


# the robust (StableOpt) sweep: the q5 model on a joint grid, axis 0 the control, axis 1 the disturbance, zero prior mean
ROBUST_COUNT, ROBUST_B = [61, 41], 1.0


def box(d):
    return np.full(d, -1.2), np.full(d, 1.2)


@functools.lru_cache(maxsize=None)
def model(name, builder=fan_model):
    k = CASES[name]
    if builder is fan_model:
        return fan_model(k["q"], k["d"], k["n"], k["seed"], k["order"])
    return builder(k["q"], k["d"], k["n"], k["seed"])          # (a counter-example model: no column order)


@functools.lru_cache(maxsize=None)
def points(name):
    k = CASES[name]
    lo, hi = box(k["d"])
    return oracle.grid_points(lo, hi, k["count"])


@functools.lru_cache(maxsize=None)
def reference(name, quirk, builder=fan_model):
    """The oracle's SafeOpt, GoOSE and trust-region results of a case, computed once per process (one posterior for the three) and
    never modified by the tests that share it."""
    k = CASES[name]
    ds, pts = model(name, builder), points(name)
    mv = oracle.gp_inference(pts, ds)
    s = oracle.safeopt_sweep(pts, ds, B, quirk_L_index=quirk, mean_var=mv)
    g = oracle.goose_sweep(pts, ds, B, quirk_L_index=quirk, mean_var=mv)
    x0, r = TR_BALL[k["d"]]
    t = oracle.tr_sweep(pts, ds, B, x0, r, mean_var=mv)
    return s, g, t


def explore_reference(pts, S, target):
    """models/GoOSE.py:116-119 on a candidate list: the safe candidate closest to ``target`` (first on ties)."""
    d2 = np.sum((pts - np.asarray(target)) ** 2, axis=1)
    return int(np.argmin(np.where(S, np.sqrt(d2), np.inf)))


def sole_excluders(lcb):
    """How many constraints are the ONLY one that keeps some candidate out of S."""
    bad = lcb[:, 1:] < 0
    only = bad & (bad.sum(axis=1, keepdims=True) == 1)
    return int(only.any(axis=0).sum())


def margins(name, quirk, builder=fan_model):
    """The smallest distances of a deciding quantity from its threshold: min |lcb_c| / max(1, Y_std_c) over candidates and
    constraints (S / U membership) and min over g in S and c of |ucb_c(g) - L_c dist(g, nearest U)| (G_c membership)."""
    ds, pts = model(name, builder), points(name)
    s, _, _ = reference(name, quirk, builder)
    ystd = np.maximum(1.0, ds["Y_std"][1:])
    m_lcb = float(np.min(np.abs(s["lcb"][:, 1:]) / ystd))
    S, U = s["S"], s["U"]
    m_g = np.inf
    if S.any() and U.any():
        xs, xu = pts[S], pts[U]
        dmin = np.full(xs.shape[0], np.inf)
        for i in range(0, xs.shape[0], 1024):
            dmin[i:i + 1024] = oracle.shifted_norm(xs[i:i + 1024, None, :], xu[None, :, :]).min(axis=1)
        for c in range(1, s["ucb"].shape[1]):
            m_g = min(m_g, float(np.min(np.abs(s["ucb"][S, c] - s["L_used"][c] * dmin))))
    return m_lcb, m_g


@functools.lru_cache(maxsize=None)
def robust_reference():
    lo, hi = box(2)
    return robust_oracle.robust_sweep(lo, hi, ROBUST_COUNT, 1, model("q5"), ROBUST_B, "ucb")
