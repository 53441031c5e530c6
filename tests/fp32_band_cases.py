"""CPU side of tests/test_gpu_fp32_band.py: the regimes (rows of REGIMES in tests/test_gpu_envelope.py at test size), their fp64 oracle
sweeps, the extended-precision posterior on the envelope file's stride-53 subsample, and the near-threshold rule.  Every reference
is computed once per regime and shared, unchanged, by the tests that need it.

Units as in tests/test_gpu_parity.py: mean / max(1, Y_std), var / max(1, Y_std)^2.

The near-threshold rule (tests/test_gpu_envelope.py): with E_formula = |oracle_fp64 - extended| a candidate may be left out of a
mask comparison only if its deciding bound lies within 8 E_formula of its threshold -- lcb_c of 0 (S, U) or lcb_0 of u* (M).  In raw
units of the bounds that is 8 (max |d mean| + b max |d sqrt(var)|).  For the regimes listed here that set is EMPTY
(the decision test asserts it before it sweeps), so the GPU tests compare every mask and index outright.
"""
import functools

import numpy as np

import oracle
from oracle import extended
from safebo_amd import synthetic

COUNT = [96, 80]
STRIDE = 53
REGIMES = [
    # config, n, log sigma_n, log ell, log sigma_f, seed of the observations (None: the config's own)
    ("B", 128, -5.0, -0.5, 0.0, None), ("B", 128, -5.0, 1.5, 0.0, None), ("B", 128, -5.0, -1.5, 0.0, None),
    # (cond(K) ~ 6e7: the fp64 formula itself is good to 1e-5 only, 8 E_formula ~ 1e-4 -- and varies by a fifth with the host's LAPACK --,
    # and with the config's own observations 1 + 3 candidates of the grid sit inside that, as with most seeds; with seed 72 the closest
    # candidate is 2.9 x 8 E_formula away and the expander set has 9 members.  Every other regime keeps a factor >= 9)
    ("B", 128, -5.0, 0.5, 1.5, 72),
    ("B", 20, -5.0, 0.5, 1.5, None), ("C", 64, -5.0, -0.5, 1.5, None), ("B", 128, -3.5, -0.5, 0.0, None),
]
IDS = ["%s%d_sn%g_ell%g_sf%g" % r[:5] for r in REGIMES]


def nerr(a, b, ystd, p):
    """max |a - b| per output, normalised; [q]"""
    d = np.abs(np.asarray(a, dtype=np.longdouble) - np.asarray(b, dtype=np.longdouble))
    return np.asarray(np.max(d, axis=0) / np.maximum(1.0, np.asarray(ystd)) ** p, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def case(i):
    cfg_name, n, log_sn, log_ell, log_sf, seed = REGIMES[i]
    cfg = synthetic.make_config(cfg_name, n=n, seed=seed)
    d, q = cfg["d"], cfg["q"]
    ds = synthetic.make_dataset(cfg["X"], cfg["Y"], synthetic.default_hypopt(d, q, log_ell=log_ell, log_sf=log_sf, log_sn=log_sn))
    lo, hi = cfg["bound"][:, 0], cfg["bound"][:, 1]
    pts = oracle.grid_points(lo, hi, COUNT)
    sub = np.arange(0, pts.shape[0], STRIDE)
    b = cfg["b"]
    so = oracle.safeopt_sweep(pts, ds, b)
    assert not so["empty_safe_set"], IDS[i]
    go = oracle.goose_sweep(pts, ds, b)
    x0 = pts[go["safe_min_index"]]
    r = 0.25 * float(np.max(hi - lo))                       # a ball through S, as in the fp32 GoOSE / trust-region parity test
    tr = oracle.tr_sweep(pts, ds, b, x0, r)
    ext = {True: extended.posterior_given_invK(pts[sub], ds), False: extended.posterior_true(pts[sub], ds)}
    near = {}
    for mode, (xm, xv) in ext.items():
        dm = np.abs(so["mean"][sub] - np.asarray(xm, dtype=np.float64)).max(axis=0)
        dsd = np.abs(np.sqrt(so["var"][sub]) - np.sqrt(np.asarray(xv, dtype=np.float64))).max(axis=0)
        band = 8.0 * (dm + b * dsd) + 1e-300                # [q], raw units of the bounds
        near_S = (np.abs(so["lcb"][:, 1:]) <= band[1:]).any(axis=1)
        near_M = np.abs(so["lcb"][:, 0] - so["u_star"]) <= band[0]
        near[mode] = {"band": band, "S": near_S, "M": near_M}
    return {"id": IDS[i], "ds": ds, "lo": lo, "hi": hi, "pts": pts, "sub": sub, "b": b, "q": q, "safeopt": so, "goose": go, "tr": tr,
            "x0": x0, "r": r, "ext": ext, "near": near}


def threshold_margin(c):
    """Smallest normalised distance of a deciding bound from its threshold over the grid (reported next to the bands)."""
    so, ys = c["safeopt"], np.maximum(1.0, c["ds"]["Y_std"])
    m = np.min(np.abs(so["lcb"][:, 1:]) / ys[1:])
    return float(min(m, np.min(np.abs(so["lcb"][:, 0] - so["u_star"])) / ys[0]))
