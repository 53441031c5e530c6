"""NumPy statements of sbo_expander_gain and the committed case list of its GPU test.

A source g is an expander when, were it measured at its optimistic value ucb_c(g) on every masked constraint c, the GP would certify
some target x.  Two routes, everything in normalised units:
  gain_naive   by the definition -- per source and constraint the full (n + 1) x (n + 1) matrix K + sn2 I over the data and g, its
               inverse, the posterior at the targets from the n + 1 observations (the last one is ucb_c(g));
  gain_rank1   by the rank-one step the device takes, on the caller's inverse: cov = k(x, g) - k_x^T invK k_g, s = v(g) + sn2,
               mu' = mu(x) + cov b sqrt(max(0, v(g))) / s, v' = v(x) - cov^2 / s.
Both return z [nc, ms, mt] (z_c(x | g) = mu' - b sqrt(max(0, v')) + Y_mean[c] / Y_std[c]), Z [ms, mt] (the minimum over the masked
constraints), count [ms] (Z >= 0), margin [ms] (max Z) and witness [ms] (its index, lowest on a tie).  A case is sharp when no
|z_c(x | g)| and no source's top-two gap of Z is below SHARP: then the device's counts and witnesses must equal the oracle's exactly
(tests/test_expander_gain_cpu.py holds every committed case to that)."""
import functools

import numpy as np

import oracle

import batch_oracle as bo
import model_remove as mr

TOL64 = mr.TOL64                      # 1e-10 normalised: the project's fp64 bar
SHARP = 1e-8                          # |z| and top-two gaps of Z above which counts and witnesses are compared exactly


def constraints_of(q, mask):
    """The constraints a mask names, ascending (0: every constraint 1 .. q - 1)."""
    return [c for c in range(1, q) if mask == 0 or mask >> c & 1]


def _model(ds, c):
    ell, sf2, sn2 = bo.params(ds, c)
    mp = float(oracle.mean_prior(ds)[c])
    return ell, sf2, sn2, mp, float(ds["Y_mean"][c] / ds["Y_std"][c])


def _summary(z):
    Z = z.min(axis=0)
    return {"z": z, "Z": Z, "count": np.sum(Z >= 0.0, axis=1).astype(np.int64), "margin": Z.max(axis=1),
            "witness": np.argmax(Z, axis=1).astype(np.int64)}


def gain_naive(ds, b, sources, targets, mask=0, only=None):
    """By the definition.  ``only``: the source rows to evaluate (the others' rows of z stay NaN)."""
    G, X = bo.normalise(ds, sources), bo.normalise(ds, targets)
    Xn = np.asarray(ds["X_norm"], dtype=np.float64)
    n, q = Xn.shape[0], ds["Y_norm"].shape[1]
    cons = constraints_of(q, mask)
    z = np.full((len(cons), G.shape[0], X.shape[0]), np.nan)
    for ci, c in enumerate(cons):
        ell, sf2, sn2, mp, shift = _model(ds, c)
        y = np.asarray(ds["Y_norm"][:, c], dtype=np.float64) - mp
        K = oracle.cov_mat(Xn, Xn, ell, sf2) + sn2 * np.eye(n)
        Kinv = np.linalg.inv(K)
        kg = oracle.cov_mat(Xn, G, ell, sf2)                                   # [n, ms]
        mu_g = mp + kg.T @ (Kinv @ y)
        v_g = sf2 - np.sum(kg * (Kinv @ kg), axis=0)
        ucb_g = mu_g + b * np.sqrt(np.maximum(0.0, v_g))
        for g in (range(G.shape[0]) if only is None else only):
            Xa = np.vstack([Xn, G[g]])
            Ka = oracle.cov_mat(Xa, Xa, ell, sf2) + sn2 * np.eye(n + 1)
            Kai = np.linalg.inv(Ka)
            ka = oracle.cov_mat(Xa, X, ell, sf2)                               # [n + 1, mt]
            ya = np.append(y, ucb_g[g] - mp)
            mu1 = mp + ka.T @ (Kai @ ya)
            v1 = sf2 - np.sum(ka * (Kai @ ka), axis=0)
            z[ci, g] = mu1 - b * np.sqrt(np.maximum(0.0, v1)) + shift
    return _summary(z)


def gain_rank1(ds, b, sources, targets, mask=0):
    """By the rank-one step on the caller's inverse (the formulas of include/safebo.h)."""
    G, X = bo.normalise(ds, sources), bo.normalise(ds, targets)
    Xn = np.asarray(ds["X_norm"], dtype=np.float64)
    q = ds["Y_norm"].shape[1]
    cons = constraints_of(q, mask)
    z = np.empty((len(cons), G.shape[0], X.shape[0]))
    for ci, c in enumerate(cons):
        ell, sf2, sn2, mp, shift = _model(ds, c)
        invK = np.asarray(ds["invKopt"][c], dtype=np.float64)
        alpha = invK @ (np.asarray(ds["Y_norm"][:, c], dtype=np.float64) - mp)
        kg, kx = oracle.cov_mat(Xn, G, ell, sf2), oracle.cov_mat(Xn, X, ell, sf2)
        Ag = invK @ kg
        mu_x, v_x = mp + kx.T @ alpha, sf2 - np.sum(kx * (invK @ kx), axis=0)
        v_g = sf2 - np.sum(kg * Ag, axis=0)
        s = v_g + sn2
        cov = oracle.cov_mat(G, X, ell, sf2) - Ag.T @ kx                       # [ms, mt]; g in the observation's place
        mu1 = mu_x[None, :] + cov * (b * np.sqrt(np.maximum(0.0, v_g)) / s)[:, None]
        v1 = v_x[None, :] - cov * cov / s[:, None]
        z[ci] = mu1 - b * np.sqrt(np.maximum(0.0, v1)) + shift
    return _summary(z)


def sharpness(res):
    """(smallest |z_c(x | g)|, smallest top-two gap of Z over the sources; inf with one target)."""
    Z = res["Z"]
    if Z.shape[1] < 2:
        return float(np.min(np.abs(res["z"]))), float("inf")
    top = np.partition(Z, Z.shape[1] - 2, axis=1)[:, -2:]
    return float(np.min(np.abs(res["z"]))), float(np.min(top[:, 1] - top[:, 0]))


# ---- the committed cases of tests/test_gpu_expander_gain.py -------------------------------------------------------------------------
# (n, ms, mt, d, q, mask, b, use_invK, seed), each edge once, not the product.  By the constants of csrc/expander.hip and
# csrc/slab_tiles.hpp (kSlabK, stage 1)
# (tests/test_expander_gain_cpu.py reads them from the source and holds this list to them):
#   k_exp_pairs    tiles of kExpTile = 64 sources x 64 targets: ms, mt in {1, 63, 64, 65, 257}; LDS slabs of kSlabK = 32 observations,
#                  t rows zero-padded to a multiple: n = 32 | 33 and 64 | 65 (a last slab that is full | holds one observation), n = 1, 2;
#                  the target tiles are split over min(tiles, kExpGridTiles / source tiles) workgroups per source tile: every case with
#                  mt > 64 gives each source a second split, ms = 1 with mt = 257 five of them; ms = 257 (5 source tiles, 204 splits)
#                  with mt = 13121 (206 target tiles) gives two splits a second tile of their own;
#   k_exp_stage1   tiers P = 32 points per workgroup up to n = 512, 16 up to 1024, 8 up to SBO_MAX_N = 2048: n in {512, 513, 1024,
#                  1025, 2048}; its LDS image n (P + 1) 8 bytes is 144 KiB at n = 2048;
#   padded lanes   d = 1 in dpad 2, d = 3 in dpad 4, d = 6 in dpad 8.
# ``log_sn``: the noise of every output (-1 keeps the oracle sharp at these n, as in tests/batch_oracle.py); ``oracle``: "rank1" where
# the naive walk (an inverse per source) would take too long; ``mixed``: some sources have count 0 and some > 0; ``shared``: the
# first targets are the first sources.
CASES = [
    dict(n=1, ms=1, mt=1, d=2, q=2, mask=0, b=3.0, use_invK=True, seed=41),
    dict(n=2, ms=63, mt=64, d=1, q=2, mask=0, b=2.0, use_invK=False, seed=42, mixed=True),
    dict(n=63, ms=64, mt=65, d=2, q=3, mask=0, b=3.0, use_invK=True, seed=43),
    dict(n=64, ms=65, mt=63, d=3, q=3, mask=4, b=0.0, use_invK=False, seed=44),
    dict(n=65, ms=257, mt=257, d=6, q=4, mask=0, b=2.0, use_invK=True, seed=45),
    dict(n=300, ms=257, mt=65, d=2, q=4, mask=2, b=3.0, use_invK=False, seed=46),
    dict(n=32, ms=65, mt=1, d=2, q=2, mask=0, b=3.0, use_invK=True, seed=47),
    dict(n=33, ms=1, mt=257, d=2, q=2, mask=2, b=2.0, use_invK=False, seed=48),
    dict(n=40, ms=257, mt=257, d=2, q=2, mask=0, b=3.0, use_invK=True, seed=49),
    dict(n=40, ms=65, mt=64, d=2, q=3, mask=0, b=2.0, use_invK=False, seed=50, shared=8),
    dict(n=8, ms=257, mt=13121, d=2, q=2, mask=0, b=3.0, use_invK=True, seed=51, mixed=True),
    dict(n=512, ms=3, mt=65, d=2, q=2, mask=0, b=3.0, use_invK=False, seed=52, log_sn=-1.0),
    dict(n=513, ms=3, mt=65, d=2, q=2, mask=0, b=3.0, use_invK=True, seed=53, log_sn=-1.0),
    dict(n=1024, ms=2, mt=65, d=2, q=2, mask=0, b=2.0, use_invK=True, seed=54, log_sn=-1.0),
    dict(n=1025, ms=2, mt=65, d=3, q=3, mask=0, b=3.0, use_invK=False, seed=55, log_sn=-1.0),
    dict(n=2048, ms=65, mt=65, d=2, q=2, mask=0, b=3.0, use_invK=False, seed=56, log_sn=-1.0, oracle="rank1"),
]


def case_id(c):
    return "n{n}-ms{ms}-mt{mt}-d{d}-q{q}-mask{mask}-b{b:g}-{src}".format(src="invK" if c["use_invK"] else "hyper", **c)


def make_case(c):
    """(ds, sources [ms, d], targets [mt, d]) of a case: batch_oracle.make_case's data and a uniform pool in its box, the sources in
    front; ``shared``: that many leading targets are the leading sources."""
    ds, pool, _ = bo.make_case(dict(n=c["n"], m=c["ms"] + c["mt"], d=c["d"], q=c["q"], seed=c["seed"], n_pending=0, output=0,
                                    **({"log_sn": c["log_sn"]} if "log_sn" in c else {})))
    sources, targets = pool[:c["ms"]].copy(), pool[c["ms"]:].copy()
    if c.get("shared"):
        targets[:c["shared"]] = sources[:c["shared"]]
    return ds, sources, targets


@functools.lru_cache(maxsize=None)
def reference(i):
    """Case i and its reference, computed once per process: (ds, sources, targets, result) -- gain_naive's, or gain_rank1's where the
    case says ``oracle="rank1"`` (tests/test_expander_gain_cpu.py ties that one to the definition on two sources)."""
    c = CASES[i]
    ds, sources, targets = make_case(c)
    gain = {"naive": gain_naive, "rank1": gain_rank1}[c.get("oracle", "naive")]
    return ds, sources, targets, gain(ds, c["b"], sources, targets, c["mask"])
