"""Host wall time of ``SweepEngine.posterior_joint`` (``sbo_posterior_joint``): mean, full covariance and S exact joint draws of a list
of m points, per-draw arg-min.  Every shape runs twice -- lean (nothing but the mean and the result block comes back) and with ``cov``
and ``draws`` read back --, and beside it run the NumPy statement of the same call on the host from ``invKopt`` (the only route a user
had: K(P, P) - k(P, X) inv(K) k(X, P), its Cholesky factor, the draws; the inverse itself is taken as given and not timed) and
``SweepEngine.sample_paths`` on the same pool with F = 1024 features and the same number of paths (approximate draws, no covariance).

Benoit data (config B's box), d = 2, fp64, log_sn = -1, the objective, noise = 0, jitter = 1e-6; points uniform in the box; the draws
of ``SweepEngine.joint_draws`` (seed 7).  Per shape: ``--warmup`` rounds, then ``--reps`` timed rounds of each route in the same process
and on the same engine; the library's calls end in their own synchronisation, so the host clock around them is the time the caller
waits (uploads and read-backs included).  Medians with the spread; one JSON line per shape with the operation counts m^2 n
(covariance, the lower triangle), m^3 / 3 (factorisation) and m^2 Spad (draws, the lower triangle).

    python tools/posterior_joint_bench.py [--shapes 512x512x16 2048x512x64 2048x2048x64] [--reps 10] [--out FILE]

``--trace-only MxNxS`` runs ``--reps`` lean calls at that shape and nothing else: the workload for a kernel trace (rocprofv3
--kernel-trace --stats, counters never in the same run), whose kernel times per call are the device time per stage.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import safebo_amd  # noqa: E402
from safebo_amd import SweepEngine, synthetic  # noqa: E402

DEFAULT_SHAPES = ["512x512x16", "2048x512x64", "2048x2048x64"]
FLOAT32_EPS = float(np.finfo(np.float32).eps)
JITTER = 1e-6


def dataset(n):
    cfg = synthetic.make_config("B", n=n, seed=5)
    ds = synthetic.make_dataset(cfg["X"], cfg["Y"], synthetic.default_hypopt(2, 2, log_sn=-1.0))
    return ds, np.asarray(cfg["bound"], dtype=np.float64)


def numpy_route(ds, invK, pts, z):
    """The same call on the host (output 0, whose prior mean is 0), from the caller's inverse: (index [S], cov [m, m])."""
    d = pts.shape[1]
    h = ds["hypopt"][:, 0]
    ell, sf2 = np.exp(2.0 * h[:d]), float(np.exp(2.0 * h[d]))
    A = np.asarray(ds["X_norm"], dtype=np.float64) / np.sqrt(ell)
    U = ((pts - ds["X_mean"]) / ds["X_std"]) / np.sqrt(ell)
    sa, su = np.sum(A * A, axis=1), np.sum(U * U, axis=1)
    kx = sf2 * np.exp(-0.5 * (-2.0 * A @ U.T + sa[:, None] + su[None, :]))
    Kpp = sf2 * np.exp(-0.5 * (-2.0 * U @ U.T + su[:, None] + su[None, :]))
    Ak = invK @ kx
    mu = Ak.T @ ds["Y_norm"][:, 0]
    Cm = Kpp - kx.T @ Ak
    Cm = 0.5 * (Cm + Cm.T)
    L = np.linalg.cholesky(Cm + JITTER * sf2 * np.eye(len(pts)))
    f = mu[:, None] + L @ z.T
    ys = float(ds["Y_std"][0])
    return np.argmin(f, axis=0), ys * ys * Cm


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "calls": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=DEFAULT_SHAPES, metavar="MxNxS")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_joint_bench.jsonl"))
    ap.add_argument("--trace-only", default="", metavar="MxNxS")
    args = ap.parse_args()
    rng = np.random.default_rng(7)
    with safebo_amd.SweepEngine(0) as eng:
        lines = []
        for shape in [args.trace_only] if args.trace_only else args.shapes:
            m, n, S = (int(x) for x in shape.split("x"))
            ds, bound = dataset(n)
            invK = np.asarray(ds["invKopt"][0], dtype=np.float64)
            pts = rng.uniform(bound[:, 0], bound[:, 1], size=(m, 2))
            z = np.ascontiguousarray(SweepEngine.joint_draws(m, S, 7))
            path_draws = tuple(np.ascontiguousarray(a) for a in SweepEngine.path_draws(2, n, S, 1024, 7))
            eng.set_model(ds, use_invK=True)
            lean = lambda: eng.posterior_joint(pts, 0, z=z, jitter=JITTER, return_cov=False)
            full = lambda: eng.posterior_joint(pts, 0, z=z, jitter=JITTER, return_cov=True, return_draws=True)
            if args.trace_only:
                for _ in range(args.reps):
                    lean()
                eng.synchronize()
                return
            t_lean, t_full, t_np, t_paths = [], [], [], []
            for rep in range(args.reps + args.warmup):          # (the first rounds: warm-up -- code objects, scratch)
                a, got = timed(lean)
                b, got_full = timed(full)
                c, ref = timed(lambda: numpy_route(ds, invK, pts, z))
                e, _ = timed(lambda: eng.sample_paths(pts, S, 0, draws=path_draws))
                if rep >= args.warmup:
                    t_lean.append(a)
                    t_full.append(b)
                    t_np.append(c)
                    t_paths.append(e)
            spad = 16 if S <= 16 else 32 if S <= 32 else 64
            rec = {"m": m, "n": n, "S": S, "d": 2, "dtype": "f64", "jitter": JITTER, "lean": stats(t_lean), "with_cov_and_draws": stats(t_full),
                   "numpy": stats(t_np), "sample_paths_F1024": stats(t_paths),
                   "cov_flops": float(m) * m * n, "chol_flops": float(m) ** 3 / 3.0, "draw_flops": float(m) * m * spad,
                   "pivot_min": got["pivot_min"], "pivot_row": got["pivot_row"],
                   "numpy_same_index": bool(np.array_equal(ref[0], got["index"])),
                   "numpy_cov_max_abs_diff": float(np.max(np.abs(ref[1] - got_full["cov"]))),
                   "lean_equals_full": bool(got["index"].tobytes() == got_full["index"].tobytes() and got["value"].tobytes() == got_full["value"].tobytes())}
            rec["numpy_over_lean"] = rec["numpy"]["median_ms"] / rec["lean"]["median_ms"]
            rec["numpy_over_full"] = rec["numpy"]["median_ms"] / rec["with_cov_and_draws"]["median_ms"]
            rec["lean_over_sample_paths"] = rec["lean"]["median_ms"] / rec["sample_paths_F1024"]["median_ms"]
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
