"""Host wall time of ``SweepEngine.sample_paths`` (``sbo_sample_paths``): S posterior sample paths over a list of m points, per-path
arg-min, no value table.  Beside every shape the exact marginal posterior of the same list (``set_points`` + ``posterior_run``: the price
one path is quoted against), and beside the first shape the NumPy statement of the same paths on the host (tests/paths_oracle.py's
formulas, restated here: the only route a user has without the call).

Benoit data (config B's box), d = 2, fp64, log_sn = -1, the objective; points uniform in the box; the draws of
``SweepEngine.path_draws`` (seed 7).  Per shape: ``--warmup`` rounds, then ``--reps`` timed rounds of one call and of one posterior
run, in the same process and on the same engine; both end in their own synchronisation, so the host clock around them is the time
the caller waits (the call's includes the upload of the points and of the draws).  Medians with the spread; one JSON line per shape
with the main kernel's operation count 2 m (F + n) Spad (Spad: S rounded up to 16 | 32 | 64; the K axis is padded to slabs of 32 on
both parts, which the count leaves out).

    python tools/sample_paths_bench.py [--shapes 65536x128x256x1 1048576x512x1024x16 1048576x512x1024x64 16777216x512x1024x64]
                                       [--reps 10] [--out FILE]

``--trace-only MxNxFxS`` runs ``--reps`` calls at that shape and nothing else: the workload for a kernel trace (rocprofv3
--kernel-trace --stats, counters never in the same run), whose kernel times per call are the device time per stage; k_path_main's
flops over its time is the rate to hold against the 72-75 TFLOP/s of the 4x4x4 form (profiles/r01_mfma_probe.txt).  Two shapes
that differ in S alone (16 | 64: the same generated operand, four times the matrix-core work) give the split of a slab's time
between generating the operand and the matrix cores.
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

DEFAULT_SHAPES = ["65536x128x256x1", "1048576x512x1024x16", "1048576x512x1024x64", "16777216x512x1024x64"]
FLOAT32_EPS = float(np.finfo(np.float32).eps)


def dataset(n):
    cfg = synthetic.make_config("B", n=n, seed=5)
    ds = synthetic.make_dataset(cfg["X"], cfg["Y"], synthetic.default_hypopt(2, 2, log_sn=-1.0))
    ds.pop("invKopt")                             # (use_invK=False: built from the hyper-parameters on the device)
    return ds, np.asarray(cfg["bound"], dtype=np.float64)


def numpy_route(ds, draws, pts, chunk=8192):
    """The same paths on the host (output 0, whose prior mean is 0): the arg-min of every path, the points in chunks."""
    omega, phase, weights, noise = draws
    d = pts.shape[1]
    h = ds["hypopt"][:, 0]
    ell, sf2, sn2 = np.exp(2.0 * h[:d]), float(np.exp(2.0 * h[d])), float(np.exp(2.0 * h[d + 1]) + FLOAT32_EPS)
    Xn = np.asarray(ds["X_norm"], dtype=np.float64)
    A, scale = Xn / np.sqrt(ell), np.sqrt(2.0 * sf2 / omega.shape[0])
    sq = np.sum(A * A, axis=1)
    K = sf2 * np.exp(-0.5 * (-2.0 * A @ A.T + sq[:, None] + sq[None, :]))
    R = ds["Y_norm"][:, :1] - scale * np.cos(A @ omega.T + phase) @ weights.T - np.sqrt(sn2) * noise.T
    Cs = np.linalg.solve(K + sn2 * np.eye(len(Xn)), R)
    best, index = np.full(weights.shape[0], np.inf), np.full(weights.shape[0], -1, dtype=np.int64)
    for lo in range(0, len(pts), chunk):
        U = ((pts[lo:lo + chunk] - ds["X_mean"]) / ds["X_std"]) / np.sqrt(ell)
        k = sf2 * np.exp(-0.5 * (-2.0 * U @ A.T + np.sum(U * U, axis=1)[:, None] + sq[None, :]))
        f = scale * np.cos(U @ omega.T + phase) @ weights.T + k @ Cs
        i = np.argmin(f, axis=0)
        v = f[i, np.arange(f.shape[1])]
        better = v < best
        best, index = np.where(better, v, best), np.where(better, i + lo, index)
    return index


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "calls": int(a.size)}


def posterior_route(eng, pts):
    eng.set_points(pts)
    eng.posterior_run()
    eng.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=DEFAULT_SHAPES, metavar="MxNxFxS")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_paths_bench.jsonl"))
    ap.add_argument("--trace-only", default="", metavar="MxNxFxS")
    args = ap.parse_args()
    rng = np.random.default_rng(7)
    with safebo_amd.SweepEngine(0) as eng:
        lines = []
        for k, shape in enumerate([args.trace_only] if args.trace_only else args.shapes):
            m, n, F, S = (int(x) for x in shape.split("x"))
            ds, bound = dataset(n)
            pts = rng.uniform(bound[:, 0], bound[:, 1], size=(m, 2))
            draws = tuple(np.ascontiguousarray(a) for a in SweepEngine.path_draws(2, n, S, F, 7))
            eng.set_model(ds, use_invK=False)
            if args.trace_only:
                for _ in range(args.reps):
                    eng.sample_paths(pts, S, 0, draws=draws)
                eng.synchronize()
                return
            t_call, t_post = [], []
            for rep in range(args.reps + args.warmup):          # (the first rounds: warm-up -- code objects, scratch)
                a, got = timed(lambda: eng.sample_paths(pts, S, 0, draws=draws))
                c, _ = timed(lambda: posterior_route(eng, pts))
                if rep >= args.warmup:
                    t_call.append(a)
                    t_post.append(c)
            spad = 16 if S <= 16 else 32 if S <= 32 else 64
            rec = {"m": m, "n": n, "F": F, "S": S, "d": 2, "dtype": "f64", "call": stats(t_call), "posterior": stats(t_post),
                   "main_flops": 2.0 * m * (F + n) * spad, "distinct_proposals": int(np.unique(got["index"]).size)}
            rec["call_ns_per_point_and_path"] = 1e6 * rec["call"]["median_ms"] / (m * S)
            rec["call_over_posterior"] = rec["call"]["median_ms"] / rec["posterior"]["median_ms"]
            if k == 0 and not args.trace_only:
                t_np = []
                for _ in range(3):
                    t, idx = timed(lambda: numpy_route(ds, draws, pts))
                    t_np.append(t)
                rec["numpy"] = stats(t_np)
                rec["numpy_same_index"] = bool(np.array_equal(idx, got["index"]))
                rec["numpy_over_call"] = rec["numpy"]["median_ms"] / rec["call"]["median_ms"]
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
