"""Host wall time of ``SweepEngine.refine_paths`` (``sbo_refine_paths``): S sample paths of the objective, K starts
each, refined off the grid under the constraint lcb_1 >= 0.  Beside every shape ``SweepEngine.refine`` of kind "mean" on the same
seeds and constraint (the same solver without the path term: what the path term and the shared preparation add), and beside the first
shape SciPy's SLSQP on the NumPy oracle (tests/refine_paths_oracle.py) from the same seeds -- the only route a user had.

Benoit data (config B's box and b), d = 2, fp64, log_sn = -1; the draws of ``SweepEngine.path_draws`` (seed 5).  The seeds are what
``SafeOpt.BO.ThompsonRefined`` hands over: path s starts from its own arg-min over the safe members of the 50 x 50 grid and, with
K > 1, from those of paths s+1 .. s+K-1 (mod S).  Per shape ``--warmup`` rounds, then ``--reps`` timed rounds of either call in the same
process on the same engine; both calls end in their own wait, so the host clock around them is the time the caller waits.  Medians with
min - max; one JSON line per shape.  Nothing is asserted.

    python tools/refine_paths_bench.py [--shapes 128x1024x16x1 512x1024x64x1 512x1024x64x8 2048x1024x16x1] [--reps 10] [--out FILE]

``--trace-only NxFxSxK`` runs ``--reps`` calls at that shape and nothing else: the workload of a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/refine_paths_bench.py --trace-only ...; counters never in the same run).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import safebo_amd  # noqa: E402
from safebo_amd import SweepEngine, synthetic  # noqa: E402

DEFAULT_SHAPES = ["128x1024x16x1", "512x1024x64x1", "512x1024x64x8", "2048x1024x16x1"]
SEED = 5


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "calls": int(a.size)}


def thompson_seeds(eng, b, lo, hi, draws, S, K):
    """[S, K, d]: every path's arg-min over the safe members of the 50 x 50 grid, and its K - 1 neighbours'."""
    eng.set_grid(lo, hi, [50, 50])
    eng.sweep_safeopt(b, want_masks=True)
    ax = [np.linspace(lo[a], hi[a], 50) for a in range(2)]
    pts = np.stack([np.tile(ax[0], 50), np.repeat(ax[1], 50)], axis=1)          # (axis 0 fastest, the sweep's flat order)
    pool = pts[np.nonzero(eng.mask("S"))[0]]
    x = eng.sample_paths(pool, S, 0, draws=draws)["x"]
    return np.ascontiguousarray(x[(np.arange(S)[:, None] + np.arange(K)[None, :]) % S]), len(pool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=DEFAULT_SHAPES, metavar="NxFxSxK")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_paths_bench.jsonl"))
    ap.add_argument("--trace-only", default="", metavar="NxFxSxK")
    args = ap.parse_args()
    with safebo_amd.SweepEngine(0) as eng:
        lines = []
        for k, shape in enumerate([args.trace_only] if args.trace_only else args.shapes):
            n, F, S, K = (int(x) for x in shape.split("x"))
            cfg = synthetic.make_config("B", n=n, seed=5)
            ds = synthetic.make_dataset(cfg["X"], cfg["Y"], synthetic.default_hypopt(2, 2, log_sn=-1.0))
            b, bound = float(cfg["b"]), np.asarray(cfg["bound"], dtype=np.float64)
            lo, hi = bound[:, 0].copy(), bound[:, 1].copy()
            eng.set_model(ds)
            draws = tuple(np.ascontiguousarray(a) for a in SweepEngine.path_draws(2, n, S, F, SEED))
            seeds, members = thompson_seeds(eng, b, lo, hi, draws, S, K)
            call = lambda: eng.refine_paths(b, seeds, 0, draws=draws, lo=lo, hi=hi)
            if args.trace_only:
                for _ in range(args.reps):
                    call()
                return
            mean = lambda: eng.refine(b, seeds.reshape(-1, 2), 0, "mean", lo=lo, hi=hi)
            t_call, t_mean = [], []
            for rep in range(args.reps + args.warmup):          # (the first rounds: warm-up -- code objects, scratch)
                a, got = timed(call)
                c, ref = timed(mean)
                if rep >= args.warmup:
                    t_call.append(a)
                    t_mean.append(c)
            ys = float(ds["Y_std"][0])
            at_seed = eng.sample_paths(seeds.reshape(-1, 2), S, 0, draws=draws, return_values=True)["values"]
            at_seed = at_seed.reshape(S, K, S)[np.arange(S), :, np.arange(S)]
            rec = {"n": n, "F": F, "S": S, "K": K, "d": 2, "dtype": "f64", "safe_grid_members": members, "call": stats(t_call),
                   "refine_mean": stats(t_mean), "evaluations": got["evaluations"], "converged": got["converged"],
                   "refine_mean_evaluations": ref["evaluations"], "refine_mean_converged": ref["converged"],
                   "gain_normalised_median": float(np.median((at_seed[:, 0] - got["best_value"]) / ys)),
                   "gain_normalised_min": float(np.min((at_seed[:, 0] - got["best_value"]) / ys))}
            rec["call_over_refine_mean"] = rec["call"]["median_ms"] / rec["refine_mean"]["median_ms"]
            rec["call_us_per_evaluation"] = 1e3 * rec["call"]["median_ms"] / max(1, got["evaluations"])
            if k == 0:
                import refine_paths_oracle as rp
                co = rp.coeffs(ds, 0, draws)
                probs = [rp.problem(ds, b, lo, hi, co, s, False, [1]) for s in range(S)]
                t_sl, worse = [], 0
                for _ in range(3):
                    t, zs = timed(lambda: [rp.slsqp(probs[s], seeds[s, j]) for s in range(S) for j in range(K)])
                    t_sl.append(t)
                vals = np.array([rp.value(probs[i // K], z) for i, z in enumerate(zs)]).reshape(S, K)
                worse = int(np.sum(got["value"] > vals + 1e-6 * ys))
                rec["slsqp"] = stats(t_sl)
                rec["slsqp_over_call"] = rec["slsqp"]["median_ms"] / rec["call"]["median_ms"]
                rec["problems_where_slsqp_is_better_by_1e-6"] = worse
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
