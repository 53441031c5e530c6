"""Host wall time of ``SweepEngine.expander_gain`` (``sbo_expander_gain``) against the only route to the same verdicts without it: per
source g ``append_sample`` of the made-up row (g, ucb_c(g)), ``set_points`` + ``posterior_run`` + ``posterior`` over the targets, the
comparison lcb_c >= 0 on the host and ``remove_sample`` -- two model changes and a full O(mt n^2) posterior of every output per source,
every plan dropped each time, and the resident candidates replaced.

Benoit data (config B's box), d = 2, fp64, log_sn = -1; with two constraints the third output is a blend of the constraint and the first
input.  Sources and targets are uniform in the box.  Per shape: ``--warmup`` rounds, then ``--reps`` rounds that alternate, in the same
process and on the same engine, one timed call over all ms sources and one timed loop over the first ``--loop-sources`` of them; both
end in their own synchronisation, so the host clock around them is the time the caller waits.  The loop's counts are compared with the
call's every round (reported, not asserted: nothing makes a random pool sharp).  Medians are reported with the spread, and both routes
per source.  One JSON line per shape, with the operation counts: the call does (ms + mt) n^2 / 2 multiply-adds per constraint in
stage 1 and ms mt n in the pair stage, the loop q mt n^2 / 2 per source.

    python tools/expander_gain_bench.py [--shapes 1024x4096x128x1 4096x16384x512x1 16384x16384x512x2] [--reps 10] [--out FILE]

``--trace-only MSxMTxNxC`` runs ``--reps`` calls at that shape and nothing else: the workload for a kernel trace
(rocprofv3 --kernel-trace --stats, counters never in the same run), whose kernel times per call are the device time per stage; the
pair kernel's 2 ms mt ldt C flops (ldt: n rounded up to 32) over its time is the rate to hold against the 72-75 TFLOP/s of the 4x4x4
form (profiles/r01_mfma_probe.txt).
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
from safebo_amd import synthetic  # noqa: E402

DEFAULT_SHAPES = ["1024x4096x128x1", "4096x16384x512x1", "16384x16384x512x2"]


def dataset(n, constraints):
    cfg = synthetic.make_config("B", n=n, seed=5)
    X, Y = np.asarray(cfg["X"], dtype=np.float64), np.asarray(cfg["Y"], dtype=np.float64)
    if constraints == 2:
        Y = np.column_stack([Y, 0.5 * Y[:, 1] + 0.1 * X[:, 0]])
    elif constraints != 1:
        raise SystemExit("constraints must be 1 or 2")
    ds = synthetic.make_dataset(X, Y, synthetic.default_hypopt(2, 1 + constraints, log_sn=-1.0))
    ds.pop("invKopt")                             # (use_invK=False: built from the hyper-parameters on the device)
    return ds, np.asarray(cfg["bound"], dtype=np.float64), float(cfg["b"])


def loop_route(eng, ds, sources, targets, b, n):
    """The verdicts without the call (the module docstring's route); returns the counts."""
    q = ds["Y_norm"].shape[1]
    eng.set_points(sources)
    eng.posterior_run()
    mean, var = eng.posterior()
    ucb = (mean - ds["Y_mean"]) / ds["Y_std"] + b * np.sqrt(var) / ds["Y_std"]           # normalised, per output
    counts = []
    for g in range(sources.shape[0]):
        eng.append_sample((sources[g] - ds["X_mean"]) / ds["X_std"], np.concatenate([[0.0], ucb[g, 1:]]))
        eng.set_points(targets)
        eng.posterior_run()
        m1, v1 = eng.posterior()
        counts.append(int(np.sum(np.all(m1[:, 1:q] - b * np.sqrt(v1[:, 1:q]) >= 0.0, axis=1))))
        eng.remove_sample(n)
    return counts


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "calls": int(a.size)}


def pools(bound, ms, mt):
    rng = np.random.default_rng(7)
    return rng.uniform(bound[:, 0], bound[:, 1], size=(ms, 2)), rng.uniform(bound[:, 0], bound[:, 1], size=(mt, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=DEFAULT_SHAPES, metavar="MSxMTxNxC")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-sources", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expander_gain_bench.jsonl"))
    ap.add_argument("--trace-only", default="", metavar="MSxMTxNxC")
    args = ap.parse_args()
    with safebo_amd.SweepEngine(0) as eng:
        if args.trace_only:
            ms, mt, n, nc = (int(x) for x in args.trace_only.split("x"))
            ds, bound, b = dataset(n, nc)
            S, T = pools(bound, ms, mt)
            eng.set_model(ds, use_invK=False)
            for _ in range(args.reps):
                eng.expander_gain(S, T, b)
            eng.synchronize()
            return
        lines = []
        for shape in args.shapes:
            ms, mt, n, nc = (int(x) for x in shape.split("x"))
            ds, bound, b = dataset(n, nc)
            S, T = pools(bound, ms, mt)
            k = min(args.loop_sources, ms)
            eng.set_model(ds, use_invK=False)
            t_call, t_loop, same = [], [], True
            for rep in range(args.reps + args.warmup):          # (the first rounds: warm-up -- code objects, scratch, the grown factor)
                a, got = timed(lambda: eng.expander_gain(S, T, b))
                c, counts = timed(lambda: loop_route(eng, ds, S[:k], T, b, n))
                same = same and got["count"][:k].tolist() == counts
                if rep >= args.warmup:
                    t_call.append(a)
                    t_loop.append(c)
            ldt = (n + 31) // 32 * 32
            rec = {"ms": ms, "mt": mt, "n": n, "constraints": nc, "d": 2, "q": 1 + nc, "dtype": "f64", "call": stats(t_call), "loop": stats(t_loop),
                   "loop_sources": k, "same_counts": bool(same), "expanders": int(np.sum(got["count"] > 0)),
                   "stage1_macs": nc * (ms + mt) * n * n / 2, "pair_macs": nc * ms * mt * ldt, "loop_macs_per_source": (1 + nc) * mt * n * n / 2}
            rec["call_us_per_source"] = 1e3 * rec["call"]["median_ms"] / ms
            rec["loop_us_per_source"] = 1e3 * rec["loop"]["median_ms"] / k
            rec["measured_ratio_per_source"] = rec["loop_us_per_source"] / rec["call_us_per_source"]
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
