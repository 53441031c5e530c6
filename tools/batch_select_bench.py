"""Host wall time of ``SweepEngine.batch_select`` (``sbo_batch_select``) against the only route to the same batch without it: per pick
``set_points`` + ``posterior_run`` + ``posterior`` over the pool, the arg-max on the host and ``append_sample`` of the pick with a
made-up y, then ``remove_sample`` k times to get the model back -- k full O(m n^2) posteriors of every output, 2 k model changes, m
values over the bus k times, and the resident candidates replaced.

Benoit data (config B's box), d = 2, q = 2, fp64, log_sn = -1; the pool is uniform in the box.  Per shape: ``--warmup`` rounds, then
``--reps`` rounds that alternate, in the same process and on the same engine, one timed call and one timed loop; both end in their
own synchronisation, so the host clock around them is the time the caller waits.  The two routes must return the same picks (checked
every round).  Medians are reported, with the spread.  One JSON line per shape, with the operation counts behind the derived ratio:
the call does m n^2 / 2 multiply-adds for v_0 plus k m (n + (k - 1) / 2) kernel evaluations, the loop k q m n^2 / 2 multiply-adds
(triangular factor) plus k q m n kernel evaluations.

    python tools/batch_select_bench.py [--shapes 4096x128x8 65536x512x8 65536x512x32 1048576x512x8] [--reps 10] [--out FILE]

``--trace-only MxNxK`` runs ``--reps`` calls at that shape and nothing else: the workload for a kernel trace
(rocprofv3 --kernel-trace --stats), whose summed kernel time per call is the device time of a call.
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

DEFAULT_SHAPES = ["4096x128x8", "65536x512x8", "65536x512x32", "1048576x512x8"]


def dataset(n):
    cfg = synthetic.make_config("B", n=n, seed=5)
    ds = synthetic.make_dataset(cfg["X"], cfg["Y"], synthetic.default_hypopt(2, 2, log_sn=-1.0))
    ds.pop("invKopt")                             # (use_invK=False: built from the hyper-parameters on the device)
    return ds, np.asarray(cfg["bound"], dtype=np.float64)


def loop_route(eng, ds, pool, k, n):
    """The batch without the call (the module docstring's route); returns the picks."""
    picks = []
    for _ in range(k):
        eng.set_points(pool)
        eng.posterior_run()
        _, var = eng.posterior()
        i = int(np.argmax(var[:, 0]))
        picks.append(i)
        eng.append_sample((pool[i] - ds["X_mean"]) / ds["X_std"], np.zeros(2))
    while eng.n > n:
        eng.remove_sample(eng.n - 1)
    return picks


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "calls": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=DEFAULT_SHAPES, metavar="MxNxK")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_select_bench.jsonl"))
    ap.add_argument("--trace-only", default="", metavar="MxNxK")
    args = ap.parse_args()
    with safebo_amd.SweepEngine(0) as eng:
        if args.trace_only:
            m, n, k = (int(x) for x in args.trace_only.split("x"))
            ds, bound = dataset(n)
            pool = np.random.default_rng(7).uniform(bound[:, 0], bound[:, 1], size=(m, 2))
            eng.set_model(ds, use_invK=False)
            for _ in range(args.reps):
                eng.batch_select(pool, k)
            eng.synchronize()
            return
        lines = []
        for shape in args.shapes:
            m, n, k = (int(x) for x in shape.split("x"))
            ds, bound = dataset(n)
            pool = np.random.default_rng(7).uniform(bound[:, 0], bound[:, 1], size=(m, 2))
            eng.set_model(ds, use_invK=False)
            t_call, t_loop, same = [], [], True
            for rep in range(args.reps + args.warmup):          # (the first rounds: warm-up -- code objects, scratch, the grown factor)
                a, got = timed(lambda: eng.batch_select(pool, k))
                b, picks = timed(lambda: loop_route(eng, ds, pool, k, n))
                same = same and got["index"].tolist() == picks
                if rep >= args.warmup:
                    t_call.append(a)
                    t_loop.append(b)
            macs_call, kev_call = m * n * n / 2, k * m * (n + (k - 1) / 2)
            macs_loop, kev_loop = k * 2 * m * n * n / 2, k * 2 * m * n
            rec = {"m": m, "n": n, "k": k, "d": 2, "q": 2, "dtype": "f64", "call": stats(t_call), "loop": stats(t_loop), "same_picks": bool(same),
                   "call_macs": macs_call, "call_kernel_evals": kev_call, "loop_macs": macs_loop, "loop_kernel_evals": kev_loop,
                   "derived_ratio_one_output": k * m * n * n / (m * n * n + k * m * n * (2 + 8))}
            rec["measured_ratio"] = rec["loop"]["median_ms"] / rec["call"]["median_ms"]
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
