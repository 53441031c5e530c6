"""Host wall time of ``SweepEngine.remove_sample`` (``sbo_model_remove``) against what a caller had to do without it:
``set_model(ds_without_that_row, use_invK=False)``, the O(n^3) rebuild on the device from the remaining rows.

Benoit data (config B's box), q = 2, fp64, at each n and for the removal of index 0, n / 2 and n - 1.  Per (n, index): a warm-up of
both, then ``--reps`` rounds that alternate one timed removal with one timed rebuild in the same process; the model is set back
to its n rows between the calls, outside the timed windows.  Both calls return after their device work (the removal ends in the
synchronisation of the re-pack, the rebuild in the one that fetches the positive-definiteness verdict), so the host clock around
the call is the time the caller waits.  Medians are reported, with the spread.  One JSON line per (n, index).

    python tools/model_remove_bench.py [--ns 128 512 2048] [--reps 25]

``--trace-only N`` runs ``--reps`` removals of index 0 at that n and nothing else: the workload for a kernel trace
(rocprofv3 --kernel-trace --stats) of k_model_remove_coef / k_model_remove and of the kernels that follow them.
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


def dataset(n):
    cfg = synthetic.make_config("B", n=n, seed=5)
    return synthetic.make_dataset(cfg["X"], cfg["Y"], synthetic.default_hypopt(2, 2, log_sn=-1.0))


def without(ds, j):
    out = dict(ds)
    out["X_norm"] = np.ascontiguousarray(np.delete(ds["X_norm"], j, axis=0))
    out["Y_norm"] = np.ascontiguousarray(np.delete(ds["Y_norm"], j, axis=0))
    out.pop("invKopt", None)                      # (use_invK=False: built from the hyper-parameters on the device)
    return out


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "p90_ms": float(a[int(0.9 * (a.size - 1))]), "calls": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, nargs="+", default=[128, 512, 2048])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--trace-only", type=int, default=0, metavar="N")
    args = ap.parse_args()
    if args.reps < 20 and not args.trace_only:
        ap.error("--reps must be at least 20")
    with safebo_amd.SweepEngine(0) as eng:
        if args.trace_only:
            ds = dataset(args.trace_only)
            for _ in range(args.reps):
                eng.set_model(ds, use_invK=False)
                eng.remove_sample(0)
            eng.synchronize()
            return
        for n in args.ns:
            ds = dataset(n)
            for j in (0, n // 2, n - 1):
                ds_wo = without(ds, j)
                t_rm, t_rb = [], []
                for rep in range(args.reps + 3):               # (the first three rounds: warm-up -- code objects, workspaces, the spare factor)
                    eng.set_model(ds, use_invK=False)
                    a = timed(lambda: eng.remove_sample(j))
                    eng.set_model(ds, use_invK=False)
                    b = timed(lambda: eng.set_model(ds_wo, use_invK=False))
                    if rep >= 3:
                        t_rm.append(a)
                        t_rb.append(b)
                rec = {"n": n, "q": 2, "dtype": "f64", "index": j, "remove": stats(t_rm), "rebuild": stats(t_rb)}
                rec["speedup"] = rec["rebuild"]["median_ms"] / rec["remove"]["median_ms"]
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
