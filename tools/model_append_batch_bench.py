"""Host wall time of ``SweepEngine.append_samples`` (``sbo_model_append_batch``, one block update for k rows) against the two routes a
caller had without it: the loop of k ``append_sample`` calls, and ``set_model(all_rows, use_invK=False)``, the O(n^3) rebuild on the
device.

Benoit data (config B's box), q = 2, fp64, log_sn = -1, at each (n, k).  Per shape: three warm-up rounds, then ``--reps`` rounds that
alternate one timed block call, one timed loop and one timed rebuild in the same process on one engine; the model is set back to
its n rows between the timed calls, outside the timed windows.  Every route returns after its device work (the appends end in the
synchronisation of the re-pack, the rebuild in the one that fetches the positive-definiteness verdict), so the host clock around
the call is the time the caller waits.  Medians are reported, with min - max.  One JSON line per (n, k).

    python tools/model_append_batch_bench.py [--ns 128 512 1984] [--ks 8 64] [--reps 25]

``--trace-only N`` runs ``--reps`` block calls of ``--ks``' first value at that n and nothing else: the workload for a kernel trace
(rocprofv3 --kernel-trace --stats) of the k_append_* kernels and of those that follow them.
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


def first_rows(ds, n):
    out = dict(ds)
    out["X_norm"] = np.ascontiguousarray(ds["X_norm"][:n])
    out["Y_norm"] = np.ascontiguousarray(ds["Y_norm"][:n])
    out.pop("invKopt", None)                      # (use_invK=False: built from the hyper-parameters on the device)
    return out


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "calls": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, nargs="+", default=[128, 512, 1984])
    ap.add_argument("--ks", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--trace-only", type=int, default=0, metavar="N")
    args = ap.parse_args()
    if args.reps < 20 and not args.trace_only:
        ap.error("--reps must be at least 20")
    with safebo_amd.SweepEngine(0) as eng:
        if args.trace_only:
            n, k = args.trace_only, args.ks[0]
            full = dataset(n + k)
            ds, Xk, Yk = first_rows(full, n), full["X_norm"][n:], full["Y_norm"][n:]
            for _ in range(args.reps):
                eng.set_model(ds, use_invK=False)
                eng.append_samples(Xk, Yk)
            eng.synchronize()
            return
        for n in args.ns:
            for k in args.ks:
                full = dataset(n + k)
                ds, ds_all = first_rows(full, n), first_rows(full, n + k)
                Xk, Yk = np.ascontiguousarray(full["X_norm"][n:]), np.ascontiguousarray(full["Y_norm"][n:])

                def loop():
                    for r in range(k):
                        eng.append_sample(Xk[r], Yk[r])
                t_blk, t_loop, t_rb = [], [], []
                for rep in range(args.reps + 3):               # (the first three rounds: warm-up -- code objects, workspaces, the grown factor)
                    eng.set_model(ds, use_invK=False)
                    a = timed(lambda: eng.append_samples(Xk, Yk))
                    eng.set_model(ds, use_invK=False)
                    b = timed(loop)
                    eng.set_model(ds, use_invK=False)
                    c = timed(lambda: eng.set_model(ds_all, use_invK=False))
                    if rep >= 3:
                        t_blk.append(a)
                        t_loop.append(b)
                        t_rb.append(c)
                rec = {"n": n, "k": k, "q": 2, "dtype": "f64", "block": stats(t_blk), "loop": stats(t_loop), "rebuild": stats(t_rb)}
                rec["loop_over_block"] = rec["loop"]["median_ms"] / rec["block"]["median_ms"]
                rec["rebuild_over_block"] = rec["rebuild"]["median_ms"] / rec["block"]["median_ms"]
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
