"""Host wall time of ``SweepEngine.model_loo`` (``sbo_model_loo``) against the host route it replaces -- ``np.linalg.inv`` of
K + (sn2 + float32 eps) I per output plus ``np.diag``, the O(n^3) a caller paid for the same numbers -- and against
``remove_sample(0)`` at the same n, which reads and rewrites the triangle the diagnostics only read.

Benoit data (config B's box), q = 2, fp64, log_sn = -1.  Per n: three warm-up rounds, then ``--reps`` rounds that alternate, in the
same process, one timed device call, one timed host route and one timed removal (the model is set back to its n rows after the
removal, outside the timed windows).  The device call ends in its own synchronisation and the removal in the one of its re-pack,
so the host clock around the call is the time the caller waits.  Medians are reported, with the spread.  One JSON line per n,
with the bytes of the triangles the call reads (q n (n + 1) / 2 x 8).

    python tools/model_loo_bench.py [--ns 128 512 2048] [--reps 25]

``--trace-only N`` runs ``--reps`` calls at that n and nothing else: the workload for a kernel trace
(rocprofv3 --kernel-trace --stats) of k_model_loo_colsq / k_model_loo_finish.
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

FLOAT32_EPS = float(np.finfo(np.float32).eps)


def dataset(n):
    cfg = synthetic.make_config("B", n=n, seed=5)
    ds = synthetic.make_dataset(cfg["X"], cfg["Y"], synthetic.default_hypopt(2, 2, log_sn=-1.0))
    ds.pop("invKopt")                             # (use_invK=False: built from the hyper-parameters on the device)
    return ds


def host_route(ds):
    """What a caller did without the call: K per output, its inverse, the diagonal, alpha."""
    Xn, hyp = ds["X_norm"], ds["hypopt"]
    n, d = Xn.shape
    out = []
    for o in range(hyp.shape[1]):
        Xa = Xn * np.exp(2.0 * hyp[:d, o]) ** -0.5
        dist = -2 * np.dot(Xa, Xa.T) + np.sum(Xa ** 2, axis=1)[:, None] + np.sum(Xa ** 2, axis=1)
        P = np.linalg.inv(np.exp(2.0 * hyp[d, o]) * np.exp(-0.5 * dist) + (np.exp(2.0 * hyp[d + 1, o]) + FLOAT32_EPS) * np.eye(n))
        mp = 0.0 if o == 0 else -2.0 * ds["Y_mean"][o] / ds["Y_std"][o]
        alpha = P @ (ds["Y_norm"][:, o] - mp)
        out.append((alpha / np.diag(P), 1.0 / np.diag(P)))
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
            eng.set_model(dataset(args.trace_only), use_invK=False)
            for _ in range(args.reps):
                eng.model_loo(3.0)
            eng.synchronize()
            return
        for n in args.ns:
            ds = dataset(n)
            t_loo, t_host, t_rm = [], [], []
            eng.set_model(ds, use_invK=False)
            for rep in range(args.reps + 3):                   # (the first three rounds: warm-up -- code objects, scratch, the spare factor)
                a = timed(lambda: eng.model_loo(3.0))
                b = timed(lambda: host_route(ds))
                c = timed(lambda: eng.remove_sample(0))
                eng.set_model(ds, use_invK=False)
                if rep >= 3:
                    t_loo.append(a)
                    t_host.append(b)
                    t_rm.append(c)
            rec = {"n": n, "q": 2, "dtype": "f64", "loo": stats(t_loo), "host_inverse": stats(t_host), "remove0": stats(t_rm),
                   "triangle_bytes": 2 * n * (n + 1) // 2 * 8}
            rec["speedup_vs_host"] = rec["host_inverse"]["median_ms"] / rec["loo"]["median_ms"]
            rec["loo_over_remove0"] = rec["loo"]["median_ms"] / rec["remove0"]["median_ms"]
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
