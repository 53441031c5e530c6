"""Timing of GP_Classic's multistart fit on the device (``sbo_fit_local``) against SciPy SLSQP on the host from the same starts.

For q = 2 outputs (William-Otto objective and first constraint, ``sbo_plant_wo``) and P = 10 starts at each n: the whole fit
launch, one ``sbo_nll_grad_batch`` evaluation of P members, and the host SLSQP fit of tests/nll_grad_oracle.py.  Device times
are host clocks around calls that end in a stream synchronise, after a warm-up call of the same shape.  One JSON line per n,
with the flops of one NLL + gradient evaluation from the shapes (factor n^3 / 3, inverse n^3 / 3, K^-1 contraction n^3 / 3
multiply-adds as 2 flops each, and (d + 2) n^2 for the gradient terms).  With P q = 20 workgroups on 256 CUs, one evaluation is
one CU's latency-bound factorisation: no share of the chip's peak is claimed.

    python tools/fit_bench.py [--ns 14 45 128 512] [--reps 3] [--no-host]
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
from nll_grad_oracle import classic_bounds, classic_starts, slsqp_fit  # noqa: E402


def data(eng, n, seed=3):
    rng = np.random.default_rng(seed)
    U = np.column_stack([rng.uniform(4.0, 7.0, n), rng.uniform(70.0, 100.0, n)])
    Y = eng.plant_wo(U)[:, :2]
    return (U - U.mean(0)) / U.std(0), (Y - Y.mean(0)) / Y.std(0)


def flops_per_eval(n, d):
    return 2.0 * n ** 3 + (d + 2) * n ** 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, nargs="+", default=[14, 45, 128, 512])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the SciPy SLSQP column")
    args = ap.parse_args()
    d, P = 2, 10
    B = classic_bounds(d)
    starts = classic_starts(d, P)
    with safebo_amd.SweepEngine(0) as eng:
        for n in args.ns:
            Xn, Yn = data(eng, n)
            eng.fit_local(Xn, Yn, B, starts)                       # warm-up (code objects, workspace)
            eng.nll_grad_batch(Xn, Yn[:, 0], starts)
            fit_ms, eval_ms = [], []
            for _ in range(args.reps):
                t = time.perf_counter()
                res = eng.fit_local(Xn, Yn, B, starts)
                fit_ms.append(1e3 * (time.perf_counter() - t))
                t = time.perf_counter()
                eng.nll_grad_batch(Xn, Yn[:, 0], starts)
                eval_ms.append(1e3 * (time.perf_counter() - t))
            rec = {"n": n, "d": d, "q": 2, "P": P, "fit_local_ms": min(fit_ms), "fit_local_ms_all": fit_ms,
                   "nll_grad_batch_ms": min(eval_ms), "evals_max": int(res["evals"].max()), "evals_sum": int(res["evals"].sum()),
                   "iters_max": int(res["iters"].max()), "status": res["status"].tolist(), "best_nll": res["best_nll"].tolist(),
                   "flops_per_eval": flops_per_eval(n, d)}
            if not args.no_host:
                t = time.perf_counter()
                host = [slsqp_fit(Xn, Yn[:, o], starts, B)[1] for o in range(2)]
                rec["host_slsqp_ms"] = 1e3 * (time.perf_counter() - t)
                rec["host_best_nll"] = host
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
