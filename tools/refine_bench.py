"""Timing of the off-grid refinement on the device (``sbo_refine``).

Synthetic models with q = 2 outputs (objective, one constraint) for n in {20, 128, 512, 2048}, d in {2, 4} and 1 or 64 seeds:
min lcb_0 subject to lcb_1 >= 0 on the box [-1, 1]^d, seeds spread over the box (infeasible ones are skipped by the kernel).
One JSON line per shape: host-clock milliseconds per call (a call ends in one stream synchronise), after a warm-up call of the
same shape, the evaluations summed over seeds and the tier (LDS or streamed M).  us_per_eval separates the fixed cost of a
call (upload, the two exact list evaluations, the acceptance kernel, the copies and the sync: ``ms_fixed``, a call with
max_eval = 1) from the solver: (ms_per_call - ms_fixed) over the mean evaluations per usable seed less one -- the workgroups run
side by side, so this is one evaluation's latency inside the kernel.

    python tools/refine_bench.py [--ns 20 128 512 2048] [--ds 2 4] [--seeds 1 64] [--reps 3] [--max-eval 400]
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


def model(n, d, seed=1):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, size=(n, d))
    Y = np.stack([np.sum(X ** 2, axis=1) + 0.3 * np.sin(3 * X[:, 0]), 0.8 - np.sum(np.abs(X), axis=1) / d], axis=1)
    return synthetic.make_dataset(X, Y, synthetic.default_hypopt(d, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, nargs="+", default=[20, 128, 512, 2048])
    ap.add_argument("--ds", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-eval", type=int, default=400)
    a = ap.parse_args()
    with safebo_amd.SweepEngine(0) as eng:
        for n in a.ns:
            for d in a.ds:
                eng.set_model(model(n, d))
                lo, hi = -np.ones(d), np.ones(d)
                tri = 2 * n * (n + 1) // 2 * 8
                for S in a.seeds:
                    seeds = np.random.default_rng(S).uniform(-0.6, 0.6, size=(S, d))
                    seeds[0] = 0.0
                    out = eng.refine(2.0, seeds, lo=lo, hi=hi, max_eval=a.max_eval)        # warm-up (and the work done)
                    ts = []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        eng.refine(2.0, seeds, lo=lo, hi=hi, max_eval=a.max_eval)
                        ts.append((time.perf_counter() - t0) * 1e3)
                    t1 = []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        eng.refine(2.0, seeds, lo=lo, hi=hi, max_eval=1)
                        t1.append((time.perf_counter() - t0) * 1e3)
                    usable = int(np.sum(out["status"] != 3))
                    ms = float(np.median(ts))
                    ms1 = float(np.median(t1))
                    evs = out["evaluations"] / max(usable, 1)
                    print(json.dumps({"n": n, "d": d, "q": 2, "seeds": S, "usable": usable, "ms_per_call": round(ms, 4),
                                      "evaluations": out["evaluations"], "converged": out["converged"],
                                      "ms_fixed": round(ms1, 4),
                                      "us_per_eval": round(1e3 * (ms - ms1) / evs, 3) if evs > 1 else None,
                                      "tier": "lds" if tri <= 144 * 1024 else "streamed"}), flush=True)


if __name__ == "__main__":
    main()
