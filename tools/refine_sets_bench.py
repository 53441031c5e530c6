"""Timing of ``sbo_refine_sets`` on the device: single mode against pair mode.

The synthetic q = 2 models of tools/refine_bench.py for n in {20, 128, 512}, d = 2, one seed.  Single mode: M_t's problem, max
var_0(x) s.t. lcb_1(x) >= 0 and lcb_0(x) <= level (the seed's lcb_0 plus a tenth of the objective's spread).  Pair mode: G_t's
problem, max var_0(x) s.t. lcb_1(x) >= 0, lcb_1(x') <= 0 and the link with an L that leaves half of ucb_1 at the seed.  One JSON
line per shape and mode: host-clock milliseconds per call (median), the evaluations (one per point: a pair costs two), the
fixed cost of a call (max_eval = 1 or 2) and the solver's cost per evaluated point.

    python tools/refine_sets_bench.py [--ns 20 128 512] [--reps 3] [--max-eval 400]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import safebo_amd  # noqa: E402
from refine_bench import model  # noqa: E402


def timed(fn, reps):
    out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, nargs="+", default=[20, 128, 512])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-eval", type=int, default=400)
    a = ap.parse_args()
    d, b = 2, 2.0
    lo, hi = -np.ones(d), np.ones(d)
    x, xp = np.zeros((1, d)), np.full((1, d), 0.95)
    with safebo_amd.SweepEngine(0) as eng:
        for n in a.ns:
            eng.set_model(model(n, d))
            eng.set_points(np.concatenate([x, xp]))
            lcb0, ucb1 = eng.bounds(b, 0, "lcb"), eng.bounds(b, 1, "ucb")
            lcb1 = eng.bounds(b, 1, "lcb")
            assert lcb1[0] > 0 and lcb1[1] < 0, lcb1
            L = 0.5 * ucb1[0] / float(np.sqrt(np.sum((x - xp + 1e-8) ** 2)))
            modes = {
                "single": lambda me: eng.refine_sets(b, x, objective=0, kind="var", maximize=True, level=(0, lcb0[0] + 0.1), lo=lo, hi=hi,
                                                     max_eval=me),
                "pair": lambda me: eng.refine_sets(b, x, xp, objective=0, kind="var", maximize=True, link=(1, L), lo=lo, hi=hi, max_eval=me),
            }
            for mode, call in modes.items():
                pts = 2 if mode == "pair" else 1
                out, ms = timed(lambda: call(a.max_eval), a.reps)
                _, ms1 = timed(lambda: call(pts), a.reps)
                tri = 2 * n * (n + 1) // 2 * 8 + (pts - 1) * 16 * n
                ev = out["evaluations"]
                print(json.dumps({"n": n, "d": d, "mode": mode, "ms_per_call": round(ms, 4), "evaluations": ev, "status": int(out["status"][0]),
                                  "ms_fixed": round(ms1, 4), "us_per_eval": round(1e3 * (ms - ms1) / (ev - pts), 3) if ev > pts else None,
                                  "tier": "lds" if tri <= 144 * 1024 else "streamed"}), flush=True)


if __name__ == "__main__":
    main()
