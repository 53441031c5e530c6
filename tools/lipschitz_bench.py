"""Host wall time of ``SweepEngine.lipschitz`` (``sbo_lipschitz``, default seeds and options) and of ``SweepEngine.mean_grad``
(``sbo_mean_grad``) at 10^5 points, for n in {20, 128, 512, 2048} x d in {2, 4}: medians of ``--reps`` calls after one untimed call.

d = 2: Benoit data on config B's box; d = 4: the 4-D Rosenbrock data on config D's box; q = 2, fp64, log_sn = -1, the model built
on the device from the hyper-parameters.  Both calls end in their own synchronisation, so the host clock around a call is the time
the caller waits.  Beside them, per shape: the evaluations, problems and converged count of the call, L_seed -> L per output, the
same call with the solver's streamed tier (option ``lipschitz_lds`` = 0), and -- labelled as a host figure, NumPy / SciPy on the
host's CPU -- the wall time, evaluations and L of the twin ``tests/lipschitz_oracle.box_L`` from the same seeds (its inverse of
K + sn2 I, which the device call never forms, is built outside the timed window).  One JSON line per shape.

    python tools/lipschitz_bench.py [--ns 20 128 512 2048] [--ds 2 4] [--reps 5] [--out profiles/lipschitz_bench.jsonl]
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
from safebo_amd import synthetic  # noqa: E402
import lipschitz_oracle  # noqa: E402


def dataset(n, d):
    cfg = synthetic.make_config("B" if d == 2 else "D", n=n, seed=5)
    return synthetic.make_dataset(cfg["X"], cfg["Y"], synthetic.default_hypopt(d, 2, log_sn=-1.0)), cfg["bound"]


def median_ms(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, nargs="+", default=[20, 128, 512, 2048])
    ap.add_argument("--ds", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lipschitz_bench.jsonl"))
    args = ap.parse_args()
    eng = safebo_amd.SweepEngine(0)
    rows = []
    for d in args.ds:
        for n in args.ns:
            ds, bound = dataset(n, d)
            lo, hi = bound[:, 0].copy(), bound[:, 1].copy()
            eng.set_model(ds, use_invK=False)
            pts = np.random.default_rng(n + d).uniform(lo, hi, size=(100_000, d))
            row = {"n": n, "d": d, "q": 2, "reps": args.reps, "seeds": int(eng.lipschitz_seeds(lo, hi).shape[0])}
            row["lipschitz_ms"], row["lipschitz_ms_min"], row["lipschitz_ms_max"] = median_ms(lambda: eng.lipschitz(lo, hi), args.reps)
            out = eng.lipschitz(lo, hi)
            eng.set_option("lipschitz_lds", 0)
            try:
                row["lipschitz_streamed_ms"] = median_ms(lambda: eng.lipschitz(lo, hi), args.reps)[0]
            finally:
                eng.set_option("lipschitz_lds", 1)
            row["mean_grad_1e5_ms"], row["mean_grad_1e5_ms_min"], row["mean_grad_1e5_ms_max"] = median_ms(lambda: eng.mean_grad(pts), args.reps)
            row.update(evaluations=out["evaluations"], problems=out["problems"], converged=out["converged"],
                       L_seed=out["L_seed"].tolist(), L=out["L"].tolist())
            t0 = time.perf_counter()
            twin = lipschitz_oracle.box_L(ds, lo, hi, top=4)
            row.update(host_twin_ms=1e3 * (time.perf_counter() - t0), host_twin_evaluations=twin["evaluations"],
                       host_twin_L=twin["L"].tolist())
            rows.append(row)
            print(json.dumps(row), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
