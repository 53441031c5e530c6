"""Host wall time of a whole model refit -- ``GP_initialization`` -- in mode ``fit_on_device = "model"`` (``sbo_model_fit``: DE of
all outputs side by side, polish and model build on the device) against mode ``"de"`` (``sbo_fit_de`` per output, SciPy L-BFGS-B
and ``np.linalg.inv`` on the host, upload of invK at the next sweep), in the same process on the same data.

William-Otto-like data as tools/fit_bench.py (``sbo_plant_wo``), d = 2, q = 2 and 3, at each n.  Per mode: one warm-up refit and
first sweep, then ``--reps`` timed repetitions of (refit, first SafeOpt sweep on a 256 x 256 grid); the best refit is reported with
the first sweep that followed it (which in mode "de" carries the model upload) and that sweep's ``posterior_kernel``.  Mode
"model" adds the phase split of ``sbo_fit_report``.  Times are host clocks around calls that return after their device work.
One JSON line per (q, n).

    python tools/model_fit_bench.py [--ns 14 45 128 512] [--qs 2 3] [--reps 3] [--maxiter 1000]
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
from safebo_amd import SafeOpt  # noqa: E402

BOUND = np.array([[4.0, 7.0], [70.0, 100.0]])
GRID = (256, 256)


def data(eng, n, q, seed=3):
    rng = np.random.default_rng(seed)
    U = np.column_stack([rng.uniform(4.0, 7.0, n), rng.uniform(70.0, 100.0, n)])
    return U, eng.plant_wo(U)[:, :q]


def one_mode(eng, mode, U, Y, de_options, reps):
    m = SafeOpt.BO([None] * Y.shape[1], BOUND, 2.0, grid=GRID)
    m._engine = eng
    m.fit_on_device, m.de_options = mode, dict(de_options)
    best, all_ms = None, []
    for rep in range(reps + 1):                                 # (rep 0: warm-up -- code objects, workspaces)
        t0 = time.perf_counter()
        m.GP_initialization(U, Y, "RBF", multi_hyper=1)
        t1 = time.perf_counter()
        try:
            m.sweep()
            empty = False
        except safebo_amd.EmptySafeSetError:
            empty = True
        t2 = time.perf_counter()
        rec = {"fit_ms": 1e3 * (t1 - t0), "first_sweep_ms": 1e3 * (t2 - t1), "empty_safe_set": empty,
               "posterior_kernel": eng.profile()["posterior_kernel"]}
        if mode == "model":
            rec.update({k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in m.fit_report.items() if k != "hypopt"})
        nll = [m.negative_loglikelihood(m.hypopt[:, i], m.X_norm, m.Y_norm[:, i:i + 1]) for i in range(m.ny_dim)]
        rec["host_nll"] = nll
        if rep:
            all_ms.append(rec["fit_ms"])
            if best is None or rec["fit_ms"] < best["fit_ms"]:
                best = rec
    best["fit_ms_all"] = all_ms
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, nargs="+", default=[14, 45, 128, 512])
    ap.add_argument("--qs", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--maxiter", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    de_options = {"seed": args.seed, "maxiter": args.maxiter}
    with safebo_amd.SweepEngine(0) as eng:
        for q in args.qs:
            for n in args.ns:
                U, Y = data(eng, n, q)
                rec = {"n": n, "d": 2, "q": q, "P": 60, "maxiter": args.maxiter}
                for mode in ("de", "model"):
                    rec[mode] = one_mode(eng, mode, U, Y, de_options, args.reps)
                rec["speedup_fit"] = rec["de"]["fit_ms"] / rec["model"]["fit_ms"]
                rec["speedup_fit_and_sweep"] = ((rec["de"]["fit_ms"] + rec["de"]["first_sweep_ms"])
                                                / (rec["model"]["fit_ms"] + rec["model"]["first_sweep_ms"]))
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
