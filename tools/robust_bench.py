"""Timing of one robust (StableOpt) sweep on a William-Otto-like joint grid: controls (Fb, Tr) 1024 x 1024, disturbance dFb 64 planes
(67 M candidates), q = 3 outputs of the repository's own plant (sbo_plant_wo at Fb + dFb).  Prints JSON lines: the default path
(K1t) and the forced exact kernel (K1g), each with the posterior time and the time of the reduction + mask + arg-min phase; the
latter also from posterior_ready sweeps (reduction alone), against 2 q 8 bytes per candidate.

    python tools/robust_bench.py [--reps 5] [--n 64]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import safebo_amd  # noqa: E402


def model(eng, n, seed=0):
    rng = np.random.default_rng(seed)
    lo, hi = np.array([4.0, 70.0, -0.2]), np.array([7.0, 100.0, 0.2])
    X = lo + (hi - lo) * rng.uniform(size=(n, 3))
    Y = eng.plant_wo(np.stack([X[:, 0] + X[:, 2], X[:, 1]], axis=1))
    Xm, Xs, Ym, Ys = X.mean(0), X.std(0), Y.mean(0), Y.std(0)
    Xn, Yn = (X - Xm) / Xs, (Y - Ym) / Ys
    hyp = np.zeros((5, 3))
    hyp[:3] = 0.3
    hyp[3] = 0.0
    hyp[4] = -3.0
    inv = []
    for o in range(3):
        ell, sf2, sn2 = np.exp(2 * hyp[:3, o]), np.exp(2 * hyp[3, o]), np.exp(2 * hyp[4, o]) + float(np.finfo(np.float32).eps)
        A = Xn / np.sqrt(ell)
        D = -2 * A @ A.T + (A ** 2).sum(1)[:, None] + (A ** 2).sum(1)[None, :]
        inv.append(np.linalg.inv(sf2 * np.exp(-0.5 * D) + sn2 * np.eye(n)))
    ds = {"X_mean": Xm, "X_std": Xs, "Y_mean": Ym, "Y_std": Ys, "X_norm": Xn, "Y_norm": Yn, "invKopt": inv, "hypopt": hyp}
    return ds, lo, hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=64)
    a = ap.parse_args()
    count = [1024, 1024, 64]
    N = int(np.prod(count))
    with safebo_amd.SweepEngine(0) as eng:
        ds, lo, hi = model(eng, a.n)
        results = {}
        for label, opts in (("default", {}), ("exact_K1g", {"tensor_cheb": 0})):
            for k, v in opts.items():
                eng.set_option(k, v)
            eng.set_model(ds, mean_prior=np.zeros(3))
            eng.set_grid(lo, hi, count)
            rows = []
            for r in range(a.reps + 1):
                res = eng.sweep_robust(2.0, 2, "ucb")
                p = eng.profile()
                if r:
                    rows.append((p["posterior_ms"], p["argreduce_ms"], p["total_ms"], p["posterior_kernel"], p["guard_ms"]))
            red = []
            for r in range(a.reps):
                eng.sweep_robust(2.0, 2, "ucb", posterior_ready=True)
                red.append(eng.profile()["argreduce_ms"])
            med = np.median(np.array(rows, dtype=float), axis=0)
            red_ms = float(np.median(red))
            gbytes = 2 * 3 * 8 * N / 1e9
            out = {"config": label, "candidates": N, "grid": count, "n": a.n, "q": 3, "kernel": int(rows[-1][3]),
                   "posterior_ms": med[0], "reduce_argmin_ms": med[1], "total_ms": med[2], "guard_ms": med[4],
                   "reduce_only_ms_posterior_ready": red_ms, "reduce_bytes_GB": gbytes, "reduce_TBps": gbytes / red_ms,
                   "frac_of_6.3TBps": gbytes / red_ms / 6.3, "index": res["index"], "worst_d_index": res["worst_d_index"],
                   "count_safe": res["count_safe"], "guard_band": res["guard_band"], "guard_passes": res["guard_passes"]}
            results[label] = out
            print(json.dumps(out), flush=True)
            for k in opts:
                eng.set_option(k, 1)
        d, e = results["default"], results["exact_K1g"]
        print(json.dumps({"same_result": (d["index"], d["worst_d_index"], d["count_safe"]) == (e["index"], e["worst_d_index"], e["count_safe"])}))


if __name__ == "__main__":
    main()
