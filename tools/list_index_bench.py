"""Timing of constrained SafeOpt sweeps on scattered candidate lists: the exhaustive expander evaluation (option list_index = 0)
against the spatial index of the list (list_index = 1).  The problem: points ~ U(-1, 1)^d, a smooth objective and one constraint
0.8 - 3 ||x||^2 / d >= 0, n observations, fp64.  Prints one JSON line per (size, path): sweep wall time (the index's build runs
inside the first sweep of a list and is reported apart), expander time from phase events, |S|, |U|, |G| and the leaf pairs and
skipped nodes per safe candidate.  --check compares the masks and indices of the two paths where both run.

    python tools/list_index_bench.py --d 6 --sizes 2097152 --paths exhaustive,index --reps 3
    python tools/list_index_bench.py --d 6 --sizes 10000000 --paths index
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import safebo_amd  # noqa: E402
from safebo_amd import synthetic  # noqa: E402


def problem(d, n, seed=0, log_ell=0.3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, size=(n, d))
    f = np.sin(2.0 * X).sum(1) + 0.3 * X[:, 0]
    g = 0.8 - 3.0 * (X ** 2).sum(1) / d
    hyp = synthetic.default_hypopt(d, 2, log_ell=log_ell, log_sn=-3.0)
    return synthetic.make_dataset(X, np.stack([f, g], axis=1), hyp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=6)
    ap.add_argument("--n", type=int, default=256, help="observations")
    ap.add_argument("--sizes", default="2097152")
    ap.add_argument("--paths", default="exhaustive,index")
    ap.add_argument("--b", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    ds = problem(a.d, a.n)
    with safebo_amd.SweepEngine(0) as eng:
        eng.set_model(ds, dtype="f64")
        eng.set_option("phase_events", 1)
        for N in (int(s) for s in a.sizes.split(",")):
            pts = np.random.default_rng(1).uniform(-1.0, 1.0, size=(N, a.d))
            eng.set_points(pts)
            ref = None
            for path in a.paths.split(","):
                eng.set_option("list_index", {"exhaustive": 0, "index": 1, "auto": -1}[path])
                times, prof, res = [], None, None
                build_ms = 0.0
                for r in range(a.reps):
                    t0 = time.perf_counter()
                    res = eng.sweep_safeopt(a.b, want_masks=a.check and r == a.reps - 1, posterior_ready=r > 0)
                    times.append(time.perf_counter() - t0)
                    prof = eng.profile()
                    build_ms = max(build_ms, prof["list_index_build_ms"])
                nS = max(res["count_S"], 1)
                line = {"d": a.d, "N": N, "n": a.n, "path": path, "sweep_ms_first": 1e3 * times[0],
                        "sweep_ms_best_reused_posterior": 1e3 * min(times[1:]) if len(times) > 1 else None,
                        "expander_ms": prof["expander_ms"], "index_build_ms": build_ms,
                        "count_S": res["count_S"], "count_U": res["count_U"], "count_G": int(res["count_G"][0]),
                        "L": float(res["L"][1]), "n_exact_rechecks": res["n_exact_rechecks"],
                        "leaf_pairs_per_safe": prof["list_index_leaf_pairs"] / nS,
                        "nodes_skipped_per_safe": prof["list_index_nodes_skipped"] / nS}
                if a.check:
                    cur = {k: eng.mask(k) for k in ("S", "U", "M")}
                    cur["G"] = eng.mask("G", 1)
                    cur["idx"] = (res["minimizer_index"], res["expander_index"], res["count_S"], res["count_U"], res["count_M"],
                                  int(res["count_G"][0]))
                    if ref is None:
                        ref = cur
                    else:
                        line["identical"] = all(np.array_equal(cur[k], ref[k]) for k in ("S", "U", "M", "G")) and cur["idx"] == ref["idx"]
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
