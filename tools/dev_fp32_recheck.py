"""BASELINE config B (2048 x 2048, n = 128) as an fp32 model: the band in force, the recheck share (fp64_rechecks / N) and the device
time of the SafeOpt sweep -- first sweep (the band is measured there) and the median of 15 after 3 warm-up sweeps --, for the
library's own factor and the caller's invK.  `--lib PATH` measures another build of libsafebo.so (A/B against a parent build).
Numbers: profiles/fp32_band_checks.md."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import safebo_amd  # noqa: E402
from safebo_amd import _lib, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--config", default="B")
args = ap.parse_args()
if args.lib:
    _lib.library_path = lambda: os.path.abspath(args.lib)
out = {}
with safebo_amd.SweepEngine(0) as eng:
    for use_invK in (False, True):
        cfg = synthetic.make_config(args.config)
        lo, hi, count = cfg["bound"][:, 0], cfg["bound"][:, 1], cfg["count"]
        eng.set_model(cfg["ds"], dtype="f32", use_invK=use_invK)
        eng.set_grid(lo, hi, count)
        first, tot, rec, post = None, [], [], []
        for it in range(18):
            eng.sweep_safeopt(cfg["b"])
            p = eng.profile()
            first = p["total_ms"] if first is None else first
            if it >= 3:
                tot.append(p["total_ms"])
                rec.append(p["recheck_ms"])
                post.append(p["posterior_ms"])
        N, q = int(np.prod(count)), cfg["q"]
        ys = np.maximum(1.0, cfg["ds"]["Y_std"])
        out["invK" if use_invK else "chol"] = {
            "N": N, "fp64_rechecks": int(p["fp64_rechecks"]), "share": p["fp64_rechecks"] / N, "first_sweep_total_ms": first,
            "total_ms_median": float(np.median(tot)), "recheck_ms_median": float(np.median(rec)), "posterior_ms_median": float(np.median(post)),
            "band_dm_norm": list(np.array(p.get("fp32_band_dm", [0.0] * q)[:q]) / ys),
            "band_dv_norm": list(np.array(p.get("fp32_band_dv", [0.0] * q)[:q]) / ys ** 2)}
print(json.dumps(out))
