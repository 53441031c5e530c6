"""Drives both rechecks of the set phase once, for a kernel trace or an A/B of results: SafeOpt, GoOSE and trust-region sweeps of an fp64
model on K1b's plan with the guard recheck forced (option guard_band = 2), lean SafeOpt included, then the same three sweeps of an fp32
model with its fp64 twin (fp64_recheck).  Prints one JSON line per sweep (the result struct, mask sums, recheck counters of the profile).

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/recheck_trace.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import safebo_amd  # noqa: E402
from safebo_amd import synthetic  # noqa: E402


def _line(what, eng, res, masks):
    prof = eng.profile()
    out = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in res.items()}
    out["masks"] = {f"{k}{c or ''}": int(np.sum(eng.mask(k, c))) for k, c in masks}
    out["prof"] = {k: prof[k] for k in ("posterior_kernel", "posterior_launches", "fp64_rechecks", "host_syncs") if k in prof}
    print(json.dumps({what: out}, default=float), flush=True)


def _sweeps(tag, eng, cfg):
    b, q = cfg["b"], eng.q
    x0 = 0.5 * (cfg["bound"][:, 0] + cfg["bound"][:, 1])
    r = 0.3 * float(np.min(cfg["bound"][:, 1] - cfg["bound"][:, 0]))
    sum_ = [("S", 0), ("U", 0), ("M", 0)] + [("G", c) for c in range(1, q)]
    _line(f"{tag} safeopt", eng, eng.sweep_safeopt(b, want_masks=True), sum_)
    _line(f"{tag} goose", eng, eng.sweep_goose(b, want_masks=True, posterior_ready=True), [("S", 0), ("U", 0)] + [("O", c) for c in range(1, q)])
    _line(f"{tag} tr", eng, eng.sweep_tr(b, x0, r, posterior_ready=True), [("S", 0), ("M", 0)])
    _line(f"{tag} safeopt lean", eng, eng.sweep_safeopt(b, want_masks=True, lean=2), sum_)


def main():
    with safebo_amd.SweepEngine(0) as eng:
        for name, n, count in (("B", 64, [256, 256]), ("C", 96, [260, 250])):
            cfg = synthetic.make_config(name, n=n)
            eng.set_grid(cfg["bound"][:, 0], cfg["bound"][:, 1], count)
            eng.set_option("guard_band", 2)
            eng.set_model(cfg["ds"], dtype="f64")
            eng.sweep_safeopt(cfg["b"])                    # (a model's first sweep runs on K1i; the next ones on K1b's plan)
            _sweeps(f"{name} f64 guard", eng, cfg)
            eng.set_option("guard_band", 1)
            eng.set_model(cfg["ds"], dtype="f32")
            _sweeps(f"{name} f32 recheck", eng, cfg)


if __name__ == "__main__":
    main()
