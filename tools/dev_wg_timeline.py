#!/usr/bin/env python3
"""Per-workgroup timeline of the column path's two k_bpost launches (the constraint's, then the objective's) of one lean-2 sweep of
config H, from the diagnostic build (make -C safe-bayesian-optimization_amd/csrc phaseclk; run on the GPU box as
  cp safe-bayesian-optimization_amd/libsafebo_phaseclk.so safe-bayesian-optimization_amd/libsafebo.so && python tools/dev_wg_timeline.py [--sched 0|1]
on its scratch copy).  Every workgroup records its tile, what it did (evaluated / skipped / skipped but ran the gradient phases /
past the tile list), wall_clock64 (100 MHz) at entry, at the start of its partial rows and at exit, and the XCC / SE / CU it ran on
(bilinear.hip: g_wg_trace).  Printed per launch: its span, the evaluated tiles per CU, the start times of the evaluated tiles, the
slot time the other workgroups held, and the time from the partial rows (post_partials, the S / U words, their Usum and slot
atomics) to exit."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import safebo_amd                                   # noqa: E402
from safebo_amd import synthetic                    # noqa: E402

ROWS = 1 << 13
KINDS = ("evaluated", "skipped (partial rows only)", "skipped, gradient phases run", "past the tile list (exit at once)",
         "classified from memory (k_bres)", "head launch (k_bhead: tile decisions, undecided cells from memory)")
TICK_US = 0.01                                      # wall_clock64: 100 MHz


def decode(rows):
    """rows [ROWS][8] -> dict of arrays over the written rows (dispatch order)."""
    w = (rows[:, 3] >> 31) & 1 == 1
    r = rows[w]
    hw, xcc = r[:, 4], r[:, 5] & 0xF
    return {"t0": r[:, 0].astype(np.int64), "tp": r[:, 1].astype(np.int64), "t1": r[:, 2].astype(np.int64),
            "tile": (r[:, 3] & 0xFFFFFF).astype(np.int64), "kind": ((r[:, 3] >> 24) & 0x7F).astype(np.int64),
            "cu": (xcc << 8) | (((hw >> 13) & 0x7) << 5) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 0xF)}


def report(name, d, out):
    if len(d["t0"]) == 0:
        print(f"{name}: no rows", file=out)
        return
    base = d["t0"].min()
    span = (d["t1"].max() - base) * TICK_US
    print(f"{name}: {len(d['t0'])} workgroups, span {span:.1f} us (first entry -> last exit)", file=out)
    for k, nm in enumerate(KINDS):
        m = d["kind"] == k
        if m.any():
            life = (d["t1"][m] - d["t0"][m]) * TICK_US
            print(f"   {nm:36s} {int(m.sum()):5d} workgroups, life mean {life.mean():6.2f} us, max {life.max():6.2f}, "
                  f"slot time {life.sum():8.1f} us", file=out)
    ev = d["kind"] != 3
    ev &= d["kind"] != 1
    per_cu = np.bincount(np.unique(d["cu"][ev], return_inverse=True)[1]) if ev.any() else np.zeros(0, np.int64)
    ncu = len(np.unique(d["cu"]))
    print(f"   CUs seen {ncu}; tiles with a GEMM phase per CU (over the CUs that got one: {len(per_cu)}): "
          f"histogram {{{', '.join(f'{int(a)}: {int(b)}' for a, b in zip(*np.unique(per_cu, return_counts=True)))}}}", file=out)
    st = (d["t0"][ev] - base) * TICK_US
    if len(st):
        edges = np.arange(0.0, max(st.max(), 1.0) + 5.0, 5.0)
        h, _ = np.histogram(st, bins=edges)
        print("   start times of those tiles (5 us bins from the launch's first entry): " +
              " ".join(f"{int(e)}:{c}" for e, c in zip(edges[:-1], h) if c), file=out)
        end = (d["t1"][ev] - base) * TICK_US
        print(f"   their last start {st.max():.1f} us, last exit {end.max():.1f} us", file=out)
    nev = ~ev
    if nev.any():
        st2 = (d["t0"][nev] - base) * TICK_US
        print(f"   workgroups without a GEMM phase: entries from {st2.min():.1f} to {st2.max():.1f} us", file=out)
    part = (d["t1"] - d["tp"]) * TICK_US
    for k, nm in enumerate(KINDS[:3]):
        m = d["kind"] == k
        if m.any():
            print(f"   partial rows + words + atomics, {nm:30s}: mean {part[m].mean():6.2f} us, total {part[m].sum():8.1f} us", file=out)
    m = d["kind"] == 4
    if m.any():          # (k_bres: [1] is the clock behind its loads -- entry -> loads arrived -> exit)
        print(f"   classified from memory: loads {((d['tp'][m] - d['t0'][m]) * TICK_US).mean():6.2f} us, classification + partial rows + words "
              f"{part[m].mean():6.2f} us (means)", file=out)
    m = d["kind"] == 5
    if m.any():          # (k_bhead: [1] is the clock behind the first round's tile decisions; the tile is the first mixed one the workgroup's wave 0 decided, 0xffffff: none)
        dec, rest = (d["tp"][m] - d["t0"][m]) * TICK_US, part[m]
        mixed = m & (d["tile"] != 0xFFFFFF)
        print(f"   head launch: tile decisions mean {dec.mean():6.2f} us, max {dec.max():6.2f}; cells + tile outputs mean {rest.mean():6.2f} us, max {rest.max():6.2f}", file=out)
        if mixed.any():
            print(f"   ... workgroups whose wave 0 decided a mixed tile: {int(mixed.sum())}, life mean {((d['t1'][mixed] - d['t0'][mixed]) * TICK_US).mean():6.2f} us, "
                  f"max {((d['t1'][mixed] - d['t0'][mixed]) * TICK_US).max():6.2f}", file=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sched", type=int, default=1, help="option k1_sched (0: one workgroup per tile, the grid before the tile lists)")
    ap.add_argument("--config", default="H")
    ap.add_argument("--out", default=None)
    ap.add_argument("--resident", type=int, default=1, help="option k1_resident (a library without it: ignored)")
    ap.add_argument("--cells", type=int, default=1, help="option k1_cells (a library without it: ignored)")
    args = ap.parse_args()
    lib = safebo_amd._lib.load()
    fn = lib.sbo_debug_wg_trace
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_uint64), C.c_int, C.c_int]
    buf = np.zeros((2, ROWS, 8), dtype=np.uint64)
    ptr = buf.ctypes.data_as(C.POINTER(C.c_uint64))
    cfg = synthetic.make_config(args.config)
    eng = safebo_amd.SweepEngine(0)
    eng.set_option("k1_sched", args.sched)
    try:
        eng.set_option("k1_resident", args.resident)
    except ValueError:
        pass
    try:
        eng.set_option("k1_cells", args.cells)
    except ValueError:
        pass
    eng.set_model(cfg["ds"], dtype="f64", use_invK=True)
    eng.set_grid(cfg["bound"][:, 0], cfg["bound"][:, 1], list(cfg["count"]))
    for _ in range(5):
        eng.sweep_safeopt(cfg["b"], lean=2)
    eng.synchronize()
    assert fn(ptr, ROWS, 1) == 0
    res = eng.sweep_safeopt(cfg["b"], lean=2)
    eng.synchronize()
    prof = eng.profile()
    assert fn(ptr, ROWS, 0) == 0
    out = open(args.out, "w") if args.out else sys.stdout
    print(f"config {args.config}, lean 2, k1_sched {args.sched}: k1_tiles_skipped {prof['k1_tiles_skipped']}, k1_tiles_skipped_safe {prof['k1_tiles_skipped_safe']}, count_S {res['count_S']}, "
          f"posterior_ms {prof['posterior_ms']:.4f} (diagnostic build: a clock read and a barrier at each phase boundary)", file=out)
    report("constraint launch (k_bhead, or k_bres<1> / k_bpost<1,1>)", decode(buf[1]), out)
    report("objective launch k_bpost<1,2>", decode(buf[0]), out)
    eng.close()


if __name__ == "__main__":
    main()
