#!/usr/bin/env python3
"""One sweep's kernel timeline from a rocprofv3 kernel trace: tools/timeline2.py gpurun_out/TAG [sweep index]"""
# Optional third argument: the kernel that heads a sweep (default k_bl_sched_tiles1, a lean-2 column-path sweep of a resident model;
# stage 1 runs once per plan, not per sweep; with option k1_cells, the default, pass k_bhead).
import csv, glob, sys
f = glob.glob(sys.argv[1] + "/trace/*/*_kernel_trace.csv")[0]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
names = [r["Kernel_Name"].split("(")[0].replace("void ", "").replace("sbo::", "") for r in rows]
marker = sys.argv[3] if len(sys.argv) > 3 else ("k_bhead" if any(n.startswith("k_bhead") for n in names) else "k_bl_sched_tiles1")
idx = [i for i, n in enumerate(names) if n.startswith(marker)]
k = int(sys.argv[2]) if len(sys.argv) > 2 else len(idx) // 2
i0, i1 = idx[k], idx[k + 1]
t0 = int(rows[i0]["Start_Timestamp"])
for r, n in zip(rows[i0:i1 + 1], names[i0:i1 + 1]):
    s, e = int(r["Start_Timestamp"]) - t0, int(r["End_Timestamp"]) - t0
    print(f"{n[:36]:36s} q{r.get('Queue_Id','?'):>3s} start {s/1e3:8.1f} end {e/1e3:8.1f} dur {(e-s)/1e3:7.1f}")
