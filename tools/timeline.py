"""Print the kernel timeline of one bench step from a rocprofv3 kernel trace (gpurun_out/<tag>/trace/**/_kernel_trace.csv)."""
# The default marker is the kernel that heads a lean-2 column-path sweep of a resident model (stage 1 runs once per plan, not per
# sweep) with option k1_cells off; with it (the default) a resident plan's sweep is headed by "k_bhead"; for other sweeps pass the
# kernel that heads them, e.g. "k_bpost<".
import csv, glob, sys
tag = sys.argv[1]
f = glob.glob(f"gpurun_out/{tag}/trace/**/*_kernel_trace.csv", recursive=True)[0]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
# (no marker given: k_bhead where the trace has it -- option k1_cells, the default --, else k_bl_sched_tiles1)
marker = sys.argv[2] if len(sys.argv) > 2 else ("k_bhead" if any("k_bhead" in r["Kernel_Name"] for r in rows) else "k_bl_sched_tiles1")
idx = [i for i, r in enumerate(rows) if marker in r["Kernel_Name"]]
s, e = idx[-2], idx[-1]
t0 = int(rows[s]["Start_Timestamp"]); prev = t0
for r in rows[s:e]:
    st, en = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    print(f"{(st - t0) / 1e3:8.1f} {(en - st) / 1e3:7.1f} gap {(st - prev) / 1e3:6.1f}  grid {r['Grid_Size_X']:>9}x{r['Grid_Size_Y']:<6} q{r.get('Queue_Id', '?'):>3} {r['Kernel_Name'][:64]}")
    prev = en
