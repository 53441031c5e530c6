"""Compares two kernel traces of tests/golden/colpath_steps/record.py --marks (one per build of the library), sweep by sweep:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o trace -- python tests/golden/colpath_steps/record.py /dev/null --marks DIR/marks.txt
    python tools/colpath_trace_cmp.py PARENT_DIR HEAD_DIR

A trace is cut at the fill kernels record.py launches in front of every sweep (the first fill is the creation of its buffer).  Per sweep
-- with whatever follows it up to the next mark: set_model, set_grid, mask reads, a GoOSE sweep -- the multiset of (kernel, stream, grid,
workgroup, LDS) must be the same on both sides, and so must the order of the launches on every stream; the runtime's own fill and copy
kernels count, so that a memset that appears or disappears is seen.  Streams are numbered in the order they first appear.  Exit status 1
on any difference."""
import collections
import csv
import glob
import gzip
import os
import sys


def load(d):
    path = (glob.glob(os.path.join(d, "**", "*kernel_trace.csv*"), recursive=True) or [None])[0]
    assert path, f"no kernel trace under {d}"
    rows = list(csv.DictReader(gzip.open(path, "rt") if path.endswith(".gz") else open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    marks = open(os.path.join(d, "marks.txt")).read().split()
    streams, segs, cur = {}, [], None
    for r in rows:
        if "FillFunctor<float>" in r["Kernel_Name"]:
            cur = []
            segs.append(cur)
            continue
        if cur is None:
            continue
        s = streams.setdefault(r["Stream_Id"], len(streams))
        cur.append((r["Kernel_Name"], s, tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"), tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"),
                    int(r["LDS_Block_Size"])))
    assert len(segs) == len(marks) + 1, (len(segs), len(marks))
    return marks, segs[1:]


def main():
    (ma, sa), (mb, sb) = load(sys.argv[1]), load(sys.argv[2])
    assert ma == mb, "the two runs did not sweep the same cases"
    bad = 0
    for name, a, b in zip(ma, sa, sb):
        same_set = collections.Counter(a) == collections.Counter(b)
        same_order = all([x for x in a if x[1] == s] == [x for x in b if x[1] == s] for s in {x[1] for x in a + b})
        if not (same_set and same_order):
            bad += 1
            print(f"{name}: {'multiset differs' if not same_set else 'order on a stream differs'}")
            for k, n in (collections.Counter(a) - collections.Counter(b)).items():
                print("   only parent", n, k)
            for k, n in (collections.Counter(b) - collections.Counter(a)).items():
                print("   only head  ", n, k)
    print(f"{len(ma)} sweeps, {sum(len(x) for x in sa)} / {sum(len(x) for x in sb)} launches, {bad} sweeps differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
