"""Provenance of tests/golden/stableopt/w_shape.npz: a verbatim copy of the reference project's own data file data/data_StableOpt.npz
(four plain fp32 arrays, no pickle: sampled_x [3, 2], sampled_output [3, 1], observed_x [15, 2], observed_output [15, 1]).  The inputs
are (xc, d) of the W-shape problem, f(x, d) = sin(x d) + sqrt(d) x^2 - 0.5 x on xc in [-1, 2], d in [2, 4]; the outputs are f there.
It is data -- the points a robust campaign of the reference sampled -- and drives tests/test_gpu_robust.py (kept in a subdirectory: the *.npz files directly under tests/golden/ are the sweep
goldens tests/test_oracle.py replays); run this script in a
container that has /root/reference to refresh it."""
import os
import shutil

SRC = "/root/reference/data/data_StableOpt.npz"
DST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stableopt", "w_shape.npz")

if __name__ == "__main__":
    shutil.copyfile(SRC, DST)
    print("copied", SRC, "->", DST)
