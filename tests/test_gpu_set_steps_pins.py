"""expander_set and goose_sets (csrc/sets.hip), the host functions that decide which of some thirty set-phase kernels a constraint gets,
return what they returned before they became drivers over named steps and one window type: tests/golden/set_steps/record_before_steps.npz
holds what the commit named in its ``commit`` entry returned on an MI355X for the cases listed here (tests/golden/set_steps/record.py
writes it).  The oracle tests cannot see a wrong block size of the last-axis minima, a scan list half the size, a missed 16-bit image or
an exact recheck that takes over what the transform should have decided: the masks stay right while ``n_exact_rechecks`` moves.  Here
everything is compared for equality, floats bit for bit (the device code is the same): every entry of the result of ``sweep_safeopt`` and
``sweep_goose`` (``n_exact_rechecks`` among them), the masks S, U, M and G_c (GoOSE: S, U and O_c), and from the profile ``host_syncs``,
``halo_reruns``, ``comm_calls`` and ``comm_bytes``.  Masks of more than 100 000 candidates are pinned as the SHA-256 digest of their
packed bits and their count, smaller ones as packed bits.

Cases: the smallest shapes at which each branch of the two functions is taken (kCoarse = 8; coarse bounds from 65 536 window candidates
with every axis >= 32; the paired launches from count0 >= 1024; block minima from a last axis >= 128).  fp64 models of
synthetic.make_config; option col_path = 0 wherever the model has one constraint (such a SafeOpt sweep would otherwise take the column
path and never call expander_set).  SafeOpt and GoOSE run on every case, each behind a fresh ``set_model``.

  d1               d = 1, 301 points, q = 2: the model of test_one_dimensional_model_and_grid
  A20              config A, n = 20, 50 x 37: no coarse grid, no block minima
  B320x224         config B, n = 128: coarse grid by k_coarsen_mask, separate k_block_min, scan list, lines of whole words (k_edt_decide8)
  B324x224         ... lines that are not (k_edt_decide<T, true>)
  B1024x64         paired launches, no block minima, the image in doubles
  B1024x128        paired, 16-bit image, block minima inside k_set_mid, a wave per line; GoOSE: k_block_max_w
  B1032x128        paired without wave lines
  B1024x128_<opt>  B1024x128 with scan_waves = 0, scan_waves = 32, scan_blocks = 0, set_fuse = 0, goose_pairs = 1
  B512x1024        GoOSE only: k_pdt_axis0_lds
  d3_48x40x36      the three-input model of test_sweeps_on_grids_of_any_dimension: middle-axis scans, dist2b, coarse grid on
  d3_20x18x16      ... coarse grid off
  C64_lanes<v>     config C, n = 64, q = 3, 48 x 41 with set_lanes = 1 and 0: the minimiser rides the first constraint; two lanes
  A50_lazy<v>      config A, 50 x 50, exact_lazy = 0, 1, 2: the lazy exact recheck
  C64_list_index<v>  config C's model (n = 64) on 700 scattered points, list_index = 1 and 0: list_index_expander / k_list_safe, both
                   GoOSE pair paths

Ranks on one GPU through tests/_gpu_rank_worker.py, config B, n = 128, 96 x 81, with 2 and with 3 ranks: one sweep pair (the host waits
for the keys), and a sequence with two values of b (the second sweep uses the speculative window).  On 96 x 81 the halo (16 to 24
planes) fits the smallest shard (27 planes with three ranks) and GoOSE's source exchange is always the slab exchange; the three-rank
sequence therefore runs on 96 x 21 (shards of 7 planes, a halo of 6 and a speculative one of 9), which takes the full all-gather
(SBO_DEBUG_COMM says which; the number of lines of either kind is pinned too).
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from safebo_amd import synthetic  # noqa: E402

import test_gpu_recheck_pins as rpins  # noqa: E402  (arrays / pack / unpack: the fixture's form)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(HERE, "golden", "set_steps", "record_before_steps.npz")
PROFILE_KEYS = ("host_syncs", "halo_reruns", "comm_calls", "comm_bytes")
DIGEST_ABOVE = 100_000
MARK = None                  # record.py --marks: called with "<case>/<sweep>" in front of every sweep (a kernel trace is cut at these)
DEFAULTS = {"col_path": 1, "scan_waves": 1, "scan_blocks": 1, "set_fuse": 1, "goose_pairs": 0, "set_lanes": 1, "exact_lazy": 1,
            "list_index": -1}


def _d1_model():
    rng = np.random.default_rng(4)
    X = rng.uniform(-1, 1, size=(15, 1))
    Y = np.stack([np.sin(3 * X[:, 0]), 0.6 - X[:, 0] ** 2], axis=1)
    return synthetic.make_dataset(X, Y, synthetic.default_hypopt(1, 2)), np.array([[-1.0, 1.0]]), 2.0


def _d3_model():
    d, n, off, ll = 3, 40, 0.9, -0.5
    rng = np.random.default_rng(200 + d)
    X = rng.uniform(-1, 1, size=(n, d))
    Y = np.stack([np.sin(X.sum(1)) + 0.5 * X[:, 0], off - 1.8 * (X ** 2).mean(1) + 0.3 * X[:, 1]], axis=1)
    hyp = synthetic.default_hypopt(d, 2)
    hyp[:d, :] = ll
    return synthetic.make_dataset(X, Y, hyp), np.stack([-np.ones(d), np.ones(d)], axis=1), 1.0


def _cfg_model(name, n):
    cfg = synthetic.make_config(name, n=n)
    return cfg["ds"], cfg["bound"], cfg["b"]


# name -> (model, grid count or None for the 700 scattered points, options, sweeps)
BOTH = ("safeopt", "goose")
CASES = {
    "d1": (_d1_model, [301], {}, BOTH),
    "A20": (lambda: _cfg_model("A", 20), [50, 37], {}, BOTH),
    "B320x224": (lambda: _cfg_model("B", 128), [320, 224], {}, BOTH),
    "B324x224": (lambda: _cfg_model("B", 128), [324, 224], {}, BOTH),
    "B1024x64": (lambda: _cfg_model("B", 128), [1024, 64], {}, BOTH),
    "B1024x128": (lambda: _cfg_model("B", 128), [1024, 128], {}, BOTH),
    "B1032x128": (lambda: _cfg_model("B", 128), [1032, 128], {}, BOTH),
    "B1024x128_scan_waves0": (lambda: _cfg_model("B", 128), [1024, 128], {"scan_waves": 0}, BOTH),
    "B1024x128_scan_waves32": (lambda: _cfg_model("B", 128), [1024, 128], {"scan_waves": 32}, BOTH),
    "B1024x128_scan_blocks0": (lambda: _cfg_model("B", 128), [1024, 128], {"scan_blocks": 0}, BOTH),
    "B1024x128_set_fuse0": (lambda: _cfg_model("B", 128), [1024, 128], {"set_fuse": 0}, BOTH),
    "B1024x128_goose_pairs1": (lambda: _cfg_model("B", 128), [1024, 128], {"goose_pairs": 1}, BOTH),
    "B512x1024": (lambda: _cfg_model("B", 128), [512, 1024], {}, ("goose",)),
    "d3_48x40x36": (_d3_model, [48, 40, 36], {}, BOTH),
    "d3_20x18x16": (_d3_model, [20, 18, 16], {}, BOTH),
    "C64_lanes1": (lambda: _cfg_model("C", 64), [48, 41], {"set_lanes": 1}, BOTH),
    "C64_lanes0": (lambda: _cfg_model("C", 64), [48, 41], {"set_lanes": 0}, BOTH),
    "A50_lazy0": (lambda: _cfg_model("A", None), [50, 50], {"exact_lazy": 0}, BOTH),
    "A50_lazy1": (lambda: _cfg_model("A", None), [50, 50], {"exact_lazy": 1}, BOTH),
    "A50_lazy2": (lambda: _cfg_model("A", None), [50, 50], {"exact_lazy": 2}, BOTH),
    "C64_list_index1": (lambda: _cfg_model("C", 64), None, {"list_index": 1}, BOTH),
    "C64_list_index0": (lambda: _cfg_model("C", 64), None, {"list_index": 0}, BOTH),
}
# (world, grid, b or the sequence's list of b)
RANK_CASES = {"ranks2_single": (2, [96, 81], 3.0), "ranks3_single": (3, [96, 81], 3.0), "ranks2_sequence": (2, [96, 81], [3.0, 2.0]),
              "ranks3_sequence": (3, [96, 21], [2.0, 3.0])}
RANK_MODEL = ("B", 128)


def _mask(m):
    """packed bits, or above DIGEST_ABOVE candidates the SHA-256 digest of the packed bits followed by the count's eight bytes"""
    bits = np.packbits(m)
    if m.size <= DIGEST_ABOVE:
        return bits
    return np.concatenate([np.frombuffer(hashlib.sha256(bits.tobytes()).digest(), dtype=np.uint8),
                           np.frombuffer(np.int64(np.count_nonzero(m)).tobytes(), dtype=np.uint8)])


def _record(engine, res, q, masks, per_constraint):
    out = dict(res)
    prof = engine.profile()
    for k in PROFILE_KEYS:
        out["profile_" + k] = prof[k]
    out["profile_set_path"] = prof["set_path"]
    for k in masks:
        out["mask_" + k] = _mask(engine.mask(k))
    for c in range(1, q):
        out[f"mask_{per_constraint}{c}"] = _mask(engine.mask(per_constraint, c))
    return out


def run_case(engine, name):
    model, count, options, sweeps = CASES[name]
    ds, bound, b = model()
    q = ds["Y_norm"].shape[1]
    options = dict(options, **({"col_path": 0} if q == 2 else {}))
    out = {}
    try:
        for k, val in options.items():
            engine.set_option(k, val)
        if count is None:
            engine.set_points(np.random.default_rng(700).uniform(bound[:, 0], bound[:, 1], size=(700, bound.shape[0])))
        else:
            engine.set_grid(bound[:, 0], bound[:, 1], count)
        if "safeopt" in sweeps:
            engine.set_model(ds)
            if MARK:
                MARK(name + "/safeopt")
            out["safeopt"] = _record(engine, engine.sweep_safeopt(b, want_masks=True), q, "SUM", "G")
        if "goose" in sweeps:
            engine.set_model(ds)
            if MARK:
                MARK(name + "/goose")
            out["goose"] = _record(engine, engine.sweep_goose(b, want_masks=True), q, "SU", "O")
    finally:
        for k in options:
            engine.set_option(k, DEFAULTS[k])
    return out


def check_case(got):
    """what makes a case worth pinning: the byte-mask set phase ran, on a safe set with something to expand"""
    for step, v in got.items():
        assert v["profile_set_path"] == 0, (step, v["profile_set_path"])
        assert v["count_S"] > 0 and v["count_U"] > 0, (step, v["count_S"], v["count_U"])


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def run_ranks(tmp_dir, name):
    """One rank run: what rank 0 reports, every rank's masks, and how often GoOSE's source exchange took either branch."""
    world, count, b = RANK_CASES[name]
    cfg_name, n = RANK_MODEL
    port, out = _free_port(), os.path.join(str(tmp_dir), "res.json")
    logs = [open(os.path.join(str(tmp_dir), f"err{r}.txt"), "w+") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_gpu_rank_worker.py"), str(r), str(world), port, out, cfg_name, str(n),
                               json.dumps(count), json.dumps(b)], env={**os.environ, "SBO_DEBUG_COMM": "1"}, stderr=logs[r])
             for r in range(world)]
    try:
        codes = [p.wait(timeout=600) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    text = ""
    for f in logs:
        f.seek(0)
        text += f.read()
        f.close()
    assert codes == [0] * world, (codes, text[-2000:])
    res = json.load(open(out))
    got = {}
    if isinstance(res, list):                                   # a sequence: one row per sweep pair
        for i, row in enumerate(res):
            got[f"row{i}"] = {k: np.asarray(v) for k, v in row.items()}
    else:
        flat = {k: v for k, v in res.items() if not isinstance(v, dict) and v is not None}
        flat.update({f"goose_{k}": v for k, v in (res["goose"] or {}).items()})
        got["rank0"] = flat
    for r in range(world):
        z = np.load(out + f".rank{r}.npz")
        got[f"rank{r}_masks"] = {k: (np.packbits(z[k]) if z[k].dtype == bool else z[k]) for k in z.files}
    lines = [ln for ln in text.splitlines() if "GoOSE sources" in ln]
    print("\n".join(sorted(lines)))
    got["source_exchange"] = {"slab": sum("slab exchange" in ln for ln in lines), "allgather": sum("full all-gather" in ln for ln in lines)}
    return got


def _compare(case, got):
    z = rpins.unpack(np.load(FIXTURE))
    assert got
    bad = []
    for name, a in got.items():
        want = z[name]
        same = a.dtype == want.dtype and np.array_equal(a, want)
        print(f"{name}: {a.tolist() if a.size <= 8 else a.size} {'==' if same else '!= ' + str(want.tolist() if want.size <= 8 else want.size)}")
        if not same:
            bad.append(name)
    assert not bad, bad
    recorded = {k for k in z if k.split("/")[0] == case}
    assert recorded == set(got), recorded ^ set(got)


@pytest.mark.parametrize("name", list(CASES))
def test_set_phase_returns_what_it_returned_before_the_steps(engine, name):
    got = run_case(engine, name)
    check_case(got)
    _compare(name, rpins.arrays(name, got))


@pytest.mark.parametrize("name", list(RANK_CASES))
def test_rank_set_phase_returns_what_it_returned_before_the_steps(tmp_path, name):
    got = run_ranks(tmp_path, name)
    _compare(name, rpins.arrays(name, got))
