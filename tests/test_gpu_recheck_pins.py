"""The recheck sweeps -- the fp64 twin of fp32 models and the guard-band re-evaluation of K1b / K1i (csrc/sets_recheck.inc.hpp) --
return what they returned before their two front ends became one and the shared blocks got typed layouts:
tests/golden/recheck/record_before_one_front.npz holds what the commit named in its ``commit`` entry returned on an MI355X for the
cases listed here (tests/golden/recheck/record.py writes it).  The oracle tests of these sweeps accept any ``guard_rechecks >= 0``, any
number of passes and any ``fp64_rechecks``: a front that re-evaluated another list would pass them.  Here everything is compared for
equality, floats bit for bit (the device code is the same): every entry of the result of ``sweep_safeopt``, ``sweep_goose`` and
``sweep_tr``, the masks S, U and M (a GoOSE sweep has no M: S, U and O_c; SafeOpt's G_c too), and from the profile ``fp64_rechecks``, ``posterior_launches``,
``posterior_kernel``, ``fp32_band_dm`` / ``fp32_band_dv`` and ``host_syncs``.

Cases (all small: a few thousand candidates):

fp32 model with its fp64 twin (``dtype="f32"``, the library's factor):
  f32_A20       config A, n = 20, grid 50 x 37, q = 2;
  f32_C64       config C, n = 64, grid 48 x 41, q = 3 (two expander sets);
  f32_q1        config A's data, objective only (q = 1), grid 33 x 31: no constraints, so only the contenders of the arg-min are
                re-evaluated, and the trust-region sweep builds its ball mask and runs the contender pass;
  f32_C64_list  the model of f32_C64 on an explicit list of 700 scattered points: no grid to transform, so the flag pass lists every
                possibly-safe candidate.
fp64 model with option guard_band = 2 (every sweep takes the re-evaluation path: the ``TP = double`` front), option bilinear = 1 and 2,
with the caller's invK and with the library's factor:
  f64_A64       config A, n = 64, grid 70 x 65;
  f64_B64       config B, n = 64, grid 130 x 70.
  ``posterior_kernel`` is 4 (K1b) or 6 (K1i) in each of them; the test asserts it beside the pin.

Every case runs, each group behind a fresh ``set_model``: SafeOpt fresh, then with ``posterior_ready`` right behind it; a ``lean = 1``
SafeOpt sweep, then SafeOpt with ``posterior_ready`` behind it (the one input on which the reuse rule of the SafeOpt front and that of
the GoOSE / trust-region front differ); GoOSE fresh and with ``posterior_ready``; the trust-region sweep fresh and with
``posterior_ready``.

Two ranks on one GPU through tests/_gpu_rank_worker.py: config B, n = 128, grid 96 x 81, fp32 (the case of
test_multi_rank_fp32_sweep_with_fp64_recheck_equals_the_fp64_oracle): everything rank 0 reports of its SafeOpt, GoOSE and
trust-region sweeps (``fp64_rechecks`` among it), and every mask and ``fp64_rechecks`` of both ranks.
"""
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

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(HERE, "golden", "recheck", "record_before_one_front.npz")
PROFILE_KEYS = ("fp64_rechecks", "posterior_launches", "posterior_kernel", "fp32_band_dm", "fp32_band_dv", "host_syncs")
RANK_CASE = ("B:f32", 128, [96, 81], 3.0)


def _f32_case(name):
    """-> (ds, bound, b, grid count or None, points or None)"""
    if name == "f32_A20":
        cfg = synthetic.make_config("A", n=20)
        return cfg["ds"], cfg["bound"], 3.0, [50, 37], None
    if name == "f32_q1":
        cfg = synthetic.make_config("A", n=20)
        return synthetic.make_dataset(cfg["X"], cfg["Y"][:, :1], synthetic.default_hypopt(2, 1)), cfg["bound"], 3.0, [33, 31], None
    cfg = synthetic.make_config("C", n=64)
    if name == "f32_C64":
        return cfg["ds"], cfg["bound"], 2.0, [48, 41], None
    pts = np.random.default_rng(700).uniform(cfg["bound"][:, 0], cfg["bound"][:, 1], size=(700, 2))
    return cfg["ds"], cfg["bound"], 2.0, None, pts


F32_CASES = ["f32_A20", "f32_C64", "f32_q1", "f32_C64_list"]
F64_CASES = [(cfg, count, mode, use_invK) for cfg, count in (("A", [70, 65]), ("B", [130, 70])) for mode in (1, 2) for use_invK in (True, False)]


def _f64_id(case):
    cfg, _, mode, use_invK = case
    return f"f64_{cfg}64_bilinear{mode}_{'invK' if use_invK else 'factor'}"


def _record(engine, res, q, masks="SUM", per_constraint=None):
    """The result, the pinned profile entries, the masks named in ``masks`` and the ``per_constraint`` masks G_c or O_c, bit-packed."""
    out = dict(res)
    prof = engine.profile()
    for k in PROFILE_KEYS:
        out["profile_" + k] = prof[k][:q] if isinstance(prof[k], list) else prof[k]
    if masks:
        for k in masks:
            out["mask_" + k] = np.packbits(engine.mask(k))
        for c in range(1, q) if per_constraint else ():
            out[f"mask_{per_constraint}{c}"] = np.packbits(engine.mask(per_constraint, c))
    return out


def _sweeps(engine, model, b, bound, q):
    """The eight pinned sweeps of one case (and the lean sweep between them); ``model()`` installs the model afresh."""
    x0 = 0.5 * (bound[:, 0] + bound[:, 1])
    r = 0.3 * float(np.min(bound[:, 1] - bound[:, 0]))
    out = {}
    model()
    out["safeopt_fresh"] = _record(engine, engine.sweep_safeopt(b, want_masks=True), q, per_constraint="G")
    out["safeopt_ready"] = _record(engine, engine.sweep_safeopt(b, want_masks=True, posterior_ready=True), q, per_constraint="G")
    model()
    out["safeopt_lean1"] = _record(engine, engine.sweep_safeopt(b, lean=1), q, masks="")
    out["safeopt_ready_behind_lean1"] = _record(engine, engine.sweep_safeopt(b, want_masks=True, posterior_ready=True), q, per_constraint="G")
    model()
    out["goose_fresh"] = _record(engine, engine.sweep_goose(b, want_masks=True), q, masks="SU", per_constraint="O")
    out["goose_ready"] = _record(engine, engine.sweep_goose(b, want_masks=True, posterior_ready=True), q, masks="SU", per_constraint="O")
    model()
    out["tr_fresh"] = _record(engine, engine.sweep_tr(b, x0, r), q)                     # (M: the trust region's set)
    out["tr_ready"] = _record(engine, engine.sweep_tr(b, x0, r, posterior_ready=True), q)
    return out


def run_f32(engine, name):
    ds, bound, b, count, pts = _f32_case(name)
    if count is None:
        engine.set_points(pts)
    else:
        engine.set_grid(bound[:, 0], bound[:, 1], count)
    return _sweeps(engine, lambda: engine.set_model(ds, dtype="f32", use_invK=False), b, bound, ds["Y_norm"].shape[1])


def run_f64(engine, case):
    cfg_name, count, mode, use_invK = case
    cfg = synthetic.make_config(cfg_name, n=64)
    ds = cfg["ds"] if use_invK else {k: v for k, v in cfg["ds"].items() if k != "invKopt"}
    bound = cfg["bound"]
    try:
        engine.set_option("bilinear", mode)
        engine.set_option("guard_band", 2)
        engine.set_grid(bound[:, 0], bound[:, 1], count)
        return _sweeps(engine, lambda: engine.set_model(ds, use_invK=use_invK), cfg["b"], bound, cfg["q"])
    finally:
        engine.set_option("guard_band", 1)
        engine.set_option("bilinear", 1)


def check_f32(got):
    """what makes a case worth pinning: the twin re-evaluated something in every sweep"""
    assert all(v["profile_fp64_rechecks"] > 0 for v in got.values()), {k: v["profile_fp64_rechecks"] for k, v in got.items()}


def check_f64(got):
    """... the posterior came from K1b (4) or K1i (6), and every sweep took the re-evaluation path"""
    for step, v in got.items():
        assert v["profile_posterior_kernel"] in (4, 6), (step, v["profile_posterior_kernel"])
        assert v["guard_passes"] >= 1, (step, v["guard_passes"])


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def run_ranks(tmp_dir):
    """The two-rank case: {"rank0": everything rank 0 reports, "rank<r>_masks": the masks and fp64_rechecks of rank r}."""
    cfg_name, n, count, b = RANK_CASE
    port, out = _free_port(), os.path.join(str(tmp_dir), "res.json")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_gpu_rank_worker.py"), str(r), "2", port, out, cfg_name, str(n),
                               json.dumps(count), str(b)]) for r in range(2)]
    try:
        codes = [p.wait(timeout=600) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert codes == [0, 0], codes
    res = json.load(open(out))
    flat = {k: v for k, v in res.items() if not isinstance(v, dict)}
    for sweep in ("goose", "tr"):
        flat.update({f"{sweep}_{k}": v for k, v in res[sweep].items()})
    got = {"rank0": flat}
    for r in range(2):
        z = np.load(out + f".rank{r}.npz")
        got[f"rank{r}_masks"] = {k: (np.packbits(z[k]) if z[k].dtype == bool else z[k]) for k in z.files}
    return got


def arrays(case, results):
    """{"case/step/key": array} of every entry: floats as their uint64 bit patterns, everything else as int64 / uint8."""
    flat = {}
    for step, res in results.items():
        for k, v in res.items():
            a = np.ascontiguousarray(v)
            if a.dtype == np.float64:
                a = a.view(np.uint64)
            elif a.dtype != np.uint8:
                assert a.dtype.kind in "iub", (case, step, k, a.dtype)
                a = a.astype(np.int64)
            flat[f"{case}/{step}/{k}"] = a.reshape(-1)
    return flat


def pack(flat):
    """The fixture's form -- one array per dtype, every entry a slice of it, ``index``: JSON {name: [dtype, start, size]} (two and a half
    thousand entries of a few values each: as one .npz member apiece the file would be mostly member headers)."""
    index, parts = {}, {"uint64": [], "int64": [], "uint8": []}
    for name in sorted(flat):
        a = flat[name]
        index[name] = [a.dtype.name, sum(p.size for p in parts[a.dtype.name]), a.size]
        parts[a.dtype.name].append(a)
    return {"index": np.array([json.dumps(index)]), **{t: np.concatenate(p) for t, p in parts.items()}}


def unpack(z):
    return {name: z[t][start:start + size] for name, (t, start, size) in json.loads(str(z["index"][0])).items()}


def _compare(case, got):
    z = unpack(np.load(FIXTURE))
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


@pytest.mark.parametrize("name", F32_CASES)
def test_fp32_recheck_sweeps_return_what_they_returned_before_the_one_front(engine, name):
    got = run_f32(engine, name)
    check_f32(got)
    _compare(name, arrays(name, got))


@pytest.mark.parametrize("case", F64_CASES, ids=_f64_id)
def test_guard_band_rechecks_return_what_they_returned_before_the_one_front(engine, case):
    got = run_f64(engine, case)
    check_f64(got)
    _compare(_f64_id(case), arrays(_f64_id(case), got))


def test_two_rank_fp32_recheck_returns_what_it_returned_before_the_one_front(tmp_path):
    got = run_ranks(tmp_path)
    assert got["rank0"]["fp64_rechecks"] > 0
    _compare("ranks2_B128_f32", arrays("ranks2_B128_f32", got))
