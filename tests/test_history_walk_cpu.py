"""The history walks' generator (tests/history_walk.py) on its own, without a GPU: the fixed seeds' step lists hold every transition
tests/test_gpu_history.py is there to check, and they replay exactly from the seed."""
import hashlib
import json

import numpy as np
import pytest

import history_cases as hc
import history_walk as hw
import model_append_batch as mb
import oracle

# sha256 of json.dumps(make_walk(seed)) of the first version's walks: seeds 0 .. 7 stay what they were, step for step
PINNED = {
    0: "28ada6d9df1e11fc3c0e11d3f29a98abfebe690d06d6208433404c2b2d087e92",
    1: "78f4f05fb27c46a351bc5593feee3ed1f8b5f5aebcb357b0399af52472ce8c63",
    2: "05b00bf1d17e490b41b72e951c470d4a4b8fc6d85a539bf91c3eb96aaf5d18b8",
    3: "2a6efa5d3773877f0c6d0d209dcb4922e761ce57a762db767c38b409f871147a",
    4: "31aae02bcb54e5e440bd9e453a53e857e3f06e5ffa5f9022b0593fd5ee2958a6",
    5: "e0a4535125ae27994e4ed1448487684a7cc7b143092a47df100c62433569c743",
    6: "542397f1cc943a0ccb500eaee910446a104f3fdbb3d9c21396d3f3095c332de6",
    7: "25e5b40e24f1698b2d7b606c7d1f5957de40e30362ff7275c7cd7170bea0c71f",
}
# ... and of the second generation's, taken before the third joined the generator: seeds 8 .. 15 index READ_ONLY by its length, so the
# tuple stays the eight names it was and the calls added since stand in READ_ONLY3
PINNED2 = {
    8: "2123810c7e475d3e77a8af898c4c73b73dbc24ea3000198fae54ee720f4e15ad",
    9: "e3857006437b86dfddcf96dbe0dca0cf6fa34dcba36939b224630d5418511259",
    10: "331e048e85a5a36abbc954f42664bea916463abcd41df3e963875735798b61d1",
    11: "1f15d75adb9edc211cafced4fd96a87c05aeeff9d7f04de5876e8d35f73dc236",
    12: "6296d3e5942c76d8f388147b32cf0b7fda9b15a8ca0b7dedc0a1b1cd120fa353",
    13: "fe5c8af4d0d80444bb4fc2c3a3274d9c1d9aeba1c8ed625fb9087a9a6efb896e",
    14: "d32d95b8d25c04b82a844419e329fa205faabd89bf3fdb00e0c2ebbb42059852",
    15: "a786f483de911ab762ccf1c48a0eedf3976fe014cc2023105ef5335672879d7d",
}


def test_the_first_eight_walks_are_pinned():
    assert hw.OLD_SEEDS == tuple(PINNED)
    for seed, digest in PINNED.items():
        assert hashlib.sha256(json.dumps(hw.make_walk(seed)).encode()).hexdigest() == digest, seed


def test_the_second_eight_walks_are_pinned():
    assert hw.NEW_SEEDS == tuple(PINNED2) and len(hw.READ_ONLY) == 8
    for seed, digest in PINNED2.items():
        assert hashlib.sha256(json.dumps(hw.make_walk(seed)).encode()).hexdigest() == digest, seed


def test_fixed_seeds_cover_every_required_transition():
    seen = set()
    for seed in hw.OLD_SEEDS + hw.NEW_SEEDS:
        seen |= hw.transitions(hw.make_walk(seed))
    missing = hw.REQUIRED - seen
    assert not missing, sorted(missing)
    # every read-only step stands in front of a sweep on posterior_ready, and every sweep kind stands behind one of them
    behind = hw.read_only_followers(seen)
    assert all(behind[k] for k in hw.READ_ONLY), behind
    assert set().union(*behind.values()) == set(hw.READY_KINDS), behind
    assert not {n for n in seen if n.startswith(("direct:", "f32_read_", "again_")) or n.split("->")[0] in hw.NEW_CALLS}, seen


def test_the_third_seeds_cover_what_they_add():
    """Seeds 16 .. 23 alone: every name of REQUIRED3; each of the ten read-only calls behind a sweep and in front of a sweep on
    posterior_ready, the two new ones in front of every sweep kind; each of the ten directly behind some model change, the two new
    ones behind every one of them; each of the four dtype-free calls directly behind an fp32 update, every fp32 update in front of
    one; the tail of the fp32 segment in front of a new call."""
    per_seed = {seed: hw.walk_transitions(seed) for seed in hw.THIRD_SEEDS}
    seen = set().union(*per_seed.values())
    missing = hw.REQUIRED3 - seen
    assert not missing, sorted(missing)
    behind = hw.read_only_followers(seen, hw.READ_ONLY3)
    assert all(behind[k] for k in hw.READ_ONLY3), behind
    assert all(behind[k] == set(hw.READY_KINDS) for k in hw.NEW_CALLS), behind
    leaders = hw.direct_leaders(seen)
    assert all(leaders[k] for k in hw.READ_ONLY3), leaders
    assert all(leaders[k] >= set(hw.CHANGES) for k in hw.NEW_CALLS), leaders
    f32 = hw.direct_leaders(seen, f32=True)
    assert all(f32[k] for k in hw.F32_READS) and set().union(*f32.values()) == set(hw.F32_UPDATES), f32
    assert {"append_after_f32_then_f64->" + c for c in hw.NEW_CALLS} & seen
    assert [hw.walk_problem(seed) for seed in hw.THIRD_SEEDS] == ["B", "H", "C", "A"] * 2
    for seed, names in per_seed.items():
        # per walk: sample_paths on output q - 1 and on output 0, at both ends; both calls repeated around a sweep; problem C: a one-bit mask
        assert {"sample_paths_output_0", "sample_paths_output_last", "sample_paths_max", "sample_paths_min"} <= names, seed
        assert {"again_expander_gain", "again_sample_paths"} <= names, seed
        assert {"expander_gain->sample_paths", "sample_paths->expander_gain"} & names, seed
        assert hw.walk_problem(seed) != "C" or "expander_gain_one_bit" in names, seed
        ends = [s[2] for s in hw.make_walk(seed) if s[0] == "sample_paths"]
        assert all(a != b for a, b in zip(ends, ends[1:])), (seed, "maximize alternates", ends)


def test_the_old_walks_hold_none_of_the_new_steps():
    for seed in hw.OLD_SEEDS:
        assert not [s for s in hw.make_walk(seed) if s[0] in hw.READ_ONLY + hw.MODEL_STEPS]


def test_the_first_sixteen_walks_hold_none_of_the_third_generations_steps():
    for seed in hw.OLD_SEEDS + hw.NEW_SEEDS:
        steps = hw.make_walk(seed)
        assert not [s for s in steps if s[0] in hw.NEW_CALLS + ("again", "set_prior")], seed
        assert not [s for s in steps if s[-1] == "direct" or s[:2] == ("refuse", "f64_only_on_f32") or (s[0] == "set_model" and len(s) > 3)], seed


def test_a_walk_is_its_seed():
    for seed in hw.SEEDS:
        a, b = hw.make_walk(seed), hw.make_walk(seed)
        assert a == b and json.loads(json.dumps(a)) == [list(s) for s in a]
    assert hw.make_walk(0) != hw.make_walk(1)


def test_walks_restore_the_option_defaults_and_use_the_whitelist():
    for seed in hw.SEEDS:
        steps = hw.make_walk(seed)
        opts = {}
        for s in steps:
            if s[0] == "option":
                assert s[1] in hw.OPTIONS and s[2] in hw.OPTIONS[s[1]], s
                opts[s[1]] = s[2]
        assert all(opts.get(k, v) == v for k, v in hw.DEFAULTS.items()), opts
        assert 30 <= len(steps) <= 80, len(steps)


# The dry run of the eight new walks takes about two minutes of NumPy expander references and margins in all (seed 14 alone 40 s), so
# profiles/history_walk_checks.md records every seed's smallest margin and the three quickest walks are run here.
# (The eight walks of seeds 16 .. 23 take 0.4 to 4 s each -- their sweeps are named, and few of them are SafeOpt sweeps of a changed
# model; 19, 22 and 23 are the quickest.)
@pytest.mark.parametrize("seed", [9, 10, 13, 19, 22, 23])
def test_dry_run_margins(seed):
    """Walk(None, ...): no engine, references only.  No S / U / M / G / O decision of any sweep (and no trust-region membership)
    lies within 1e-9 (normalised) of its threshold, so a mask that differs on the device is the device's fault.  Seeds 16 ..: the
    references of expander_gain and sample_paths decide every count, witness and index by more than SHARP (the driver raises otherwise)."""
    w = hw.Walk(None, seed, hw.make_walk(seed))
    w.run()
    assert len(w.margins) >= 15 and {"safeopt", "goose", "tr", "robust"} <= {r[1] for r in w.margins}
    worst = min(w.margins, key=lambda r: r[2])
    print("seed", seed, "smallest margin (step, kind, margin):", worst)
    assert worst[2] >= 1e-9, worst
    new = [r for r in w.margins if r[1] in hw.NEW_CALLS]
    if seed in hw.THIRD_SEEDS:
        assert {r[1] for r in new} == set(hw.NEW_CALLS) and min(r[2] for r in new) > hw.SHARP, new
        print("seed", seed, "smallest sharpness of a new step:", min(new, key=lambda r: r[2]))
    else:
        assert not new


def test_twin_models_can_be_told_apart():
    """tests/history_cases.py: B's fp64 lcb_1 lies DELTA from zero at the K picked candidates, A's MARGIN, on the same sides; every
    other decision of B's sweep keeps 100 DELTA, so the rechecked masks of B are the oracle's and its fp32-only masks need not be."""
    m = hc.twin_models()
    A, B, pts, picked, side = m["A"], m["B"], m["pts"], m["picked"], m["side"]
    for k in ("X_norm", "X_mean", "X_std", "Y_mean", "Y_std", "hypopt"):
        assert A[k].shape == B[k].shape and (k.startswith("Y") or A[k].tobytes() == B[k].tobytes()), k
    assert A["Y_norm"].shape == B["Y_norm"].shape and len(picked) == hc.K and (side > 0).sum() >= 4 and (side < 0).sum() >= 4
    ys = max(1.0, float(B["Y_std"][1]))
    sb, sa = oracle.safeopt_sweep(pts, B, hc.B_CONF), oracle.safeopt_sweep(pts, A, hc.B_CONF)
    lb, la = sb["lcb"][:, 1] / ys, sa["lcb"][:, 1] / ys
    assert np.max(np.abs(lb[picked] - side * hc.DELTA)) < 1e-3 * hc.DELTA and np.max(np.abs(la[picked] - side * hc.MARGIN)) < 1e-6
    rest = np.delete(np.arange(len(pts)), picked)
    assert np.min(np.abs(lb[rest])) > 100 * hc.DELTA
    assert np.min(np.abs(sb["lcb"][sb["S"], 0] - sb["u_star"])) / max(1.0, float(B["Y_std"][0])) > 100 * hc.DELTA
    assert sb["S"].sum() > 100 and sb["M"].any() and sa["S"].sum() > 100


def test_the_single_append_the_stale_twin_would_refuse():
    """Sequence a of tests/test_gpu_history.py: x_iso again has a positive pivot on both outputs of the consistent model and a
    pivot far below zero on output 1 of the model its stale twin holds."""
    ds = mb.refusal_model()
    ok = mb.with_rows(ds, ds["X_norm"], ds["Y_norm"])
    x, y = ds["X_norm"][-1][None], np.array([[0.1, 0.2]])
    assert min(float(mb.block_pivots(ok, x, y, o)[0]) for o in range(2)) >= 0.02 and mb.block_pivots(ds, x, y, 1)[0] < -2.0
