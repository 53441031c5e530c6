"""Exact ties and on-threshold candidates in front of every sweep reduction (constructions: tests/tie_cases.py).

The reference of a reduction is its plain NumPy statement -- np.argmax / np.argmin return the FIRST extreme, the reference's rule
(models/SafeOpt.py:119-122, models/GoOSE.py:110-119) -- applied to the posterior the device reduction saw (lean = 0 sweeps, read back
with ``posterior()``).  All comparisons are exact.  A tie test first proves from the read-back posterior that it saw a tie: at
least two candidates inside the reduction's mask hold the extreme bitwise, and the winner is the lowest of them.

Which construction gives which kernel real ties (measured on an MI355X; the "saw a tie" assertions keep it true):
  generic (1), generic chunked (2), K1g (3): the mirror model on a grid -- mirror partners bitwise equal, every reduction a
  two-way tie across tiles, workgroups and ranks -- on the byte-mask set path; generic and chunked also the duplicate list.
  K1b (4), K1i (6), K1t (5): their stored values are not bitwise mirror images, so an exact tie is a near-tie inside the guard
  band there (guard_band 2, guard_passes 2 for SafeOpt and GoOSE, 1 / 1 for TR on every case below); the sweep re-evaluates and
  must return K1g's result on the same model and grid.  The column-word set path exists only behind K1b / K1i (one constraint,
  one rank), so it never sees a bitwise tie of the mirror model: its sweeps end in the guard re-evaluation, whose last pass -- the
  one the profile names -- is on the byte-mask path.  Its own tie cases are the explore_safeset targets behind a column-path sweep.
  (A model that does not depend on the last axis at all -- length scale e^30 there -- was tried with the guard band off: K1b's
  and K1i's columns are still not bitwise constant, so the column kernels' take_max never meets a bitwise tie in this file.)
"""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import oracle  # noqa: E402
import robust_oracle  # noqa: E402
import tie_cases as tc  # noqa: E402
from safebo_amd import synthetic  # noqa: E402
from test_gpu_parity import _free_port, _wait_ranks  # noqa: E402

pytestmark = pytest.mark.gpu

B = 2.0
TR_X0, TR_R = np.array([0.25, 0.0]), 0.75          # a ball centred on the mirror line: T is mirror-symmetric too
TR_X0_3 = np.array([0.25, 0.0, 0.0])
DEFAULTS = {"posterior_path": 0, "bilinear": 1, "tensor_cheb": 1, "col_path": 1, "fuse_classify": -1, "set_fuse": 1, "set_lanes": 1,
            "result_mirror": 1, "scan_waves": 1, "scan_blocks": 1, "list_index": -1, "guard_band": 1}
KERNEL_OPTS = {1: {"posterior_path": 1}, 2: {"posterior_path": 2}, 3: {"bilinear": 0, "tensor_cheb": 0},
               4: {"bilinear": 2}, 6: {"bilinear": 1}, 5: {}}


@contextlib.contextmanager
def options(engine, **kv):
    """Engine options for the block, every one restored to its default afterwards."""
    try:
        for k, v in kv.items():
            engine.set_option(k, v)
        yield
    finally:
        for k in kv:
            engine.set_option(k, DEFAULTS[k])


def _lcb0(mean, var, b):
    return oracle.bounds(mean.astype(np.float64), var.astype(np.float64), b)[0][:, 0]


def _first_min(values, mask):
    return int(np.argmin(np.where(mask, values, np.inf))) if mask.any() else -1


def _first_max(values, mask):
    return int(np.argmax(np.where(mask, values, -np.inf))) if mask.any() else -1


def saw_tie(values, mask, winner, what):
    """The proof that a reduction was given a tie: >= 2 candidates inside the mask hold the winner's value bitwise, and the
    winner is the lowest of them."""
    t = tc.tied(values, mask, winner)
    print(f"[tie] {what}: winner {winner}, tied {t[:6].tolist()} ({t.size})")
    assert t.size >= 2, (what, "no tie in front of this reduction", winner)
    assert winner == int(t[0]), (what, winner, t[:6])
    return t


def bundle(engine, ds, b, dtype="f64", lean=0, tr=None, goose=True, use_invK=True):
    """SafeOpt on a fresh posterior of the resident candidates (the posterior kernel runs inside the sweep), then GoOSE and the
    trust-region sweep on that resident posterior: results, masks, the read-back posterior, kernel and set path."""
    q = ds["Y_norm"].shape[1]
    engine.set_model(ds, dtype=dtype, use_invK=use_invK)
    s = engine.sweep_safeopt(b, want_masks=True, lean=lean)
    prof = engine.profile()
    out = {"s": s, "kernel": prof["posterior_kernel"], "set_path": prof["set_path"], "q": q, "b": b}
    masks = {k: engine.mask(k) for k in ("S", "U", "M")}
    masks.update({f"G{c}": engine.mask("G", c) for c in range(1, q)})
    if not lean:
        out["mean"], out["var"] = engine.posterior()
    if goose and q > 1:
        out["g"] = engine.sweep_goose(b, want_masks=True, posterior_ready=not lean)
        masks.update({f"O{c}": engine.mask("O", c) for c in range(1, q)})
        masks["S_g"] = engine.mask("S")
    if tr is not None:
        out["t"] = engine.sweep_tr(b, tr[0], tr[1], posterior_ready=not lean)
    out["masks"] = masks
    return out


def check_reductions(bn, pts, ties=(), tr=None):
    """Every index field of the bundle against the NumPy statement of its reduction on the device's posterior and masks.
    ``ties``: the reductions that must have seen a tie."""
    mean, var, m, q, b = bn["mean"], bn["var"], bn["masks"], bn["q"], bn["b"]
    var0 = var[:, 0].astype(np.float64)
    lcb0 = _lcb0(mean, var, b)
    s = bn["s"]
    assert s["minimizer_index"] == _first_max(var0, m["M"])
    assert (s["count_S"], s["count_U"], s["count_M"]) == (m["S"].sum(), m["U"].sum(), m["M"].sum())
    if "minimizer" in ties:
        saw_tie(var0, m["M"], s["minimizer_index"], "minimizer")
    e_idx = [_first_max(var0, m[f"G{c}"]) for c in range(1, q)]
    assert list(s["expander_index_c"]) == e_idx and list(s["count_G"]) == [m[f"G{c}"].sum() for c in range(1, q)]
    e_std = np.array([np.sqrt(var0[e]) if e >= 0 else -np.inf for e in e_idx])
    best = int(np.argmax(e_std)) + 1 if any(e >= 0 for e in e_idx) else 0      # first maximum (models/SafeOpt.py:119-122)
    assert s["expander_best_c"] == best and s["expander_index"] == (e_idx[best - 1] if best else -1)
    assert s["choose_minimizer"] == bool(np.sqrt(var0[s["minimizer_index"]]) > (e_std[best - 1] if best else 0.0))
    if "expander" in ties:
        assert any(e >= 0 for e in e_idx), "no expander set to tie in"
        for c in range(1, q):
            if e_idx[c - 1] >= 0:
                saw_tie(var0, m[f"G{c}"], e_idx[c - 1], f"expander {c}")
    if "g" in bn:
        g = bn["g"]
        assert np.array_equal(m["S_g"], m["S"])
        assert g["safe_min_index"] == _first_min(lcb0, m["S"])
        t_idx = [_first_min(lcb0, m[f"O{c}"]) for c in range(1, q)]
        assert list(g["target_index_c"]) == t_idx and list(g["count_O"]) == [m[f"O{c}"].sum() for c in range(1, q)]
        t_lcb = np.array([lcb0[t] if t >= 0 else np.inf for t in t_idx])
        tbest = int(np.argmin(t_lcb)) + 1 if any(t >= 0 for t in t_idx) else 0   # first minimum (models/GoOSE.py:110-112)
        assert g["target_best_c"] == tbest and g["target_index"] == (t_idx[tbest - 1] if tbest else -1)
        if tbest:
            assert g["explore_index"] == tc.nearest_in(pts, m["S"], pts[g["target_index"]])[0]
            assert g["choose_safe_min"] == bool(lcb0[g["safe_min_index"]] <= t_lcb[tbest - 1])
        if "safe_min" in ties:
            saw_tie(lcb0, m["S"], g["safe_min_index"], "safe minimum")
        if "target" in ties:
            assert tbest, "no optimistic set to tie in"
            for c in range(1, q):
                if t_idx[c - 1] >= 0:
                    saw_tie(lcb0, m[f"O{c}"], t_idx[c - 1], f"target {c}")
    if "t" in bn:
        dist = np.sqrt(((pts - tr[0]) ** 2).sum(axis=1))
        T = m["S"] & (dist <= tr[1])
        assert bn["t"]["index"] == _first_min(lcb0, T) and bn["t"]["count_T"] == T.sum() and bn["t"]["count_S"] == m["S"].sum()
        if "tr" in ties:
            saw_tie(lcb0, T, bn["t"]["index"], "trust region")


def check_oracle_masks(bn, pts, ds, tr=None):
    """Masks and indices against the oracle's sweeps on the device's posterior (small candidate sets: brute-force expanders)."""
    mv = (bn["mean"].astype(np.float64), bn["var"].astype(np.float64))
    ref = oracle.safeopt_sweep(pts, ds, bn["b"], mean_var=mv)
    m, q = bn["masks"], bn["q"]
    for k in ("S", "U", "M"):
        assert np.array_equal(m[k], ref[k]), k
    for c in range(1, q):
        assert np.array_equal(m[f"G{c}"], ref["G"][c - 1]), f"G{c}"
    s = bn["s"]
    assert s["minimizer_index"] == ref["minimizer_index"] and list(s["expander_index_c"]) == list(ref["expander_index"])
    assert s["expander_best_c"] == ref["expander_best"] and s["expander_index"] == ref["expander_best_index"]
    assert s["choose_minimizer"] == ref["choose_minimizer"]
    if "g" in bn:
        gref = oracle.goose_sweep(pts, ds, bn["b"], mean_var=mv)
        g = bn["g"]
        for c in range(1, q):
            assert np.array_equal(m[f"O{c}"], gref["O"][c - 1]), f"O{c}"
        assert g["safe_min_index"] == gref["safe_min_index"] and list(g["target_index_c"]) == list(gref["target_index_c"])
        assert g["target_best_c"] == gref["target_best"] and g["target_index"] == gref["target_index"]
        assert g["explore_index"] == gref["explore_index"] and g["choose_safe_min"] == gref["choose_safe_min"]
    if "t" in bn:
        tref = oracle.tr_sweep(pts, ds, bn["b"], tr[0], tr[1], mean_var=mv)
        assert bn["t"]["index"] == tref["index"] and bn["t"]["count_T"] == tref["T"].sum()


ALL_TIES = ("minimizer", "expander", "safe_min", "target", "tr")
INDEX_KEYS = {"s": ("minimizer_index", "expander_index_c", "expander_best_c", "expander_index", "choose_minimizer", "count_S", "count_U",
                    "count_M", "count_G"),
              "g": ("safe_min_index", "target_index_c", "target_best_c", "target_index", "explore_index", "choose_safe_min", "count_O"),
              "t": ("index", "count_T", "count_S")}


def same_indices(a, b_):
    for part, keys in INDEX_KEYS.items():
        if part in a or part in b_:
            for k in keys:
                assert np.array_equal(np.asarray(a[part][k]), np.asarray(b_[part][k])), (part, k, a[part][k], b_[part][k])
    for k, v in a["masks"].items():
        assert np.array_equal(v, b_["masks"][k]), k


# ------------------------------------------------------------------------------------- mirror model, exact kernels, byte-mask path
@pytest.mark.parametrize("kernel", [1, 2, 3])
@pytest.mark.parametrize("grid,q,same", [("small", 2, False), ("even", 3, False), ("small", 3, True)])
def test_mirror_model_exact_kernels(engine, kernel, grid, q, same):
    """SafeOpt, GoOSE and TR on the mirror model through the generic (1), the chunked generic (2) and the separable-table kernel
    K1g (3): mirror partners are bitwise equal, so the minimiser, every expander, the safe minimum, every target and the
    trust-region winner are two-way ties across tiles and workgroups, and the lower flat index must win.  q = 3 with identical
    constraints: G_1 == G_2 and O_1 == O_2, both expanders / targets are one candidate, expander_best_c = target_best_c = 1."""
    ds = tc.mirror_model(q=q, same_constraints=same)
    lo, hi, count = tc.mirror_grid(grid)
    pts = oracle.grid_points(lo, hi, count)
    with options(engine, **KERNEL_OPTS[kernel]):
        engine.set_grid(lo, hi, count)
        bn = bundle(engine, ds, B, tr=(TR_X0, TR_R))
    assert bn["kernel"] == kernel and bn["set_path"] == 0
    plane = count[0]
    for a in (bn["mean"], bn["var"]):
        a3 = a.reshape(count[1], plane, q)
        assert np.array_equal(a3, a3[::-1]), "mirror partners are not bitwise equal under this kernel"
    check_reductions(bn, pts, ties=ALL_TIES, tr=(TR_X0, TR_R))
    check_oracle_masks(bn, pts, ds, tr=(TR_X0, TR_R))
    if same:
        assert np.array_equal(bn["masks"]["G1"], bn["masks"]["G2"]) and np.array_equal(bn["masks"]["O1"], bn["masks"]["O2"])
        assert bn["s"]["expander_index_c"][0] == bn["s"]["expander_index_c"][1] and bn["s"]["expander_best_c"] == 1
        assert bn["g"]["target_index_c"][0] == bn["g"]["target_index_c"][1] and bn["g"]["target_best_c"] == 1


@pytest.mark.parametrize("opts,q", [({"set_fuse": 0}, 2), ({"set_fuse": 0}, 3), ({"result_mirror": 0}, 2), ({"result_mirror": 0}, 3),
                                    ({"set_lanes": 0}, 3)])
def test_mirror_model_set_phase_options(engine, opts, q):
    """What a small grid (65 x 32) reaches of the set phase's launch variants, on K1g's bitwise-symmetric posterior: the minimiser
    not deferred into the first constraint's launch (set_fuse 0), no mirrored result block, and one lane for two constraints
    (set_lanes needs q >= 3).  The same tied reductions, the same lowest-index winners, masks against the oracle.  (scan_waves,
    scan_blocks and the shared launches are behind size gates: test_mirror_model_large_grid_set_phase_options.)"""
    ds = tc.mirror_model(q=q)
    lo, hi, count = tc.mirror_grid("even")
    pts = oracle.grid_points(lo, hi, count)
    with options(engine, **KERNEL_OPTS[3], **opts):
        engine.set_grid(lo, hi, count)
        bn = bundle(engine, ds, B, tr=(TR_X0, TR_R))
    assert bn["kernel"] == 3 and bn["set_path"] == 0
    check_reductions(bn, pts, ties=ALL_TIES, tr=(TR_X0, TR_R))
    check_oracle_masks(bn, pts, ds, tr=(TR_X0, TR_R))


@pytest.mark.parametrize("opts,q", [({"scan_waves": 0}, 2), ({"scan_blocks": 0}, 2), ({"set_fuse": 0}, 2), ({"result_mirror": 0}, 2),
                                    ({"scan_waves": 0, "scan_blocks": 0}, 2), ({"set_lanes": 0}, 3), ({"scan_waves": 0}, 3),
                                    ({"scan_blocks": 0}, 3), ({"set_fuse": 0}, 3)])
def test_mirror_model_large_grid_set_phase_options(engine, opts, q):
    """1024 x 128, the mirror model, K1g: large enough for every size gate of the expander and GoOSE set phase -- the window has
    2^17 >= 2^16 candidates and >= 32 points per axis (coarse transform), 128 coarse columns and count0 >= 128 (the shared
    launches set_fuse switches), a last axis of 128 = 4 x 32 (block minima, scan_blocks; the 16-bit image and the list scan,
    scan_waves), count0 >= 512 (GoOSE's axis-0 blocks).  Each option at its non-default value must see the same tied reductions
    and return the lowest-index winners, and every mask and index of the default launch order."""
    ds = tc.mirror_model(q=q)
    lo, hi, count = tc.mirror_grid("wide")
    pts = oracle.grid_points(lo, hi, count)
    out = {}
    for key, o in (("default", {}), ("opt", opts)):
        with options(engine, **KERNEL_OPTS[3], **o):
            engine.set_grid(lo, hi, count)
            out[key] = bundle(engine, ds, B, tr=(TR_X0, TR_R))
        assert out[key]["kernel"] == 3 and out[key]["set_path"] == 0
        check_reductions(out[key], pts, ties=ALL_TIES, tr=(TR_X0, TR_R))
    m = out["opt"]["masks"]
    assert all(m[f"G{c}"].any() and m[f"O{c}"].any() for c in range(1, q)) and m["U"].any()
    same_indices(out["opt"], out["default"])


def test_mirror_model_large_grid_byte_mask_path(engine):
    """1024 x 1024 (the scans, block minima and shared launches of the large-grid set phase are on), K1g: every reduction tied
    across the two halves of the grid."""
    ds = tc.mirror_model(q=2)
    lo, hi, count = tc.mirror_grid("column")
    pts = oracle.grid_points(lo, hi, count)
    with options(engine, **KERNEL_OPTS[3]):
        engine.set_grid(lo, hi, count)
        bn = bundle(engine, ds, B, tr=(TR_X0, TR_R))
    assert bn["kernel"] == 3 and bn["set_path"] == 0
    check_reductions(bn, pts, ties=ALL_TIES, tr=(TR_X0, TR_R))


# ------------------------------------------------------------------------------ approximating posteriors and the column-word path
@pytest.mark.parametrize("grid", ["tiles", "column"])
@pytest.mark.parametrize("kernel,col", [(4, 0), (4, 2), (6, 0), (6, 2)])
def test_mirror_model_approximating_kernels_equal_k1g(engine, grid, kernel, col):
    """K1b (4) and K1i (6) on the mirror model, byte-mask (col_path 0) and column-word set path (col_path 2, one constraint):
    their stored values are not bitwise mirror images, so K1g's exact ties are near-ties inside the guard band here, and the
    sweep must re-evaluate and return K1g's result -- every index and mask (K1g itself is pinned to NumPy above).  Measured on
    an MI355X: see the printed guard_band / guard_passes (a run with guard_band = 0 and winners different from K1g's is the bug
    this test exists for).  NumPy's reductions on the read-back posterior hold as well."""
    ds = tc.mirror_model(q=2)
    lo, hi, count = tc.mirror_grid(grid)
    pts = oracle.grid_points(lo, hi, count)
    with options(engine, **KERNEL_OPTS[3]):
        engine.set_grid(lo, hi, count)
        ref = bundle(engine, ds, B, tr=(TR_X0, TR_R))
    assert ref["kernel"] == 3
    check_reductions(ref, pts, ties=ALL_TIES, tr=(TR_X0, TR_R))
    with options(engine, fuse_classify=1, col_path=col, **KERNEL_OPTS[kernel]):
        engine.set_grid(lo, hi, count)
        bn = bundle(engine, ds, B, tr=(TR_X0, TR_R))
    print(f"[tie] kernel {bn['kernel']} set_path {bn['set_path']}: guard_band {bn['s']['guard_band']} passes {bn['s']['guard_passes']}; "
          f"goose {bn['g']['guard_band']}/{bn['g']['guard_passes']}; tr {bn['t']['guard_band']}/{bn['t']['guard_passes']}")
    # (behind a guard re-evaluation the profile names the sweep's last pass: the byte-mask path, and for K1i possibly the K1b plan)
    if bn["s"]["guard_passes"] == 0:
        assert bn["kernel"] == kernel and bn["set_path"] == (1 if col else 0)
    else:
        assert bn["kernel"] in ((4,) if kernel == 4 else (4, 6)) and bn["set_path"] in ((0, 1) if col else (0,))
    same_indices(bn, ref)


def test_mirror_model_3d_k1t_equals_k1g(engine):
    """The 3-D mirror model (mirrored in the last axis) on 128 x 128 x 256 candidates: K1g gives bitwise mirror images and tied
    reductions; the Chebyshev-node interpolation K1t (5) must return K1g's indices and masks."""
    ds = tc.mirror_model(q=2, d=3, n=40)
    lo, hi, count = tc.mirror_grid("cube_k1t")
    pts = oracle.grid_points(lo, hi, count)
    with options(engine, **KERNEL_OPTS[3]):
        engine.set_grid(lo, hi, count)
        ref = bundle(engine, ds, B, tr=(TR_X0_3, TR_R))
    assert ref["kernel"] == 3
    check_reductions(ref, pts, ties=ALL_TIES, tr=(TR_X0_3, TR_R))
    engine.set_grid(lo, hi, count)
    bn = bundle(engine, ds, B, tr=(TR_X0_3, TR_R))
    print(f"[tie] K1t: guard_band {bn['s']['guard_band']} passes {bn['s']['guard_passes']}; goose {bn['g']['guard_band']}/"
          f"{bn['g']['guard_passes']}; tr {bn['t']['guard_band']}/{bn['t']['guard_passes']}")
    assert bn["kernel"] == 5
    same_indices(bn, ref)


def test_mirror_model_3d_small_exact(engine):
    """The 3-D mirror model on a small grid through K1g and the generic kernel, against the oracle's sweeps."""
    ds = tc.mirror_model(q=2, d=3, n=40)
    lo, hi, count = tc.mirror_grid("cube_small")
    pts = oracle.grid_points(lo, hi, count)
    for kernel in (3, 1):
        with options(engine, **{**KERNEL_OPTS[3], **KERNEL_OPTS[kernel]}):
            engine.set_grid(lo, hi, count)
            bn = bundle(engine, ds, B, tr=(TR_X0_3, TR_R))
        assert bn["kernel"] == kernel
        check_reductions(bn, pts, ties=("minimizer", "safe_min", "tr"), tr=(TR_X0_3, TR_R))
        check_oracle_masks(bn, pts, ds, tr=(TR_X0_3, TR_R))


# ----------------------------------------------------------------------------------------------------------------- lean levels
@pytest.mark.parametrize("kernel,col", [(3, 0), (4, 0), (4, 2)])
def test_mirror_model_lean_levels_return_the_same_indices(engine, kernel, col):
    """lean = 0, 1, 2 on the mirror model (lean 2 from the plan's second sweep on): the same indices, counts and masks."""
    ds = tc.mirror_model(q=2)
    lo, hi, count = tc.mirror_grid("tiles")
    out = []
    with options(engine, fuse_classify=1, col_path=col, **KERNEL_OPTS[kernel]):
        engine.set_grid(lo, hi, count)
        engine.set_model(ds)
        for lean in (0, 0, 1, 2, 2):
            s = engine.sweep_safeopt(B, want_masks=True, lean=lean)
            prof = engine.profile()
            assert prof["posterior_kernel"] == kernel
            # (the mirror model's near-ties send the approximating kernel's sweep through a guard re-evaluation, whose last pass
            # -- the one the profile names -- is on the byte-mask path)
            assert prof["set_path"] in (0, 1) if col and s["guard_passes"] else prof["set_path"] == (1 if col else 0)
            out.append((s, {k: engine.mask(k) for k in ("S", "U", "M")}, engine.mask("G", 1)))
            if len(out) == 1 and kernel == 3:
                # the proof that these sweeps reduce over ties (K1g; behind K1b they are the guard band's near-ties)
                var0 = engine.posterior()[1][:, 0]
                saw_tie(var0, out[0][1]["M"], s["minimizer_index"], "minimizer")
                saw_tie(var0, out[0][2], int(s["expander_index_c"][0]), "expander 1")
    for s, m, G in out[1:]:
        for k in INDEX_KEYS["s"]:
            assert np.array_equal(np.asarray(s[k]), np.asarray(out[0][0][k])), k
        assert all(np.array_equal(m[k], out[0][1][k]) for k in m) and np.array_equal(G, out[0][2])


# ------------------------------------------------------------------------------------------------------------------------ b = 0
@pytest.mark.parametrize("kernel", [1, 3])
def test_b_zero_on_the_mirror_model(engine, kernel):
    """b = 0: ucb = lcb = mean, u* = min_S mean_0 and M = {g in S : mean_0(g) == u*} is itself a tie set -- on the mirror grid
    without a centre row it has an even number of members, and the minimiser is the lower one."""
    ds = tc.mirror_model(q=2)
    lo, hi, count = tc.mirror_grid("even")
    pts = oracle.grid_points(lo, hi, count)
    with options(engine, **KERNEL_OPTS[kernel]):
        engine.set_grid(lo, hi, count)
        bn = bundle(engine, ds, 0.0, tr=(TR_X0, TR_R))
    assert bn["kernel"] == kernel
    M = bn["masks"]["M"]
    mean0 = bn["mean"][:, 0]
    assert M.sum() >= 2 and M.sum() % 2 == 0 and np.all(mean0[M] == mean0[M][0]) and bn["s"]["u_star"] == mean0[M][0]
    assert np.array_equal(M, bn["masks"]["S"] & (mean0 == mean0[bn["masks"]["S"]].min()))
    check_reductions(bn, pts, ties=("minimizer", "safe_min", "tr"), tr=(TR_X0, TR_R))
    check_oracle_masks(bn, pts, ds, tr=(TR_X0, TR_R))


def test_b_zero_on_a_random_config(engine):
    """b = 0 on a BASELINE-style random config (C, two constraints): masks and indices against the oracle on the device's posterior."""
    cfg = synthetic.make_config("C", n=64)
    lo, hi, count = cfg["bound"][:, 0], cfg["bound"][:, 1], [48, 40]
    pts = oracle.grid_points(lo, hi, count)
    with options(engine, **KERNEL_OPTS[3]):
        engine.set_grid(lo, hi, count)
        x0 = 0.5 * (lo + hi)
        r = 0.3 * float(np.min(hi - lo))
        bn = bundle(engine, cfg["ds"], 0.0, tr=(x0, r))
    assert bn["kernel"] == 3
    check_reductions(bn, pts, tr=(x0, r))
    check_oracle_masks(bn, pts, cfg["ds"], tr=(x0, r))
    assert bn["masks"]["M"].any() and bn["masks"]["U"].any()


# --------------------------------------------------------------------------------------------------------------- duplicate lists
@pytest.mark.parametrize("list_index", [0, 1])
@pytest.mark.parametrize("pdtype", [np.float64, np.float32])
@pytest.mark.parametrize("kernel", [1, 2])
def test_duplicate_list(engine, list_index, pdtype, kernel):
    """An explicit list whose every point appears three times at scattered positions (fp64 and fp32 points, with and without the
    spatial index): the generic kernels give the repeats bitwise-equal values, so every reduction is a three-way tie and the
    lowest position must win; masks against the oracle.  (Model: the mirror model with two constraints, as a plain smooth model.)"""
    ds = tc.mirror_model(q=3)
    pts, origin = tc.duplicate_list([-1.0, -1.0], [1.0, 1.0], m=1500, dtype=pdtype)
    with options(engine, list_index=list_index, **KERNEL_OPTS[kernel]):
        engine.set_points(pts)
        bn = bundle(engine, ds, B, tr=(TR_X0, TR_R))
    assert bn["kernel"] == kernel
    p64 = pts.astype(np.float64)
    first = np.full(origin.max() + 1, -1)
    first[origin[::-1]] = np.arange(origin.size)[::-1]          # the lowest position of every base point
    for a in (bn["mean"], bn["var"]):
        assert np.array_equal(a, a[first[origin]]), "repeats of a point are not bitwise equal under this kernel"
    check_reductions(bn, p64, ties=ALL_TIES, tr=(TR_X0, TR_R))
    for part, k in (("s", "minimizer_index"), ("g", "safe_min_index"), ("t", "index")):
        assert (origin == origin[bn[part][k]]).sum() == 3 and bn[part][k] == first[origin[bn[part][k]]]
    check_oracle_masks(bn, p64, ds, tr=(TR_X0, TR_R))


# ------------------------------------------------------------------------------------------------------------ explore_safeset
def _explore_all(engine, pts, S, targets):
    for name, (t, nearest) in targets.items():
        want, dist = tc.nearest_in(pts, S, t)
        idx, x = engine.explore_safeset(t)
        tied = np.flatnonzero(S & (dist == dist[want]))
        print(f"[tie] explore {name}: got {idx}, want {want}, tied {tied.tolist()}")
        assert idx == want and np.array_equal(x, pts[idx]), (name, idx, want)
        yield name, want, tied, nearest


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["grid", "list"])
def test_explore_safeset_cell_centre_targets(engine, dtype, kind):
    """explore_safeset with targets at a cell centre (four equidistant corners), at edge midpoints (two) and on a grid point, on a
    dyadic grid and on the same points as a list, fp64 and fp32 models; q = 1, so S is every candidate.  The lowest flat index of
    the tied corners must be returned."""
    lo, hi, count, targets = tc.cell_targets()
    pts = oracle.grid_points(lo, hi, count)
    ds = tc.flat_model()
    if kind == "grid":
        engine.set_grid(lo, hi, count)
    else:
        engine.set_points(pts)
    engine.set_model(ds, dtype=dtype, use_invK=(dtype == "f64"))
    engine.sweep_safeopt(B)
    S = np.ones(pts.shape[0], dtype=bool)
    for name, want, tied, nearest in _explore_all(engine, pts, S, targets):
        assert tied.tolist() == nearest and want == nearest[0], (name, tied, nearest)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_explore_safeset_lowest_tied_corner_unsafe(engine, dtype):
    """The cell-centre target whose two lowest-index corners are unsafe (grid column 11 is outside S): the arg-min runs over S
    only, and of the two remaining tied corners the lower one wins."""
    lo, hi, count, targets = tc.cell_targets()
    pts = oracle.grid_points(lo, hi, count)
    ds = tc.corner_model()
    with options(engine, **KERNEL_OPTS[3]):
        engine.set_grid(lo, hi, count)
        engine.set_model(ds, dtype=dtype, use_invK=(dtype == "f64"))
        engine.sweep_safeopt(0.0, want_masks=True)
        S = engine.mask("S")
        t, nearest = targets["centre"]
        assert not S[nearest[0]] and not S[nearest[2]] and S[nearest[1]] and S[nearest[3]]
        for name, want, tied, _ in _explore_all(engine, pts, S, {"centre": targets["centre"]}):
            assert tied.tolist() == [nearest[1], nearest[3]] and want == nearest[1]


def test_explore_safeset_after_a_column_path_sweep(engine):
    """explore_safeset behind a column-path sweep expands the safe set from the column words (cbS).  Config B on a dyadic grid
    (steps 2^-7): targets at the centre of a cell with four safe corners (four-way tie), at the midpoint of a safe edge (two-way),
    and at the centre of a cell whose two lowest-index corners are unsafe."""
    cfg = synthetic.make_config("B", n=96)
    lo, count = np.array([-0.5, -1.0]), [256, 128]
    hi = lo + (np.array(count) - 1) * 2.0 ** -7
    pts = oracle.grid_points(lo, hi, count)
    ax0, ax1 = oracle.grid_axes(lo, hi, count)
    with options(engine, fuse_classify=1, col_path=2):
        engine.set_grid(lo, hi, count)
        engine.set_model(cfg["ds"])
        engine.sweep_safeopt(cfg["b"], want_masks=True)
        assert engine.profile()["set_path"] == 1
        S = engine.mask("S")
        S2 = S.reshape(count[1], count[0])
        full = S2[:-1, :-1] & S2[:-1, 1:] & S2[1:, :-1] & S2[1:, 1:]
        half = ~S2[:-1, :-1] & S2[:-1, 1:] & ~S2[1:, :-1] & S2[1:, 1:]
        assert full.any() and half.any()
        jf, i_f = [int(v[v.size // 2]) for v in np.nonzero(full)]
        jh, ih = [int(v[0]) for v in np.nonzero(half)]
        targets = {"centre": (np.array([ax0[i_f] + 2.0 ** -8, ax1[jf] + 2.0 ** -8]), None),
                   "edge": (np.array([ax0[i_f] + 2.0 ** -8, ax1[jf]]), None),
                   "half_safe": (np.array([ax0[ih] + 2.0 ** -8, ax1[jh] + 2.0 ** -8]), None)}
        seen = {}
        for name, want, tied, _ in _explore_all(engine, pts, S, targets):
            seen[name] = tied
            assert want == int(tied[0])
        assert seen["centre"].size == 4 and seen["edge"].size == 2 and seen["half_safe"].size == 2
        assert seen["half_safe"].tolist() == [jh * count[0] + ih + 1, (jh + 1) * count[0] + ih + 1]


# ------------------------------------------------------------------------------------------------------- on-sphere trust region
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_trust_region_counts_the_points_on_its_sphere(engine, dtype):
    """x_0 a lattice point, spacing h = 2^-5, r = 5 h: the twelve Pythagorean lattice points are at distance exactly r and belong
    to the ball (NonlinearConstraint(norm(x - x_0), 0, r), models/GP_TR.py:43-51); r = nextafter(5 h, 0) excludes exactly them."""
    lo, hi, count, x0, r, r_below, on = tc.sphere_case()
    pts = oracle.grid_points(lo, hi, count)
    dist = np.sqrt(((pts - x0) ** 2).sum(axis=1))
    ds = tc.flat_model()
    engine.set_grid(lo, hi, count)
    engine.set_model(ds, dtype=dtype, use_invK=(dtype == "f64"))
    engine.sweep_safeopt(B)
    mean, var = engine.posterior()
    t_in = engine.sweep_tr(B, x0, r, posterior_ready=True)
    t_out = engine.sweep_tr(B, x0, r_below, posterior_ready=True)
    assert t_in["count_T"] == (dist <= r).sum() and t_out["count_T"] == (dist <= r_below).sum()
    assert t_in["count_T"] - t_out["count_T"] == len(on) == 12
    # (an fp32 model's sweep is rechecked in fp64: its winner is the fp64 oracle's)
    lcb0 = _lcb0(mean, var, B) if dtype == "f64" else _lcb0(*oracle.gp_inference(pts, ds), B)
    assert t_in["index"] == _first_min(lcb0, dist <= r) and t_out["index"] == _first_min(lcb0, dist <= r_below)


# ---------------------------------------------------------------------------------------------------------------- fp32 near-tie
def test_fp32_explore_distance_is_compared_in_double(engine):
    """Two safe candidates at fp64 distances 1.0 (index 0) and 0.99999999 (last index) from the target, everything else farther:
    the distances collide when rounded to fp32.  An fp32 model's explore step must still return the nearer point -- the fp64
    arg-min, as for an fp64 model (README: fp32 models get fp64-exact masks and indices).  On the parent commit the fp32 model's
    arg-min ran on distances rounded to float and returned index 0 here."""
    pts, target, near, far = tc.near_tie_list()
    ds = tc.flat_model()
    lo, hi, count, tg, gnear, gfar = tc.near_tie_grid()
    for dtype in ("f64", "f32"):
        engine.set_points(pts)
        engine.set_model(ds, dtype=dtype, use_invK=(dtype == "f64"))
        engine.sweep_safeopt(B)
        idx, x = engine.explore_safeset(target)
        print(f"[tie] near-tie list, {dtype} model: explore {idx}, fp64 arg-min {near}, fp32-rounded arg-min {far}")
        assert idx == near and np.array_equal(x, pts[near]), (dtype, idx, near)
        engine.set_grid(lo, hi, count)
        engine.set_model(ds, dtype=dtype, use_invK=(dtype == "f64"))
        engine.sweep_safeopt(B)
        idx, x = engine.explore_safeset(tg)
        print(f"[tie] near-tie grid, {dtype} model: explore {idx}, fp64 arg-min {gnear}, fp32-rounded arg-min {gfar}")
        assert idx == gnear, (dtype, idx, gnear)


def test_fp32_goose_sweep_explore_step_near_tie(engine):
    """A full GoOSE sweep of an fp32 model whose target (the one unsafe candidate, the origin) has two safe candidates at fp64
    distances 1.0 (index 0) and 0.99999999 (last index): every index must be the fp64 oracle's, explore_index the nearer one."""
    ds, b, pts, t, near, far = tc.near_tie_goose()
    gref = oracle.goose_sweep(pts, ds, b)
    assert gref["target_index"] == t and gref["explore_index"] == near
    for dtype in ("f64", "f32"):
        engine.set_points(pts)
        engine.set_model(ds, dtype=dtype, use_invK=(dtype == "f64"))
        g = engine.sweep_goose(b, want_masks=True)
        print(f"[tie] near-tie GoOSE, {dtype} model: target {g['target_index']} explore {g['explore_index']} (fp64 {near}, fp32-rounded {far})")
        assert np.array_equal(engine.mask("S"), gref["S"]) and np.array_equal(engine.mask("O", 1), gref["O"][0])
        assert g["safe_min_index"] == gref["safe_min_index"] and g["target_index"] == t
        assert g["explore_index"] == near, (dtype, g["explore_index"], near)


# ------------------------------------------------------------------------------------------------------------------------ robust
@pytest.mark.parametrize("axis", [1, 0])
@pytest.mark.parametrize("kind", ["ucb", "mean"])
def test_robust_sweep_ties(engine, axis, kind):
    """sbo_sweep_robust on the mirror model.  Mirrored in the disturbance axis (axis 1): max_d of the objective's bound is reached
    on two disturbance planes, worst_d_index must be the lower.  Mirrored in the control axis (axis 0): two control points have
    bitwise-equal max_d, index must be the lower.  Reference: robust_oracle on the read-back posterior and arrays."""
    ds = tc.mirror_model(q=2, axis=axis)
    lo, hi, count = tc.robust_mirror_grid(axis)
    nc = count[0]
    with options(engine, **KERNEL_OPTS[3]):
        engine.set_model(ds, mean_prior=np.zeros(2))
        engine.set_grid(lo, hi, count)
        res = engine.sweep_robust(B, 1, kind)
        assert engine.profile()["posterior_kernel"] == 3
        f, g = engine.robust_arrays()
        mean, var = engine.posterior()
    r = robust_oracle.robust_from_posterior(mean, var, nc, B, kind)
    assert np.array_equal(f, r["f"]) and np.array_equal(g, r["g"])
    assert res["count_safe"] == r["count_safe"] > 0
    f_all = robust_oracle.bound_of(mean[:, 0], var[:, 0], B, kind).reshape(count[1], nc)
    if axis == 1:
        col = f_all[:, r["index"]]
        saw_tie(col, np.ones(count[1], dtype=bool), r["worst_d_index"], "worst disturbance")
    else:
        saw_tie(r["f"], r["safe"], r["index"], "robust control")
    assert (res["index"], res["worst_d_index"], res["candidate_index"]) == (r["index"], r["worst_d_index"], r["candidate_index"])
    assert res["value"] == r["value"]


# -------------------------------------------------------------------------------------------------------------------- multi-rank
def _spawn(worker, world, args_of):
    port = _free_port()
    return [subprocess.Popen([sys.executable, os.path.join(HERE, worker), str(r), str(world), port] + args_of(r)) for r in range(world)]


@pytest.mark.parametrize("world", [2, 3])
def test_multi_rank_mirror_model_equals_single_rank(engine, tmp_path, world):
    """The mirror model on 64 x 33 candidates sharded over 2 and 3 ranks (uneven plane counts): the mirrored axis is the sharded
    one, so the two tied winners of every reduction live on different ranks, and the host merge of the per-rank rows must keep the
    lower flat index.  SafeOpt, GoOSE with its explore step and TR: field by field the single-rank result of the same grid."""
    q = 3
    ds = tc.mirror_model(q=q)
    lo, hi, count = tc.mirror_grid("planes33")
    pts = oracle.grid_points(lo, hi, count)
    out = str(tmp_path / "res.json")
    procs = _spawn("_gpu_rank_worker.py", world, lambda r: [out, f"tie:planes33:{q}", "24", json.dumps(count), str(B)])
    try:
        with options(engine, **KERNEL_OPTS[3]):
            engine.set_grid(lo, hi, count)
            ref = bundle(engine, ds, B, tr=(TR_X0, TR_R))
        check_reductions(ref, pts, ties=ALL_TIES, tr=(TR_X0, TR_R))
    except BaseException:
        for p in procs:
            p.kill()
            p.wait()
        raise
    assert _wait_ranks(procs) == [0] * world
    res = json.load(open(out))
    parts = [np.load(out + f".rank{r}.npz") for r in range(world)]
    assert res["posterior_kernel"] == 3
    plane = count[0]
    assert [(int(p["first"]) // plane, (int(p["first"]) + int(p["n_local"])) // plane) for p in parts] == tc.plane_shards(count, world)
    # the tied winners of every reduction are on different ranks
    var0, lcb0 = ref["var"][:, 0], _lcb0(ref["mean"], ref["var"], B)
    dist = np.sqrt(((pts - TR_X0) ** 2).sum(axis=1))
    slots = [(var0, ref["masks"]["M"], ref["s"]["minimizer_index"]), (lcb0, ref["masks"]["S"], ref["g"]["safe_min_index"]),
             (lcb0, ref["masks"]["S"] & (dist <= TR_R), ref["t"]["index"])]
    for c in range(1, q):
        slots += [(var0, ref["masks"][f"G{c}"], ref["s"]["expander_index_c"][c - 1]), (lcb0, ref["masks"][f"O{c}"], ref["g"]["target_index_c"][c - 1])]
    for vals, mask, win in slots:
        t = tc.tied(vals, mask, win)
        assert len({tc.rank_of(i, count, world) for i in t}) >= 2, (win, t)
    for k, want in ref["masks"].items():
        if k != "S_g":
            assert np.array_equal(np.concatenate([p[k] for p in parts]), want), k
    for part, r in (("s", res), ("g", res["goose"]), ("t", res["tr"])):
        for k in INDEX_KEYS[part]:
            assert np.array_equal(np.asarray(r[k]), np.asarray(ref[part][k])), (part, k, r[k], ref[part][k])


@pytest.mark.parametrize("world", [2, 3])
def test_multi_rank_robust_mirror_model_equals_single_rank(engine, tmp_path, world):
    """The robust sweep of the mirror model (mirrored in the disturbance axis, which is the sharded one) on 2 and 3 ranks: the two
    tied worst disturbances are on different ranks ("ties -> lowest plane"); every field equals the single-rank sweep."""
    ds = tc.mirror_model(q=2)
    lo, hi, count = tc.mirror_grid("planes33")
    out = str(tmp_path / "res.npz")
    spec = {"tie": 1, "q": 2, "count": count, "lo": lo.tolist(), "hi": hi.tolist(), "b": B, "nca": 1, "kind": "ucb"}
    procs = _spawn("_gpu_robust_rank_worker.py", world, lambda r: [out, json.dumps(spec)])
    try:
        with options(engine, **KERNEL_OPTS[3]):
            engine.set_model(ds, mean_prior=np.zeros(2))
            engine.set_grid(lo, hi, count)
            ref = engine.sweep_robust(B, 1, "ucb")
            f, g = engine.robust_arrays()
            mean, var = engine.posterior()
    except BaseException:
        for p in procs:
            p.kill()
            p.wait()
        raise
    assert _wait_ranks(procs) == [0] * world
    r = robust_oracle.robust_from_posterior(mean, var, count[0], B, "ucb")
    col = robust_oracle.bound_of(mean[:, 0], var[:, 0], B, "ucb").reshape(count[1], count[0])[:, r["index"]]
    t = saw_tie(col, np.ones(count[1], dtype=bool), r["worst_d_index"], "worst disturbance")
    assert len({tc.rank_of(int(j) * count[0], count, world) for j in t}) >= 2
    assert (ref["index"], ref["worst_d_index"]) == (r["index"], r["worst_d_index"])
    got = np.load(out)
    assert np.array_equal(got["f"], f) and np.array_equal(got["g"], g)
    for k in ("index", "worst_d_index", "candidate_index", "value", "count_safe", "count_control", "count_disturbance"):
        assert got[k] == ref[k], (k, got[k], ref[k])
