"""CPU side of sbo_expander_gain: the two NumPy routes to the hallucinated-observation verdicts agree (the rank-one identity the device
epilogue rests on), every committed case of the GPU test is sharp by the oracle alone (no |z_c(x | g)| and no source's top-two gap of
Z below expander_oracle.SHARP = 1e-8: the condition under which the device's counts and witnesses must equal the oracle's exactly), the
symbol, its structure and its caps are what include/safebo.h declares, the argument checks of SweepEngine.expander_gain and of the
SafeOpt.BO constructor fire before anything touches the device, and target chunks merge as one call would answer (the C call stubbed;
the device call itself is checked under the gpu marker, tests/test_gpu_expander_gain.py).

Agreement of the routes over the committed cases (normalised units, every z_c(x | g)): within 2.0e-11 (n = 1025, d = 3), then 1.3e-11
(n = 300, q = 4, one-bit mask) and 1.8e-12 (n = 1024); every case below n = 300 stays under 1.5e-12; at n = 2048, where the rank-one
route is the reference, it differs from the definition (two full 2049 x 2049 inverses, sources 0 and 64) by 5.2e-12.  The assertion
is TOL64 = 1e-10.  Smallest |z| of a case: 2.1e-7 (n = 65, d = 6, q = 4, 198 147 values); smallest top-two gap: 1.2e-5 (n = 2).

The case list is held to the constants of csrc/expander.hip, csrc/whiten.hpp and csrc/slab_tiles.hpp, read from the source (test_the_case_list_covers_every_edge)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from safebo_amd import SafeOpt, SweepEngine, _lib

import expander_oracle as eo
import model_remove as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [eo.case_id(c) for c in eo.CASES]


@pytest.mark.parametrize("i", range(len(eo.CASES)), ids=IDS)
def test_the_two_routes_agree_and_the_case_is_sharp(i):
    c = eo.CASES[i]
    ds, S, T, a = eo.reference(i)
    assert a["z"].shape == (len(eo.constraints_of(c["q"], c["mask"])), c["ms"], c["mt"])
    if c.get("oracle") == "rank1":
        two = [0, c["ms"] - 1]                               # the definition enters through two sources, one per source tile
        b = eo.gain_naive(ds, c["b"], S, T, c["mask"], only=two)
        err = float(np.max(np.abs(a["z"][:, two] - b["z"][:, two])))
        assert np.array_equal(a["count"][two], np.sum(b["z"][:, two].min(axis=0) >= 0.0, axis=1))
    else:
        b = eo.gain_rank1(ds, c["b"], S, T, c["mask"])
        err = float(np.max(np.abs(a["z"] - b["z"])))
        assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["witness"], b["witness"])
    zmin, gap = eo.sharpness(a)
    print(eo.case_id(c), "routes", err, "min |z|", zmin, "min gap", gap)
    assert err < eo.TOL64, err
    assert zmin > eo.SHARP and gap > eo.SHARP, (zmin, gap)
    if c.get("mixed"):
        assert (a["count"] == 0).any() and (a["count"] > 0).any()
    if c.get("shared"):
        assert np.array_equal(T[:c["shared"]], S[:c["shared"]])


def _constant(text, pattern, what):
    hit = re.search(pattern, text)
    assert hit, f"csrc/expander.hip, csrc/whiten.hpp or csrc/slab_tiles.hpp no longer states {what} in the form this test reads: revisit expander_oracle.CASES and the pattern"
    return [int(g) for g in hit.groups()]


def test_the_case_list_covers_every_edge():
    col = lambda key: {c[key] for c in eo.CASES}
    text = open(os.path.join(ROOT, "safe-bayesian-optimization_amd", "csrc", "expander.hip")).read()
    shared = open(os.path.join(ROOT, "safe-bayesian-optimization_amd", "csrc", "whiten.hpp")).read()     # whiten_tile
    tiles = open(os.path.join(ROOT, "safe-bayesian-optimization_amd", "csrc", "slab_tiles.hpp")).read()  # stage 1, the slab and tile steps
    const = lambda name, src=text: _constant(src, r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", name)[0]
    tile, slab, grid, threads, rows = const("kExpTile"), const("kSlabK", tiles), const("kExpGridTiles"), const("kWhitenThreads", shared), const("kWhitenRows", shared)
    assert "tile64_product(sA, sB," in text and "k0 < K; k0 += kSlabK" in tiles       # (k_exp_pairs walks t in these slabs)
    assert re.search(r"__launch_bounds__\(kWhitenThreads\)\s*void\s+k_exp_stage1", text) and "whiten_stage1_launch(k_exp_stage1<D>" in text and \
        "const int P = whiten_tier(n);" in tiles
    t1, p1, t2, p2, p3 = _constant(shared, r"int\s+whiten_tier\(int\s+n\)\s*\{\s*return\s+n\s*<=\s*(\d+)\s*\?\s*(\d+)\s*:\s*n\s*<=\s*(\d+)\s*\?\s*(\d+)\s*:\s*(\d+)\s*;",
                                   "the tiers of whiten_tile")
    lds = _constant(tiles, r"constexpr\s+size_t\s+kWhitenS1Lds\s*=\s*(\d+)\s*\*\s*1024\s*;", "kWhitenS1Lds")[0] * 1024
    assert re.search(r"nsplit\s*=\s*\(int\)std::min<long long>\(ntt,\s*std::max<long long>\(1,\s*kExpGridTiles\s*/\s*nst\)\)\s*;", text), \
        "csrc/expander.hip no longer splits the targets in the form this test reads: revisit expander_oracle.CASES"
    header = open(os.path.join(ROOT, "include", "safebo.h")).read()
    max_n = int(re.search(r"#define\s+SBO_MAX_N\s+(\d+)", header).group(1))
    assert (tile, slab, grid, threads, rows, max_n) == (64, 32, 1024, 1024, 4, _lib.SBO_MAX_N)
    assert (t1, p1, t2, p2, p3) == (512, 32, 1024, 16, 8)
    assert max(8 * t * (p + 1) for t, p in ((t1, p1), (t2, p2), (max_n, p3))) == 8 * max_n * (p3 + 1) == lds     # (the last tier ends at the LDS it asks for)
    # the issue's shapes
    assert col("n") >= {1, 2, 63, 64, 65, 300, 2048} and col("d") == {1, 2, 3, 6} and col("q") == {2, 3, 4} and col("b") == {0.0, 2.0, 3.0}
    assert col("ms") >= {1, tile - 1, tile, tile + 1, 257} and col("mt") >= {1, tile - 1, tile, tile + 1, 257}
    assert col("use_invK") == {True, False} and len(col("seed")) == len(eo.CASES)
    for q in (3, 4):                                         # the full mask and a one-bit mask
        assert any(c["q"] == q and c["mask"] == 0 for c in eo.CASES) and any(c["q"] == q and bin(c["mask"]).count("1") == 1 for c in eo.CASES)
    # the kernels' constants: a case on each side of a K-slab edge and of a stage-1 tier edge
    assert {slab, slab + 1, 2 * slab, 2 * slab + 1} <= col("n")
    for t in (t1, t2):
        assert {t, t + 1} <= col("n"), t
    assert any(c["n"] == max_n and c["ms"] == tile + 1 and c["mt"] == tile + 1 for c in eo.CASES)
    splits = lambda c: min(-(-c["mt"] // tile), max(1, grid // -(-c["ms"] // tile)))
    assert any(c["ms"] == 1 and splits(c) >= 2 for c in eo.CASES)                           # a second split on every source
    assert any(-(-c["mt"] // tile) > splits(c) for c in eo.CASES)                           # a workgroup with a second target tile
    assert any(c.get("mixed") for c in eo.CASES) and any(c.get("shared") for c in eo.CASES)
    assert any(c["mt"] % p for p in (p1, p2, p3) for c in eo.CASES)


def test_symbol_structure_and_caps_match_the_header(tmp_path):
    text = open(os.path.join(ROOT, "include", "safebo.h")).read()
    assert int(re.search(r"#define\s+SBO_EXPANDER_MAX_POINTS\s+(\d+)", text).group(1)) == _lib.SBO_EXPANDER_MAX_POINTS == 65536
    assert int(re.search(r"#define\s+SBO_EXPANDER_MAX_SCRATCH\s+(\d+)ULL", text).group(1)) == _lib.SBO_EXPANDER_MAX_SCRATCH == 1 << 32
    assert "sbo_expander_gain" in {n for n, _, _ in _lib.SYMBOLS}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safebo.h"\nint main(void) { printf("%zu %zu %zu %d\\n", '
                   'sizeof(sbo_expander_opts), offsetof(sbo_expander_opts, constraint_mask), offsetof(sbo_expander_opts, reserved), '
                   'SBO_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.ExpanderOpts), _lib.ExpanderOpts.constraint_mask.offset, _lib.ExpanderOpts.reserved.offset, 3]
    assert C.sizeof(_lib.ExpanderOpts) == 16
    lib = _lib.load()
    assert hasattr(C.CDLL(_lib.library_path()), "sbo_expander_gain")
    assert lib.sbo_expander_gain(None, None, 1, None, 1, None, None, None, None) == _lib.SBO_E_INVALID
    count, margin, witness = np.full(3, 7, dtype=np.int64), np.zeros(3), np.full(3, 5, dtype=np.int64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.sbo_expander_gain(None, None, 3, None, 1, None, ptr(count), ptr(margin), ptr(witness)) == _lib.SBO_E_INVALID
    assert count.tolist() == [0, 0, 0] and np.isnan(margin).all() and witness.tolist() == [-1, -1, -1]


def _bare_engine(d=2, q=3, n=40):
    """An engine object without a context: every call that reached the library would fail on it."""
    eng = SweepEngine.__new__(SweepEngine)
    eng._ctx, eng._lib, eng.d, eng.q, eng.n = None, None, d, q, n
    return eng


Z2 = np.zeros((4, 2))


@pytest.mark.parametrize("kwargs", [
    dict(sources=np.zeros((4, 3)), targets=Z2, b=3.0), dict(sources=np.zeros((0, 2)), targets=Z2, b=3.0),
    dict(sources=np.zeros((2, 2, 2)), targets=Z2, b=3.0), dict(sources=Z2, targets=np.zeros((4, 3)), b=3.0),
    dict(sources=Z2, targets=np.zeros((0, 2)), b=3.0), dict(sources=Z2, targets=Z2, b=-1.0), dict(sources=Z2, targets=Z2, b=float("nan")),
    dict(sources=Z2, targets=Z2, b=float("inf")), dict(sources=Z2, targets=Z2, b="3"), dict(sources=Z2, targets=Z2, b=True),
    dict(sources=Z2, targets=Z2, b=3.0, constraints=[0]), dict(sources=Z2, targets=Z2, b=3.0, constraints=[3]),
    dict(sources=Z2, targets=Z2, b=3.0, constraints=[1.0]), dict(sources=Z2, targets=Z2, b=3.0, constraints=[]),
    dict(sources=Z2, targets=Z2, b=3.0, constraints=[-1]), dict(sources=np.array([[0.0, np.nan]]), targets=Z2, b=3.0),
    dict(sources=Z2, targets=np.array([[np.inf, 0.0]]), b=3.0), dict(sources=np.zeros((65537, 2)), targets=Z2, b=3.0),
])
def test_expander_gain_checks_its_arguments_on_the_host(kwargs):
    with pytest.raises(ValueError):
        _bare_engine().expander_gain(**kwargs)


def test_a_model_without_constraints_is_refused_on_the_host():
    with pytest.raises(ValueError):
        _bare_engine(q=1).expander_gain(Z2, Z2, 3.0)


def test_accepted_arguments_come_back_in_library_form():
    src, tgt, b, mask = SweepEngine.expander_arguments(2, 4, [0.5, 1.0], [[1.0, 2.0]], 2, [3, np.int64(1)])
    assert src.shape == (1, 2) and tgt.shape == (1, 2) and src.dtype == np.float64 and (b, mask) == (2.0, 0b1010)
    assert SweepEngine.expander_arguments(2, 4, Z2, Z2, 0.0)[3] == 0
    assert SweepEngine.expander_arguments(0, 0, np.zeros((3, 5)), np.zeros((1, 5)), 1.0, [6])[3] == 1 << 6     # (no model: the library answers)


def test_target_chunks_merge_as_one_call(monkeypatch):
    """SweepEngine.expander_gain with the C call stubbed by a table Z [ms, mt]: chunks of 5 targets (one source's best value
    sits in two chunks -- the lower global index wins --, one source has NaN in a whole chunk, one everywhere) merge into the counts,
    margins and witnesses of the whole table."""
    rng = np.random.default_rng(7)
    ms, mt = 6, 23
    Z = rng.standard_normal((ms, mt))
    Z[1, 3] = Z[1, 17] = 9.0                                 # a tie across chunks
    Z[2, 5:10] = np.nan                                      # a chunk without a value
    Z[3, :] = np.nan                                         # no value at all
    Z[4, 20] = 11.0                                          # the best in the last, short chunk
    targets = np.column_stack([np.arange(mt, dtype=np.float64), np.zeros(mt)])
    calls = []

    def stub(self, opts, src, tgt, want_margin):
        idx = tgt[:, 0].astype(int)
        calls.append(idx.tolist())
        z = Z[:, idx]
        count = np.sum(z >= 0.0, axis=1).astype(np.int64)
        some = ~np.isnan(z).all(axis=1)
        w = np.where(some, np.argmax(np.where(np.isnan(z), -np.inf, z), axis=1), -1).astype(np.int64)
        m = np.where(some, np.nanmax(np.where(some[:, None], z, 0.0), axis=1), np.nan)
        return (count, m, w) if want_margin else (count, None, None)

    monkeypatch.setattr(SweepEngine, "_expander_call", stub)
    monkeypatch.setattr(SweepEngine, "_expander_chunk", 5)
    eng = _bare_engine(q=2)
    got = eng.expander_gain(np.zeros((ms, 2)), targets, 3.0, return_margin=True)
    assert calls == [list(range(lo, min(lo + 5, mt))) for lo in range(0, mt, 5)]
    assert np.array_equal(got["count"], np.sum(Z >= 0.0, axis=1)) and np.array_equal(got["expander"], got["count"] > 0)
    assert got["witness"].tolist() == [int(np.argmax(Z[0])), 3, int(np.nanargmax(Z[2])), -1, 20, int(np.argmax(Z[5]))]
    want = np.array([Z[0].max(), 9.0, np.nanmax(Z[2]), np.nan, 11.0, Z[5].max()])
    assert np.array_equal(got["margin"], want, equal_nan=True)
    lean = eng.expander_gain(np.zeros((ms, 2)), targets, 3.0)
    assert set(lean) == {"count", "expander"} and np.array_equal(lean["count"], got["count"])


def test_the_scratch_cap_shrinks_the_chunk(monkeypatch):
    """n = 2048 and seven constraints: a row of whitened vectors is 2048 * 7 * 8 bytes, 4 GiB hold 37 449 of them -- with 30 000
    sources the targets go in chunks of 7 449; 40 000 sources leave no room and are refused."""
    sizes = []
    monkeypatch.setattr(SweepEngine, "_expander_call",
                        lambda self, opts, src, tgt, want: (sizes.append(len(tgt)) or np.zeros(len(src), dtype=np.int64), None, None))
    eng = _bare_engine(q=8, n=2048)
    eng.expander_gain(np.zeros((30000, 2)), np.zeros((10000, 2)), 3.0)
    assert sizes == [7449, 2551]
    with pytest.raises(ValueError):
        eng.expander_gain(np.zeros((40000, 2)), np.zeros((10, 2)), 3.0)


@pytest.mark.parametrize("kwargs", [dict(expanders="optimistic"), dict(expanders="hallucinated", refine=True), dict(expander_sources=0),
                                    dict(expander_sources=2.5), dict(expander_sources=True)])
def test_the_constructor_checks_the_expander_options(kwargs):
    with pytest.raises(ValueError):
        SafeOpt.BO([mr.benoit_f, mr.benoit_g], mr.BOUND, 3.0, grid=(20, 20), **kwargs)


def test_the_hallucinated_mode_is_an_option_and_says_what_it_is():
    m = SafeOpt.BO([mr.benoit_f, mr.benoit_g], mr.BOUND, 3.0, grid=(20, 20))
    assert m.expanders == "lipschitz" and m.expander_sources == 4096 and m.expander_witness is None
    h = SafeOpt.BO([mr.benoit_f, mr.benoit_g], mr.BOUND, 3.0, grid=(20, 20), expanders="hallucinated", expander_sources=16)
    assert h.expanders == "hallucinated" and h.expander_sources == 16
    with pytest.raises(ValueError):
        h.Expander(refine=True)                              # (refused before anything touches the device)
    doc = SafeOpt.BO._expander_hallucinated.__doc__
    assert "not reference behaviour" in doc and "lowest flat index" in doc and "Lipschitz" in doc
