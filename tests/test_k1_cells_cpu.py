"""CPU checks behind tests/test_gpu_k1_cells.py (option k1_cells; csrc/bilinear_post.inc.hpp: k_bhead).

1. encl_safe / encl_unsafe WITH their band test and the per-candidate classification (post_classify_row / post_classify_cand: the sign
   test on P = m m against Q = b b v, the fallback through the root, the band count) restated in NumPy, on random boxes: no candidate
   inside a box a predicate proves is classified otherwise, and none is counted in the band.  k_bhead takes a proved cell's 64 bits
   and its zero band count from this.  (tests/test_skip_safe_cpu.py checks the predicates without the band test, per tile, on the
   oracle's posterior of two grids; this is the statement per box, band included, over many orders of magnitude.)
2. The census of the 384 x 192 window of config H the GPU tests walk, by the predicates of tests/skip_safe_cases.py on the oracle's
   posterior: at the b values of the walk the nine tiles hold proved tiles of each sign, mixed tiles with cells of both proved signs,
   and undecided cells -- the counts of that file's docstring."""
import numpy as np
import pytest

import oracle
import skip_safe_cases as ssc
import test_gpu_colpath_pins as pins

C48, TINY, HUGE, MG = 1.0 + 2.0 ** -48, 1e-250, 1e300, 2.0 ** -40


def encl_unsafe(mlo, mhi, vlo, vhi, b, band):
    """scalar restatement of the device's predicate; band = None or (c1, c0)"""
    bb = b * b
    if not (b >= 0.0 and vlo >= 0.0 and vlo <= vhi and mlo <= mhi):
        return False
    ql, qh = bb * vlo, bb * vhi
    if not mhi < 0.0:
        ph = mhi * mhi
        if not (ph < HUGE and qh < HUGE and ql > TINY and ph * C48 <= ql):
            return False
    if band is None:
        return True
    c1, c0 = band
    amax = max(abs(mlo), abs(mhi))
    amin = 0.0 if (mlo <= 0.0 <= mhi) else min(abs(mlo), abs(mhi))
    pmax, pmin = amax * amax, amin * amin
    rhs = amax * c1 + c0
    if not (amax < 1e150 and qh < HUGE and rhs < HUGE):
        return False
    qdom = (ql - pmax) - MG * (ql + pmax) > rhs * (1.0 + MG)
    pdom = mhi < 0.0 and (pmin - qh) - MG * (pmin + qh) > rhs * (1.0 + MG)
    return bool(qdom or pdom)


def encl_safe(mlo, mhi, vlo, vhi, b, band):
    bb = b * b
    if not (b >= 0.0 and vlo >= 0.0 and vlo <= vhi and mlo <= mhi and mlo > 0.0):
        return False
    pl, ph, qh = mlo * mlo, mhi * mhi, bb * vhi
    if not (ph < HUGE and qh < HUGE and pl > TINY and pl >= qh * C48):
        return False
    if band is None:
        return True
    c1, c0 = band
    rhs = mhi * c1 + c0
    if not (mhi < 1e150 and rhs < HUGE):
        return False
    return bool((pl - qh) - MG * (pl + qh) > rhs * (1.0 + MG))


def classify(m, v, b, band):
    """(ge, le, near) of candidates m, v (arrays): the per-candidate arithmetic of the device"""
    bb = b * b
    with np.errstate(over="ignore", invalid="ignore"):
        p, q = m * m, bb * v
        near = np.zeros(m.shape, bool) if band is None else ~(np.abs(p - q) > np.abs(m) * band[0] + band[1])
        ok = (b >= 0.0) & (v >= 0.0)
        rng = (p < HUGE) & (q < HUGE)
        neg = ok & (m < 0.0)
        ge = ok & ~neg & rng & (p > TINY) & (p >= q * C48)
        le = neg | (ok & rng & ~ge & (q > TINY) & (p * C48 <= q) & (m >= 0.0))
        und = ~ge & ~le
        sd = b * np.sqrt(v)
    ge = np.where(und, m >= sd, ge)
    le = np.where(und, m <= sd, le)
    return ge, le, near


def _boxes(rng, count):
    """random boxes over many magnitudes, centred near the threshold m = b sqrt v as often as away from it"""
    for _ in range(count):
        b = float(rng.choice([0.0, 0.25, 1.0, 2.0, 3.0, 64.0, 10.0 ** rng.uniform(-3, 3)]))
        v0 = 10.0 ** rng.uniform(-12, 2)
        vw = v0 * 10.0 ** rng.uniform(-6, 0)
        thr = b * np.sqrt(v0)
        m0 = float(rng.choice([thr * (1.0 + rng.normal() * 10.0 ** rng.uniform(-6, 0)), rng.normal() * 10.0 ** rng.uniform(-6, 2), -abs(rng.normal())]))
        mw = abs(m0) * 10.0 ** rng.uniform(-8, 0) + 10.0 ** rng.uniform(-12, -3)
        band = None if rng.random() < 0.4 else (2.2 * 10.0 ** rng.uniform(-12, -6), 1.1 * 10.0 ** rng.uniform(-20, -8))
        yield m0, m0 + mw, v0, v0 + vw, b, band


def test_no_candidate_of_a_proved_box_is_classified_otherwise():
    rng = np.random.default_rng(20261021)
    proved = {"safe": 0, "unsafe": 0, "open": 0}
    for mlo, mhi, vlo, vhi, b, band in _boxes(rng, 20000):
        safe, unsafe = encl_safe(mlo, mhi, vlo, vhi, b, band), encl_unsafe(mlo, mhi, vlo, vhi, b, band)
        assert not (safe and unsafe)
        if not (safe or unsafe):
            proved["open"] += 1
            continue
        # 64 candidates: the four corners, points on the edges, the rest uniform inside
        u, w = rng.random(64), rng.random(64)
        u[:4], w[:4] = [0, 0, 1, 1], [0, 1, 0, 1]
        u[4:8], w[8:12] = [0, 1, 0, 1], [0, 1, 0, 1]
        m = np.minimum(mlo + u * (mhi - mlo), mhi)
        v = np.minimum(vlo + w * (vhi - vlo), vhi)
        ge, le, near = classify(m, v, b, band)
        assert not near.any(), (mlo, mhi, vlo, vhi, b, band)
        if safe:
            proved["safe"] += 1
            assert ge.all() and not le.any(), (mlo, mhi, vlo, vhi, b, band)
        else:
            proved["unsafe"] += 1
            assert le.all() and not ge.any(), (mlo, mhi, vlo, vhi, b, band)
    print(proved)
    assert min(proved.values()) > 1000, proved


# b -> (tiles proved safe, proved unsafe, mixed, mixed with cells of both proved signs, undecided cells of the mixed tiles)
WINDOW = {0.0: (6, 0, 3, 2, 25), 1.0: (5, 0, 4, 3, 61), 2.0: (2, 0, 7, 7, 77), 2.5: (1, 0, 8, 6, 98), 3.0: (0, 1, 8, 7, 110),
          6.0: (0, 3, 6, 6, 88), 64.0: (0, 9, 0, 0, 0)}


@pytest.fixture(scope="module")
def window_cells():
    c0, c1 = pins.GRIDS["Hwin"][2]
    mean, var = oracle.gp_inference(oracle.grid_points(*pins.box("Hwin"), pins.GRIDS["Hwin"][2]), pins.config("Hwin")["ds"])
    cells = []
    for a, red in ((mean[:, 1], np.min), (mean[:, 1], np.max), (var[:, 1], np.min), (var[:, 1], np.max)):
        cells.append(red(a.reshape(c1 // 64, 8, 8, c0 // 128, 16, 8), axis=(2, 5)).transpose(0, 2, 1, 3))
    return cells


@pytest.mark.parametrize("b", list(WINDOW))
def test_census_of_the_window(window_cells, b):
    nsf = ssc.encl_safe(*window_cells, b).sum(axis=(2, 3))
    nus = ssc.encl_unsafe(*window_cells, b).sum(axis=(2, 3))
    mixed = (nsf < 128) & (nus < 128)
    got = (int((nsf == 128).sum()), int((nus == 128).sum()), int(mixed.sum()), int((mixed & (nsf > 0) & (nus > 0)).sum()),
           int((128 - nsf - nus)[mixed].sum()))
    assert got == WINDOW[b], (b, got)


def test_the_figures_the_gpu_test_asserts(window_cells):
    """tests/test_gpu_k1_cells.py compares the device's counter with these (guard_band 0: no band test on the device either)."""
    import test_gpu_k1_cells as gpu
    assert gpu.CENSUS_UNDECIDED["Hwin"] == {b: WINDOW[b][4] for b in gpu.CENSUS_UNDECIDED["Hwin"]}
    assert int(ssc.encl_unsafe(*window_cells, 1.0).sum()) == gpu.CENSUS_UNSAFE_CELLS_B1 and not ssc.encl_unsafe(*window_cells, 1.0).all(axis=(2, 3)).any()
    c0, c1 = pins.GRIDS["A128x64"][2]
    mean, var = oracle.gp_inference(oracle.grid_points(*pins.box("A128x64"), pins.GRIDS["A128x64"][2]), pins.config("A128x64")["ds"])
    cells = [red(a.reshape(c1 // 64, 8, 8, c0 // 128, 16, 8), axis=(2, 5)).transpose(0, 2, 1, 3)
             for a, red in ((mean[:, 1], np.min), (mean[:, 1], np.max), (var[:, 1], np.min), (var[:, 1], np.max))]
    for b, want in gpu.CENSUS_UNDECIDED["A128x64"].items():
        nsf, nus = int(ssc.encl_safe(*cells, b).sum()), int(ssc.encl_unsafe(*cells, b).sum())
        assert (128 - nsf - nus if nus < 128 else 0) == want, (b, nsf, nus)


def test_the_walk_holds_every_kind_of_tile():
    walk = [WINDOW[b] for b in (1.0, 2.0, 2.5, 3.0, 6.0, 64.0)]
    assert any(w[0] > 0 and w[2] > 0 for w in walk) and any(w[1] > 0 and w[2] > 0 for w in walk)      # proved tiles of each sign beside mixed ones
    assert all(w[3] > 0 and w[4] > 0 for w in walk if w[2] > 0)                                      # mixed tiles: both proved signs, undecided cells
    assert len({w[:3] for w in walk}) == len(walk)                                                   # the classes change at every step
