"""The oracle alone on every case of tests/many_constraints.py (no GPU): the preconditions that make
tests/test_gpu_many_constraints.py meaningful -- a device sweep must never agree with the oracle because its input was empty.
Checked for both values of reference_quirk_L_index, since the GPU file sweeps both."""
import numpy as np
import pytest

import many_constraints as mc


def _distinct(planes):
    return len({p.tobytes() for p in planes if p.any()})


def check_case(name, builder=mc.fan_model):
    """Every per-case precondition; returns the quantities the case-table ones need."""
    k = mc.CASES[name]
    q = k["q"]
    out = {}
    for quirk in (True, False):
        s, g, t = mc.reference(name, quirk, builder)
        assert not s["empty_safe_set"] and s["S"].any() and s["U"].any() and s["M"].any(), (name, quirk)
        nG, nO = s["G"].sum(axis=1), g["O"].sum(axis=1)
        assert (nG > 0).sum() >= q - 2 and (nO > 0).sum() >= q - 2, (name, quirk, nG.tolist(), nO.tolist())
        assert _distinct(s["G"]) >= q - 2 and _distinct(g["O"]) >= q - 2, (name, quirk)
        if q >= 5:
            both = (nG > 0) & (nO > 0)                     # both[c - 1]: constraint c; lane = (c - 1) & 1
            assert both[0::2].sum() >= 2 and both[1::2].sum() >= 2, (name, quirk, both.tolist())
        assert mc.sole_excluders(s["lcb"]) >= 3, (name, quirk)
        assert 0 < t["T"].sum() < s["S"].sum(), (name, quirk)
        m_lcb, m_g = mc.margins(name, quirk, builder)
        assert m_lcb >= 1e-6, (name, quirk, m_lcb)         # 1e4 x the 1e-10 posterior tolerance: no S / U bit hangs on rounding
        assert m_g >= 1e-9, (name, quirk, m_g)             # below that the oracle's own rounding would decide a G_c bit
        out[quirk] = (s, g, m_lcb, m_g)
    on, off = out[True], out[False]
    assert not (np.array_equal(on[0]["G"], off[0]["G"]) and np.array_equal(on[1]["O"], off[1]["O"])), name
    return out


@pytest.mark.parametrize("name", list(mc.CASES))
def test_every_constraint_matters_in_every_case(name):
    check_case(name)


def test_the_case_table_moves_the_tie_rule_winners_off_constraint_one():
    """expander_best_c / target_best_c ("first on ties, most uncertain kept") with a winner beyond constraint 1, on the small grids
    (the large ones repeat their models)."""
    eb, tb = set(), set()
    for name, k in mc.CASES.items():
        if k["count"] != [40, 36]:
            continue
        for quirk in (True, False):
            s, g, _ = mc.reference(name, quirk)
            eb.add(s["expander_best"])
            tb.add(g["target_best"])
    assert max(eb) >= 2 and max(tb) >= 2, (eb, tb)
    assert len(eb) >= 3 and len(tb) >= 3, (eb, tb)


def test_the_case_table_covers_three_four_and_seven_constraints():
    assert {k["q"] for k in mc.CASES.values()} == {4, 5, 8}
    assert all(np.prod(k["count"]) <= 72 * 70 for k in mc.CASES.values())


@pytest.mark.parametrize("name", ["q4", "q5", "q8"])
def test_shifted_discs_fail_the_preconditions(name):
    """The counter-example: with discs around shifted centres U lies far from S and the per-constraint sets are empty -- the
    preconditions must notice, or they would let the GPU tests run on nothing."""
    s, g, _ = mc.reference(name, True, mc.disc_model)
    assert s["S"].any() and s["U"].any() and not s["G"].any() and not g["O"].any()
    with pytest.raises(AssertionError):
        check_case(name, builder=mc.disc_model)


def test_the_robust_grid_has_safe_and_unsafe_controls_and_every_constraint_binds():
    """The joint grid of the robust-sweep test: some controls robust-safe, some not, and min_d lcb_c < 0 somewhere for every c."""
    r = mc.robust_reference()
    assert 0 < r["count_safe"] < mc.ROBUST_COUNT[0] and r["index"] >= 0
    assert (r["g"] < 0).any(axis=1).all() and r["g"].shape[0] == 4
    assert np.min(np.abs(r["g"])) >= 1e-6
