"""The history walks' generator (tests/history_walk.py) on its own, without a GPU: the fixed seeds' step lists hold every transition
tests/test_gpu_history.py is there to check, and they replay exactly from the seed."""
import json

import history_walk as hw


def test_fixed_seeds_cover_every_required_transition():
    seen = set()
    for seed in hw.SEEDS:
        seen |= hw.transitions(hw.make_walk(seed))
    missing = hw.REQUIRED - seen
    assert not missing, sorted(missing)


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
