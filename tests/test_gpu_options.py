"""sbo_set_option, key by key, on a throw-away context: what each key accepts, what it rejects and with which message.  The keys,
bounds and messages below were copied from the strcmp chain that api.hip held before the options became a table; they are the
expectation, not the table."""
import ctypes as C

import pytest

import safebo_amd
from safebo_amd import _lib

pytestmark = pytest.mark.gpu

# key -> (values every one of which must be accepted, None or (lowest accepted, highest accepted, message outside))
OPTIONS = {
    "halo_spec": ((0, 1, 7), None),
    "comm_events": ((0, 1), None),
    "cheb_tol_e17": ((400, 0, 100000), None),
    "tensor_guess_pct": ((10, 100, 400), (10, 400, "tensor_guess_pct must be within 10 .. 400")),
    "tensor_cheb": ((0, 1), None),
    "exact_lazy": ((0, 1, 2, -1, 3), None),                  # (outside 0 .. 2: the default, no error)
    "chol_async": ((0, 1), None),
    "bilinear": ((0, 1, 2), (0, 2, "bilinear must be 0 (off), 1 (on; a model's first sweep by node interpolation) or 2 (on, K1b's plan from the first sweep)")),
    "phase_events": ((0, 1), None),
    "scan_waves": ((0, 1, 8, 16, 32, 64, 5, -3), None),      # (stored as given)
    "set_lanes": ((0, 1), None),
    "result_mirror": ((0, 1), None),
    "set_fuse": ((0, 1), None),
    "col_path": ((0, 1, 2), (0, 2, "col_path must be 0 (never), 1 (auto) or 2 (whenever the grid's shape allows)")),
    "guard_audit": ((0, 1024, 1 << 20), (0, 1 << 20, "guard_audit: samples per sweep, 0 (off) .. 1048576")),
    "guard_audit_scale_ppm": ((1, 1000000, 1000000000), (1, 1000000000, "guard_audit_scale_ppm: 1 .. 1e9")),
    "guard_audit_every": ((1, 16, 1 << 20), (1, 1 << 20, "guard_audit_every: 1 .. 1048576 sweeps")),
    "grad_defer": ((0, 1, 2, 3), (0, 3, "grad_defer must be 0 .. 3")),
    "k1_sched": ((0, 1), None),
    "col_overlap": ((0, 1), None),
    "scan_blocks": ((0, 1), None),
    "fuse_classify": ((-1, 0, 1), (-1, 1, "fuse_classify must be -1 (auto), 0 or 1")),
    "goose_pairs": ((0, 1), None),
    "guard_band": ((0, 1, 2), (0, 2, "guard_band must be 0 (off), 1 (on) or 2 (re-evaluate on every sweep)")),
    "fp64_recheck": ((0, 1), None),
    "comm_selftest": ((0,), None),                            # (1 needs a communicator: below)
    "refine_lds": ((0, 1), (0, 1, "refine_lds must be 0 (stream M) or 1 (LDS when it fits)")),
    "list_index": ((-1, 0, 1), (-1, 1, "list_index must be -1 (auto), 0 (never) or 1 (always)")),
    "posterior_path": ((0, 1, 2), (0, 2, "posterior_path must be 0 (auto), 1 (generic) or 2 (generic, chunked)")),
}


@pytest.fixture(scope="module")
def scratch():
    """A context of its own, without a model: nothing set here reaches the session's engine."""
    eng = safebo_amd.SweepEngine(0)
    yield eng
    eng.close()


def _set(eng, key, value):
    lib = _lib.load()
    rc = lib.sbo_set_option(eng._ctx, key.encode(), C.c_int64(value))
    return rc, lib.sbo_last_error().decode()


@pytest.mark.parametrize("key", sorted(OPTIONS))
def test_option_accepts_and_rejects(scratch, key):
    good, bounds = OPTIONS[key]
    for v in good:
        rc, msg = _set(scratch, key, v)
        assert rc == _lib.SBO_OK, (key, v, msg)
    if bounds is not None:
        lo, hi, text = bounds
        for v in (lo - 1, hi + 1):
            rc, msg = _set(scratch, key, v)
            assert rc == _lib.SBO_E_INVALID and msg == text, (key, v, rc, msg)
        rc, msg = _set(scratch, key, good[0])                # (a rejected value leaves the key settable)
        assert rc == _lib.SBO_OK, (key, msg)


def test_unknown_key_and_selftest_without_communicator(scratch):
    for key in ("no_such_option", "guard_audit_scale", ""):
        rc, msg = _set(scratch, key, 1)
        assert rc == _lib.SBO_E_INVALID and msg == "unknown option " + key
    rc, msg = _set(scratch, "comm_selftest", 1)
    assert rc == _lib.SBO_E_INVALID
    assert msg == "comm_selftest needs a communicator: call sbo_comm_init(ctx, 1, 0, id) with a unique id first"
    assert _set(scratch, "comm_selftest", 0)[0] == _lib.SBO_OK
