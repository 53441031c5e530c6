"""CPU tests of the C-ABI boundary: the library loads without a GPU, exports what include/safebo.h declares,
fails loudly instead of falling back, and the product package never touches the oracle."""
import ctypes as C
import os
import subprocess
import re

import pytest

import safebo_amd
from safebo_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "safebo.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sbo_[a-z0-9_]+)\s*\(", text)) - {"sbo_relay_allreduce_fn", "sbo_relay_allgather_fn"})


def test_library_exports_every_declared_symbol():
    lib = C.CDLL(_lib.library_path())
    names = _declared_symbols()
    assert len(names) >= 20
    for name in names:
        assert hasattr(lib, name), f"{name} declared in include/safebo.h but not exported"
    bound = {n for n, _, _ in _lib.SYMBOLS}
    assert bound == set(names), (sorted(bound - set(names)), sorted(set(names) - bound))


def test_version_and_struct_layout(tmp_path):
    lib = _lib.load()
    assert lib.sbo_version() == 3
    # the ctypes mirrors must have the sizes a C compiler gives the header's structs
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "safebo.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(sbo_sweep_opts), sizeof(sbo_profile), sizeof(sbo_safeopt_result), sizeof(sbo_goose_result), '
                   'sizeof(sbo_tr_result), sizeof(int64_t)); return 0; }\n')
    exe = tmp_path / "sizes"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.check_call(["gcc", "-I", inc, str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes[:5] == [C.sizeof(_lib.SweepOpts), C.sizeof(_lib.Profile), C.sizeof(_lib.SafeOptResult),
                         C.sizeof(_lib.GooseResult), C.sizeof(_lib.TRResult)]
    assert C.sizeof(_lib.SweepOpts) == 24


def test_profile_ends_with_the_fp32_band(tmp_path):
    """The band of the last fp32 sweep is the tail of sbo_profile: two arrays of SBO_MAX_Q doubles at the offsets the C compiler gives them,
    nothing behind them, and profile_dict hands them out as lists."""
    src = tmp_path / "tail.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safebo.h"\nint main(void) { printf("%zu %zu %zu %d\\n", '
                   'offsetof(sbo_profile, fp32_band_dm), offsetof(sbo_profile, fp32_band_dv), sizeof(sbo_profile), SBO_MAX_Q); return 0; }\n')
    exe = tmp_path / "tail"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    off_dm, off_dv, size, max_q = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert max_q == _lib.SBO_MAX_Q
    assert (_lib.Profile.fp32_band_dm.offset, _lib.Profile.fp32_band_dv.offset, C.sizeof(_lib.Profile)) == (off_dm, off_dv, size)
    assert [name for name, _ in _lib.Profile._fields_][-2:] == ["fp32_band_dm", "fp32_band_dv"]
    assert off_dv + 8 * max_q == size and off_dv - off_dm == 8 * max_q
    d = safebo_amd.SweepEngine.profile_dict(_lib.Profile())
    assert d["fp32_band_dm"] == [0.0] * max_q and d["fp32_band_dv"] == [0.0] * max_q and d["guard_dm"] == [0.0] * max_q
    assert d["fp64_rechecks"] == 0 and d["guard_ms"] == 0.0


def test_null_arguments_are_invalid_not_crashes():
    lib = _lib.load()
    assert lib.sbo_init(0, None) == _lib.SBO_E_INVALID
    assert lib.sbo_posterior_run(None) == _lib.SBO_E_INVALID
    assert lib.sbo_sweep_safeopt(None, None, None) == _lib.SBO_E_INVALID
    assert lib.sbo_model_set(None, 0, b"RBF", 1, 1, 1, None, None, None, None, None, None, None, None) == _lib.SBO_E_INVALID
    with pytest.raises(ValueError):
        _lib.check(lib.sbo_candidates_grid(None, 2, None, None, None, 0, 0))


def _has_gpu():
    n = C.c_int(0)
    _lib.load().sbo_device_count(C.byref(n))
    return n.value > 0


@pytest.mark.skipif(_has_gpu(), reason="this check is about the GPU-less build container")
def test_no_cpu_fallback_without_device():
    with pytest.raises(safebo_amd.SafeBOError) as e:
        safebo_amd.SweepEngine(0)
    assert e.value.code == _lib.SBO_E_HIP
    assert "no CPU fallback" in str(e.value)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "safe-bayesian-optimization_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", text, flags=re.M), f
                assert "gp_oracle" not in text, f
