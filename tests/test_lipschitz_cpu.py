"""CPU tests of the Lipschitz bound over the box: the NumPy / SciPy twin against oracle.mean_grad, and the ABI of
sbo_mean_grad / sbo_lipschitz.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import lipschitz_oracle as lo_
from safebo_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(lo_.CASES)


def _probe_points(c, count=40, seed=7):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(c["lo"], c["hi"], size=(count, c["lo"].shape[0]))
    pts[0], pts[1] = c["lo"], c["hi"]
    return pts


@pytest.mark.parametrize("name", NAMES)
def test_twin_value_is_the_oracles(name):
    c = lo_.case(name)
    pts = _probe_points(c)
    want = oracle.mean_grad(pts, c["ds"])
    q = want.shape[1]
    for o in range(q):
        got = np.array([lo_.grad(x, c["ds"], o) for x in pts])
        assert np.max(np.abs(got - want[:, o, :])) <= 1e-11 * np.max(np.abs(want[:, o, :])), (name, o)


@pytest.mark.parametrize("name", NAMES)
def test_hessian_row_matches_central_differences(name):
    """Step 1e-5 span; bound 1e-6 of the row's largest entry (the differences' own error: h^2 f''' / 6 ~ 1e-10 relative in span
    units plus eps / h ~ 1e-11; measured worst 5.6e-8, config C)."""
    c = lo_.case(name)
    ds, span = c["ds"], c["hi"] - c["lo"]
    d, q = span.shape[0], ds["Y_norm"].shape[1]
    worst = 0.0
    for x in _probe_points(c, count=6, seed=11)[2:]:
        plus = np.array([oracle.mean_grad((x + 1e-5 * span[b] * np.eye(d)[b])[None, :], ds)[0] for b in range(d)])    # [b, q, a]
        minus = np.array([oracle.mean_grad((x - 1e-5 * span[b] * np.eye(d)[b])[None, :], ds)[0] for b in range(d)])
        for o in range(q):
            for a in range(d):
                row = lo_.hess_row(x, ds, o, a)
                fd = (plus[:, o, a] - minus[:, o, a]) / (2e-5 * span)
                worst = max(worst, float(np.max(np.abs(row - fd)) / np.max(np.abs(row))))
    print(f"{name}: worst relative deviation of a Hessian row from central differences {worst:.2e}")
    assert worst <= 1e-6


def test_default_seeds_rule():
    assert [lo_.seeds_per_axis(d) for d in range(1, 9)] == [33, 33, 16, 8, 5, 4, 3, 2]
    c = lo_.case("A")
    S = lo_.default_seeds(c["ds"], c["lo"], c["hi"])
    n = c["ds"]["X_norm"].shape[0]
    assert S.shape == (33 * 33 + n, 2)
    assert np.array_equal(S[0], c["lo"]) and np.array_equal(S[33 * 33 - 1], c["hi"]) and S[1, 0] > S[0, 0] and S[1, 1] == S[0, 1]
    assert np.all((S >= c["lo"]) & (S <= c["hi"]))
    assert np.allclose(S[33 * 33:], c["ds"]["X_norm"] * c["ds"]["X_std"] + c["ds"]["X_mean"])


@pytest.mark.parametrize("name", NAMES)
def test_twin_box_L_covers_the_fine_grid(name):
    """The twin's L is attained (oracle.mean_grad at x), at least its best seed's, and no fine-grid point beats it."""
    c = lo_.case(name)
    t = c["twin"]
    q = c["fine"].shape[0]
    print(f"{name}: twin L {t['L']}, L_seed {t['L_seed']}, fine grid {c['fine']}, {t['evaluations']} evaluations / {t['problems']} problems")
    assert np.all((t["x"] >= c["lo"]) & (t["x"] <= c["hi"]))
    for o in range(q):
        # (oracle.mean_grad sums in NumPy's order for the batch it is given: the same point alone differs by rounding, n eps)
        assert t["L"][o] == pytest.approx(np.max(np.abs(oracle.mean_grad(t["x"][o][None, :], c["ds"])[0, o])), rel=1e-11)
        assert t["L"][o] >= t["L_seed"][o]
        assert t["L"][o] >= c["fine"][o], (name, o, t["L"][o], c["fine"][o])


def test_abi_binds_both_symbols_and_mirrors_the_structs(tmp_path):
    """_lib binds sbo_mean_grad and sbo_lipschitz, and the two ctypes structs have the sizes and field offsets gcc gives the header's."""
    bound = {n for n, _, _ in _lib.SYMBOLS}
    assert {"sbo_mean_grad", "sbo_lipschitz"} <= bound
    lib = C.CDLL(_lib.library_path())
    assert hasattr(lib, "sbo_mean_grad") and hasattr(lib, "sbo_lipschitz")
    pairs = (("sbo_lipschitz_opts", _lib.LipschitzOpts), ("sbo_lipschitz_result", _lib.LipschitzResult))
    lines = []
    for cname, cls in pairs:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        lines += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "lip.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safebo.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "lip"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for _, cls in pairs:
        want.append(C.sizeof(cls))
        want += [getattr(cls, f).offset for f, _ in cls._fields_]
    assert got == want
    assert _lib.load().sbo_version() == 3
