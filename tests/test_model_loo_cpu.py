"""CPU side of sbo_model_loo: the three NumPy statements of the leave-one-out diagnostics agree (the identity the device pass rests
on), the symbol and its result structure are what include/safebo.h declares, and the argument checks of
add_sample(..., refit_when=fn) fire before anything touches the device (the device call itself is checked under the gpu marker,
tests/test_gpu_model_loo.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
from safebo_amd import SafeOpt, _lib, synthetic

import model_loo as ml
import model_remove as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [17, 90])
def test_the_three_numpy_routes_agree(n):
    """Config B (q = 2, default hyper-parameters): e and v from diag(invK), from the column sums of squares of the lower factor, and
    from n true leave-one-out predictions (the model rebuilt without row i, predicting at x_i, plus the noise) agree within TOL64;
    so do logdet, lpd and nll of the first two."""
    ds = synthetic.make_config("B", n=n, seed=5)["ds"]
    a, f = ml.loo_from_invK(ds), ml.loo_factor_route(ds)
    err = ml.errors(f, a)
    assert all(v < ml.TOL64 for v in err.values()), err
    e, v = ml.loo_brute(ds, range(n))
    assert np.max(np.abs(e - a["resid"])) < ml.TOL64 and np.max(np.abs(v / a["var"] - 1.0)) < ml.TOL64
    assert np.max(np.abs(e - f["resid"])) < ml.TOL64 and np.max(np.abs(v / f["var"] - 1.0)) < ml.TOL64
    # the reference's NLL form r^T alpha + logdet, from the inverse itself
    mp = oracle.mean_prior(ds)
    for o in range(2):
        r = ds["Y_norm"][:, o] - mp[o]
        K = np.linalg.inv(ds["invKopt"][o])
        want = r @ ds["invKopt"][o] @ r + np.linalg.slogdet((K + K.T) / 2)[1]
        assert abs(a["nll"][o] - want) < ml.TOL64 * max(1.0, abs(want))


def test_symbol_is_exported_and_bound():
    lib = C.CDLL(_lib.library_path())
    assert hasattr(lib, "sbo_model_loo")
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    assert "sbo_model_loo" in bound
    res, args = bound["sbo_model_loo"]
    assert res is C.c_int and len(args) == 5 and args[1] is C.c_double and args[4] is C.POINTER(_lib.ModelLooResult)
    assert _lib.load().sbo_version() == 3


def test_null_context_is_invalid():
    lib = _lib.load()
    assert lib.sbo_model_loo(None, 3.0, None, None, None) == _lib.SBO_E_INVALID
    res = _lib.ModelLooResult()
    assert lib.sbo_model_loo(None, 3.0, None, None, C.byref(res)) == _lib.SBO_E_INVALID


def test_result_structure_layout(tmp_path):
    """sizeof(sbo_model_loo_result) and the offset of every field, as a C compiler lays the header's structure out."""
    fields = [name for name, _ in _lib.ModelLooResult._fields_]
    assert fields == ["n", "q", "logdet", "lpd", "z_max", "z_argmax", "outside"]
    offs = ", ".join(f"offsetof(sbo_model_loo_result, {f})" for f in fields)
    fmt = " ".join(["%zu"] * (len(fields) + 1))
    src = tmp_path / "loo.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safebo.h"\n'
                   f'int main(void) {{ printf("{fmt} %d\\n", sizeof(sbo_model_loo_result), {offs}, SBO_MAX_Q); return 0; }}\n')
    exe = tmp_path / "loo"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[-1] == _lib.SBO_MAX_Q
    assert out[0] == C.sizeof(_lib.ModelLooResult)
    assert out[1:-1] == [getattr(_lib.ModelLooResult, f).offset for f in fields]


class _NoDevice:
    def __init__(self):
        self.calls = []

    def append_sample(self, xn, yn):
        self.calls.append("append")

    def remove_sample(self, index):
        self.calls.append("remove")

    def model_loo(self, b, Y_norm=None):
        self.calls.append("loo")
        raise AssertionError("the device must not be reached")


@pytest.mark.parametrize("kw", [dict(refit_when=lambda d: True), dict(incremental=False, refit_when=lambda d: True),
                                dict(incremental=True, refit_when=3), dict(incremental=True, refit_when="always"),
                                dict(incremental=True, window=8, refit_when=0.5)])
def test_refit_when_value_errors_touch_nothing(kw):
    """refit_when without incremental=True, or a refit_when that is not callable: ValueError, and neither the host state nor the
    engine has been touched (not even the window's removal)."""
    m = mr.init_bo(SafeOpt.BO, n=8)
    m._engine = _NoDevice()
    m._uploaded_version = m._model_version
    v0, X0 = m._model_version, m.X.copy()
    x = np.array([1.35, -0.75])
    with pytest.raises(ValueError):
        m.add_sample(x, m.calculate_plant_outputs(x), **kw)
    assert m._engine.calls == [] and m.n_point == 8 and np.array_equal(m.X, X0) and m._model_version == v0
