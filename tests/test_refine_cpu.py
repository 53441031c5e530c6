"""CPU tests of sbo_refine's pieces that need no GPU: the NumPy reference gradients the GPU tests compare against, and the ctypes
mirrors of the refine structs against a C compiler's layout of include/safebo.h."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from safebo_amd import _lib, synthetic

import refine_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return synthetic.make_dataset(z["X"], z["Y"], z["hypopt"]), float(z["b"]), z["bound"]


@pytest.mark.parametrize("name", ["benoit_n20_50x50", "rosen4_n128_9x8x7x6"])
def test_reference_gradients_match_central_differences(name):
    ds, b, bound = _fixture(name)
    rng = np.random.default_rng(7)
    d = bound.shape[0]
    for _ in range(4):
        x = bound[:, 0] + rng.uniform(0.1, 0.9, d) * (bound[:, 1] - bound[:, 0])
        for o in range(2):
            for kind in ("mean", "var", "ucb", "lcb"):
                f, g = ro.bound_grad(x, ds, b, o, kind)
                fd = np.empty(d)
                for a in range(d):
                    h = 1e-5 * (bound[a, 1] - bound[a, 0])
                    e = np.zeros(d)
                    e[a] = h
                    fd[a] = (ro.bound_grad(x + e, ds, b, o, kind)[0] - ro.bound_grad(x - e, ds, b, o, kind)[0]) / (2 * h)
                np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-6 * (1.0 + np.max(np.abs(fd))), err_msg=f"{kind} {o}")


def test_reference_values_match_the_oracle_posterior():
    import oracle
    ds, b, bound = _fixture("rosen4_n128_9x8x7x6")
    x = np.array([0.3, -0.7, 1.1, 0.2])
    m, v, _, _ = ro.posterior_grad(x, ds)
    om, ov = oracle.gp_inference(x[None, :], ds)
    np.testing.assert_allclose(m, om[0], rtol=1e-12)
    np.testing.assert_allclose(v, ov[0], rtol=1e-10)


def test_refine_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safebo.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(sbo_refine_opts), sizeof(sbo_refine_result), offsetof(sbo_refine_opts, constraint_mask), '
                   'offsetof(sbo_refine_opts, lo), offsetof(sbo_refine_opts, use_ball), offsetof(sbo_refine_opts, x_0), '
                   'offsetof(sbo_refine_opts, tol), offsetof(sbo_refine_result, best_value), offsetof(sbo_refine_result, converged), '
                   '(size_t)SBO_REFINE_ON_BOUNDARY); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    O, R = _lib.RefineOpts, _lib.RefineResult
    assert got == [C.sizeof(O), C.sizeof(R), O.constraint_mask.offset, O.lo.offset, O.use_ball.offset, O.x_0.offset, O.tol.offset,
                   R.best_value.offset, R.converged.offset, _lib.SBO_REFINE_ON_BOUNDARY]


def test_refine_is_bound_with_its_declared_signature():
    lib = _lib.load()
    assert lib.sbo_refine.restype is C.c_int
    assert len(lib.sbo_refine.argtypes) == 8
    res = _lib.RefineResult()
    assert lib.sbo_refine(None, None, 1, None, None, None, None, C.byref(res)) == _lib.SBO_E_INVALID
