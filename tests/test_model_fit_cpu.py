"""CPU side of sbo_model_fit / sbo_fit_de_batch and of GP_Safe's ``fit_on_device = "model"``: the ABI (exports, NULL context, struct
sizes), the lazy ``invKopt`` and the precedence of ``fixed_hyper``.  No device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np

from safebo_amd import GP_Robust, SafeOpt, _lib, synthetic
from safebo_amd.GP_Safe import FLOAT32_EPS, GP, LazyInvK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_bound_and_refuse_a_null_context():
    lib = _lib.load()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in ("sbo_fit_de_batch", "sbo_model_fit"):
        assert hasattr(C.CDLL(_lib.library_path()), name) and name in bound
    assert lib.sbo_fit_de_batch(None, 4, 2, 1, None, None, 8, None, None, None, None, 1, 0.01, 0.0, None, None, None) == _lib.SBO_E_INVALID
    assert lib.sbo_model_fit(None, 0, b"RBF", 4, 2, 1, None, None, None, None, None, None, None, None, None, None, None) == _lib.SBO_E_INVALID
    assert b"ctx" in lib.sbo_last_error()
    assert lib.sbo_version() == 3


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safebo.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(sbo_fit_opts), sizeof(sbo_fit_report), offsetof(sbo_fit_opts, lo), offsetof(sbo_fit_opts, seed), '
                   'offsetof(sbo_fit_report, de_ms), offsetof(sbo_fit_report, host_syncs)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [C.sizeof(_lib.FitOpts), C.sizeof(_lib.FitReport), _lib.FitOpts.lo.offset, _lib.FitOpts.seed.offset,
                     _lib.FitReport.de_ms.offset, _lib.FitReport.host_syncs.offset]


def _gp(n, d, seed):
    rng = np.random.default_rng(seed)
    m = GP([lambda u, noise=0: 0.0])
    m.kernel, m.nx_dim, m.n_point, m.ny_dim = "RBF", d, n, 3
    return m, rng.standard_normal((n, d))


def test_lazy_invk_is_the_host_expression_and_costs_nothing_until_read():
    n, d, q = 9, 2, 3
    m, X_norm = _gp(n, d, 0)
    rng = np.random.default_rng(1)
    hypopt = np.vstack([rng.uniform(-1.5, 1.5, size=(d + 1, q)), rng.uniform(-5.0, -2.0, size=(1, q))])
    calls = []

    def compute(i):
        calls.append(i)
        return m._invK(X_norm, hypopt, i)

    lazy = LazyInvK(compute, q)
    assert len(lazy) == q and calls == [] and lazy.materialised is False
    for i in (2, 0):
        ell, sf2 = np.exp(2.0 * hypopt[:d, i]), np.exp(2.0 * hypopt[d, i])
        sn2 = np.exp(2.0 * hypopt[d + 1, i]) + FLOAT32_EPS
        K = m.Cov_mat(m.kernel, X_norm, X_norm, ell, sf2) + sn2 * np.eye(m.n_point)     # determine_hyperparameters' expression
        assert np.array_equal(lazy[i], np.linalg.inv(K))
        assert lazy[i] is lazy[i]
    assert calls == [2, 0] and lazy.materialised is False
    assert [a.shape for a in lazy] == [(n, n)] * q and calls == [2, 0, 1] and lazy.materialised is True
    assert np.array_equal(lazy[-1], lazy[2])
    lazy[1] = np.eye(n)                                    # (add_sample(incremental=True) writes the bordered inverse back)
    assert np.array_equal(lazy[1], np.eye(n))
    # the fixed-hyper host path forms the same matrices through the same helper
    m.fixed_hyper = hypopt
    h2, inv2 = m.determine_hyperparameters(X_norm, np.zeros((n, q)))
    assert np.array_equal(h2, hypopt) and all(np.array_equal(inv2[i], m._invK(X_norm, hypopt, i)) for i in range(q))


class _NoFitEngine:
    """Stands in for the SweepEngine: any fit call is an error."""

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} touched although fixed_hyper is set")


def benoit_f(u, noise=0):
    return u[0] ** 2 + u[1] ** 2 + u[0] * u[1]


def benoit_g(u, noise=0):
    return -(1. - u[0] + u[1] ** 2 + 2. * u[1])


def test_fixed_hyper_keeps_precedence_over_the_model_mode():
    for cls in (SafeOpt.BO, None):
        if cls is None:
            m = GP_Robust.GP([benoit_f, benoit_g])
        else:
            m = cls([benoit_f, benoit_g], np.array([[-.6, 1.5], [-1., 1.]]), 3.0, grid=(20, 20))
        m._engine = _NoFitEngine()
        m.fit_on_device = "model"
        m.fixed_hyper = synthetic.default_hypopt(2, 2)
        X, Y = m.Data_sampling(8, np.array([1.4, -.8]), 0.3)
        m.GP_initialization(X, Y, "RBF", multi_hyper=5)
        assert np.array_equal(m.hypopt, m.fixed_hyper)
        assert isinstance(m.invKopt, list) and m.invKopt[0].shape == (8, 8)
        assert m._uploaded_version != m._model_version      # nothing was built on the device: the next sweep uploads
        m.add_sample(X[0] + 0.01, Y[0])
        assert isinstance(m.invKopt, list) and m.invKopt[0].shape == (9, 9) and m._uploaded_version != m._model_version


def test_model_mode_makes_one_fit_call_and_marks_the_device_model_current():
    """The host flow of the mode on a stand-in engine: one model_fit per (re)fit with the "de" mode's population and seed, a lazy
    invKopt, and no upload pending afterwards."""
    calls = []

    class _Engine:
        def model_fit(self, ds, bounds, init_pop, **kw):
            calls.append((ds, np.array(bounds), np.array(init_pop), kw))
            q = ds["Y_norm"].shape[1]
            return {"hypopt": np.tile(np.array([[0.1], [0.2], [0.0], [-3.0]]), (1, q))}

        def set_model(self, *a, **k):
            raise AssertionError("upload although the device model is current")

    m = GP_Robust.GP([benoit_f, benoit_g])
    m._engine = _Engine()
    m.fit_on_device = "model"
    m.de_options = {"seed": 7, "maxiter": 33, "tol": 1e-3, "popsize": 5}
    X, Y = m.Data_sampling(8, np.array([1.4, -.8]), 0.3)
    m.GP_initialization(X, Y, "RBF", multi_hyper=5)
    m._sync_model()
    assert len(calls) == 1 and m._uploaded_version == m._model_version
    ds, bounds, pop, kw = calls[0]
    assert "invKopt" not in ds and "hypopt" not in ds
    assert np.array_equal(bounds, np.array([[-1.5, 1.5]] * 3 + [[-8.0, -2.0]])) and pop.shape == (20, 4)
    from scipy.stats import qmc
    assert np.array_equal(pop, qmc.scale(qmc.LatinHypercube(4, seed=7).random(20), bounds[:, 0], bounds[:, 1]))
    assert kw["seed"] == 7 and kw["maxiter"] == 33 and kw["tol"] == 1e-3 and kw["atol"] == 0.0 and kw["polish"] is True
    assert np.array_equal(kw["mean_prior"], np.zeros(2)) and kw["dtype"] == "f64"
    assert isinstance(m.inference_datasets["invKopt"], LazyInvK) and not m.invKopt.materialised
    m.add_sample(X[0] + 0.01, Y[0])
    m._sync_model()
    assert len(calls) == 2 and calls[1][0]["X_norm"].shape == (9, 2) and m._uploaded_version == m._model_version
    assert np.array_equal(m.invKopt[1], m._invK(m.X_norm, m.hypopt, 1))
