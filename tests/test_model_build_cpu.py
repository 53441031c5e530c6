"""CPU checks of tests/model_build.py: the generator, the sharpness of the fp64 oracle at every shape the GPU file builds, the
degenerate inputs a build must refuse, and the oracle's own distance from the true posterior that sets the bar of the
hyper-parameter build.  NumPy only."""
import numpy as np
import pytest

import oracle
from oracle import extended

import model_build as mb
import model_loo as ml

ORACLE_BAR = mb.TOL64 / 10            # the oracle's own error leaves nine tenths of TOL64 to the device


def test_the_generator_gives_what_it_says():
    for n, d, q in ((1, 2, 2), (2, 2, 2), (15, 2, 2), (16, 2, 2), (97, 3, 8), (129, 8, 8), (96, 1, 1)):
        ds, lo, hi = mb.make_model(n, d, q)
        assert ds["X_norm"].shape == (n, d) and ds["Y_norm"].shape == (n, q) and ds["hypopt"].shape == (d + 2, q)
        assert len(ds["invKopt"]) == q and all(P.shape == (n, n) for P in ds["invKopt"])
        assert all(np.all(np.isfinite(ds[k])) for k in ("X_mean", "X_std", "Y_mean", "Y_std", "X_norm", "Y_norm"))
        X = ds["X_norm"] * ds["X_std"] + ds["X_mean"]
        assert np.all(X >= lo - 1e-12) and np.all(X <= hi + 1e-12)
        for o in range(1, q):                                   # no two outputs share hyper-parameters, data or inverse
            assert np.all(ds["hypopt"][:, o] != ds["hypopt"][:, o - 1])
            assert not np.allclose(ds["Y_norm"][:, o], ds["Y_norm"][:, o - 1]) or n == 1
            assert not np.allclose(ds["invKopt"][o], ds["invKopt"][o - 1])
        pts = mb.point_list(ds, lo, hi, 50)
        assert pts.shape == (50, d)
        xn = (pts - ds["X_mean"]) / ds["X_std"]
        on = [np.min(np.max(np.abs(ds["X_norm"] - x), axis=1)) < 1e-12 for x in xn]
        assert sum(on) == min(8, n) and on[-1] and not on[0]
    assert mb.log_sn_for(257) == -2.0 and mb.log_sn_for(300) == -1.0 and mb.log_sn_for(2047) == -1.0
    a, b = mb.make_model(33, 2, 2)[0], mb.make_model(33, 2, 2)[0]
    assert np.array_equal(a["X_norm"], b["X_norm"]) and np.array_equal(a["invKopt"][1], b["invKopt"][1])


def _oracle_error(n, d, q, npts):
    ds, lo, hi = mb.make_model(n, d, q)
    pts = mb.point_list(ds, lo, hi, npts)
    om, ov = oracle.gp_inference(pts, ds)
    return max(mb.distance_from_truth(om, ov, extended.posterior_given_invK(pts, ds), ds)
               + mb.distance_from_truth(om, ov, extended.posterior_true(pts, ds), ds))


@pytest.mark.parametrize("n", mb.SHAPE_RANGE)
def test_the_oracle_is_sharp_over_the_shape_range(n):
    """d = 2, q = 2: the fp64 oracle against its formula on the stored inverse and against the true posterior, both in extended
    precision, on the points the GPU test uses (the first 60 random ones and every one on an observation); the three NumPy routes
    to the leave-one-out diagnostics agree."""
    err = _oracle_error(n, 2, 2, 60)
    ds = mb.make_model(n, 2, 2)[0]
    loo = max(ml.errors(ml.loo_factor_route(ds), ml.loo_from_invK(ds)).values())
    print(n, err, loo)
    assert err < ORACLE_BAR and loo < ORACLE_BAR, (n, err, loo)


@pytest.mark.parametrize("d,q", mb.WIDE_DQ)
def test_the_oracle_is_sharp_in_other_dimensions(d, q):
    for n in mb.WIDE_N:
        err = _oracle_error(n, d, q, 40)
        print(n, d, q, err)
        assert err < ORACLE_BAR, (n, d, q, err)


def test_the_oracle_is_sharp_at_the_largest_model():
    """n = 2048 (2047 differs by one row), (d, q) = (3, 2), log_sn = -1: extended precision is out of reach here, so two fp64
    routes that share no rounding -- the explicit inverse and triangular solves with the Cholesky factor -- are compared."""
    d, q = mb.LARGE_DQ
    ds, lo, hi = mb.cached_model(2048, d, q)
    pts = mb.point_list(ds, lo, hi, 200)
    om, ov = oracle.gp_inference(pts, ds)
    cm, cv = mb.cholesky_route(pts, ds)
    em, ev = mb.nerrs(cm, cv, om, ov, ds)
    print(em, ev)
    assert em < ORACLE_BAR and ev < ORACLE_BAR, (em, ev)


@pytest.mark.parametrize("n", mb.TRUE_N)
def test_the_distance_of_the_oracle_from_the_true_posterior(n):
    """What sets the bar of test_the_hyper_parameter_build_against_the_true_posterior: at log_sn = -3 the oracle (explicit inverse)
    is about 9e-13 / 2.5e-13 (n = 97) and 1.2e-12 to 1.5e-12 / 3e-13 (n = 161, by LAPACK) from the truth; the Cholesky route in IEEE
    arithmetic, the form the device's hyper-parameter build takes, is 30 to 40 times closer (asserted: inside a quarter)."""
    ds, lo, hi, pts = mb.true_case(n)
    truth = extended.posterior_true(pts, ds)
    dm, dv = mb.distance_from_truth(*oracle.gp_inference(pts, ds), truth, ds)
    cm, cv = mb.distance_from_truth(*mb.cholesky_route(pts, ds), truth, ds)
    print(n, "oracle", dm, dv, "cholesky route", cm, cv)
    assert 1e-13 < dm < ORACLE_BAR and 1e-14 < dv < ORACLE_BAR
    assert cm < 0.25 * dm and cv < 0.25 * dv


def _cholesky_fails(K):
    try:
        np.linalg.cholesky(K)
    except np.linalg.LinAlgError:
        return True
    return False


@pytest.mark.parametrize("n,first_row", [(161, 0), (161, 64), (40, 3)])
def test_the_singular_K_is_refused_by_numpy_too(n, first_row):
    """Output 1 of model_build.degenerate_hyper_model: the block of the identical rows holds one fp64 number (so the matrix as
    stored is singular: x = e_i - e_k gives x^T K x = 0 exactly) and NumPy's Cholesky fails; outputs 0 and 2 factor."""
    ds = mb.make_model(n, 2, 3)[0]
    bad = mb.degenerate_hyper_model(ds, 1, first_row)
    rows = slice(first_row, first_row + mb.DUP_ROWS)
    assert "invKopt" not in bad and np.array_equal(bad["Y_norm"], ds["Y_norm"])
    K = mb.kernel_matrix(bad, 1)
    assert np.unique(K[rows, rows]).size == 1 and K[first_row, first_row] > 2.0 ** 33
    assert _cholesky_fails(K)
    for o in (0, 2):
        Ko = mb.kernel_matrix(bad, o)
        assert not _cholesky_fails(Ko) and np.linalg.cond(Ko) < 1e6


@pytest.mark.parametrize("n,index", [(161, 160), (161, 80), (161, 0), (40, 20)])
def test_the_indefinite_invK_is_indefinite_in_one_output_only(n, index):
    ds = mb.make_model(n, 2, 3)[0]
    bad = mb.indefinite_invK(ds, 1, index)
    assert _cholesky_fails(bad["invKopt"][1]) and np.min(np.linalg.eigvalsh(bad["invKopt"][1])) < -1.0
    for o in (0, 2):
        assert np.array_equal(bad["invKopt"][o], ds["invKopt"][o]) and not _cholesky_fails(ds["invKopt"][o])
    assert ds["invKopt"][1][index, index] > 0
    # the reversed matrix puts original index i at pivot n - 1 - i: 160 -> panel 0, 80 -> panel 2, 0 -> the one-row panel 5
    assert [(n - 1 - i) // mb.PANEL for i in (160, 80, 0)] == [0, 2, 5] or n != 161


def test_the_skew_part_shows_in_alpha_and_not_in_the_variance():
    """n = 129: alpha from the matrix as given and from its symmetric part differ by several times the bound the GPU test allows
    (so that test tells the two apart); the oracle's variance does not see the skew part beyond rounding."""
    ds0, lo, hi = mb.make_model(129, 2, 2)
    ds = mb.skewed(ds0)
    sym = mb.symmetrised(ds)
    mp = oracle.mean_prior(ds)
    for o in range(2):
        P, S, rhs = ds["invKopt"][o], sym["invKopt"][o], ds["Y_norm"][:, o] - mp[o]
        assert 1e-14 < np.max(np.abs(P - P.T)) / np.max(np.abs(P)) < 1e-12
        bound = 16.0 * np.finfo(np.float64).eps * (np.abs(P) @ np.abs(rhs))
        ratio = np.abs(S @ rhs - P @ rhs) / bound
        print(o, float(np.max(ratio)))
        assert np.max(ratio) > 3.0
    pts = mb.point_list(ds, lo, hi)
    (_, v1), (_, v2) = oracle.gp_inference(pts, ds), oracle.gp_inference(pts, sym)
    assert mb.nerrs(v1, v1, v2, v2, ds)[1] < ORACLE_BAR
