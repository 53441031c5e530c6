"""The model build (csrc/model.hip) over its whole shape range and from both sources: the single-workgroup form below
kBlockedFrom = 96 rows, the blocked look-ahead chain from it (full and short last panels, one panel up to 64), every (d, q) up to
SBO_MAX_D / SBO_MAX_Q, SBO_MAX_N and SBO_MAX_N - 1, fp32 images, refused builds and builds of different shapes back to back.

After each build the resident factor is probed three ways (tests/model_build.py: probe): model_loo (alpha, diag(M^T M), log det),
the posterior on ~300 listed points -- a few of them on observations -- through both generic kernels, and for d = 2 a small grid
on K1g, which reads the packed images.  References: model_loo.loo_from_invK and oracle.gp_inference at TOL64 = 1e-10 / TOL32 = 1e-4,
normalised units; tests/test_model_build_cpu.py shows the oracle itself within 1e-11 of the extended-precision posterior at every
shape used here."""
import numpy as np
import pytest

import oracle
from oracle import extended
import safebo_amd
from safebo_amd import _lib

import model_build as mb
import model_loo as ml
from model_build import TOL32, TOL64

pytestmark = pytest.mark.gpu


def test_the_constants_this_file_is_built_on():
    assert (_lib.SBO_MAX_N, _lib.SBO_MAX_D, _lib.SBO_MAX_Q) == (2048, 8, 8)
    assert mb.BLOCKED_FROM - 1 in mb.SHAPE_RANGE and mb.BLOCKED_FROM in mb.SHAPE_RANGE and mb.BLOCKED_FROM + 1 in mb.SHAPE_RANGE
    blocked = [n for n in mb.SHAPE_RANGE if n >= mb.BLOCKED_FROM]
    assert {n % mb.PANEL for n in blocked} >= {0, 1, mb.PANEL - 1}           # full, one-row and 31-row last panels
    assert {n // mb.PANEL for n in blocked if n % mb.PANEL} >= {3, 4, 5, 7, 8}


# ------------------------------------------------------------------------------------------ 1. shape range, both sources
@pytest.mark.parametrize("use_invK", [True, False])
@pytest.mark.parametrize("n", mb.SHAPE_RANGE)
def test_every_shape_from_both_sources(engine, n, use_invK):
    """d = 2, q = 2: one row, the 16-row padding, one panel and its neighbours, the switch between the two forms (95 | 96 | 97), last
    panels of 1, 31 and 32 rows behind three, four and seven full ones."""
    ds, lo, hi = mb.make_model(n, 2, 2)
    mb.build_and_probe(engine, ds, lo, hi, use_invK, label=("range", n, use_invK))


@pytest.mark.parametrize("use_invK", [True, False])
@pytest.mark.parametrize("d,q", mb.WIDE_DQ)
@pytest.mark.parametrize("n", mb.WIDE_N)
def test_other_dimensions_and_output_counts_around_the_switch(engine, n, d, q, use_invK):
    """(d, q) = (1, 1), (3, 8), (8, 8): dpad 2 / 4 / 8, blockIdx.y up to SBO_MAX_Q and the q n^2 strides of work / F / Dg on both
    forms, every output with its own hyper-parameters."""
    ds, lo, hi = mb.make_model(n, d, q)
    mb.build_and_probe(engine, ds, lo, hi, use_invK, label=("wide", n, d, q, use_invK))


@pytest.mark.parametrize("use_invK", [True, False])
@pytest.mark.parametrize("n", mb.LARGE_N)
def test_the_largest_models(engine, n, use_invK):
    """SBO_MAX_N - 1 (a 31-row last panel behind 63 full ones) and SBO_MAX_N, (d, q) = (3, 2), log_sn = -1, 200 points; the oracle's
    inverse is built once per n."""
    d, q = mb.LARGE_DQ
    ds, lo, hi = mb.cached_model(n, d, q)
    mb.build_and_probe(engine, ds, lo, hi, use_invK, label=("large", n, use_invK), npts=200)


# ------------------------------------------------------------------------------------------ 2. mode 0 details
def test_an_asymmetric_invK_is_read_as_given_for_alpha(engine):
    """n = 129, q = 2, invK with a skew part of relative size 1e-13.  alpha (model_loo: resid / var) equals invK_as_given @ rhs
    row by row within the rounding of that dot product as the device sums it, 16 eps sum_j |P_ij rhs_j| (64 strided partial sums
    of ceil(n / 64) terms, six shuffle steps, two divisions) -- the symmetrised matrix gives an alpha several times that bound
    away (tests/test_model_build_cpu.py).  The posterior equals the oracle's with the matrix as given for the mean and its
    symmetric part for the variance."""
    ds0, lo, hi = mb.make_model(129, 2, 2)
    ds = mb.skewed(ds0)
    pts = mb.point_list(ds, lo, hi)
    engine.set_points(pts)
    engine.set_model(ds)
    got = engine.model_loo(3.0)
    mp = oracle.mean_prior(ds)
    for o in range(2):
        P, rhs = ds["invKopt"][o], ds["Y_norm"][:, o] - mp[o]
        err = np.abs(got["resid"][:, o] / got["var"][:, o] - P @ rhs)
        bound = 16.0 * np.finfo(np.float64).eps * (np.abs(P) @ np.abs(rhs))
        print("asym alpha", o, float(np.max(err / bound)))
        assert np.all(err <= bound), (o, float(np.max(err / bound)))
    om, _ = oracle.gp_inference(pts, ds)
    _, ov = oracle.gp_inference(pts, mb.symmetrised(ds))
    mb.probe(engine, ds, lo, hi, pts, label="asym", ref=(om, ov), loo=False)


def test_a_deferred_chain_equals_the_immediate_one(engine):
    """n = 129, q = 2 with a K1b-capable grid resident: chol_async = 1 leaves the chain to the first consumer of the factor,
    chol_async = 0 runs it inside set_model.  The posterior on the point list agrees between the two within 1e-11 normalised and
    both pass the probes."""
    ds, lo, hi = mb.make_model(129, 2, 2)
    pts = mb.point_list(ds, lo, hi)
    ref = oracle.gp_inference(pts, ds)
    got = {}
    try:
        for mode in (1, 0):
            engine.set_option("chol_async", mode)
            engine.set_grid(lo, hi, [96, 80])
            engine.set_model(ds)
            engine.posterior_run()                               # (the grid is one the GEMM posterior takes: it needs no factor)
            assert engine.profile()["posterior_kernel"] in (4, 6), (mode, engine.profile()["posterior_kernel"])
            got[mode] = [mb.list_posterior(engine, pts, path) for path in (1, 2)]
            mb.probe(engine, ds, lo, hi, pts, label=("async", mode), ref=ref)
    finally:
        engine.set_option("chol_async", 1)
    ys = np.maximum(1.0, ds["Y_std"])
    for (m1, v1), (m0, v0) in zip(got[1], got[0]):
        em, ev = float(np.max(np.abs(m1 - m0) / ys)), float(np.max(np.abs(v1 - v0) / ys ** 2))
        print("async 1 vs 0", em, ev)
        assert em < 1e-11 and ev < 1e-11, (em, ev)


# ------------------------------------------------------------------------------------------ 3. against the true posterior
@pytest.mark.parametrize("n", mb.TRUE_N)
def test_the_hyper_parameter_build_against_the_true_posterior(engine, n):
    """d = 2, q = 2, log_sn = -3, 100 points, oracle.extended.posterior_true.  The build from the hyper-parameters is no further
    from the truth than TRUE_MARGIN = 4 times the fp64 oracle's own distance (the oracle rounds an explicit inverse: about
    9e-13 / 2.5e-13 at n = 97 and 1.2e-12 to 1.5e-12 / 3e-13 at n = 161 for mean / variance, depending on the LAPACK that inverts,
    so it is measured here; an IEEE Cholesky route sits at 3e-14; the reasoning behind the factor and the device's measured
    distances are in profiles/model_build_checks.md).  The build from the
    oracle's inverse is held to the oracle at TOL64; its distance from the truth is printed."""
    ds, lo, hi, pts = mb.true_case(n)
    truth = extended.posterior_true(pts, ds)
    om, ov = oracle.gp_inference(pts, ds)
    dm, dv = mb.distance_from_truth(om, ov, truth, ds)
    engine.set_points(pts)
    for use_invK in (False, True):
        engine.set_model(ds, use_invK=use_invK)
        for path in (1, 2):
            mean, var = mb.list_posterior(engine, pts, path)
            gm, gv = mb.distance_from_truth(mean, var, truth, ds)
            em, ev = mb.nerrs(mean, var, om, ov, ds)
            print("truth", n, "invK" if use_invK else "hyper", "path", path, "device", gm, gv, "oracle", dm, dv)
            assert em < TOL64 and ev < TOL64, (n, use_invK, path, em, ev)
            if not use_invK:
                assert gm <= mb.TRUE_MARGIN * dm and gv <= mb.TRUE_MARGIN * dv, (n, path, gm, gv, dm, dv)


# ------------------------------------------------------------------------------------------ 4. fp32 models
@pytest.mark.parametrize("n", [95, 97, 129, 161])
def test_an_fp32_model_on_both_forms(engine, n):
    """dtype f32 from the hyper-parameters: k_pack_factor<float> of the single-workgroup (95) and of the blocked factor with one-row
    last panels (97, 129, 161); the posterior within TOL32, model_loo within the fp64 bar (the factor it reads is fp64)."""
    ds, lo, hi = mb.make_model(n, 2, 2)
    mb.build_and_probe(engine, ds, lo, hi, False, dtype="f32", label=("f32", n))


# ------------------------------------------------------------------------------------------ 5. refused builds
def _assert_refused_then_good(engine, bad, use_invK, good, lo, hi, label):
    pts = mb.point_list(good, lo, hi)
    engine.set_points(pts)
    try:
        engine.set_option("chol_async", 0)
        with pytest.raises(ValueError, match="not positive definite"):
            engine.set_model(bad, use_invK=use_invK)
    finally:
        engine.set_option("chol_async", 1)
    with pytest.raises(safebo_amd.SafeBOError) as ei:          # no model is left behind
        engine.posterior_run()
    assert ei.value.code == _lib.SBO_E_NO_MODEL, label
    engine.set_model(good, use_invK=use_invK)
    mb.probe(engine, good, lo, hi, pts, label=label)


@pytest.mark.parametrize("index,where", [(160, "first panel"), (80, "middle panel"), (0, "short last panel")])
def test_an_indefinite_invK_is_refused_in_every_panel(engine, index, where):
    """n = 161 = 5 x 32 + 1, q = 3, invKopt[1][index][index] negated.  The factorisation runs on the reversed matrix: original
    index 160 is pivot 0 of the first panel, 80 lies in the third, 0 is the single row of the last."""
    ds, lo, hi = mb.make_model(161, 2, 3)
    _assert_refused_then_good(engine, mb.indefinite_invK(ds, 1, index), True, ds, lo, hi, ("refused invK", where))


@pytest.mark.parametrize("index,where", [(160, "first panel"), (80, "middle panel"), (0, "short last panel")])
def test_a_deferred_chain_reports_an_indefinite_invK_from_every_panel(engine, index, where):
    """The same three matrices with a K1b-capable grid resident and chol_async on: set_model accepts them (nothing on that path
    factors), the first consumer of the factor -- the generic posterior on a point list -- reports the verdict of the chain on the
    side stream, and a good build follows."""
    ds, lo, hi = mb.make_model(161, 2, 3)
    pts = mb.point_list(ds, lo, hi)
    engine.set_grid(lo, hi, [96, 80])
    engine.set_model(mb.indefinite_invK(ds, 1, index))
    with pytest.raises(ValueError, match="not positive definite"):
        mb.list_posterior(engine, pts, 1)
    engine.set_points(pts)
    engine.set_model(ds)
    mb.probe(engine, ds, lo, hi, pts, label=("deferred refusal", where))


def test_an_indefinite_invK_is_refused_by_the_single_workgroup_form(engine):
    ds, lo, hi = mb.make_model(40, 2, 3)
    _assert_refused_then_good(engine, mb.indefinite_invK(ds, 1, 20), True, ds, lo, hi, "refused invK n=40")


@pytest.mark.parametrize("n,first_row", [(161, 0), (161, 64), (40, 3)])
def test_a_singular_K_is_refused(engine, n, first_row):
    """q = 3 from the hyper-parameters, output 1 alone degenerate: model_build.DUP_ROWS = 32 identical input rows (rows 0-31: the
    first panel; 64-95: the third; n = 40: the single-workgroup form) with log sigma_f = 12 and log sigma_n = -40 for that output,
    so that sn2 + float32 eps (1.19e-7) is below half an ulp of sf2 (3.8e-6) and the 32 x 32 block of K + sn2 I holds one fp64
    number.  Two identical rows alone would leave the verdict to the sign of one rounding (the pivot is exactly 0 in exact
    arithmetic on the stored matrix, +-1 ulp in floating point); 32 of them shrink the block by 2^-49 per pivot until a pivot
    is <= 0 or underflows to 0, whatever the roundings (model_build.degenerate_hyper_model).  NumPy's Cholesky of that K fails
    and that of the other outputs succeeds (tests/test_model_build_cpu.py)."""
    ds, lo, hi = mb.make_model(n, 2, 3)
    _assert_refused_then_good(engine, mb.degenerate_hyper_model(ds, 1, first_row), False, ds, lo, hi, ("refused K", n, first_row))


def test_one_row_too_many_is_refused_and_touches_nothing(engine):
    """n = SBO_MAX_N + 1 is refused on the arguments alone: the model resident before the call still answers, bit for bit, and the
    next build is correct."""
    ds, lo, hi = mb.make_model(129, 2, 2)
    pts = mb.point_list(ds, lo, hi)
    engine.set_points(pts)
    engine.set_model(ds)
    before = mb.list_posterior(engine, pts, 1)
    n = _lib.SBO_MAX_N + 1
    rng = np.random.default_rng(5)
    big = dict(ds)
    big["X_norm"], big["Y_norm"] = rng.standard_normal((n, 2)), rng.standard_normal((n, 2))
    with pytest.raises(ValueError, match="SBO_MAX_N"):
        engine.set_model(big, use_invK=False)
    assert engine.n == 129
    after = mb.list_posterior(engine, pts, 1)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    ds2, lo2, hi2 = mb.make_model(97, 2, 2)
    mb.build_and_probe(engine, ds2, lo2, hi2, False, label="after n = 2049")


# ------------------------------------------------------------------------------------------ 6. back-to-back builds
def test_builds_of_different_shapes_back_to_back(engine):
    """(n, d, q) = (2048, 2, 1) -> (17, 8, 8) -> (129, 3, 4) -> (96, 1, 2) -> (97, 2, 2) on one context, the source alternating from
    the caller's invK.  mwork, Fplain, Fpk and alpha64 only grow: a smaller model works in the front of the larger one's buffers
    and must read none of its leftovers (k_pack_factor writes every image element, only the over-read pad is cleared).  All
    three probes after every step, the 2048-row one included."""
    use_invK = True
    for n, d, q in ((2048, 2, 1), (17, 8, 8), (129, 3, 4), (96, 1, 2), (97, 2, 2)):
        ds, lo, hi = mb.make_model(n, d, q)
        mb.build_and_probe(engine, ds, lo, hi, use_invK, label=("sequence", n, d, q, use_invK), npts=200 if n > 1000 else 300)
        use_invK = not use_invK
