"""Shared helpers of the sbo_model_loo tests: the NumPy statements of the leave-one-out diagnostics -- from
the inverse, from the factor the way the device sums it, and by actually leaving the observation out -- and the comparison of an
engine result with them.  Everything in normalised units."""
import numpy as np

import oracle

import model_remove as mr

TOL64, TOL32 = mr.TOL64, mr.TOL32
STRIP = 64                            # csrc/model.hip: kLooStrip, the columns one wave of k_model_loo_colsq walks
ROWS = 64                             # csrc/model.hip: kLooRows, the rows of one chunk of a strip
FLOAT32_EPS = oracle.FLOAT32_EPS


def _summaries(e, v, Y_norm, mp, logdet):
    lpd = -0.5 * np.sum(np.log(2.0 * np.pi * v) + e * e / v, axis=0)
    nll = np.sum((Y_norm - mp) * e / v, axis=0) + logdet
    return {"resid": e, "var": v, "z": e / np.sqrt(v), "logdet": logdet, "lpd": lpd, "nll": nll}


def loo_from_invK(ds):
    """With P = invK: e_i = alpha_i / P_ii, v_i = 1 / P_ii, log det(K + sn2 I) = -log det P."""
    n, q = ds["Y_norm"].shape
    mp = oracle.mean_prior(ds)
    e, v, logdet = np.empty((n, q)), np.empty((n, q)), np.empty(q)
    for o in range(q):
        P = np.asarray(ds["invKopt"][o])
        alpha = P @ (ds["Y_norm"][:, o] - mp[o])
        e[:, o], v[:, o] = alpha / np.diag(P), 1.0 / np.diag(P)
        logdet[o] = -np.linalg.slogdet(P)[1]
    return _summaries(e, v, ds["Y_norm"], mp, logdet)


def loo_from_factor(M, alpha):
    """The sum the device performs on one output: P_ii = sum_{t >= i} M[t][i]^2 over the lower factor (M^T M = invK), e = alpha / P,
    v = 1 / P, log det(K + sn2 I) = -2 sum_i log M[i][i]."""
    P = np.sum(np.tril(M) ** 2, axis=0)
    return alpha / P, 1.0 / P, -2.0 * np.sum(np.log(np.diag(M)))


def loo_factor_route(ds):
    n, q = ds["Y_norm"].shape
    mp = oracle.mean_prior(ds)
    e, v, logdet = np.empty((n, q)), np.empty((n, q)), np.empty(q)
    for o in range(q):
        alpha = ds["invKopt"][o] @ (ds["Y_norm"][:, o] - mp[o])
        e[:, o], v[:, o], logdet[o] = loo_from_factor(mr.lower_factor(ds["invKopt"][o]), alpha)
    return _summaries(e, v, ds["Y_norm"], mp, logdet)


def noise(ds):
    d = ds["X_norm"].shape[1]
    return np.exp(2.0 * ds["hypopt"][d + 1]) + FLOAT32_EPS


def loo_brute(ds, idx):
    """A true leave-one-out: the model rebuilt without row i under the frozen constants predicts at x_i; the noise the stored
    inverse carries (sn2 + float32 eps) is added to the variance.  Returns (resid [len(idx), q], var [len(idx), q])."""
    q = ds["Y_norm"].shape[1]
    e, v = np.empty((len(idx), q)), np.empty((len(idx), q))
    for r, i in enumerate(idx):
        x = ds["X_norm"][i:i + 1] * ds["X_std"] + ds["X_mean"]
        mean, var = oracle.gp_inference(x, mr.without(ds, i))
        e[r] = ds["Y_norm"][i] - (mean[0] - ds["Y_mean"]) / ds["Y_std"]
        v[r] = var[0] / ds["Y_std"] ** 2 + noise(ds)
    return e, v


def errors(got, ref):
    """Residuals absolutely, variances relatively, the three sums against max(1, |value|)."""
    out = {"resid": float(np.max(np.abs(got["resid"] - ref["resid"]))), "var": float(np.max(np.abs(got["var"] / ref["var"] - 1.0)))}
    for k in ("logdet", "lpd", "nll"):
        if k in got:
            out[k] = float(np.max(np.abs(got[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k]))))
    return out


def summaries_of(z, b):
    """max |z| per output, its lowest index, #{|z| > b}."""
    az = np.abs(z)
    return az.max(axis=0), az.argmax(axis=0), (az > b).sum(axis=0)


def check_loo(eng, ds, tol, label, b=3.0):
    """model_loo of the resident model against loo_from_invK(ds): shapes, the arrays, the sums, and the summaries consistent with
    the returned z (bit for bit: the device forms z from the e and v it returns)."""
    n, q = ds["Y_norm"].shape
    got = eng.model_loo(b, ds["Y_norm"])
    ref = loo_from_invK(ds)
    assert got["resid"].shape == got["var"].shape == got["z"].shape == (n, q), label
    for k in ("logdet", "lpd", "z_max", "z_argmax", "outside", "nll"):
        assert got[k].shape == (q,), (label, k)
    err = errors(got, ref)
    print(label, err)
    assert all(val < tol for val in err.values()), (label, err)
    zmax, zarg, outside = summaries_of(got["z"], b)
    assert np.array_equal(got["z_max"], zmax) and np.array_equal(got["z_argmax"], zarg) and np.array_equal(got["outside"], outside), label
    assert np.max(np.abs(got["z_max"] - np.abs(ref["z"]).max(axis=0))) < tol * np.maximum(1.0, np.abs(ref["z"]).max()), label
    return got, ref
