"""A NumPy twin of the refine solver (csrc/refine.hip: ref_terms, ref_step and the barrier stages; csrc/pbfgs.hpp: the projected
BFGS) on the reference gradients of refine_oracle.posterior_grad -- test infrastructure only.

It separates the two things a device result depends on: the posterior gradient (ref_eval, what tests/test_gpu_refine_shapes.py is
about) and the solver's own behaviour.  Where the twin, on exact gradients, stalls far above the barrier's floor, a device that
does not converge either says nothing about ref_eval.  What the twin shows: with one box face and one constraint active in three or more dimensions -- a free direction along the curved
constraint boundary -- the barrier stages at weights 1e-4 .. 1e-5 stall for tens of thousands of evaluations, on the device and here
alike (profiles/refine_shape_checks.md).

One point, safe terms and the box only; the sums are NumPy's, so the twin follows the device's iterates closely, not bit for bit.
"""
import numpy as np

import refine_oracle as ro
import refine_sets_oracle as rs

MU0, MUSTEP, MUFLOOR, TOL = 1e-3, 0.1, 1e-11, 1e-9       # kRefMu0, kRefMuStep, kRefMuFloor, kRefDefaultTol
DEFAULT_EVAL = 400                                       # kRefDefaultEval


def run(P, seed, max_eval=DEFAULT_EVAL):
    """(status, evaluations, final barrier weight, x, value) of the twin from ``seed`` on problem P (refine_sets_oracle.problem)."""
    assert not P["pair"] and P["level"] is None and P["ball"] is None and P["kind"] in ("lcb", "ucb", "var")
    ds, b, lo, hi, d = P["ds"], P["b"], P["lo"], P["hi"], P["d"]
    ys = ds["Y_std"]
    sg = -1.0 if P["maximize"] else 1.0
    span = hi - lo; D2 = span * span; cap = 0.1

    def terms(x):
        m, v, gm, gv = ro.posterior_grad(x, ds)
        o = P["objective"]
        if P["kind"] == "var":
            f, gf = v[o], gv[o]
        else:
            s = 1.0 if P["kind"] == "ucb" else -1.0
            sd = np.sqrt(v[o]); f = m[o] + s * b * sd; gf = gm[o] + s * b * gv[o] / (2 * sd)
        fo, go = sg * f / ys[o], sg * gf / ys[o]
        B, gB = 0.0, np.zeros(d)
        for c in P["safe"]:
            sd = np.sqrt(v[c]); gc = m[c] - b * sd
            if not gc > 0: return False, 0, 0, 0, 0, 0
            ggc = gm[c] - b * gv[c] / (2 * sd)
            B -= np.log(gc / ys[c]); gB -= ggc / gc
        return True, fo, go, B, gB, sg * f

    st = dict(x=np.array(seed, float), H=np.diag(D2), hid=1, t=0.0, halv=0)
    nev = 0
    ok, fo, go, B, gB, obj = terms(st["x"]); nev += 1
    mu = MU0 if P["safe"] else MUFLOOR
    S_ = dict(fo=fo, go=go, B=B, gB=gB)

    def pgnorm(g):
        return np.max(np.abs(np.clip(st["x"] - D2 * g, lo, hi) - st["x"]) / span)

    def new_iter():
        nonlocal mu
        while True:
            st["f"] = S_["fo"] + mu * S_["B"]
            st["g"] = S_["go"] + mu * S_["gB"]
            stol = max(TOL, mu) if mu > MUFLOOR else TOL
            if pgnorm(st["g"]) > stol: break
            if mu <= MUFLOOR: return None
            mu = max(MUFLOOR, mu * MUSTEP)
        g, x = st["g"], st["x"]
        fr = ~(((x <= lo) & (g > 0)) | ((x >= hi) & (g < 0)))
        p = np.where(fr, -(st["H"] * fr[None, :]) @ g, 0.0)
        if not (g @ p < 0):
            st["H"] = np.diag(D2); st["hid"] = 1
            p = np.where(fr, -D2 * g, 0.0)
        pn = np.max(np.abs(p) / span)
        st["p"] = p; st["t"] = min(1.0, cap / pn) if st["hid"] else 1.0; st["halv"] = 0
        return np.clip(x + st["t"] * p, lo, hi)

    def stage_end():
        nonlocal mu
        if mu <= MUFLOOR: return None
        mu = max(MUFLOOR, mu * MUSTEP)
        return new_iter()

    trial = new_iter()
    status = "CONVERGED"
    while trial is not None:
        ok, fo, go, B, gB, obj = terms(trial); nev += 1
        dec = st["g"] @ (trial - st["x"]); moved = bool(np.any(trial != st["x"]))
        if ok and moved and fo + mu * B <= st["f"] + 1e-4 * dec:
            S_.update(fo=fo, go=go, B=B, gB=gB)
            tg = go + mu * gB
            s, yv = trial - st["x"], tg - st["g"]
            sy, ss, yy = s @ yv, s @ s, yv @ yv
            st["x"], st["g"] = trial.copy(), tg
            if sy > 1e-10 * np.sqrt(ss * yy):
                if st["hid"]:
                    st["H"] = np.diag(sy / (yv @ (D2 * yv)) * D2); st["hid"] = 0
                H = st["H"]; Hy = H @ yv; rho = 1 / sy; cc = rho * rho * (yv @ Hy) + rho
                st["H"] = H + cc * np.outer(s, s) - rho * (np.outer(Hy, s) + np.outer(s, Hy))
            fprev = st["f"]
            if nev >= max_eval: status = "MAX_EVAL"; break
            if abs(fprev - (fo + mu * B)) <= 1e-15 * (1 + abs(fprev)): trial = stage_end()
            else: trial = new_iter()
            continue
        if nev >= max_eval: status = "MAX_EVAL"; break
        if moved and st["halv"] < 60:
            st["halv"] += 1; st["t"] *= 0.5; trial = np.clip(st["x"] + st["t"] * st["p"], lo, hi); continue
        if st["hid"]: trial = stage_end(); continue
        st["H"] = np.diag(D2); st["hid"] = 1
        trial = new_iter()
    return status, nev, mu, st["x"], rs.value(P, st["x"])
