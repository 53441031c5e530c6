"""NumPy statements of sbo_refine_paths and the committed case list of its tests -- test infrastructure only.

A sample path f_s is paths_oracle's (pathwise conditioning, c_s by np.linalg.solve on K + sn2 I); here it is a function of one raw
point with its analytic gradient:
  u = xn / sqrt(ell),  f_s(x) = mp + sum_f W[s][f] cos(omega_f . u + phase_f) + sum_j c_s[j] k(X_j, xn),  W = sqrt(2 sf2 / F) weights,
  d f_s / d xn_a = -sum_f W[s][f] sin(.) omega[f][a] / sqrt(ell_a) + sum_j c_s[j] k_j (X_j - xn)_a / ell_a,
  value = Y_mean + Y_std f_s,  gradient in raw coordinates = Y_std (d f_s / d xn) / X_std.
coeffs():          W and c_s of every path of a set of draws;
path_value / path_grad / path_values: the path at a point, its gradient, the path at a list;
problem():         refine_sets_oracle.problem with the path as the objective (the constraint terms are refine_sets_oracle.terms');
objective(), kkt_residual(), slsqp(): as refine_sets_oracle's, on the path objective;
run():             the NumPy twin of the solver (refine_solver_twin.run's loop: csrc/refine.hip's ref_step and barrier stages,
                   csrc/pbfgs.hpp) on the path objective; ``drop`` leaves the last feature or the last observation out of the gradient;
CASES, make_case(): the committed cases, their models, draws and seeds.
"""
import functools

import numpy as np

import oracle
from safebo_amd import SweepEngine, synthetic

import batch_oracle as bo
import model_remove as mr
import paths_oracle as po
import refine_sets_oracle as rs
import refine_shapes as sh
import refine_solver_twin as tw

TOL64 = po.TOL64
KKT_BOX, KKT_TERMS = sh.KKT_BOX, sh.KKT_TERMS        # tests/test_gpu_refine.py's bars: box only / with constraint terms
PROGRESS = 1e-6                                      # tests/test_gpu_refine.py: "real progress"
STATUS = {"CONVERGED": 0, "MAX_EVAL": 1, "NO_PROGRESS": 2, "INFEASIBLE_SEED": 3, "ON_BOUNDARY": 4}
B = 2.0


# ---- the path as a function of one point -----------------------------------------------------------------------------------------------
def coeffs(ds, o, draws):
    """The per-path image of a set of draws on output o: W [S, F] (scaled weights), C [S, n] (c_s), and the constants."""
    omega, phase, weights, noise = (np.asarray(a, dtype=np.float64) for a in draws)
    ell, sf2, sn2 = bo.params(ds, o)
    mp = float(oracle.mean_prior(ds)[o])
    Xn = np.asarray(ds["X_norm"], dtype=np.float64)
    rs_ = 1.0 / np.sqrt(ell)
    W = np.sqrt(2.0 * sf2 / omega.shape[0]) * weights
    prior_X = np.cos((Xn * rs_) @ omega.T + phase) @ W.T                                    # [n, S]
    R = (np.asarray(ds["Y_norm"][:, o], dtype=np.float64) - mp)[:, None] - prior_X - np.sqrt(sn2) * noise.T
    C = np.linalg.solve(oracle.cov_mat(Xn, Xn, ell, sf2) + sn2 * np.eye(Xn.shape[0]), R).T
    return dict(o=o, W=W, C=C, omega=omega, phase=phase, ell=ell, sf2=sf2, mp=mp, Xn=Xn, ds=ds)


def _value_grad(co, s, x, drop=None):
    ds, o, ell = co["ds"], co["o"], co["ell"]
    xn = (np.asarray(x, dtype=np.float64) - ds["X_mean"]) / ds["X_std"]
    arg = co["omega"] @ (xn / np.sqrt(ell)) + co["phase"]
    w = co["W"][s]
    diff = co["Xn"] - xn
    k = co["sf2"] * np.exp(-0.5 * np.sum(diff * diff / ell, axis=1))
    c = co["C"][s]
    f = co["mp"] + w @ np.cos(arg) + c @ k
    gw, gc = w * np.sin(arg), c * k
    if drop == "feature":
        gw = gw[:-1]
    if drop == "observation":
        gc = gc[:-1]
    g = -(gw @ co["omega"][:len(gw)]) / np.sqrt(ell) + gc @ (diff[:len(gc)] / ell)
    ys = ds["Y_std"][o]
    return float(ys * f + ds["Y_mean"][o]), ys * g / ds["X_std"]


def path_value(co, s, x):
    """Path s at the raw point x [d], un-normalised."""
    return _value_grad(co, s, x)[0]


def path_grad(co, s, x, drop=None):
    """Its gradient [d] in raw coordinates."""
    return _value_grad(co, s, x, drop)[1]


def path_values(ds, o, draws, points):
    """Every path at a list [m, d] -> [m, S], un-normalised, by paths_oracle.paths_solve."""
    return ds["Y_mean"][o] + ds["Y_std"][o] * po.paths_solve(ds, o, draws, points)


# ---- the problem -----------------------------------------------------------------------------------------------------------------------
def problem(ds, b, lo, hi, co, s, maximize=False, safe=None):
    P = rs.problem(ds, b, lo, hi, "path", objective=co["o"], maximize=maximize, safe=safe)
    P["path"] = (co, s)
    return P


def objective(P, x, drop=None):
    """(f, grad) of the minimised function: the sign-adjusted path."""
    co, s = P["path"]
    f, g = _value_grad(co, s, x, drop)
    sg = -1.0 if P["maximize"] else 1.0
    return sg * f, sg * g


def value(P, x):
    return path_value(*P["path"], x)


def kkt_residual(P, x, active=1e-6):
    """refine_sets_oracle.kkt_residual with the path as f: ||grad f - sum lambda_i grad g_i||_inf / (1 + ||grad f||_inf), lambda >= 0
    by NNLS over the safe terms within ``active`` (relative: of Y_std_c + ||grad g||) of zero and the box faces x sits on."""
    from scipy.optimize import nnls
    x = np.asarray(x, dtype=np.float64)
    _, gf = objective(P, x)
    G = []
    ystd = np.abs(P["ds"]["Y_std"])
    for name, g, j in rs.terms(P, x):
        c = int("".join(ch for ch in name if ch.isdigit()))
        if g <= active * (ystd[c] + np.linalg.norm(j)):
            G.append(j)
    span = P["hi"] - P["lo"]
    for a in range(len(x)):
        e = np.zeros(len(x))
        if x[a] <= P["lo"][a] + active * span[a]:
            e[a] = 1.0
            G.append(e)
        elif x[a] >= P["hi"][a] - active * span[a]:
            e[a] = -1.0
            G.append(e)
    if G:
        A = np.array(G).T
        lam, _ = nnls(A, gf)
        res = gf - A @ lam
    else:
        res = gf
    return float(np.max(np.abs(res)) / (1.0 + np.max(np.abs(gf))))


def feasible(P, x):
    x = np.asarray(x, dtype=np.float64)
    return bool(np.all(np.isfinite(x))) and rs.feasible(P, x)[0]


def slsqp(P, seed):
    """SciPy SLSQP from the seed on the path objective, made feasible by bisection towards the seed: the yardstick."""
    from scipy.optimize import minimize
    n_terms = len(rs.terms(P, np.asarray(seed, float)))
    cons = [{"type": "ineq", "fun": (lambda z, i=i: rs.terms(P, z)[i][1]), "jac": (lambda z, i=i: rs.terms(P, z)[i][2])}
            for i in range(n_terms)]
    res = minimize(lambda z: objective(P, z), np.asarray(seed, dtype=np.float64), jac=True, method="SLSQP",
                   bounds=list(zip(P["lo"], P["hi"])), constraints=cons, options={"maxiter": 500, "ftol": 1e-14})
    return rs.make_feasible(P, np.clip(res.x, P["lo"], P["hi"]), seed)


# ---- the solver's twin on the path objective ---------------------------------------------------------------------------------------------
def run(P, seed, max_eval=tw.DEFAULT_EVAL, drop=None):
    """(status, evaluations, final barrier weight, x) of the twin from ``seed``: refine_solver_twin.run's loop with the path as the
    objective (k_refine_path: ref_path_eval, ref_path_advance).  ``drop``: "feature" / "observation" leaves the last one out of the
    path's gradient -- the faults the KKT bar has to tell."""
    import refine_oracle as ro
    ds, b, lo, hi, d = P["ds"], P["b"], P["lo"], P["hi"], P["d"]
    ys = ds["Y_std"]
    MU0, MUSTEP, MUFLOOR, TOL = tw.MU0, tw.MUSTEP, tw.MUFLOOR, tw.TOL
    span = hi - lo; D2 = span * span; cap = 0.1
    o = P["objective"]

    def terms(x):
        sf, sgf = objective(P, x, drop)
        fo, go = sf / ys[o], sgf / ys[o]
        B_, gB = 0.0, np.zeros(d)
        if P["safe"]:
            m, v, gm, gv = ro.posterior_grad(x, ds)
            for c in P["safe"]:
                if not v[c] > 0: return False, 0, 0, 0, 0
                sd = np.sqrt(v[c]); gc = m[c] - b * sd
                if not gc > 0: return False, 0, 0, 0, 0
                ggc = gm[c] - b * gv[c] / (2 * sd)
                B_ -= np.log(gc / ys[c]); gB -= ggc / gc
        ok = bool(np.isfinite(fo) and np.all(np.isfinite(go)) and np.isfinite(B_) and np.all(np.isfinite(gB)))
        return ok, fo, go, B_, gB

    st = dict(x=np.array(seed, float), H=np.diag(D2), hid=1, t=0.0, halv=0)
    nev = 0
    ok, fo, go, B_, gB = terms(st["x"]); nev += 1
    if not ok:
        return "NO_PROGRESS", nev, 0.0, st["x"]
    mu = MU0 if P["safe"] else MUFLOOR
    S_ = dict(fo=fo, go=go, B=B_, gB=gB)

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

    if nev >= max_eval:
        return "MAX_EVAL", nev, mu, st["x"]
    trial = new_iter()
    status = "CONVERGED"
    while trial is not None:
        ok, fo, go, B_, gB = terms(trial); nev += 1
        dec = st["g"] @ (trial - st["x"]); moved = bool(np.any(trial != st["x"]))
        if ok and moved and fo + mu * B_ <= st["f"] + 1e-4 * dec:
            S_.update(fo=fo, go=go, B=B_, gB=gB)
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
            if abs(fprev - (fo + mu * B_)) <= 1e-15 * (1 + abs(fprev)): trial = stage_end()
            else: trial = new_iter()
            continue
        if nev >= max_eval: status = "MAX_EVAL"; break
        if moved and st["halv"] < 60:
            st["halv"] += 1; st["t"] *= 0.5; trial = np.clip(st["x"] + st["t"] * st["p"], lo, hi); continue
        if st["hid"]: trial = stage_end(); continue
        st["H"] = np.diag(D2); st["hid"] = 1
        trial = new_iter()
    return status, nev, mu, st["x"]


# ---- the committed cases ---------------------------------------------------------------------------------------------------------------
# Each edge once, not the product.  By the constants of csrc/refine.hip (tests/test_refine_paths_cpu.py reads them from the source):
#   ref_path_eval  threads stride over the F features, then over the n observations: 256 threads up to n = 256 (F in {1, 255, 256,
#                  257}), 1024 above (F in {1023, 1025}); the cap F = SBO_MAX_FEATURES = 8192; n in {1, 2, 20, 256, 257, 512};
#   LDS tier       the constraint slots' packed triangles fit kRefLdsM = 144 KiB up to n = 191 at one slot and 135 at two: both sides;
#   budget         n = SBO_MAX_N = 2048 with max_eval = 60 (tests/test_gpu_refine.py's large case);
#   grid           S in {1, 17, 64}, K in {1, 3, 64}, and S K = 4096 workgroups at n = 20;
#   padded lanes   d in {1, 2, 3, 4, 6, 8};  outputs: q in {1 (empty mask), 2, 4}, the first and the last output as the path's, one case
#                  whose path output is also a constraint; both values of maximize; both factor sources.
# Replaced on the twin's evidence (tests/test_refine_paths_cpu.py): n = 256, d = 3 maximised ends with one box face and the constraint
# active, where twin and device stall alike (refine_solver_twin.py's note) -- it is minimised; the shared-output case (the path of
# constraint 1 minimised onto lcb_1 = 0) needs 331 - 709 evaluations on the twin: it runs under tests/refine_shapes.py's raised budget.
# ``safe``: the constraint outputs; ``bad``: the last start of the last path is replaced by an infeasible seed; ``kkt``: "diag" holds only
# the problems (s, s) to the KKT bar and the twin (4096 twin runs are minutes of NumPy).
def _c(n, F, S, K, d, q, output, safe, maximize, use_invK, seed, **kw):
    return dict(n=n, F=F, S=S, K=K, d=d, q=q, output=output, safe=list(safe), maximize=maximize, use_invK=use_invK, seed=seed, **kw)


N1, N2 = sh.largest_staged(1), sh.largest_staged(2)          # 191, 135
CASES = [
    _c(1, 1, 1, 1, 2, 1, 0, (), 0, True, 201),
    _c(2, 255, 17, 3, 1, 2, 1, (), 1, False, 202, bad=True),
    _c(20, 256, 4, 3, 2, 2, 0, (1,), 0, True, 203, bad=True),
    _c(256, 257, 3, 2, 3, 2, 0, (1,), 0, False, 204),
    _c(257, 1023, 2, 2, 4, 4, 0, (1, 2, 3), 0, True, 205),
    _c(512, 1025, 2, 1, 6, 4, 3, (1, 2), 1, False, 206),
    _c(40, 8192, 2, 1, 2, 2, 0, (1,), 0, True, 207),
    _c(N1, 64, 2, 2, 2, 2, 0, (1,), 0, True, 208),
    _c(N1 + 1, 64, 2, 2, 2, 2, 0, (1,), 0, False, 209),
    _c(N2, 64, 2, 2, 2, 4, 0, (1, 2), 0, True, 210),
    _c(N2 + 1, 64, 2, 2, 2, 4, 0, (1, 2), 0, False, 211),
    _c(2048, 256, 2, 1, 2, 2, 0, (1,), 0, False, 212, max_eval=60, log_sn=-1.0),
    _c(20, 64, 64, 1, 2, 2, 0, (1,), 0, True, 213),
    _c(20, 64, 1, 64, 2, 2, 0, (1,), 1, True, 214),
    _c(20, 32, 64, 64, 2, 2, 0, (1,), 0, True, 215, kkt="diag"),
    _c(200, 128, 2, 2, 8, 2, 0, (1,), 0, True, 216),
    _c(40, 128, 3, 2, 2, 2, 1, (1,), 0, False, 217, max_eval=sh.RAISED_EVAL),
]


def case_id(c):
    return "n{n}-F{F}-S{S}-K{K}-d{d}-q{q}-o{output}-c{nc}-{end}-{src}".format(
        nc=len(c["safe"]), end="max" if c["maximize"] else "min", src="invK" if c["use_invK"] else "hyper", **c)


def model(n, d, q, seed, log_sn=None):
    """Uniform rows in [-1, 1]^d; output 0 a bowl with a ripple, constraint c = 0.8 - 0.1 (c - 1) - mean |x| + a ripple: safe around
    the centre.  n < 30 takes the first rows of a 30-row set under that set's constants (batch_oracle.make_case's rule)."""
    rng = np.random.default_rng(5000 + seed)
    X = rng.uniform(-1.0, 1.0, size=(max(n, 30), d))
    cols = [np.sum(X ** 2, axis=1) + 0.3 * np.sin(3.0 * X[:, 0])]
    for c in range(1, q):
        cols.append(0.8 - 0.1 * (c - 1) - np.sum(np.abs(X), axis=1) / d + 0.05 * np.sin(2.0 * X[:, c % d] + c))
    hyp = synthetic.default_hypopt(d, q, log_ell=-0.5 if d <= 2 else 0.0 if d <= 4 else 0.5, **({} if log_sn is None else {"log_sn": log_sn}))
    ds0 = synthetic.make_dataset(X, np.stack(cols, axis=1), hyp)
    return ds0 if n == X.shape[0] else mr.with_rows(ds0, ds0["X_norm"][:n], ds0["Y_norm"][:n])


MARGIN = 0.02        # a seed's lcb_c, in Y_std_c: strictly inside the safe set
POOL = 256


def pick_seeds(ds, c, draws, lo, hi, rng):
    """[S, K, d]: per path the K members of a pool (256 uniform box points and the observed inputs) that are safe with a margin and have
    the best path values -- what a host class hands over from a grid.  ``bad``: the last start of the last path is the pool's least
    safe member (with constraints) or a point outside the box."""
    d, S, K, o = c["d"], c["S"], c["K"], c["output"]
    pool = np.vstack([rng.uniform(lo, hi, size=(POOL, d)), ds["X_norm"] * ds["X_std"] + ds["X_mean"]])
    pool = pool[np.all((pool >= lo) & (pool <= hi), axis=1)]
    m, v = oracle.gp_inference(pool, ds)
    lcb = (m - B * np.sqrt(v)) / ds["Y_std"]
    ok = np.all(lcb[:, c["safe"]] >= MARGIN, axis=1) if c["safe"] else np.ones(len(pool), dtype=bool)
    assert ok.any(), case_id(c)
    f = path_values(ds, o, draws, pool[ok])
    order = np.argsort(-f if c["maximize"] else f, axis=0, kind="stable")                  # [members, S]
    seeds = np.stack([pool[ok][order[np.arange(K) % order.shape[0], s]] for s in range(S)])
    if c.get("bad"):
        seeds[-1, -1] = pool[np.argmin(lcb[:, c["safe"]].min(axis=1))] if c["safe"] else hi + 0.5
    return seeds


@functools.lru_cache(maxsize=None)
def make_case(i):
    """Case i, computed once per process and never modified: dict(ds, lo, hi, draws, co, seeds [S, K, d], problems [S] (one per path))."""
    c = CASES[i]
    ds = model(c["n"], c["d"], c["q"], c["seed"], c.get("log_sn"))
    lo, hi = -np.ones(c["d"]), np.ones(c["d"])
    draws = SweepEngine.path_draws(c["d"], c["n"], c["S"], c["F"], c["seed"])
    co = coeffs(ds, c["output"], draws)
    seeds = pick_seeds(ds, c, draws, lo, hi, np.random.default_rng(7000 + c["seed"]))
    seeds.setflags(write=False)
    probs = [problem(ds, B, lo, hi, co, s, bool(c["maximize"]), c["safe"]) for s in range(c["S"])]
    return dict(ds=ds, lo=lo, hi=hi, draws=draws, co=co, seeds=seeds, problems=probs)


def held(c):
    """The problems (s, k) of a case that are held to the KKT bar and run through the twin (none where the budget is cut to 60)."""
    if c["n"] == 2048:
        return []
    if c.get("kkt") == "diag":
        return [(s, s) for s in range(min(c["S"], c["K"]))]
    return [(s, k) for s in range(c["S"]) for k in range(c["K"])]


def kkt_bar(c):
    return KKT_TERMS if c["safe"] else KKT_BOX


def engine_args(c, case):
    """Keyword arguments of SweepEngine.refine_paths for the case."""
    return dict(output=c["output"], draws=case["draws"], maximize=bool(c["maximize"]), constraints=c["safe"], lo=case["lo"], hi=case["hi"],
                max_eval=c.get("max_eval"))
