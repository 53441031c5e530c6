"""NumPy / SciPy reference for sbo_refine and sbo_refine_sets -- test infrastructure only.

sbo_refine's problem (a bound of one output s.t. lcb_c(x) >= 0, the box and the trust-region ball) and the four set-valued steps
as continuous problems on z = x (single mode) or z = (x, x') (pair mode), built on refine_oracle.bound_grad:

    M_t      max var_0(x)    s.t. lcb_c(x) >= 0, lcb_0(x) <= u*                                   models/SafeOpt.py:53-66
    G_t      max var_0(x)    s.t. lcb_c(x) >= 0, lcb_c(x') <= 0, ucb_i(x) - L ||x - x' + 1e-8|| >= 0      :90-124
    target   min lcb_0(x')   s.t. the same                                                        models/GoOSE.py:80-114
    explore  min ||x - t||   s.t. lcb_c(x) >= 0                                                           :116-119

problem():       a problem description (a dict);
terms():         every inequality term g_i(z) >= 0 with its analytic Jacobian;
objective():     the minimised function (sign-adjusted) with its gradient, and value(): what the device reports;
feasible():      the exact predicate checker (closed predicates, box included) and the smallest slack;
slsqp():         SciPy SLSQP from a seed;  make_feasible(): bisection back to the feasible seed for pairs too;
kkt_residual():  stationarity residual at a point, multipliers of the (nearly) active terms and box faces by NNLS;
grid_case():     the grid sweep of a fixture and the seeds the host classes take from it.
"""
import os

import numpy as np

import oracle
import refine_oracle as ro

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRIDS = {"benoit_n20_50x50": [50, 50], "benoit_n128_64x48": [64, 48], "wo3_n64_48x40": [48, 40], "benoit_n4_40x40": [40, 40],
         "rosen4_n128_9x8x7x6": [9, 8, 7, 6]}


def problem(ds, b, lo, hi, kind, objective=0, at="x", maximize=False, safe=None, unsafe=None, level=None, link=None, target=None,
            pair=False, ball=None):
    """``ball``: (x_0, r) of the term r^2 - ||x - x_0||^2 >= 0."""
    q = ds["Y_norm"].shape[1]
    return {"ds": ds, "b": float(b), "lo": np.asarray(lo, float), "hi": np.asarray(hi, float), "kind": kind, "objective": objective,
            "at": at, "maximize": maximize, "safe": list(range(1, q)) if safe is None else list(safe),
            "unsafe": (list(range(1, q)) if pair else []) if unsafe is None else list(unsafe), "level": level, "link": link,
            "target": None if target is None else np.asarray(target, float), "pair": pair, "d": len(lo),
            "ball": None if ball is None else (np.asarray(ball[0], float), float(ball[1]))}


def split(P, z):
    z = np.asarray(z, dtype=np.float64)
    d = P["d"]
    return z[:d], (z[d:] if P["pair"] else None)


def engine_args(P):
    """Keyword arguments of SweepEngine.refine_sets for the problem."""
    x_0, r = P["ball"] if P["ball"] is not None else (None, None)
    return dict(objective=P["objective"], kind=P["kind"], at=P["at"], maximize=P["maximize"], safe=P["safe"], unsafe=P["unsafe"],
                level=P["level"], link=P["link"], target=P["target"], lo=P["lo"], hi=P["hi"], x_0=x_0, r=r)


def shifted(x, xp):
    diff = x - xp + 1e-8
    return np.sqrt(np.sum(diff * diff)), diff


def terms(P, z):
    """[(name, g, jac [len z])] with g >= 0 feasible: safe, ball, level, unsafe, link (no box)."""
    x, xp = split(P, z)
    d, nz, ds, b = P["d"], len(z), P["ds"], P["b"]
    out = []
    for c in P["safe"]:
        g, gg = ro.bound_grad(x, ds, b, c, "lcb")
        j = np.zeros(nz)
        j[:d] = gg
        out.append((f"safe{c}", g, j))
    if P["ball"] is not None:
        x_0, r = P["ball"]
        j = np.zeros(nz)
        j[:d] = -2.0 * (x - x_0)
        out.append(("ball", r * r - np.sum((x - x_0) ** 2), j))
    if P["level"] is not None:
        o, lv = P["level"]
        g, gg = ro.bound_grad(x, ds, b, o, "lcb")
        j = np.zeros(nz)
        j[:d] = -gg
        out.append(("level", lv - g, j))
    for c in P["unsafe"]:
        g, gg = ro.bound_grad(xp, ds, b, c, "lcb")
        j = np.zeros(nz)
        j[d:] = -gg
        out.append((f"unsafe{c}", -g, j))
    if P["link"] is not None:
        c, L = P["link"]
        u, gu = ro.bound_grad(x, ds, b, c, "ucb")
        nrm, diff = shifted(x, xp)
        j = np.zeros(nz)
        j[:d] = gu - L * diff / nrm
        j[d:] = L * diff / nrm
        out.append(("link", u - L * nrm, j))
    return out


def value(P, z):
    """The figure the device reports: the bound at the objective's point, or the Euclidean distance to the target."""
    x, xp = split(P, z)
    if P["kind"] == "dist":
        return float(np.sqrt(np.sum((x - P["target"]) ** 2)))
    return float(ro.bound_grad(xp if P["at"] == "xp" else x, P["ds"], P["b"], P["objective"], P["kind"])[0])


def objective(P, z):
    """(f, grad) of the minimised function (dist: the squared distance)."""
    x, xp = split(P, z)
    d = P["d"]
    g = np.zeros(len(z))
    if P["kind"] == "dist":
        f = float(np.sum((x - P["target"]) ** 2))
        g[:d] = 2.0 * (x - P["target"])
        return f, g
    at_p = P["at"] == "xp"
    f, gf = ro.bound_grad(xp if at_p else x, P["ds"], P["b"], P["objective"], P["kind"])
    if at_p:
        g[d:] = gf
    else:
        g[:d] = gf
    sg = -1.0 if P["maximize"] else 1.0
    return sg * f, sg * g


def box(P):
    reps = 2 if P["pair"] else 1
    return np.tile(P["lo"], reps), np.tile(P["hi"], reps)


def feasible(P, z):
    """(every term holds under the closed predicates -- box included --, the smallest slack over the terms)."""
    lo, hi = box(P)
    z = np.asarray(z, dtype=np.float64)
    if not (np.all(z >= lo) and np.all(z <= hi)):
        return False, -np.inf
    gs = [g for _, g, _ in terms(P, z)]
    slack = min(gs) if gs else np.inf
    return bool(slack >= 0.0), float(slack)


def slsqp(P, seed):
    from scipy.optimize import minimize
    lo, hi = box(P)
    names = [t[0] for t in terms(P, np.asarray(seed, float))]
    cons = [{"type": "ineq", "fun": (lambda z, i=i: terms(P, z)[i][1]), "jac": (lambda z, i=i: terms(P, z)[i][2])}
            for i in range(len(names))]
    res = minimize(lambda z: objective(P, z), np.asarray(seed, dtype=np.float64), jac=True, method="SLSQP", bounds=list(zip(lo, hi)),
                   constraints=cons, options={"maxiter": 500, "ftol": 1e-14})
    return np.clip(res.x, lo, hi), res


def make_feasible(P, z, seed, steps=80):
    """z when every term holds there, else the feasible end of a bisection on the segment from the feasible seed towards z."""
    z, seed = np.asarray(z, dtype=np.float64), np.asarray(seed, dtype=np.float64)
    if feasible(P, z)[0]:
        return z
    lo_t, hi_t = 0.0, 1.0
    for _ in range(steps):
        t = 0.5 * (lo_t + hi_t)
        if feasible(P, seed + t * (z - seed))[0]:
            lo_t = t
        else:
            hi_t = t
    return seed + lo_t * (z - seed)


def kkt_residual(P, z, active=1e-6):
    """||grad f - sum lambda_i grad g_i||_inf / (1 + ||grad f||_inf), lambda >= 0 by NNLS over the terms within ``active``
    (relative: of Y_std_c + ||grad g||, the ball of r^2) of their bound and the box faces z sits on.  f is the minimised function."""
    from scipy.optimize import nnls
    z = np.asarray(z, dtype=np.float64)
    _, gf = objective(P, z)
    if P["kind"] == "dist":
        gf = gf / max(float(np.sum((P["hi"] - P["lo"]) ** 2)), 1e-300)
    G = []
    ystd = np.abs(P["ds"]["Y_std"])
    for name, g, j in terms(P, z):
        if name == "ball":
            near = active * P["ball"][1] * P["ball"][1]
        else:
            c = P["level"][0] if name == "level" else P["link"][0] if name == "link" else int("".join(ch for ch in name if ch.isdigit()))
            near = active * (ystd[c] + np.linalg.norm(j))
        if g <= near:
            G.append(j)
    lo, hi = box(P)
    span = hi - lo
    for a in range(len(z)):
        e = np.zeros(len(z))
        if z[a] <= lo[a] + active * span[a]:
            e[a] = 1.0
            G.append(e)
        elif z[a] >= hi[a] - active * span[a]:
            e[a] = -1.0
            G.append(e)
    if G:
        A = np.array(G).T
        lam, _ = nnls(A, gf)
        res = gf - A @ lam
    else:
        res = gf
    return float(np.max(np.abs(res)) / (1.0 + np.max(np.abs(gf))))


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    from safebo_amd import synthetic
    return synthetic.make_dataset(z["X"], z["Y"], z["hypopt"]), float(z["b"]), z["bound"][:, 0].copy(), z["bound"][:, 1].copy()


_cases = {}


def grid_case(name, quirk=True):
    """The fixture's grid sweeps (NumPy oracle) and the problems with the seeds the host classes take from them:
    {"M": (P, seed), "G": [(P, seed) per constraint with a non-empty G_c], "T": [(P, seed) per non-empty O_c], "E": (P, seed)}."""
    if (name, quirk) in _cases:
        return _cases[(name, quirk)]
    ds, b, lo, hi = load(name)
    pts = oracle.grid_points(lo, hi, GRIDS[name])
    mv = oracle.gp_inference(pts, ds)
    so = oracle.safeopt_sweep(pts, ds, b, quirk, mean_var=mv)
    go = oracle.goose_sweep(pts, ds, b, quirk, mean_var=mv)
    q = mv[0].shape[1]
    case = {"ds": ds, "b": b, "lo": lo, "hi": hi, "pts": pts, "safeopt": so, "goose": go, "G": [], "T": []}
    case["M"] = (problem(ds, b, lo, hi, "var", maximize=True, level=(0, float(so["u_star"]))), pts[so["minimizer_index"]].copy())
    Uidx = np.nonzero(so["U"])[0]
    for c in range(1, q):
        Lc = float(so["L_used"][c])
        g = int(so["expander_index"][c - 1])
        if g >= 0:
            h = Uidx[np.argmin(oracle.shifted_norm(pts[g][None, :], pts[Uidx]))]
            case["G"].append((problem(ds, b, lo, hi, "var", maximize=True, link=(c, Lc), pair=True), np.concatenate([pts[g], pts[h]])))
        t = int(go["target_index_c"][c - 1])
        if t >= 0:
            ok = so["S"] & (so["ucb"][:, c] - Lc * oracle.shifted_norm(pts, pts[t][None, :]) >= 0)
            idx = np.nonzero(ok)[0]
            g = idx[np.argmin(oracle.shifted_norm(pts[idx], pts[t][None, :]))]
            case["T"].append((problem(ds, b, lo, hi, "lcb", at="xp", link=(c, Lc), pair=True), np.concatenate([pts[g], pts[t]])))
    if go["target_index"] >= 0:
        case["E"] = (problem(ds, b, lo, hi, "dist", target=pts[go["target_index"]]), pts[go["explore_index"]].copy())
    _cases[(name, quirk)] = case
    return case


def yardstick(P, seed):
    """(value at the seed, value of the feasible SLSQP answer, that answer)."""
    z, _ = slsqp(P, seed)
    z = make_feasible(P, z, seed)
    return value(P, seed), value(P, z), z
