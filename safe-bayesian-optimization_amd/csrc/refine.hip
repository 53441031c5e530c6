// refine.hip -- sbo_refine: local refinement of an acquisition optimum off the candidate grid.
//
// The sweeps restate every continuous acquisition of the reference (SciPy DE in models/SafeOpt.py:47-51, models/GoOSE.py:63-67,
// models/GP_TR.py:43-51; SLSQP multistarts in models/BayesRTOjax.py:17-85) as an arg-min over candidates.  This file polishes such
// a winner: one workgroup per seed runs a projected BFGS on a log-barrier function of the exact fp64 posterior (box by projection,
// lcb_c >= 0 and the trust-region ball by the barrier), the whole iteration inside one launch.  The projected BFGS is the core
// k_fit_local runs (pbfgs.hpp), here in the metric of the box spans; the barrier stages and the evaluation budget are this file's.  The
// candidates it returns are then re-evaluated by the library's exact list evaluator (launch_posterior_on_list, the values
// sbo_bounds gives at those points) and accepted only when they pass the sweep's S predicate there and are no worse than the seed.
//
// sbo_refine_sets runs the same solver on the set-valued steps (SafeOpt's M_t / G_t, GoOSE's target and explore_safeset): the
// variables are one point x or a pair z = (x, x'), and the barrier also carries a level term (level - lcb_o(x) >= 0), U-membership
// of x' (lcb_c(x') <= 0) and the Lipschitz link ucb_c(x) - L ||x - x' + 1e-8|| >= 0.  A pair is evaluated in one pass over M's rows.
//
// sbo_refine_robust solves StableOpt's min-max (models/StableOpt.py:97-152) by outer approximation over a small set of disturbance
// scenarios: k_refine polishes the separation's points over d with the controls held, and k_refine_robust runs the same barrier
// stages on z = (xc, t), evaluating the scenarios' joint points with ref_eval.
#include <algorithm>
#include <cmath>
#include <vector>
#include "internal.hpp"
#include "device_common.hpp"
#include "pbfgs.hpp"

namespace sbo {

constexpr int kRefWaves = 16;                    // (1024 threads at most)
constexpr double kRefMu0 = 1e-3;                 // barrier weight of the first stage (normalised objective units)
constexpr double kRefMuStep = 0.1;               // geometric decrease per stage ...
constexpr double kRefMuFloor = 1e-11;            // ... down to this floor
constexpr int kRefDefaultEval = 400;             // posterior + gradient evaluations per seed
constexpr int kRefMaxEval = 20000;               // ceiling of max_eval, lowered further for large n (sbo_refine)
constexpr double kRefDefaultTol = 1e-9;          // projected-gradient inf-norm of the barrier function, in box-scaled coordinates
constexpr size_t kRefLdsM = 144 * 1024;          // LDS tier: the used outputs' packed lower triangles of M fit in this many bytes

struct RefineArgs {
  ModelConst mc;
  int nu;                    // distinct outputs evaluated (objective first)
  int obj_slot;              // (always 0; unused by SBO_REFINE_DIST)
  int con_slots;             // bit u: slot u is a constraint (lcb >= 0 at x)
  int kind, maximize, use_ball, max_eval, f_cap, a_ld, pad;
  int outs[kMaxQ];           // slot -> output index
  double b, tol, r;
  double lo[kMaxD], hi[kMaxD], x0[kMaxD];   // lo / hi: the box of every solver variable (pair: the point's box twice)
  // sbo_refine_sets (sbo_refine: np = 1, nz = d, no further term)
  int np, nz;                // points per variable vector (1: x, 2: x and x') and solver variables np * d
  int obj_point;             // the point the objective is taken at
  int unsafe_slots;          // bit u: lcb of slot u <= 0 at x'
  int level_slot, link_slot; // -1, or the slot of the level term (lcb <= level at x) / of the link (ucb at x)
  double level, L, dscale;   // dscale: SBO_REFINE_DIST's normalisation (the box diagonal squared)
  double tgt[kMaxD];         // SBO_REFINE_DIST: the point t of ||x - t||^2
};

// one evaluation of one point: per used slot the un-normalised mean / var and their gradients
struct RefEval {
  double m[kMaxQ], v[kMaxQ], gm[kMaxQ][kMaxD], gv[kMaxQ][kMaxD];
  int clamp[kMaxQ];
};

struct RefState {
  PbfgsState<kMaxD> s;                    // the shared core's state (pbfgs.hpp); s.g = go + mu gB
  double D2[kMaxD], span[kMaxD], xb[kMaxD];   // the metric span^2, the (ball-limited) box widths, the best-objective iterate
  double fo, B, go[kMaxD], gB[kMaxD];     // objective part and barrier sum at x, with gradients
  double f, mu, obj, objb;                // f = fo + mu B; obj / objb: sign-adjusted objective at x / at xb
  int phase, nev, status, nbar;
};
enum { REF_PH_START = 0, REF_PH_SEARCH = 1 };

// the box of the solver's variables in the metric of its spans; a steepest-descent step moves at most a tenth of the
// (ball-limited) box
__device__ __forceinline__ PbfgsBox ref_box(const RefState& S, const RefineArgs& A) { return {A.lo, A.hi, S.D2, S.span, 0.1}; }

// the LDS tier's copy of M: the used outputs' lower triangles out of the resident factor, packed row after row (one wave per row) -> Ml
__device__ __forceinline__ void ref_load_M(const RefineArgs& A, const double* F, double* Ml) {
  const int n = A.mc.n, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const size_t tri = (size_t)n * (n + 1) / 2;
  for (int u = 0; u < A.nu; ++u) {
    const double* Fo = F + (size_t)A.outs[u] * A.f_cap * A.f_cap;
    for (int i = wave; i < n; i += nw)
      for (int j = lane; j <= i; j += 64) Ml[u * tri + (size_t)i * (i + 1) / 2 + j] = Fo[(size_t)i * A.f_cap + j];
  }
}

// mean / var and their gradients at the kP points of x (LDS, point p at x + p d) for every used output -> E[p].  M rows: LDS
// packed triangles (kLds) or the resident factor (stride f_cap); every element of M is read once per pass and serves the kP points (kv / uv
// [kP][n], red [kP][2 (kMaxD + 1)], uup [kP][kRefWaves]).  Each point's sums run in the order of a one-point evaluation.
template <bool kLds, int kP>
__device__ void ref_eval(const RefineArgs& A, const double* x, const double* F, const double* Ml, const double* alpha,
                         const double* Xn, double* kv, double* uv, double (*part)[kMaxD + 1], double* red, double* uup, RefEval* E) {
  const ModelConst& mc = A.mc;
  const int n = mc.n, d = mc.d, dp = mc.dpad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6, bd = blockDim.x;
  const size_t tri = (size_t)n * (n + 1) / 2;
  constexpr int kRed = 2 * (kMaxD + 1);
  double xn[kP][kMaxD];
#pragma unroll
  for (int p = 0; p < kP; ++p)
#pragma unroll
    for (int a = 0; a < kMaxD; ++a) xn[p][a] = a < d ? (x[p * d + a] - mc.X_mean[a]) / mc.X_std[a] : 0.0;
  for (int u = 0; u < A.nu; ++u) {
    const int o = A.outs[u];
    const double* Mo = kLds ? Ml + (size_t)u * tri : F + (size_t)o * A.f_cap * A.f_cap;
    const double* al = alpha + (size_t)o * A.a_ld;
    const double sf2 = mc.sf2[o];
    double ie[kMaxD];
#pragma unroll
    for (int a = 0; a < kMaxD; ++a) ie[a] = mc.inv_ell[o][a];
    // k_j, k . alpha and its gradient
    double acc[kP][kMaxD + 1];
#pragma unroll
    for (int p = 0; p < kP; ++p)
#pragma unroll
      for (int a = 0; a < kMaxD + 1; ++a) acc[p][a] = 0.0;
    for (int j = tid; j < n; j += bd) {
#pragma unroll
      for (int p = 0; p < kP; ++p) {
        double diff[kMaxD], dist = 0.0;
#pragma unroll
        for (int a = 0; a < kMaxD; ++a) {
          diff[a] = a < d ? Xn[(size_t)j * dp + a] - xn[p][a] : 0.0;
          if (a < d) dist += diff[a] * diff[a] * ie[a];
        }
        const double kj = sf2 * exp(-0.5 * dist);
        kv[p * n + j] = kj;
        const double ak = al[j] * kj;
        acc[p][0] += ak;
#pragma unroll
        for (int a = 0; a < kMaxD; ++a)
          if (a < d) acc[p][1 + a] += ak * diff[a] * ie[a];
      }
    }
#pragma unroll
    for (int p = 0; p < kP; ++p) block_sum_cols(acc[p], d + 1, part, red + p * kRed);   // (its barriers also publish kv)
    // u = M k (one wave per row, rows in order), u . u
    double uu[kP];
#pragma unroll
    for (int p = 0; p < kP; ++p) uu[p] = 0.0;
    for (int i = wave; i < n; i += nw) {
      const double* row = Mo + (kLds ? (size_t)i * (i + 1) / 2 : (size_t)i * A.f_cap);
      double s[kP];
#pragma unroll
      for (int p = 0; p < kP; ++p) s[p] = 0.0;
      for (int j = lane; j <= i; j += 64) {
        const double mij = row[j];
#pragma unroll
        for (int p = 0; p < kP; ++p) s[p] += mij * kv[p * n + j];
      }
#pragma unroll
      for (int p = 0; p < kP; ++p) {
        for (int off = 32; off > 0; off >>= 1) s[p] += __shfl_xor(s[p], off);
        if (lane == 0) {
          uv[p * n + i] = s[p];
          uu[p] += s[p] * s[p];
        }
      }
    }
    if (lane == 0)
#pragma unroll
      for (int p = 0; p < kP; ++p) uup[p * kRefWaves + wave] = uu[p];
    __syncthreads();
    // w = M^T u, and sum_j w_j dk_j / dx
    double gacc[kP][kMaxD + 1];
#pragma unroll
    for (int p = 0; p < kP; ++p)
#pragma unroll
      for (int a = 0; a < kMaxD + 1; ++a) gacc[p][a] = 0.0;
    for (int j0 = 0; j0 < n; j0 += bd) {
      const int j = j0 + tid;
      const int jw = j0 + (wave << 6);              // the wave's first column: rows above it hold nothing for the wave
      double w[kP];
#pragma unroll
      for (int p = 0; p < kP; ++p) w[p] = 0.0;
      for (int i = jw; i < n; ++i)
        if (i >= j && j < n) {
          const double mij = Mo[(kLds ? (size_t)i * (i + 1) / 2 : (size_t)i * A.f_cap) + j];
#pragma unroll
          for (int p = 0; p < kP; ++p) w[p] += mij * uv[p * n + i];
        }
      if (j < n) {
#pragma unroll
        for (int p = 0; p < kP; ++p) {
          const double wk = w[p] * kv[p * n + j];
#pragma unroll
          for (int a = 0; a < kMaxD; ++a)
            if (a < d) gacc[p][a] += wk * (Xn[(size_t)j * dp + a] - xn[p][a]) * ie[a];
        }
      }
    }
#pragma unroll
    for (int p = 0; p < kP; ++p) block_sum_cols(gacc[p], d, part, red + p * kRed + kMaxD + 1);
    if (tid == 0) {
      for (int p = 0; p < kP; ++p) {
        const double* rd = red + p * kRed;
        double s = 0.0;
        for (int w = 0; w < nw; ++w) s += uup[p * kRefWaves + w];
        const double ys = mc.Y_std[o], vn = sf2 - s;
        E[p].m[u] = ys * (mc.mp[o] + rd[0]) + mc.Y_mean[o];
        E[p].v[u] = ys * ys * (vn > 0.0 ? vn : 0.0);
        E[p].clamp[u] = !(vn > 0.0);
        for (int a = 0; a < d; ++a) {
          E[p].gm[u][a] = ys * rd[1 + a] / mc.X_std[a];
          E[p].gv[u][a] = -2.0 * ys * ys * rd[kMaxD + 1 + a] / mc.X_std[a];
        }
      }
    }
    __syncthreads();                                // (kv / uv are rewritten for the next output)
  }
}

// lcb (sgn = -1) or ucb (+1) of slot u at an evaluation, with its gradient; false where the variance gives none
__device__ bool ref_conf(const RefEval& E, int u, double b, double sgn, int d, double& g, double* gg) {
  g = E.m[u];
  for (int a = 0; a < d; ++a) gg[a] = E.gm[u][a];
  if (b != 0.0) {
    if (E.clamp[u] || !(E.v[u] > 0.0)) return false;
    const double sd = sqrt(E.v[u]);
    g = E.m[u] + sgn * b * sd;
    for (int a = 0; a < d; ++a) gg[a] += sgn * b * E.gv[u][a] / (2.0 * sd);
  }
  return true;
}

// the safe-set terms lcb_c(x) > 0 of the constraint slots, in slot order, added to the barrier sum (B, gB); false: the trial is rejected
__device__ __forceinline__ bool ref_safe_terms(const RefineArgs& A, const RefEval& E, double& B, double* gB) {
  const int d = A.mc.d;
  for (int u = 0; u < A.nu; ++u) {
    if (!((A.con_slots >> u) & 1)) continue;
    double gc, ggc[kMaxD];
    if (!ref_conf(E, u, A.b, -1.0, d, gc, ggc)) return false;
    if (!(gc > 0.0)) return false;
    B -= log(gc / A.mc.Y_std[A.outs[u]]);
    for (int a = 0; a < d; ++a) gB[a] -= ggc[a] / gc;
  }
  return true;
}

// objective part (fo, go; obj = sign-adjusted objective) and barrier sum (B, gB) at x (pair: x, x') from the evaluation of its
// points; false: the trial is rejected
__device__ bool ref_terms(const RefineArgs& A, const RefEval* Ev, const double* x, double& fo, double* go, double& B, double* gB, double& obj) {
  const int d = A.mc.d, nz = A.nz;
  const double b = A.b;
  const RefEval& E = Ev[0];                               // (the evaluation at x)
  double f, gf[kMaxD], ys;
  for (int a = 0; a < nz; ++a) gf[a] = 0.0;
  if (A.kind == SBO_REFINE_DIST) {
    f = 0.0;
    for (int a = 0; a < d; ++a) {
      const double df = x[a] - A.tgt[a];
      f += df * df;
      gf[a] = 2.0 * df;
    }
    ys = A.dscale;
  } else {
    const RefEval& Eo = Ev[A.obj_point];
    double* gp = gf + A.obj_point * d;
    const int u0 = A.obj_slot;
    if (A.kind == SBO_MEAN || ((A.kind == SBO_UCB || A.kind == SBO_LCB) && b == 0.0)) {
      f = Eo.m[u0];
      for (int a = 0; a < d; ++a) gp[a] = Eo.gm[u0][a];
    } else if (A.kind == SBO_VAR) {
      if (Eo.clamp[u0]) return false;
      f = Eo.v[u0];
      for (int a = 0; a < d; ++a) gp[a] = Eo.gv[u0][a];
    } else {
      if (Eo.clamp[u0] || !(Eo.v[u0] > 0.0)) return false;
      const double sd = sqrt(Eo.v[u0]), sg = A.kind == SBO_UCB ? 1.0 : -1.0;
      f = Eo.m[u0] + sg * b * sd;
      for (int a = 0; a < d; ++a) gp[a] = Eo.gm[u0][a] + sg * b * Eo.gv[u0][a] / (2.0 * sd);
    }
    ys = A.mc.Y_std[A.outs[u0]];
  }
  const double sg = A.maximize ? -1.0 : 1.0;
  obj = sg * f;
  fo = obj / ys;
  bool ok = isfinite(fo);
  for (int a = 0; a < nz; ++a) {
    go[a] = sg * gf[a] / ys;
    gB[a] = 0.0;
    ok = ok && isfinite(go[a]);
  }
  B = 0.0;
  if (!ref_safe_terms(A, E, B, gB)) return false;
  if (A.use_ball) {
    double ss = 0.0;
    for (int a = 0; a < d; ++a) ss += (x[a] - A.x0[a]) * (x[a] - A.x0[a]);
    const double h = A.r * A.r - ss;
    if (!(h > 0.0)) return false;
    B -= log(h / (A.r * A.r));
    for (int a = 0; a < d; ++a) gB[a] += 2.0 * (x[a] - A.x0[a]) / h;
  }
  if (A.level_slot >= 0) {                                // level - lcb(x) > 0
    double l, gl[kMaxD];
    if (!ref_conf(E, A.level_slot, b, -1.0, d, l, gl)) return false;
    const double gc = A.level - l;
    if (!(gc > 0.0)) return false;
    B -= log(gc / A.mc.Y_std[A.outs[A.level_slot]]);
    for (int a = 0; a < d; ++a) gB[a] += gl[a] / gc;
  }
  for (int u = 0; u < A.nu; ++u) {                        // x' in U: -lcb_c(x') > 0
    if (!((A.unsafe_slots >> u) & 1)) continue;
    double l, gl[kMaxD];
    if (!ref_conf(Ev[1], u, b, -1.0, d, l, gl)) return false;
    const double gc = -l;
    if (!(gc > 0.0)) return false;
    B -= log(gc / A.mc.Y_std[A.outs[u]]);
    for (int a = 0; a < d; ++a) gB[d + a] += gl[a] / gc;
  }
  if (A.link_slot >= 0) {                                 // ucb_c(x) - L ||x - x' + 1e-8|| > 0
    double uc, gu[kMaxD], df[kMaxD], ss = 0.0;
    if (!ref_conf(E, A.link_slot, b, 1.0, d, uc, gu)) return false;
    for (int a = 0; a < d; ++a) {
      df[a] = x[a] - x[d + a] + 1e-8;
      ss += df[a] * df[a];
    }
    const double nrm = sqrt(ss), gc = uc - A.L * nrm;
    if (!(gc > 0.0)) return false;
    B -= log(gc / A.mc.Y_std[A.outs[A.link_slot]]);
    for (int a = 0; a < d; ++a) {
      const double gn = nrm > 0.0 ? A.L * df[a] / nrm : 0.0;
      gB[a] -= (gu[a] - gn) / gc;
      gB[d + a] -= gn / gc;
    }
  }
  ok = ok && isfinite(B);
  for (int a = 0; a < nz; ++a) ok = ok && isfinite(gB[a]);
  return ok;
}

// Next search direction at the accepted point (lowering the barrier weight between stages): true with the first trial in `trial`
__device__ bool ref_new_iteration(RefState& S, const RefineArgs& A, double* trial) {
  const int d = A.nz;                 // (the solver's variables)
  const PbfgsBox bx = ref_box(S, A);
  for (;;) {
    S.f = S.fo + S.mu * S.B;
    for (int a = 0; a < d; ++a) S.s.g[a] = S.go[a] + S.mu * S.gB[a];
    const double stol = S.mu > kRefMuFloor ? fmax(A.tol, S.mu) : A.tol;
    if (pbfgs_pgnorm(S.s, bx, d) > stol) break;
    if (S.mu <= kRefMuFloor) { S.status = SBO_REFINE_CONVERGED; return false; }
    S.mu = fmax(kRefMuFloor, S.mu * kRefMuStep);
  }
  pbfgs_direction(S.s, bx, d, trial);
  S.phase = REF_PH_SEARCH;
  return true;
}

// the end of a stage's line search without an acceptable point: the next stage, or the end at the floor
__device__ bool ref_stage_end(RefState& S, const RefineArgs& A, double* trial) {
  if (S.mu <= kRefMuFloor) { S.status = SBO_REFINE_CONVERGED; return false; }
  S.mu = fmax(kRefMuFloor, S.mu * kRefMuStep);
  return ref_new_iteration(S, A, trial);
}

// The one barrier step: consume the problem's terms at `trial` (ok: usable; go is overwritten), which cost nev point evaluations; true
// when `trial` holds the next point to evaluate
__device__ __forceinline__ bool ref_step(RefState& S, const RefineArgs& A, bool ok, double fo, double* go, double B, const double* gB, double obj,
                                         int nev, double* trial) {
  const int d = A.nz;                 // (the solver's variables)
  S.nev += nev;
  if (S.phase == REF_PH_START) {
    if (!ok) { S.status = SBO_REFINE_NO_PROGRESS; return false; }   // the solver's own arithmetic cannot start at the seed
    S.fo = fo; S.B = B; S.obj = S.objb = obj;
    for (int a = 0; a < d; ++a) { S.go[a] = go[a]; S.gB[a] = gB[a]; }
    S.mu = S.nbar ? kRefMu0 : kRefMuFloor;
    if (S.nev >= A.max_eval) { S.status = SBO_REFINE_MAX_EVAL; return false; }
    return ref_new_iteration(S, A, trial);
  }
  const PbfgsBox bx = ref_box(S, A);
  bool moved;
  if (pbfgs_armijo(S.s, d, trial, ok, fo + S.mu * B, S.f, moved)) {
    for (int a = 0; a < d; ++a) {
      S.go[a] = go[a];
      S.gB[a] = gB[a];
      go[a] += S.mu * gB[a];          // (from here on the barrier function's gradient at this stage's weight)
    }
    pbfgs_update(S.s, bx, d, trial, go);
    const double fprev = S.f;
    S.fo = fo; S.B = B; S.obj = obj;
    if (obj < S.objb) {
      S.objb = obj;
      for (int a = 0; a < d; ++a) S.xb[a] = S.s.x[a];
    }
    if (S.nev >= A.max_eval) { S.status = SBO_REFINE_MAX_EVAL; return false; }
    if (fabs(fprev - (S.fo + S.mu * S.B)) <= 1e-15 * (1.0 + fabs(fprev))) return ref_stage_end(S, A, trial);
    return ref_new_iteration(S, A, trial);   // (recomputes s.g from go and gB: the same expression, or a lower weight's)
  }
  if (S.nev >= A.max_eval) { S.status = SBO_REFINE_MAX_EVAL; return false; }
  if (pbfgs_backtrack(S.s, bx, d, moved, trial)) return true;
  if (S.s.h_identity) return ref_stage_end(S, A, trial);
  pbfgs_reset_h(S.s, bx, d);                                         // the quasi-Newton direction failed: one steepest-descent try
  return ref_new_iteration(S, A, trial);
}

// consume the evaluation of `trial` (one posterior + gradient evaluation per point); true when `trial` holds the next point to evaluate
__device__ __noinline__ bool ref_advance(RefState& S, const RefineArgs& A, const RefEval* E, double* trial) {
  double fo, go[kMaxD], B, gB[kMaxD], obj;
  const bool ok = ref_terms(A, E, trial, fo, go, B, gB, obj);
  return ref_step(S, A, ok, fo, go, B, gB, obj, A.np, trial);
}

// the exact bound of models/SafeOpt.py:34-45 as k_bound computes it (posterior.hip)
__device__ __forceinline__ double ref_bound(double m, double v, double b, int kind) {
  if (kind == SBO_MEAN) return m;
  if (kind == SBO_VAR) return v;
  const double sd = mul_rn(b, sqrt_rn(v));
  return kind == SBO_UCB ? add_rn(m, sd) : sub_rn(m, sd);
}

// every term of the problem at x (pair: x, x') under exact values (mean / var [q][ld], the first point at column g, x' behind it),
// judged with the sweeps' closed predicates: 0 infeasible, 1 feasible, 2 feasible on a barrier's boundary (some lcb_c == 0, the
// ball's sphere, lcb == level, or a link of exactly 0)
__device__ int ref_feasible(const RefineArgs& A, const double* x, const double* m, const double* v, long long ld, long long g) {
  const int d = A.mc.d;
  bool edge = false;
  for (int a = 0; a < A.nz; ++a)
    if (!(x[a] >= A.lo[a] && x[a] <= A.hi[a])) return 0;          // (NaN / inf included)
  if (A.use_ball) {
    double ss = 0.0;
    for (int a = 0; a < d; ++a) {
      const double df = x[a] - A.x0[a];
      ss = (a == 0) ? df * df : ss + df * df;                      // (k_ball_mask's formula)
    }
    const double dist = sqrt(ss);
    if (!(dist <= A.r)) return 0;
    edge = edge || dist == A.r;
  }
  for (int u = 0; u < A.nu; ++u) {
    if (!((A.con_slots >> u) & 1)) continue;
    const int o = A.outs[u];
    const double l = ref_bound(m[(size_t)o * ld + g], v[(size_t)o * ld + g], A.b, SBO_LCB);
    if (!(l >= 0.0)) return 0;
    edge = edge || l == 0.0;
  }
  if (A.level_slot >= 0) {                                         // (the sweep's M: lcb_0 <= u*)
    const int o = A.outs[A.level_slot];
    const double l = ref_bound(m[(size_t)o * ld + g], v[(size_t)o * ld + g], A.b, SBO_LCB);
    if (!(l <= A.level)) return 0;
    edge = edge || l == A.level;
  }
  for (int u = 0; u < A.nu; ++u) {                                 // (the sweep's U: every lcb_c <= 0)
    if (!((A.unsafe_slots >> u) & 1)) continue;
    const int o = A.outs[u];
    const double l = ref_bound(m[(size_t)o * ld + g + 1], v[(size_t)o * ld + g + 1], A.b, SBO_LCB);
    if (!(l <= 0.0)) return 0;
    edge = edge || l == 0.0;
  }
  if (A.link_slot >= 0) {                                          // (lipschitz_pair's expression, sets_expander.inc.hpp)
    const int o = A.outs[A.link_slot];
    const double ucb = ref_bound(m[(size_t)o * ld + g], v[(size_t)o * ld + g], A.b, SBO_UCB);
    double ss = 0.0;
    for (int a = 0; a < d; ++a) {
      const double df = add_rn(sub_rn(x[a], x[d + a]), 1e-8);
      ss = (a == 0) ? mul_rn(df, df) : add_rn(ss, mul_rn(df, df));
    }
    const double val = sub_rn(ucb, mul_rn(A.L, sqrt_rn(ss)));
    if (!(val >= 0.0)) return 0;
    edge = edge || val == 0.0;
  }
  return edge ? 2 : 1;
}

// the exact objective at x: the bound of the objective's output at its point, or the Euclidean distance to the target
__device__ double ref_objective(const RefineArgs& A, const double* x, const double* m, const double* v, long long ld, long long g) {
  if (A.kind == SBO_REFINE_DIST) {
    double ss = 0.0;
    for (int a = 0; a < A.mc.d; ++a) {
      const double df = sub_rn(x[a], A.tgt[a]);
      ss = (a == 0) ? mul_rn(df, df) : add_rn(ss, mul_rn(df, df));
    }
    return sqrt_rn(ss);
  }
  const int o = A.outs[A.obj_slot];
  return ref_bound(m[(size_t)o * ld + g + A.obj_point], v[(size_t)o * ld + g + A.obj_point], A.b, A.kind);
}

// seeds / cand hold nz values per entry; m0 / v0 are [q][kP S] (seed s: columns kP s ..)
template <bool kLds, int kP>
__global__ __launch_bounds__(1024) void k_refine(const RefineArgs* __restrict__ Ap, const double* __restrict__ F, const double* __restrict__ alpha,
                                                 const double* __restrict__ Xn, const double* __restrict__ seeds,
                                                 const double* __restrict__ m0, const double* __restrict__ v0, long long S,
                                                 double* __restrict__ cand, int* __restrict__ st_out, int* __restrict__ nev_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ RefState R;
  __shared__ RefEval E[kP];
  __shared__ double trial[kMaxD], red[kP * 2 * (kMaxD + 1)], uup[kP * kRefWaves];
  __shared__ double part[kRefWaves][kMaxD + 1];
  __shared__ int go;
  const RefineArgs& A = *Ap;                        // (in global memory: a kernarg copy indexed by output would go to scratch)
  const ModelConst& mc = A.mc;
  const int n = mc.n, d = mc.d, nz = A.nz;
  const long long s = blockIdx.x;
  double* kv = reinterpret_cast<double*>(smem);     // [kP][n]
  double* uv = kv + kP * n;                         // [kP][n]
  double* Ml = uv + kP * n;
  if (kLds) ref_load_M(A, F, Ml);
  if (threadIdx.x == 0) {
    for (int a = 0; a < nz; ++a) {
      trial[a] = seeds[s * nz + a];
      R.s.x[a] = R.xb[a] = trial[a];
      const double w = A.hi[a] - A.lo[a];
      R.span[a] = (A.use_ball && a < d) ? fmin(w, 2.0 * A.r) : w;
      R.D2[a] = R.span[a] * R.span[a];
    }
    const int fe = ref_feasible(A, trial, m0, v0, kP * S, kP * s);
    R.nev = 0;
    R.status = fe == 0 ? SBO_REFINE_INFEASIBLE_SEED : fe == 2 ? SBO_REFINE_ON_BOUNDARY : -1;
    R.nbar = __popc((unsigned)A.con_slots) + (A.use_ball ? 1 : 0) + __popc((unsigned)A.unsafe_slots) + (A.level_slot >= 0 ? 1 : 0) +
             (A.link_slot >= 0 ? 1 : 0);
    R.phase = REF_PH_START;
    pbfgs_reset_h(R.s, ref_box(R, A), nz);
    go = R.status < 0;
  }
  __syncthreads();
  while (go) {
    ref_eval<kLds, kP>(A, trial, F, Ml, alpha, Xn, kv, uv, part, red, uup, E);
    if (threadIdx.x == 0) go = ref_advance(R, A, E, trial);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    for (int a = 0; a < nz; ++a) {
      cand[(2 * s) * nz + a] = R.s.x[a];
      cand[(2 * s + 1) * nz + a] = R.xb[a];
    }
    st_out[s] = R.status;
    nev_out[s] = R.nev;
  }
}

// acceptance under exact values: the final iterate or the best-objective iterate when feasible there and no worse than the seed
// (the better of the two, ties to the final iterate), else the seed.  m0 / v0 [q][np S], m1 / v1 [q][2 np S]
__global__ void k_refine_accept(const RefineArgs* __restrict__ Ap, long long S, const double* __restrict__ seeds, const double* __restrict__ m0,
                                const double* __restrict__ v0, const double* __restrict__ cand, const double* __restrict__ m1,
                                const double* __restrict__ v1, int* __restrict__ st, double* __restrict__ x_out,
                                double* __restrict__ val_out) {
  const RefineArgs& A = *Ap;
  const int nz = A.nz, np = A.np;
  const double sg = A.maximize ? -1.0 : 1.0;
  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += (long long)gridDim.x * blockDim.x) {
    const double fs = ref_objective(A, seeds + s * nz, m0, v0, np * S, np * s);
    int status = st[s];
    int pick = -1;                                   // -1 seed, 0 final iterate, 1 best iterate
    double fv = fs;
    if (status != SBO_REFINE_INFEASIBLE_SEED && status != SBO_REFINE_ON_BOUNDARY) {
      double best = 0.0;
      for (int k = 0; k < 2; ++k) {
        const long long g = 2 * s + k;
        if (!ref_feasible(A, cand + g * nz, m1, v1, 2 * np * S, np * g)) continue;
        const double f = ref_objective(A, cand + g * nz, m1, v1, 2 * np * S, np * g);
        if (!(sg * f <= sg * fs)) continue;
        if (pick < 0 || sg * f < best) { pick = k; best = sg * f; fv = f; }
      }
      if (pick < 0) status = SBO_REFINE_NO_PROGRESS;
    }
    const double* xs = pick < 0 ? seeds + s * nz : cand + (2 * s + pick) * nz;
    for (int a = 0; a < nz; ++a) x_out[s * nz + a] = xs[a];
    val_out[s] = fv;
    st[s] = status;
  }
}

// ---- sbo_refine_paths: the objective is a posterior sample path f_s -------------------------------------------
// RefineArgs holds the constraints alone (every slot a constraint, no objective slot, as with SBO_REFINE_DIST); the path comes as the
// packed image of paths.hip.  Problem p = s K + k: path s = p / K, start k.
struct RefPathArgs {               // by value (kernarg segment)
  const double *Bt, *om, *ph;      // [S][F + n] scaled weights then c_s | omega [..][dpad] | phase
  int F, o, K, pad;                // features, the paths' output, starts per path
};

// value and gradient (raw coordinates, un-normalised) of the path with image bt [F + n] at x -> pv [1 + d].  Threads stride over the
// features (one sincos each), then over the observations under output o's hyper-parameters in ref_eval's form of k . alpha; the d + 1
// columns are summed by block_sum_cols, so the order is fixed by (F, n, block size) alone.
__device__ __noinline__ void ref_path_eval(const RefineArgs& A, const RefPathArgs& PA, const double* bt, const double* x, const double* Xn,
                              double (*part)[kMaxD + 1], double* red, double* pv) {
  const ModelConst& mc = A.mc;
  const int n = mc.n, d = mc.d, dp = mc.dpad, o = PA.o, F = PA.F, tid = threadIdx.x, bd = blockDim.x;
  double acc[kMaxD + 1];
#pragma unroll
  for (int a = 0; a < kMaxD + 1; ++a) acc[a] = 0.0;
  {                                                 // the features: sum_f bt[f] cos(omega_f . u + phase_f), u = xn vinv
    double u[kMaxD];
#pragma unroll
    for (int a = 0; a < kMaxD; ++a) u[a] = a < d ? ((x[a] - mc.X_mean[a]) / mc.X_std[a]) * mc.vinv[o][a] : 0.0;
    for (int f = tid; f < F; f += bd) {
      const double* omf = PA.om + (size_t)f * dp;
      double arg = 0.0;
#pragma unroll
      for (int a = 0; a < kMaxD; ++a)
        if (a < d) arg += omf[a] * u[a];
      arg += PA.ph[f];
      double sn, cs;
      sincos(arg, &sn, &cs);
      const double bf = bt[f], bs = -bf * sn;
      acc[0] += bf * cs;
#pragma unroll
      for (int a = 0; a < kMaxD; ++a)
        if (a < d) acc[1 + a] += bs * omf[a];
    }
#pragma unroll
    for (int a = 0; a < kMaxD; ++a)
      if (a < d) acc[1 + a] *= mc.vinv[o][a];       // (d u / d xn; the columns now hold d / d xn, as the observations' terms do)
  }
  const double* cf = bt + F;                        // c_s
  const double sf2 = mc.sf2[o];
  double xn[kMaxD];
#pragma unroll
  for (int a = 0; a < kMaxD; ++a) xn[a] = a < d ? (x[a] - mc.X_mean[a]) / mc.X_std[a] : 0.0;
  for (int j = tid; j < n; j += bd) {
    const double* Xj = Xn + (size_t)j * dp;
    double dist = 0.0;
#pragma unroll
    for (int a = 0; a < kMaxD; ++a)
      if (a < d) {
        const double diff = Xj[a] - xn[a];
        dist += diff * diff * mc.inv_ell[o][a];
      }
    const double ck = cf[j] * (sf2 * exp(-0.5 * dist));
    acc[0] += ck;
#pragma unroll
    for (int a = 0; a < kMaxD; ++a)
      if (a < d) acc[1 + a] += ck * (Xj[a] - xn[a]) * mc.inv_ell[o][a];
  }
  block_sum_cols(acc, d + 1, part, red);
  if (tid == 0) {
    const double ys = mc.Y_std[o];
    pv[0] = ys * (mc.mp[o] + red[0]) + mc.Y_mean[o];
    for (int a = 0; a < d; ++a) pv[1 + a] = ys * red[1 + a] / mc.X_std[a];
  }
  __syncthreads();
}

// ref_advance with the path as the objective: pv from ref_path_eval, the constraints' evaluation in E
__device__ __noinline__ bool ref_path_advance(RefState& S, const RefineArgs& A, const RefEval& E, const double* pv, int o, double* trial) {
  const int d = A.nz;
  const double sg = A.maximize ? -1.0 : 1.0, ys = A.mc.Y_std[o];
  double go[kMaxD], B = 0.0, gB[kMaxD];
  const double obj = sg * pv[0], fo = obj / ys;
  bool ok = isfinite(fo);
  for (int a = 0; a < d; ++a) {
    go[a] = sg * pv[1 + a] / ys;
    gB[a] = 0.0;
    ok = ok && isfinite(go[a]);
  }
  ok = ok && ref_safe_terms(A, E, B, gB) && isfinite(B);
  for (int a = 0; a < d; ++a) ok = ok && isfinite(gB[a]);
  return ref_step(S, A, ok, fo, go, B, gB, obj, 1, trial);
}

// One workgroup per problem.  seeds [P][d]; m0 / v0 [q][P] the exact values at the seeds (not read without constraints);
// cand [2 P][d]: the final and the best-objective iterate
template <bool kLds>
__global__ __launch_bounds__(1024) void k_refine_path(const RefineArgs* __restrict__ Ap, const RefPathArgs PA, const double* __restrict__ F,
                                                      const double* __restrict__ alpha, const double* __restrict__ Xn,
                                                      const double* __restrict__ seeds, const double* __restrict__ m0,
                                                      const double* __restrict__ v0, long long P, double* __restrict__ cand,
                                                      int* __restrict__ st_out, int* __restrict__ nev_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ RefState R;
  __shared__ RefEval E;
  __shared__ double trial[kMaxD], red[2 * (kMaxD + 1)], uup[kRefWaves], pv[kMaxD + 1];
  __shared__ double part[kRefWaves][kMaxD + 1];
  __shared__ int go;
  const RefineArgs& A = *Ap;
  const int n = A.mc.n, d = A.mc.d;
  const long long p = blockIdx.x;
  const double* bt = PA.Bt + (size_t)(p / PA.K) * (PA.F + n);
  double* kv = reinterpret_cast<double*>(smem);     // [n]
  double* uv = kv + n;                              // [n]
  double* Ml = uv + n;
  if (kLds) ref_load_M(A, F, Ml);
  if (threadIdx.x == 0) {
    for (int a = 0; a < d; ++a) {
      trial[a] = seeds[p * d + a];
      R.s.x[a] = R.xb[a] = trial[a];
      R.span[a] = A.hi[a] - A.lo[a];
      R.D2[a] = R.span[a] * R.span[a];
    }
    const int fe = ref_feasible(A, trial, m0, v0, P, p);
    R.nev = 0;
    R.status = fe == 0 ? SBO_REFINE_INFEASIBLE_SEED : fe == 2 ? SBO_REFINE_ON_BOUNDARY : -1;
    R.nbar = __popc((unsigned)A.con_slots);
    R.phase = REF_PH_START;
    pbfgs_reset_h(R.s, ref_box(R, A), d);
    go = R.status < 0;
  }
  __syncthreads();
  while (go) {
    ref_eval<kLds, 1>(A, trial, F, Ml, alpha, Xn, kv, uv, part, red, uup, &E);   // (the constraint slots; nothing without them)
    ref_path_eval(A, PA, bt, trial, Xn, part, red, pv);
    if (threadIdx.x == 0) go = ref_path_advance(R, A, E, pv, PA.o, trial);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    for (int a = 0; a < d; ++a) {
      cand[(2 * p) * d + a] = R.s.x[a];
      cand[(2 * p + 1) * d + a] = R.xb[a];
    }
    st_out[p] = R.status;
    nev_out[p] = R.nev;
  }
}

// k_refine_accept with the path's exact values: vals [3 P][S] are k_path_main's on the list seeds | candidates, and problem p reads
// column p / K of its rows.  m0 / v0 [q][P], m1 / v1 [q][2 P]
__global__ void k_refine_path_accept(const RefineArgs* __restrict__ Ap, long long P, int K, int S, const double* __restrict__ pts,
                                     const double* __restrict__ vals, const double* __restrict__ m0, const double* __restrict__ v0,
                                     const double* __restrict__ m1, const double* __restrict__ v1, int* __restrict__ st,
                                     double* __restrict__ x_out, double* __restrict__ val_out) {
  const RefineArgs& A = *Ap;
  const int d = A.nz;
  const double sg = A.maximize ? -1.0 : 1.0;
  const double* cand = pts + P * d;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long long)gridDim.x * blockDim.x) {
    const int s = (int)(p / K);
    const double fs = vals[p * S + s];
    int status = st[p];
    int pick = -1;                                   // -1 seed, 0 final iterate, 1 best iterate
    double fv = fs;
    if (status != SBO_REFINE_INFEASIBLE_SEED && status != SBO_REFINE_ON_BOUNDARY) {
      double best = 0.0;
      for (int k = 0; k < 2; ++k) {
        const long long g = 2 * p + k;
        if (!ref_feasible(A, cand + g * d, m1, v1, 2 * P, g)) continue;
        const double f = vals[(P + g) * S + s];
        if (!(sg * f <= sg * fs)) continue;
        if (pick < 0 || sg * f < best) { pick = k; best = sg * f; fv = f; }
      }
      if (pick < 0) status = SBO_REFINE_NO_PROGRESS;
    }
    const double* xs = pick < 0 ? pts + p * d : cand + (2 * p + pick) * d;
    for (int a = 0; a < d; ++a) x_out[p * d + a] = xs[a];
    val_out[p] = fv;
    st[p] = status;
  }
}

// the ceiling of max_eval: one launch holds a CU for max_eval evaluations of O(n^2) each, which keeps a call near a few seconds at n = 2048
static int refine_eval_cap(int n) { return (int)std::min<double>(kRefMaxEval, std::max<double>(kRefDefaultEval, 4e9 / ((double)n * n))); }
static int refine_threads(int n) { return n > 256 ? 1024 : 256; }

// The dynamic LDS of a launch that evaluates `pts` points per pass over `tris` outputs' triangles of M: the points' k and u = M k, and
// M itself (tier) when it fits kRefLdsM beside the vectors of every point but the first and `extra` bytes
static size_t refine_lds_bytes(const sbo_ctx* c, int tris, int pts, size_t extra, bool& tier) {
  const int n = c->mc.n;
  const size_t tri_bytes = sizeof(double) * (size_t)tris * n * (n + 1) / 2, kvuv = sizeof(double) * 2 * (size_t)n;
  tier = c->opt.refine_lds && tri_bytes + (pts - 1) * kvuv + extra <= kRefLdsM;
  return pts * kvuv + (tier ? tri_bytes : 0);
}

// the model's constants and leading dimensions, and the tolerance (<= 0: the default), of a problem on c's model
static void refine_fill(const sbo_ctx* c, double tol, RefineArgs& A) {
  A.mc = c->mc;
  A.f_cap = c->factor.ld();
  A.a_ld = c->factor.a_ld();
  A.tol = tol > 0.0 ? tol : kRefDefaultTol;
}

// the checks every refine entry point makes: of b and tol, and of the box of the d axes
static int refine_check(double b, double tol) {
  if (!(b >= 0.0) || !std::isfinite(b)) return fail(SBO_E_INVALID, "confidence multiplier b must be finite and >= 0");
  if (std::isnan(tol)) return fail(SBO_E_INVALID, "tol is NaN");
  return SBO_OK;
}
static int refine_check_box(const double* lo, const double* hi, int d) {
  for (int a = 0; a < d; ++a)
    if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || !(lo[a] <= hi[a])) return fail(SBO_E_INVALID, "box needs finite lo <= hi");
  return SBO_OK;
}

template <bool kLds, int kP>
static int refine_launch(sbo_ctx* c, size_t lds, int threads, long long S, const RefineArgs* dA, const double* dseed, const double* m0,
                         const double* v0, double* cand, int* dst, int* dnev) {
  SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_refine<kLds, kP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_refine<kLds, kP>), dim3((unsigned)S), dim3(threads), lds, c->stream, dA, c->factor.F(),
                     c->factor.alpha(), (const double*)c->Xn.p, dseed, m0, v0, S, cand, dst, dnev);
  SBO_HIP(hipGetLastError());
  return SBO_OK;
}

// what sbo_refine and sbo_refine_sets share once their arguments are checked and A describes the problem (outs, slots, terms, box):
// the exact values at the seeds, the solver launch, the exact check.  hz [S][nz], hv [S], hs [2 S] (status, then evaluations)
static int refine_run(sbo_ctx* c, RefineArgs& A, int max_eval, double tol, long long S, const double* seeds, std::vector<double>& hz,
                      std::vector<double>& hv, std::vector<int>& hs) {
  const ModelConst& mc = c->mc;
  const int q = mc.q, np = A.np, nz = A.nz;
  int rc;
  if ((rc = model_reader_begin(c, "sbo_refine", true))) return rc;   // (the fp64 factor may still be in the making: the deferred factor chain)
  refine_fill(c, tol, A);
  A.max_eval = max_eval > 0 ? std::min(max_eval, refine_eval_cap(mc.n)) : kRefDefaultEval;
  // scratch: the arguments | seeds [S][nz] | mean0 var0 [q][np S] | cand [2 S][nz] | mean1 var1 [q][2 np S] | x_out [S][nz] | val [S] |
  // status, evaluations [S]
  const size_t P = (size_t)np * S;
  RefineArgs* dA;
  double *dseed, *m0, *v0, *cand, *m1, *v1, *dx, *dval;
  int *dst, *dnev;
  auto layout = [&](Carve cv) {
    cv.take(dA, 1, 256);
    cv.take(dseed, (size_t)S * nz, 256);
    cv.take(m0, q * P); cv.take(v0, q * P);
    cv.take(cand, 2 * (size_t)S * nz);
    cv.take(m1, 2 * q * P); cv.take(v1, 2 * q * P);
    cv.take(dx, (size_t)S * nz); cv.take(dval, S);
    cv.take(dst, S); cv.take(dnev, S);
    return cv.off;
  };
  if ((rc = carve(c->refbuf, layout))) return rc;
  SBO_HIP(hipMemcpyAsync(dA, &A, sizeof(RefineArgs), hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dseed, seeds, sizeof(double) * (size_t)S * nz, hipMemcpyHostToDevice, c->stream));
  if ((rc = launch_posterior_on_list(c, dseed, (long long)P, m0, v0))) return rc;   // (a pair's points are consecutive rows of d)
  bool lds_tier;
  const size_t lds = refine_lds_bytes(c, A.nu, np, 0, lds_tier);
  const int threads = refine_threads(mc.n);
  if (S > 0x7fffffffLL) return fail(SBO_E_UNSUPPORTED, "too many seeds for one launch");
  if (np == 1)
    rc = lds_tier ? refine_launch<true, 1>(c, lds, threads, S, dA, dseed, m0, v0, cand, dst, dnev)
                  : refine_launch<false, 1>(c, lds, threads, S, dA, dseed, m0, v0, cand, dst, dnev);
  else
    rc = lds_tier ? refine_launch<true, 2>(c, lds, threads, S, dA, dseed, m0, v0, cand, dst, dnev)
                  : refine_launch<false, 2>(c, lds, threads, S, dA, dseed, m0, v0, cand, dst, dnev);
  if (rc) return rc;
  if ((rc = launch_posterior_on_list(c, cand, 2 * (long long)P, m1, v1))) return rc;
  hipLaunchKernelGGL(k_refine_accept, dim3((unsigned)std::min<long long>((S + 255) / 256, 1024)), dim3(256), 0, c->stream, (const RefineArgs*)dA, S,
                     (const double*)dseed, (const double*)m0, (const double*)v0, (const double*)cand, (const double*)m1,
                     (const double*)v1, dst, dx, dval);
  SBO_HIP(hipGetLastError());
  hz.resize((size_t)S * nz);
  hv.resize(S);
  hs.resize(2 * (size_t)S);
  SBO_HIP(hipMemcpyAsync(hz.data(), dx, sizeof(double) * (size_t)S * nz, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipMemcpyAsync(hv.data(), dval, sizeof(double) * S, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipMemcpyAsync(hs.data(), dst, sizeof(int) * 2 * (size_t)S, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipStreamSynchronize(c->stream));
  return SBO_OK;
}

// slot of output o in A.outs, appended when new
static int refine_slot(RefineArgs& A, int o) {
  for (int u = 0; u < A.nu; ++u)
    if (A.outs[u] == o) return u;
  A.outs[A.nu] = o;
  return A.nu++;
}

// The one problem path of sbo_refine_sets and sbo_refine (its single-point case), behind their own NULL / model / dtype checks:
// checks the options, lays the outputs out in slots (objective first, then ascending outputs), fills RefineArgs, packs the seeds
// [S][np][d], runs the solver and the exact check (refine_run) and picks the best seed.
static int refine_problem(sbo_ctx* c, const sbo_refine_sets_opts* opts, int64_t n_seeds, const double* seeds, const double* seeds_p,
                          double* x_out, double* xp_out, double* value_out, int32_t* status_out, sbo_refine_sets_result* result) {
  const ModelConst& mc = c->mc;
  const int d = mc.d, q = mc.q;
  if (opts->pair != 0 && opts->pair != 1) return fail(SBO_E_INVALID, "pair must be 0 or 1");
  const bool pair = opts->pair != 0;
  if (pair && 2 * d > SBO_MAX_D) return fail(SBO_E_UNSUPPORTED, "sbo_refine_sets: pair mode needs 2 d <= SBO_MAX_D (d <= 4)");
  if (pair && !seeds_p) return fail(SBO_E_INVALID, "pair mode needs seeds_p");
  if (n_seeds < 1 || n_seeds > (1LL << 24)) return fail(SBO_E_INVALID, "n_seeds out of range");
  const bool dist = opts->kind == SBO_REFINE_DIST;
  if (!dist && (opts->kind < SBO_MEAN || opts->kind > SBO_VAR)) return fail(SBO_E_INVALID, "bad objective kind");
  if (!dist && (opts->objective < 0 || opts->objective >= q)) return fail(SBO_E_INVALID, "objective output out of range");
  if (opts->maximize != 0 && opts->maximize != 1) return fail(SBO_E_INVALID, "maximize must be 0 or 1");
  if (dist && opts->maximize) return fail(SBO_E_INVALID, "the distance objective is minimised only");
  if (opts->objective_point != 0 && !(opts->objective_point == 1 && pair && !dist))
    return fail(SBO_E_INVALID, "objective_point: 0 (x), or 1 (x') for a bound in pair mode");
  if ((opts->safe_mask & 1u) || (q < 32 && (opts->safe_mask >> q) != 0))
    return fail(SBO_E_INVALID, "safe_mask: bit 0 must be clear and no bit may reach q");
  if ((opts->unsafe_mask & 1u) || (q < 32 && (opts->unsafe_mask >> q) != 0))
    return fail(SBO_E_INVALID, "unsafe_mask: bit 0 must be clear and no bit may reach q");
  if (opts->unsafe_mask && !pair) return fail(SBO_E_INVALID, "unsafe_mask constrains x': pair mode only");
  if (opts->use_level != 0 && opts->use_level != 1) return fail(SBO_E_INVALID, "use_level must be 0 or 1");
  if (opts->use_level && (opts->level_output < 0 || opts->level_output >= q || !std::isfinite(opts->level)))
    return fail(SBO_E_INVALID, "the level term needs an output in [0, q) and a finite level");
  if (opts->use_link != 0 && opts->use_link != 1) return fail(SBO_E_INVALID, "use_link must be 0 or 1");
  if (opts->use_link && !pair) return fail(SBO_E_INVALID, "the link joins x and x': pair mode only");
  if (opts->use_link && (opts->link_output < 1 || opts->link_output >= q || !(opts->L >= 0.0) || !std::isfinite(opts->L)))
    return fail(SBO_E_INVALID, "the link needs a constraint output in [1, q) and a finite L >= 0");
  int rc;
  if ((rc = refine_check(opts->b, opts->tol)) || (rc = refine_check_box(opts->lo, opts->hi, d))) return rc;
  if (opts->use_ball != 0 && opts->use_ball != 1) return fail(SBO_E_INVALID, "use_ball must be 0 or 1");
  if (opts->use_ball && (!(opts->r > 0.0) || !std::isfinite(opts->r))) return fail(SBO_E_INVALID, "ball radius must be finite and > 0");
  for (int a = 0; a < d; ++a) {
    if (opts->use_ball && !std::isfinite(opts->x_0[a])) return fail(SBO_E_INVALID, "ball centre must be finite");
    if (dist && !std::isfinite(opts->target[a])) return fail(SBO_E_INVALID, "the distance objective needs a finite target");
  }
  RefineArgs A{};
  A.np = pair ? 2 : 1;
  A.nz = A.np * d;
  A.kind = opts->kind;
  A.maximize = opts->maximize;
  A.obj_point = opts->objective_point;
  A.obj_slot = 0;
  if (!dist) refine_slot(A, opts->objective);         // (objective first; a constraint that is the objective shares slot 0)
  for (int o = 1; o < q; ++o)
    if ((opts->safe_mask >> o) & 1u) A.con_slots |= 1 << refine_slot(A, o);
  for (int o = 1; o < q; ++o)
    if ((opts->unsafe_mask >> o) & 1u) A.unsafe_slots |= 1 << refine_slot(A, o);
  A.level_slot = opts->use_level ? refine_slot(A, opts->level_output) : -1;
  A.link_slot = opts->use_link ? refine_slot(A, opts->link_output) : -1;
  A.level = opts->use_level ? opts->level : 0.0;
  A.L = opts->use_link ? opts->L : 0.0;
  A.use_ball = opts->use_ball;
  A.b = opts->b;
  A.r = opts->use_ball ? opts->r : 0.0;
  A.dscale = 0.0;
  for (int a = 0; a < d; ++a) {
    for (int p = 0; p < A.np; ++p) {
      A.lo[p * d + a] = opts->lo[a];
      A.hi[p * d + a] = opts->hi[a];
    }
    A.x0[a] = opts->use_ball ? opts->x_0[a] : 0.0;
    A.tgt[a] = dist ? opts->target[a] : 0.0;
    A.dscale += (opts->hi[a] - opts->lo[a]) * (opts->hi[a] - opts->lo[a]);
  }
  if (!(A.dscale > 0.0)) A.dscale = 1.0;
  const long long S = n_seeds;
  std::vector<double> hseed((size_t)S * A.nz);          // [S][np][d]
  for (long long s = 0; s < S; ++s)
    for (int a = 0; a < d; ++a) {
      hseed[(size_t)s * A.nz + a] = seeds[(size_t)s * d + a];
      if (pair) hseed[(size_t)s * A.nz + d + a] = seeds_p[(size_t)s * d + a];
    }
  std::vector<double> hz, hv;
  std::vector<int> hs;
  if ((rc = refine_run(c, A, opts->max_eval, opts->tol, S, hseed.data(), hz, hv, hs))) return rc;
  // the seed whose returned point is best (ties: the lowest index; infeasible seeds and NaN values never), -1 if none
  sbo_refine_sets_result res{};
  res.best = -1;
  const double sg = opts->maximize ? -1.0 : 1.0;
  for (long long s = 0; s < S; ++s) {
    res.evaluations += hs[S + s];
    if (hs[s] == SBO_REFINE_CONVERGED) ++res.converged;
    if (hs[s] == SBO_REFINE_INFEASIBLE_SEED || std::isnan(hv[s])) continue;
    if (res.best < 0 || sg * hv[s] < sg * hv[res.best]) res.best = s;
  }
  res.best_value = res.best >= 0 ? hv[res.best] : NAN;
  for (int a = 0; a < SBO_MAX_D; ++a) {
    const bool on = res.best >= 0 && a < d;
    res.best_x[a] = on ? hz[(size_t)res.best * A.nz + a] : 0.0;
    res.best_xp[a] = (on && pair) ? hz[(size_t)res.best * A.nz + d + a] : 0.0;
  }
  *result = res;
  for (long long s = 0; s < S; ++s)
    for (int a = 0; a < d; ++a) {
      if (x_out) x_out[(size_t)s * d + a] = hz[(size_t)s * A.nz + a];
      if (xp_out && pair) xp_out[(size_t)s * d + a] = hz[(size_t)s * A.nz + d + a];
    }
  if (value_out) std::copy(hv.begin(), hv.end(), value_out);
  if (status_out)
    for (long long s = 0; s < S; ++s) status_out[s] = hs[s];
  return SBO_OK;
}

template <bool kLds>
static int refine_path_launch(sbo_ctx* c, size_t lds, int threads, long long P, const RefineArgs* dA, const RefPathArgs& PA, const double* dseed,
                              const double* m0, const double* v0, double* cand, int* dst, int* dnev) {
  SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_refine_path<kLds>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_refine_path<kLds>), dim3((unsigned)P), dim3(threads), lds, c->stream, dA, PA, c->factor.F(), c->factor.alpha(),
                     (const double*)c->Xn.p, dseed, m0, v0, P, cand, dst, dnev);
  SBO_HIP(hipGetLastError());
  return SBO_OK;
}

static void refine_paths_clear(sbo_refine_paths_result* r) {
  *r = sbo_refine_paths_result{};
  for (int s = 0; s < SBO_MAX_PATHS; ++s) {
    r->best[s] = -1;
    r->best_value[s] = NAN;
  }
}

// sbo_refine_paths behind its NULL / model / dtype checks: the options, the shared preparation of paths.hip (which also holds the list
// seeds | candidates and the path's values there), the solver launch, the exact check, the best start per path
static int refine_paths(sbo_ctx* c, const sbo_refine_paths_opts* opts, PathDraws& dr, const double* seeds, double* x_out, double* value_out,
                        int32_t* status_out, sbo_refine_paths_result* result) {
  const ModelConst& mc = c->mc;
  const int d = mc.d, q = mc.q, S = opts->n_paths, K = opts->n_starts;
  int rc;
  if (K < 1 || K > SBO_REFINE_PATHS_MAX_STARTS) return fail(SBO_E_INVALID, "n_starts must be in [1, SBO_REFINE_PATHS_MAX_STARTS]");
  if (opts->maximize != 0 && opts->maximize != 1) return fail(SBO_E_INVALID, "maximize must be 0 or 1");
  if ((opts->constraint_mask & 1u) || (q < 32 && (opts->constraint_mask >> q) != 0))
    return fail(SBO_E_INVALID, "constraint_mask: bit 0 must be clear and no bit may reach q");
  if ((rc = refine_check(opts->b, opts->tol)) || (rc = refine_check_box(opts->lo, opts->hi, d)) || (rc = paths_check_draws(c, dr))) return rc;
  if ((rc = model_reader_begin(c, "sbo_refine_paths", true))) return rc;
  RefineArgs A{};
  refine_fill(c, opts->tol, A);
  A.max_eval = opts->max_eval > 0 ? std::min(opts->max_eval, refine_eval_cap(mc.n)) : kRefDefaultEval;
  A.np = 1;
  A.nz = d;
  A.maximize = opts->maximize;
  A.level_slot = A.link_slot = -1;
  A.b = opts->b;
  for (int o = 1; o < q; ++o)
    if ((opts->constraint_mask >> o) & 1u) A.con_slots |= 1 << refine_slot(A, o);
  for (int a = 0; a < d; ++a) {
    A.lo[a] = opts->lo[a];
    A.hi[a] = opts->hi[a];
  }
  const long long P = (long long)S * K;               // (<= 4096 workgroups)
  // scratch: the arguments | mean0 var0 [q][P] | mean1 var1 [q][2 P] | x_out [P][d] | val [P] | status, evaluations [P]; the list
  // seeds | candidates [3 P][d] and its path values [3 P][S] stand in the paths' own scratch
  RefineArgs* dA;
  double *m0, *v0, *m1, *v1, *dx, *dval;
  int *dst, *dnev;
  auto layout = [&](Carve cv) {
    cv.take(dA, 1, 256);
    cv.take(m0, q * (size_t)P, 256); cv.take(v0, q * (size_t)P);
    cv.take(m1, 2 * q * (size_t)P); cv.take(v1, 2 * q * (size_t)P);
    cv.take(dx, (size_t)P * d); cv.take(dval, P);
    cv.take(dst, P); cv.take(dnev, P);
    return cv.off;
  };
  if ((rc = carve(c->refbuf, layout))) return rc;
  PathImage img{};
  auto enqueue = [&]() -> int {
    int r;
    if ((r = paths_prepare_list(c, dr, 3 * P, &img))) return r;
    double* cand = img.pts + (size_t)P * d;
    SBO_HIP(hipMemcpyAsync(dA, &A, sizeof(RefineArgs), hipMemcpyHostToDevice, c->stream));
    SBO_HIP(hipMemcpyAsync(img.pts, seeds, sizeof(double) * (size_t)P * d, hipMemcpyHostToDevice, c->stream));
    if (A.nu && (r = launch_posterior_on_list(c, img.pts, P, m0, v0))) return r;
    bool lds_tier;
    const size_t lds = refine_lds_bytes(c, A.nu, 1, 0, lds_tier);
    const int threads = refine_threads(mc.n);
    const RefPathArgs PA{img.Bt, img.om, img.ph, img.F, img.output, K, 0};
    r = lds_tier ? refine_path_launch<true>(c, lds, threads, P, dA, PA, img.pts, m0, v0, cand, dst, dnev)
                 : refine_path_launch<false>(c, lds, threads, P, dA, PA, img.pts, m0, v0, cand, dst, dnev);
    if (r) return r;
    if (A.nu && (r = launch_posterior_on_list(c, cand, 2 * P, m1, v1))) return r;
    if ((r = paths_eval_list(c, img))) return r;
    hipLaunchKernelGGL(k_refine_path_accept, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, c->stream, (const RefineArgs*)dA, P, K, S,
                       (const double*)img.pts, (const double*)img.vals, (const double*)m0, (const double*)v0, (const double*)m1,
                       (const double*)v1, dst, dx, dval);
    SBO_HIP(hipGetLastError());
    return SBO_OK;
  };
  std::vector<double> hz((size_t)P * d), hv(P);
  std::vector<int> hs(2 * (size_t)P);
  rc = enqueue();
  hipError_t e = hipSuccess;
  if (!rc) {
    e = hipMemcpyAsync(hz.data(), dx, sizeof(double) * (size_t)P * d, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hv.data(), dval, sizeof(double) * P, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hs.data(), dst, sizeof(int) * 2 * (size_t)P, hipMemcpyDeviceToHost, c->stream);
  }
  const hipError_t ew = hipStreamSynchronize(c->stream);   // the one wait (nothing may still read the caller's arrays behind it)
  if (rc) return rc;
  SBO_HIP(e);
  SBO_HIP(ew);
  // per path the start whose returned point is best (ties: the lowest; infeasible seeds and NaN values never)
  sbo_refine_paths_result res;
  refine_paths_clear(&res);
  const double sg = opts->maximize ? -1.0 : 1.0;
  for (int s = 0; s < S; ++s) {
    long long best = -1;
    for (int k = 0; k < K; ++k) {
      const size_t p = (size_t)s * K + k;
      res.evaluations += hs[P + p];
      if (hs[p] == SBO_REFINE_CONVERGED) ++res.converged;
      if (hs[p] == SBO_REFINE_INFEASIBLE_SEED || std::isnan(hv[p])) continue;
      if (best < 0 || sg * hv[p] < sg * hv[(size_t)s * K + best]) best = k;
    }
    res.best[s] = best;
    if (best < 0) continue;
    res.best_value[s] = hv[(size_t)s * K + best];
    for (int a = 0; a < d; ++a) res.best_x[s][a] = hz[((size_t)s * K + best) * d + a];
  }
  *result = res;
  if (x_out) std::copy(hz.begin(), hz.end(), x_out);
  if (value_out) std::copy(hv.begin(), hv.end(), value_out);
  if (status_out) std::copy(hs.begin(), hs.begin() + P, status_out);
  return SBO_OK;
}

// ---- sbo_refine_robust: StableOpt's min-max by outer approximation -----------------------------------------------------------------
// The scenario set D lives on the device.  A round is: the exact values on {xc} x (check grid), their arg-max / arg-min per output
// (k_rob_pick), one k_refine launch per output over the joint point with the control axes held by a box of width zero (the polish
// over d), the exact values at the polished points, the decision which of them enter D (k_rob_select), and the outer step
// (k_refine_robust) -- all in stream order behind one another, with one read-back of the control block at the end of the round.
constexpr int kRobMaxScen = SBO_ROBUST_MAX_SCEN;
constexpr int kRobDefaultRounds = 6;
constexpr int kRobPolishEval = 200;              // evaluations of one polish over d

struct RobustArgs {
  RefineArgs A;              // mc, every output in its own slot, b, f_cap / a_ld, tol, the outer step's max_eval; nz, lo, hi: z = (xc, t)
  int nxc, nd, kind, max_scen;
  double bobj, sobj;         // the objective's bound is mean + sobj bobj sqrt(var)
  double lo_d[kMaxD], hi_d[kMaxD], xc0[kMaxD];   // the disturbance box; the seed
  double sep_tol;
};

// the control block of a call (device memory, read back once per round)
struct RobustCtl {
  double scen[kRobMaxScen][kMaxD];   // D: d_k [nd]
  double slack[kRobMaxScen];         // of scenario k at the outer solution, in Y_std units (the smallest of its terms)
  double z[kMaxD + 1];               // the outer solution: xc, then t
  double gap;
  int K, added, round, stop;         // stop: sbo_refine_status that ends the call at the seed (-1: none)
  int outer_status, nev, pad0, pad1; // nev: evaluations so far (polishes and outer steps)
};

// bound_0 and every lcb_c at (xc, d_k), with their gradients in xc
struct RobScen {
  double f[kRobMaxScen], gf[kRobMaxScen][kMaxD], l[kRobMaxScen][kMaxQ], gl[kRobMaxScen][kMaxQ][kMaxD];
  int ok[kRobMaxScen];
};

__device__ void rob_store(const RobustArgs& R, const RefEval& E, int k, RobScen& Sc) {
  const int d = R.A.mc.d, q = R.A.mc.q;
  bool ok = ref_conf(E, 0, R.bobj, R.sobj, d, Sc.f[k], Sc.gf[k]);   // (gradients land in place: the entries past nxc are not read)
  for (int c = 1; c < q; ++c) ok = ref_conf(E, c, R.A.b, -1.0, d, Sc.l[k][c], Sc.gl[k][c]) && ok;
  Sc.ok[k] = ok;
}

// t / Y_std_0 and the barrier sum over the scenarios at z = (xc, t), scenarios in order; false: the trial is rejected
__device__ bool rob_terms(const RobustArgs& R, const RobScen& Sc, int K, const double* z, double& fo, double* go, double& B, double* gB) {
  const int nxc = R.nxc, q = R.A.mc.q;
  const double t = z[nxc], ys0 = R.A.mc.Y_std[0];
  fo = t / ys0;
  for (int a = 0; a <= nxc; ++a) go[a] = gB[a] = 0.0;
  go[nxc] = 1.0 / ys0;
  B = 0.0;
  for (int k = 0; k < K; ++k) {
    if (!Sc.ok[k]) return false;
    const double h = t - Sc.f[k];
    if (!(h > 0.0)) return false;
    B -= log(h / ys0);
    for (int a = 0; a < nxc; ++a) gB[a] += Sc.gf[k][a] / h;
    gB[nxc] -= 1.0 / h;
    for (int c = 1; c < q; ++c) {
      const double l = Sc.l[k][c];
      if (!(l > 0.0)) return false;
      B -= log(l / R.A.mc.Y_std[c]);
      for (int a = 0; a < nxc; ++a) gB[a] -= Sc.gl[k][c][a] / l;
    }
  }
  bool ok = isfinite(fo) && isfinite(B);
  for (int a = 0; a <= nxc; ++a) ok = ok && isfinite(gB[a]);
  return ok;
}

// ref_advance on the epigraph problem: the function is rob_terms on the scenarios' evaluation at `trial`, the step ref_step with t as
// the objective (so its best-iterate tracking runs here too; xb is not read).  The first evaluation of a step only places t above
// the largest bound_0: refused outside t's box or where a scenario's evaluation is unusable, which ref_step ends as an unusable start.
__device__ __noinline__ bool rob_advance(RefState& S, const RobustArgs& R, const RobScen& Sc, int K, double* trial) {
  const RefineArgs& A = R.A;
  const int nxc = R.nxc;
  bool ok = true;
  if (S.phase == REF_PH_START) {
    double fmax = -INFINITY;
    for (int k = 0; k < K; ++k) {
      ok = ok && Sc.ok[k];
      fmax = fmax > Sc.f[k] ? fmax : Sc.f[k];
    }
    const double t = fmax + kRefMu0 * A.mc.Y_std[0];
    ok = ok && t >= A.lo[nxc] && t <= A.hi[nxc];
    trial[nxc] = S.s.x[nxc] = t;
  }
  double fo = 0.0, go[kMaxD], B = 0.0, gB[kMaxD];
  ok = ok && rob_terms(R, Sc, K, trial, fo, go, B, gB);
  return ref_step(S, A, ok, fo, go, B, gB, trial[nxc], K, trial);
}

// the outer step's evaluation workspace (LDS): the joint points of a pass, ref_eval's sums and results, the scenarios' terms
struct RobWork {
  RefEval E[2];
  RobScen Sc;
  double pts[2 * kMaxD], red[2 * 2 * (kMaxD + 1)], uup[2 * kRefWaves], part[kRefWaves][kMaxD + 1];
};

// bound_0 and every lcb_c at the K joint points (xc, d_k), xc = trial's first nxc entries -> W.Sc: two points per pass over M
// (ref_eval<kLds, 2>), an odd last one alone, in scenario order
template <bool kLds>
__device__ __forceinline__ void rob_eval_scenarios(const RobustArgs& RA, const RobustCtl* ctl, int K, const double* trial, const double* F,
                                                const double* Ml, const double* alpha, const double* Xn, double* kv, double* uv, RobWork& W) {
  const RefineArgs& A = RA.A;
  const int d = A.mc.d, nxc = RA.nxc, nd = RA.nd;
  for (int k0 = 0; k0 < K; k0 += 2) {
    const int np = K - k0 >= 2 ? 2 : 1;
    if (threadIdx.x == 0)
      for (int p = 0; p < np; ++p) {
        for (int a = 0; a < nxc; ++a) W.pts[p * d + a] = trial[a];
        for (int a = 0; a < nd; ++a) W.pts[p * d + nxc + a] = ctl->scen[k0 + p][a];
      }
    __syncthreads();
    if (np == 2) ref_eval<kLds, 2>(A, W.pts, F, Ml, alpha, Xn, kv, uv, W.part, W.red, W.uup, W.E);
    else ref_eval<kLds, 1>(A, W.pts, F, Ml, alpha, Xn, kv, uv, W.part, W.red, W.uup, W.E);
    if (threadIdx.x == 0)
      for (int p = 0; p < np; ++p) rob_store(RA, W.E[p], k0 + p, W.Sc);
    __syncthreads();
  }
}

// The outer step: one workgroup minimises t over z = (xc, t) on the barrier function of the scenarios, from the current outer
// solution when that is strictly inside every scenario's terms, else from the seed.
template <bool kLds>
__global__ __launch_bounds__(1024) void k_refine_robust(const RobustArgs* __restrict__ Rp, const double* __restrict__ F,
                                                        const double* __restrict__ alpha, const double* __restrict__ Xn,
                                                        RobustCtl* __restrict__ ctl) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ RefState R;
  __shared__ RobWork W;
  __shared__ double trial[kMaxD];
  __shared__ int go, attempt;
  const RobustArgs& RA = *Rp;
  const RefineArgs& A = RA.A;
  if (ctl->added == 0 || ctl->stop >= 0) return;    // (the separation ended the call: uniform over the workgroup)
  const int n = A.mc.n, nz = A.nz, nxc = RA.nxc, K = ctl->K;
  double* kv = reinterpret_cast<double*>(smem);     // [2][n]
  double* uv = kv + 2 * n;                          // [2][n]
  double* Ml = uv + 2 * n;
  if (kLds) ref_load_M(A, F, Ml);
  if (threadIdx.x == 0) {
    for (int a = 0; a < nz; ++a) {
      R.span[a] = A.hi[a] - A.lo[a];
      R.D2[a] = R.span[a] * R.span[a];
    }
    R.nev = 0;
    R.nbar = K * A.mc.q;                            // (every scenario's terms; > 0, so the first stage's weight is kRefMu0)
    attempt = 0;
  }
  __syncthreads();
  for (;;) {                                        // attempt 0: from the outer solution; 1: from the seed
    if (threadIdx.x == 0) {
      for (int a = 0; a < nxc; ++a) trial[a] = R.s.x[a] = attempt == 0 ? ctl->z[a] : RA.xc0[a];
      trial[nxc] = R.s.x[nxc] = 0.0;
      R.status = -1;
      R.phase = REF_PH_START;
      pbfgs_reset_h(R.s, ref_box(R, A), nz);
      go = 1;
    }
    __syncthreads();
    while (go) {
      rob_eval_scenarios<kLds>(RA, ctl, K, trial, F, Ml, alpha, Xn, kv, uv, W);
      if (threadIdx.x == 0) go = rob_advance(R, RA, W.Sc, K, trial);
      __syncthreads();
    }
    const bool retry = R.status == SBO_REFINE_NO_PROGRESS && R.phase == REF_PH_START && attempt == 0;
    __syncthreads();
    if (!retry) break;
    if (threadIdx.x == 0) attempt = 1;
    __syncthreads();
  }
  const bool started = !(R.status == SBO_REFINE_NO_PROGRESS && R.phase == REF_PH_START);
  if (started) {                                    // the scenarios' slack at the point the step returns
    if (threadIdx.x == 0)
      for (int a = 0; a < nz; ++a) trial[a] = R.s.x[a];
    __syncthreads();
    rob_eval_scenarios<kLds>(RA, ctl, K, trial, F, Ml, alpha, Xn, kv, uv, W);
  }
  if (threadIdx.x == 0) {
    if (started) {
      for (int a = 0; a < nz; ++a) ctl->z[a] = R.s.x[a];
      for (int k = 0; k < K; ++k) {
        double s = (R.s.x[nxc] - W.Sc.f[k]) / A.mc.Y_std[0];
        for (int c = 1; c < A.mc.q; ++c) s = fmin(s, W.Sc.l[k][c] / A.mc.Y_std[c]);
        ctl->slack[k] = W.Sc.ok[k] ? s : 0.0;
      }
      R.nev += K;
    }
    ctl->outer_status = started ? R.status : -2;     // -2: no strictly feasible start
    ctl->nev += R.nev;
  }
}

// arg-max (arg-min: of the negated value, which is exact) over i < N of `kind` of (m[i], v[i]) by the workgroup, ties to the lower
// index, a NaN never wins: every thread returns the result (nothing qualified: val = 0, idx = -1).  sv / sk: one slot per wave
__device__ void rob_argext(const double* m, const double* v, long long N, double b, int kind, bool want_max, double* sv,
                           long long* sk, double& val, long long& idx) {
  double bv = 0.0;
  long long bk = kArgNone;
  for (long long i = threadIdx.x; i < N; i += blockDim.x) {
    const double f = ref_bound(m[i], v[i], b, kind);
    arg_take(bv, bk, want_max ? f : -f, isnan(f) ? kArgNone : i);
  }
  arg_block_best_all(bv, bk, sv, sk);
  const bool none = bk == kArgNone;
  val = none ? 0.0 : (want_max ? bv : -bv);
  idx = none ? -1 : bk;
}

// the separation's grid seeds: output 0's arg-max of the objective's bound and every constraint's arg-min of its lcb over the list
// pts [N][d] (values m / v [q][N]) -> seeds [q][d], their values sval [q]
__global__ __launch_bounds__(256) void k_rob_pick(const RobustArgs* __restrict__ Rp, const double* __restrict__ pts, const double* __restrict__ m,
                                                  const double* __restrict__ v, long long N, double* __restrict__ seeds, double* __restrict__ sval) {
  __shared__ double sv[256 / 64];
  __shared__ long long sk[256 / 64];
  const RobustArgs& R = *Rp;
  const int d = R.A.mc.d, q = R.A.mc.q;
  for (int u = 0; u < q; ++u) {
    double val;
    long long idx;
    rob_argext(m + (size_t)u * N, v + (size_t)u * N, N, R.A.b, u == 0 ? R.kind : SBO_LCB, u == 0, sv, sk, val, idx);
    if (threadIdx.x == 0) {
      if (idx < 0) idx = 0;                          // (no finite value on the list: the first point)
      for (int a = 0; a < d; ++a) seeds[u * d + a] = pts[idx * d + a];
      sval[u] = val;
    }
  }
}

// Which polished points enter D.  cand [q][2][d] (k_refine's final and best iterate of output u's polish), m1 / v1 [q][2 q] their
// exact values; seeds / sval: the grid seeds.  One thread.
__global__ void k_rob_select(const RobustArgs* __restrict__ Rp, RobustCtl* __restrict__ ctl, const double* __restrict__ seeds,
                             const double* __restrict__ sval, const double* __restrict__ cand, const double* __restrict__ m1,
                             const double* __restrict__ v1, const int* __restrict__ pnev) {
  if (threadIdx.x || blockIdx.x) return;
  const RobustArgs& R = *Rp;
  const int d = R.A.mc.d, q = R.A.mc.q, nxc = R.nxc, nd = R.nd;
  const bool first = ctl->round == 0;
  const double t = ctl->z[nxc];
  int added = 0, stop = -1;
  double gap = 0.0;
  for (int u = 0; u < q; ++u) {
    ctl->nev += pnev[u];
    const double* p = seeds + u * d;                 // the kept point: the grid seed, or a polished point no better for the caller
    double pv = sval[u];
    for (int k = 0; k < 2; ++k) {
      const double* x = cand + (size_t)(2 * u + k) * d;
      bool in = true;
      for (int a = 0; a < nd; ++a) in = in && x[nxc + a] >= R.lo_d[a] && x[nxc + a] <= R.hi_d[a];
      for (int a = 0; a < nxc; ++a) in = in && x[a] == seeds[u * d + a];
      if (!in) continue;
      const double f = ref_bound(m1[(size_t)u * 2 * q + 2 * u + k], v1[(size_t)u * 2 * q + 2 * u + k], R.A.b, u == 0 ? R.kind : SBO_LCB);
      if (u == 0 ? f > pv : f < pv) { pv = f; p = x; }
    }
    const double ys = R.A.mc.Y_std[u];
    const double viol = u == 0 ? (first ? INFINITY : (pv - t) / ys) : -pv / ys;
    if (!first && viol > gap) gap = viol;
    if (first && u > 0) {
      if (pv < 0.0) stop = SBO_REFINE_INFEASIBLE_SEED;
      else if (pv == 0.0 && stop < 0) stop = SBO_REFINE_ON_BOUNDARY;
    }
    if (!(first || viol > R.sep_tol)) continue;
    bool dup = false;
    for (int k = 0; k < ctl->K && !dup; ++k) {
      bool same = true;
      for (int a = 0; a < nd; ++a) same = same && ctl->scen[k][a] == p[nxc + a];
      dup = same;
    }
    if (dup) continue;
    int slot = ctl->K;
    if (slot >= R.max_scen) {                        // full: the scenario of largest slack (ties: the lowest) makes room
      slot = 0;
      for (int k = 1; k < ctl->K; ++k)
        if (ctl->slack[k] > ctl->slack[slot]) slot = k;
      ctl->slack[slot] = -INFINITY;                  // (not replaced twice in one round)
    } else {
      ctl->slack[slot] = -INFINITY;
      ++ctl->K;
    }
    for (int a = 0; a < nd; ++a) ctl->scen[slot][a] = p[nxc + a];
    ++added;
  }
  ctl->added = added;
  ctl->gap = first ? 0.0 : gap;
  if (stop >= 0) ctl->stop = stop;
  ++ctl->round;
}

struct RobustFinal {
  double value[2], g_min[2][kMaxQ];   // [0] the seed, [1] the final xc, over C
  long long worst[2];
};

// the exact check: lists {seed} x C and {xc} x C of NC points each, values m / v [q][2 NC]
__global__ __launch_bounds__(256) void k_rob_final(const RobustArgs* __restrict__ Rp, const double* __restrict__ m, const double* __restrict__ v,
                                                   long long NC, RobustFinal* __restrict__ out) {
  __shared__ double sv[256 / 64];
  __shared__ long long sk[256 / 64];
  const RobustArgs& R = *Rp;
  const int q = R.A.mc.q;
  for (int w = 0; w < 2; ++w)
    for (int u = 0; u < q; ++u) {
      double val;
      long long idx;
      const size_t off = (size_t)u * 2 * NC + (size_t)w * NC;
      rob_argext(m + off, v + off, NC, R.A.b, u == 0 ? R.kind : SBO_LCB, u == 0, sv, sk, val, idx);
      if (threadIdx.x == 0) {
        if (u == 0) {
          out->value[w] = idx >= 0 ? val : NAN;
          out->worst[w] = idx;
        } else {
          out->g_min[w][u] = idx >= 0 ? val : NAN;
        }
      }
    }
}

template <bool kLds>
static int robust_outer_launch(sbo_ctx* c, size_t lds, int threads, const RobustArgs* dR, RobustCtl* ctl) {
  SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_refine_robust<kLds>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_refine_robust<kLds>), dim3(1), dim3(threads), lds, c->stream, dR, c->factor.F(),
                     c->factor.alpha(), (const double*)c->Xn.p, ctl);
  SBO_HIP(hipGetLastError());
  return SBO_OK;
}

static int refine_robust(sbo_ctx* c, const sbo_refine_robust_opts* opts, const double* xc_seed, double* scenarios_out,
                         sbo_refine_robust_result* result) {
  const ModelConst& mc = c->mc;
  const int d = mc.d, q = mc.q, n = mc.n;
  const int nxc = opts->n_control_axes;
  if (nxc < 1 || nxc > d - 1) return fail(SBO_E_INVALID, "n_control_axes must lie in [1, d - 1]");
  if (nxc + 1 > kMaxD) return fail(SBO_E_UNSUPPORTED, "sbo_refine_robust: the solver's variables (xc, t) need n_control_axes + 1 <= SBO_MAX_D");
  const int nd = d - nxc;
  if (opts->kind != SBO_MEAN && opts->kind != SBO_UCB && opts->kind != SBO_LCB) return fail(SBO_E_INVALID, "kind must be SBO_MEAN, SBO_UCB or SBO_LCB");
  int rc;
  if ((rc = refine_check(opts->b, opts->tol))) return rc;
  if (opts->max_scenarios > kRobMaxScen) return fail(SBO_E_INVALID, "max_scenarios is at most SBO_ROBUST_MAX_SCEN");
  if ((rc = refine_check_box(opts->lo, opts->hi, d))) return rc;
  long long Nd = 1;
  for (int a = 0; a < nd; ++a) {
    if (opts->count_d[a] < 1 || opts->count_d[a] > (1LL << 24)) return fail(SBO_E_INVALID, "count_d needs at least one point per disturbance axis");
    Nd *= opts->count_d[a];
    if (Nd > (1LL << 24)) return fail(SBO_E_INVALID, "the check grid holds at most 2^24 points");
  }
  for (int a = 0; a < nxc; ++a)
    if (!std::isfinite(xc_seed[a])) return fail(SBO_E_INVALID, "the seed must be finite");
  if ((rc = model_reader_begin(c, "sbo_refine_robust", true))) return rc;
  const int max_rounds = opts->max_rounds > 0 ? opts->max_rounds : kRobDefaultRounds;
  const int eval_cap = refine_eval_cap(n);
  const int max_eval = opts->max_eval > 0 ? std::min(opts->max_eval, eval_cap) : eval_cap;

  RobustArgs R{};
  refine_fill(c, opts->tol, R.A);
  R.A.nu = q;
  for (int u = 0; u < q; ++u) R.A.outs[u] = u;
  R.A.kind = opts->kind;
  R.A.b = opts->b;
  R.A.np = 1;
  R.A.nz = nxc + 1;
  R.A.level_slot = R.A.link_slot = -1;
  R.nxc = nxc;
  R.nd = nd;
  R.kind = opts->kind;
  R.max_scen = opts->max_scenarios > 0 ? opts->max_scenarios : kRobMaxScen;
  R.bobj = opts->kind == SBO_MEAN ? 0.0 : opts->b;
  R.sobj = opts->kind == SBO_LCB ? -1.0 : 1.0;
  R.sep_tol = R.A.tol;
  bool seed_in_box = true;
  for (int a = 0; a < nxc; ++a) {
    R.A.lo[a] = opts->lo[a];
    R.A.hi[a] = opts->hi[a];
    R.xc0[a] = xc_seed[a];
    seed_in_box = seed_in_box && xc_seed[a] >= opts->lo[a] && xc_seed[a] <= opts->hi[a];
  }
  for (int a = 0; a < nd; ++a) {
    R.lo_d[a] = opts->lo[nxc + a];
    R.hi_d[a] = opts->hi[nxc + a];
  }
  // the box of t, which sets its metric and first step: the prior mean of output 0 +- (8 + b sf_0) Y_std_0, wide of any bound of
  // normalised data; an outer step whose t would start outside it does not start
  const double tw = mc.Y_std[0] * (8.0 + opts->b * std::sqrt(mc.sf2[0])), tc = mc.Y_std[0] * mc.mp[0] + mc.Y_mean[0];
  R.A.lo[nxc] = tc - tw;
  R.A.hi[nxc] = tc + tw;
  // the check grid of the disturbance box, the arithmetic of sbo_candidates_grid
  std::vector<double> hgrid((size_t)Nd * nd);
  for (long long j = 0; j < Nd; ++j) {
    long long f = j;
    for (int a = 0; a < nd; ++a) {
      const long long cnt = opts->count_d[a], i = f % cnt;
      f /= cnt;
      const double step = cnt > 1 ? (R.hi_d[a] - R.lo_d[a]) / (double)(cnt - 1) : 0.0;
      hgrid[(size_t)j * nd + a] = (i == cnt - 1 && cnt > 1) ? R.hi_d[a] : R.lo_d[a] + (double)i * step;
    }
  }
  // scratch: (q + 1) argument blocks | control | final | list [2 NC][d] | mean var [q][2 NC] | seeds [q][d] | sval [q] | cand [2 q][d] |
  // mean1 var1 [q][2 q] | polish status, evaluations [q]
  const long long NC = Nd + kRobMaxScen;
  const size_t asz = (std::max(sizeof(RobustArgs), sizeof(RefineArgs)) + 255) / 256 * 256;   // (the stride of the argument blocks)
  unsigned char* dargs;
  RobustCtl* dctl;
  RobustFinal* dfin;
  double *dlist, *mL, *vL, *dseed, *dsval, *dcand, *m1, *v1;
  int *dst, *dnev;
  auto layout = [&](Carve cv) {
    cv.take(dargs, (size_t)(q + 1) * asz, 256);
    cv.take(dctl, 1, 256);
    cv.take(dfin, 1, 256);
    cv.take(dlist, 2 * (size_t)NC * d, 256);
    cv.take(mL, 2 * (size_t)q * NC); cv.take(vL, 2 * (size_t)q * NC);
    cv.take(dseed, (size_t)q * d); cv.take(dsval, q);
    cv.take(dcand, 2 * (size_t)q * d);
    cv.take(m1, 2 * (size_t)q * q); cv.take(v1, 2 * (size_t)q * q);
    cv.take(dst, q); cv.take(dnev, q);
    return cv.off;
  };
  if ((rc = carve(c->refbuf, layout))) return rc;
  RobustArgs* dR = (RobustArgs*)dargs;

  bool lds_polish, lds_outer;
  const size_t lds_p = refine_lds_bytes(c, 1, 1, 0, lds_polish);
  const size_t lds_o = refine_lds_bytes(c, q, 2, 8192, lds_outer);   // (two points' vectors, as a pair of k_refine; 8192: the scenarios' terms)
  const int threads = refine_threads(n);

  RobustCtl hctl{};
  for (int a = 0; a < nxc; ++a) hctl.z[a] = xc_seed[a];
  hctl.stop = -1;
  hctl.added = 1;
  int status = -1, rounds = 0;
  if (!seed_in_box) status = SBO_REFINE_INFEASIBLE_SEED;
  std::vector<double> hlist((size_t)2 * NC * d);
  std::vector<RefineArgs> hP(q);
  SBO_HIP(hipMemcpyAsync(dctl, &hctl, sizeof(RobustCtl), hipMemcpyHostToDevice, c->stream));
  while (status < 0) {
    const int left = max_eval - hctl.nev;
    if (rounds >= max_rounds || left <= 0) { status = SBO_REFINE_MAX_EVAL; break; }
    R.A.max_eval = std::max(1, left - q * kRobPolishEval);
    // separation at xc = hctl.z
    for (long long j = 0; j < Nd; ++j) {
      for (int a = 0; a < nxc; ++a) hlist[(size_t)j * d + a] = hctl.z[a];
      for (int a = 0; a < nd; ++a) hlist[(size_t)j * d + nxc + a] = hgrid[(size_t)j * nd + a];
    }
    SBO_HIP(hipMemcpyAsync(dlist, hlist.data(), sizeof(double) * (size_t)Nd * d, hipMemcpyHostToDevice, c->stream));
    for (int u = 0; u < q; ++u) {                    // output u's polish over d: the control axes held by a box of width zero
      RefineArgs& P = hP[u];
      P = RefineArgs{};
      refine_fill(c, opts->tol, P);
      P.nu = 1;
      P.outs[0] = u;
      P.kind = u == 0 ? opts->kind : SBO_LCB;
      P.maximize = u == 0;
      P.max_eval = kRobPolishEval;
      P.b = opts->b;
      P.np = 1;
      P.nz = d;
      P.level_slot = P.link_slot = -1;
      for (int a = 0; a < d; ++a) {
        P.lo[a] = a < nxc ? hctl.z[a] : opts->lo[a];
        P.hi[a] = a < nxc ? hctl.z[a] : opts->hi[a];
      }
      SBO_HIP(hipMemcpyAsync(dargs + (size_t)(u + 1) * asz, &P, sizeof(RefineArgs), hipMemcpyHostToDevice, c->stream));
    }
    SBO_HIP(hipMemcpyAsync(dR, &R, sizeof(RobustArgs), hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_posterior_on_list(c, dlist, Nd, mL, vL))) return rc;
    hipLaunchKernelGGL(k_rob_pick, dim3(1), dim3(256), 0, c->stream, (const RobustArgs*)dR, (const double*)dlist, (const double*)mL,
                       (const double*)vL, Nd, dseed, dsval);
    SBO_HIP(hipGetLastError());
    for (int u = 0; u < q; ++u) {
      const RefineArgs* dP = (const RefineArgs*)(dargs + (size_t)(u + 1) * asz);
      rc = lds_polish ? refine_launch<true, 1>(c, lds_p, threads, 1, dP, dseed + (size_t)u * d, mL, vL, dcand + 2 * (size_t)u * d, dst + u, dnev + u)
                      : refine_launch<false, 1>(c, lds_p, threads, 1, dP, dseed + (size_t)u * d, mL, vL, dcand + 2 * (size_t)u * d, dst + u, dnev + u);
      if (rc) return rc;
    }
    if ((rc = launch_posterior_on_list(c, dcand, 2 * q, m1, v1))) return rc;
    hipLaunchKernelGGL(k_rob_select, dim3(1), dim3(1), 0, c->stream, (const RobustArgs*)dR, dctl, (const double*)dseed, (const double*)dsval,
                       (const double*)dcand, (const double*)m1, (const double*)v1, (const int*)dnev);
    SBO_HIP(hipGetLastError());
    rc = lds_outer ? robust_outer_launch<true>(c, lds_o, threads, dR, dctl) : robust_outer_launch<false>(c, lds_o, threads, dR, dctl);
    if (rc) return rc;
    SBO_HIP(hipMemcpyAsync(&hctl, dctl, sizeof(RobustCtl), hipMemcpyDeviceToHost, c->stream));
    SBO_HIP(hipStreamSynchronize(c->stream));        // (the round's one wait)
    ++rounds;
    if (hctl.stop >= 0) status = hctl.stop;
    else if (hctl.added == 0) status = SBO_REFINE_CONVERGED;
    else if (hctl.outer_status == -2) status = SBO_REFINE_MAX_EVAL;     // the outer step cannot start: the last solution stands, unconverged
    else if (hctl.outer_status == SBO_REFINE_MAX_EVAL && hctl.nev >= max_eval) status = SBO_REFINE_MAX_EVAL;
  }
  // the exact check on C = the check grid, then the scenarios
  const int K = hctl.K;
  const long long NCu = Nd + K;
  for (int w = 0; w < 2; ++w)
    for (long long j = 0; j < NCu; ++j) {
      double* row = hlist.data() + ((size_t)w * NCu + j) * d;
      for (int a = 0; a < nxc; ++a) row[a] = w == 0 ? xc_seed[a] : hctl.z[a];
      for (int a = 0; a < nd; ++a) row[nxc + a] = j < Nd ? hgrid[(size_t)j * nd + a] : hctl.scen[j - Nd][a];
    }
  SBO_HIP(hipMemcpyAsync(dlist, hlist.data(), sizeof(double) * 2 * (size_t)NCu * d, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dR, &R, sizeof(RobustArgs), hipMemcpyHostToDevice, c->stream));
  if ((rc = launch_posterior_on_list(c, dlist, 2 * NCu, mL, vL))) return rc;
  hipLaunchKernelGGL(k_rob_final, dim3(1), dim3(256), 0, c->stream, (const RobustArgs*)dR, (const double*)mL, (const double*)vL, NCu, dfin);
  SBO_HIP(hipGetLastError());
  RobustFinal fin{};
  SBO_HIP(hipMemcpyAsync(&fin, dfin, sizeof(RobustFinal), hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipStreamSynchronize(c->stream));
  // the seed's verdict on C comes first; then the final xc against it
  bool seed_bad = !seed_in_box, seed_edge = false;
  for (int u = 1; u < q; ++u) {
    seed_bad = seed_bad || !(fin.g_min[0][u] >= 0.0);
    seed_edge = seed_edge || fin.g_min[0][u] == 0.0;
  }
  if (std::isnan(fin.value[0])) seed_bad = true;
  int pick = 0;
  if (seed_bad) status = SBO_REFINE_INFEASIBLE_SEED;
  else if (seed_edge) status = SBO_REFINE_ON_BOUNDARY;
  else {
    bool ok = fin.value[1] <= fin.value[0];
    for (int a = 0; a < nxc; ++a) ok = ok && hctl.z[a] >= opts->lo[a] && hctl.z[a] <= opts->hi[a];
    for (int u = 1; u < q; ++u) ok = ok && fin.g_min[1][u] >= 0.0;
    if (ok) pick = 1;
    else status = SBO_REFINE_NO_PROGRESS;
    if (status == SBO_REFINE_INFEASIBLE_SEED || status == SBO_REFINE_ON_BOUNDARY) status = SBO_REFINE_NO_PROGRESS;   // (the loop's verdict was on fewer points)
  }
  sbo_refine_robust_result res{};
  res.status = status;
  res.rounds = rounds;
  res.scenarios = K;
  res.evaluations = hctl.nev;
  res.value = fin.value[pick];
  res.seed_value = fin.value[0];
  res.gap = hctl.gap;
  for (int a = 0; a < nxc; ++a) res.xc[a] = pick ? hctl.z[a] : xc_seed[a];
  for (int u = 1; u < q; ++u) res.g_min[u] = fin.g_min[pick][u];
  if (fin.worst[pick] >= 0)
    for (int a = 0; a < nd; ++a)
      res.worst_d[a] = fin.worst[pick] < Nd ? hgrid[(size_t)fin.worst[pick] * nd + a] : hctl.scen[fin.worst[pick] - Nd][a];
  *result = res;
  if (scenarios_out)
    for (int k = 0; k < kRobMaxScen; ++k)
      for (int a = 0; a < nd; ++a) scenarios_out[(size_t)k * nd + a] = k < K ? hctl.scen[k][a] : 0.0;
  return SBO_OK;
}

}  // namespace sbo

using namespace sbo;

extern "C" int sbo_refine_robust(sbo_ctx* c, const sbo_refine_robust_opts* opts, const double* xc_seed, double* scenarios_out,
                                 sbo_refine_robust_result* result) {
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (!opts || !xc_seed || !result) return fail(SBO_E_INVALID, "NULL argument");
  if (const int rcm = model_reader_check(c, "sbo_refine_robust", true)) return rcm;
  return refine_robust(c, opts, xc_seed, scenarios_out, result);
}

extern "C" int sbo_refine_paths(sbo_ctx* c, const sbo_refine_paths_opts* opts, const double* omega, const double* phase, const double* weights,
                                const double* noise, const double* seeds, double* x_out, double* value_out, int32_t* status_out,
                                sbo_refine_paths_result* result) {
  if (result) refine_paths_clear(result);
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (!opts || !omega || !phase || !weights || !noise || !seeds || !result) return fail(SBO_E_INVALID, "NULL argument");
  if (const int rcm = model_reader_check(c, "sbo_refine_paths", true)) return rcm;
  PathDraws dr{opts->output, opts->n_paths, opts->n_features, omega, phase, weights, noise, {}};
  return refine_paths(c, opts, dr, seeds, x_out, value_out, status_out, result);
}

// the single-point case of the set problem: no level, no link, no unsafe_mask, and the constraints as its safe_mask
extern "C" int sbo_refine(sbo_ctx* c, const sbo_refine_opts* opts, int64_t n_seeds, const double* seeds, double* x_out,
                          double* value_out, int32_t* status_out, sbo_refine_result* result) {
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (!opts || !seeds || !result) return fail(SBO_E_INVALID, "NULL argument");
  if (const int rcm = model_reader_check(c, "sbo_refine", true)) return rcm;
  const int q = c->mc.q;
  if (n_seeds < 1 || n_seeds > (1LL << 24)) return fail(SBO_E_INVALID, "n_seeds out of range");
  if (opts->objective < 0 || opts->objective >= q) return fail(SBO_E_INVALID, "objective output out of range");
  if (opts->kind < SBO_MEAN || opts->kind > SBO_VAR) return fail(SBO_E_INVALID, "bad bound kind");
  if (opts->maximize != 0 && opts->maximize != 1) return fail(SBO_E_INVALID, "maximize must be 0 or 1");
  if ((opts->constraint_mask & 1u) || (q < 32 && (opts->constraint_mask >> q) != 0))
    return fail(SBO_E_INVALID, "constraint_mask: bit 0 must be clear and no bit may reach q");
  sbo_refine_sets_opts so{};
  so.b = opts->b;
  so.objective = opts->objective;
  so.kind = opts->kind;
  so.maximize = opts->maximize;
  so.safe_mask = opts->constraint_mask;
  so.use_ball = opts->use_ball;
  so.max_eval = opts->max_eval;
  so.r = opts->r;
  so.tol = opts->tol;
  for (int a = 0; a < SBO_MAX_D; ++a) {
    so.lo[a] = opts->lo[a];
    so.hi[a] = opts->hi[a];
    so.x_0[a] = opts->x_0[a];
  }
  sbo_refine_sets_result sr{};
  const int rc = refine_problem(c, &so, n_seeds, seeds, nullptr, x_out, nullptr, value_out, status_out, &sr);
  if (rc) return rc;
  sbo_refine_result res{};
  res.best = sr.best;
  res.best_value = sr.best_value;
  res.evaluations = sr.evaluations;
  res.converged = sr.converged;
  std::copy(sr.best_x, sr.best_x + SBO_MAX_D, res.best_x);
  *result = res;
  return SBO_OK;
}

extern "C" int sbo_refine_sets(sbo_ctx* c, const sbo_refine_sets_opts* opts, int64_t n_seeds, const double* seeds, const double* seeds_p,
                               double* x_out, double* xp_out, double* value_out, int32_t* status_out, sbo_refine_sets_result* result) {
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (!opts || !seeds || !result) return fail(SBO_E_INVALID, "NULL argument");
  if (const int rcm = model_reader_check(c, "sbo_refine_sets", true)) return rcm;
  return refine_problem(c, opts, n_seeds, seeds, seeds_p, x_out, xp_out, value_out, status_out, result);
}
