// pbfgs.hpp -- projected BFGS on a box in a diagonal metric: the solver core of k_fit_local (fit.hip) and k_refine (refine.hip).
//
// One thread runs the algebra on a state in LDS while its workgroup evaluates the trial points.  The core owns the iterate, its
// gradient, the search direction and the inverse Hessian; the caller owns the function (how a trial is evaluated and when it is
// unusable), the function value and every stopping rule.  A line search is the projection arc x(t) = clip(x + t p): the first
// trial comes from pbfgs_direction, each evaluated trial goes to pbfgs_armijo and from there to pbfgs_update or pbfgs_backtrack;
// when that gives up too, the caller resets H (pbfgs_reset_h) for one steepest-descent try, or ends if H was the reset one
// already.  Every sum runs in a fixed order and association: the kernels' results are pinned bit for bit
// (tests/test_gpu_solver_bits.py).
#pragma once

namespace sbo {

// the box and the metric of the problem: H is reset to diag(D2), lengths along axis a are measured in units of span[a] (an axis of
// span 0 is held), and a steepest-descent step is capped at `cap` of those units.  The unit metric is D2 = span = 1.
struct PbfgsBox {
  const double *lo, *hi, *D2, *span;
  double cap;
};

template <int kD>
struct PbfgsState {
  double x[kD], g[kD], p[kD], H[kD * kD];   // accepted point, gradient there, search direction, inverse Hessian [D][D]
  double t;                                 // step along p of the trial under evaluation
  int halvings, h_identity;                 // h_identity: H is still the reset one (no update since)
};

__device__ __forceinline__ double clip_to(double v, double lo, double hi) { return v < lo ? lo : v > hi ? hi : v; }

template <int kD>
__device__ void pbfgs_reset_h(PbfgsState<kD>& S, const PbfgsBox& bx, int D) {
  for (int a = 0; a < D * D; ++a) S.H[a] = 0.0;
  for (int a = 0; a < D; ++a) S.H[a * D + a] = bx.D2[a];
  S.h_identity = 1;
}

// inf-norm of the projected (metric) gradient step at x, in span units
template <int kD>
__device__ double pbfgs_pgnorm(const PbfgsState<kD>& S, const PbfgsBox& bx, int D) {
  double pg = 0.0;
  for (int a = 0; a < D; ++a)
    if (bx.span[a] > 0.0) pg = fmax(pg, fabs(clip_to(S.x[a] - bx.D2[a] * S.g[a], bx.lo[a], bx.hi[a]) - S.x[a]) / bx.span[a]);
  return pg;
}

template <int kD>
__device__ void pbfgs_trial(const PbfgsState<kD>& S, const PbfgsBox& bx, int D, double* trial) {
  for (int a = 0; a < D; ++a) trial[a] = clip_to(S.x[a] + S.t * S.p[a], bx.lo[a], bx.hi[a]);
}

// The search direction at the accepted point (x, g) and the first trial of its line search -> trial
template <int kD>
__device__ void pbfgs_direction(PbfgsState<kD>& S, const PbfgsBox& bx, int D, double* trial) {
  bool fr[kD];
  for (int a = 0; a < D; ++a)         // held: at a face with the gradient pointing out of the box (or a degenerate axis)
    fr[a] = bx.span[a] > 0.0 && !((S.x[a] <= bx.lo[a] && S.g[a] > 0.0) || (S.x[a] >= bx.hi[a] && S.g[a] < 0.0));
  double gp = 0.0;
  for (int a = 0; a < D; ++a) {
    double s = 0.0;
    if (fr[a])
      for (int c = 0; c < D; ++c)
        if (fr[c]) s += S.H[a * D + c] * S.g[c];
    S.p[a] = -s;
    gp += S.g[a] * S.p[a];
  }
  if (!(gp < 0.0)) {                  // not a descent direction: restart from (scaled) steepest descent
    pbfgs_reset_h(S, bx, D);
    for (int a = 0; a < D; ++a) S.p[a] = fr[a] ? -bx.D2[a] * S.g[a] : 0.0;
  }
  double pn = 0.0;
  for (int a = 0; a < D; ++a)
    if (bx.span[a] > 0.0) pn = fmax(pn, fabs(S.p[a]) / bx.span[a]);
  S.t = S.h_identity ? fmin(1.0, bx.cap / pn) : 1.0;   // a steepest-descent step moves at most `cap` span units
  S.halvings = 0;
  pbfgs_trial(S, bx, D, trial);
}

// Armijo along the projection arc for the evaluated trial (value ft; ok: the caller could use the evaluation) against the value f
// at x: true when the trial is acceptable -- pbfgs_update then takes it.  moved: the trial is not x itself.
template <int kD>
__device__ bool pbfgs_armijo(const PbfgsState<kD>& S, int D, const double* trial, bool ok, double ft, double f, bool& moved) {
  double dec = 0.0;
  moved = false;
  for (int a = 0; a < D; ++a) {
    dec += S.g[a] * (trial[a] - S.x[a]);
    moved = moved || trial[a] != S.x[a];
  }
  return ok && moved && ft <= f + 1e-4 * dec;
}

// The accepted trial with its gradient tg becomes (x, g), and H takes its BFGS update
template <int kD>
__device__ void pbfgs_update(PbfgsState<kD>& S, const PbfgsBox& bx, int D, const double* trial, const double* tg) {
  double s[kD], yv[kD], sy = 0.0, ss = 0.0, yy = 0.0;
  for (int a = 0; a < D; ++a) {
    s[a] = trial[a] - S.x[a];
    yv[a] = tg[a] - S.g[a];
    sy += s[a] * yv[a];
    ss += s[a] * s[a];
    yy += yv[a] * yv[a];
    S.x[a] = trial[a];
    S.g[a] = tg[a];
  }
  if (sy > 1e-10 * sqrt(ss * yy)) {   // BFGS update of the inverse Hessian, skipped unless s^T y > 0
    if (S.h_identity) {
      double yDy = 0.0;
      for (int a = 0; a < D; ++a) yDy += yv[a] * bx.D2[a] * yv[a];
      const double scale = sy / yDy;
      for (int a = 0; a < D; ++a) S.H[a * D + a] = scale * bx.D2[a];
      S.h_identity = 0;
    }
    double Hy[kD], yHy = 0.0;
    for (int a = 0; a < D; ++a) {
      double v = 0.0;
      for (int c = 0; c < D; ++c) v += S.H[a * D + c] * yv[c];
      Hy[a] = v;
      yHy += yv[a] * v;
    }
    const double rho = 1.0 / sy;
    const double cc = rho * rho * yHy + rho;
    for (int a = 0; a < D; ++a)
      for (int c = 0; c < D; ++c) S.H[a * D + c] += cc * s[a] * s[c] - rho * (Hy[a] * s[c] + s[a] * Hy[c]);
  }
}

// Halve the step after a refused trial: true with the next trial in `trial`, false after 60 halvings or when the arc no longer moves
template <int kD>
__device__ bool pbfgs_backtrack(PbfgsState<kD>& S, const PbfgsBox& bx, int D, bool moved, double* trial) {
  if (!moved || S.halvings >= 60) return false;
  ++S.halvings;
  S.t *= 0.5;
  pbfgs_trial(S, bx, D, trial);
  return true;
}

}  // namespace sbo
