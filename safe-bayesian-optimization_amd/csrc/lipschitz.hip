// lipschitz.hip -- sbo_mean_grad and sbo_lipschitz: the gradient of the mean at a point list, and the bound
// max over the box of ||grad MEAN_o||_inf by a multistart local search.
//
// The reference maximises max_a |d MEAN_i / d x_a| over the box with SciPy DE (models/SafeOpt.py:79-83, models/GoOSE.py:74-78);
// the sweeps take the maximum over their candidates, which is a lower bound of that.  Here
//   max_x ||grad MEAN_o(x)||_inf = max over (axis a, sign s) of max_x s g_a(x),      g_a = d MEAN_o / d x_a,
// and every inner problem is smooth: stage 1 evaluates g at the seeds (k_mean_grad, the kernel of sbo_mean_grad), keeps the `top`
// seeds of largest s g_a per (output, axis, sign), and stage 2 (k_lipschitz) runs one projected BFGS per kept seed -- the core of
// pbfgs.hpp in the metric of the box spans, with the row a of the mean's Hessian as the gradient of the objective.  The final
// iterates go through k_mean_grad again, and the answer is the largest |g_a| over the usable seeds and those points: a value that
// is attained, never an extrapolation of the solver's own arithmetic.
//
// Only the fp64 alpha and X_norm are read: no n x n matrix, no variance, nothing resident is written.
#include <algorithm>
#include <cmath>
#include <vector>
#include "internal.hpp"
#include "device_common.hpp"
#include "pbfgs.hpp"

namespace sbo {

constexpr int kLipChunk = 512;                   // observations of one LDS chunk of k_mean_grad (X_norm: 32 KiB at dpad = 8)
constexpr int kLipThreads = 256;
constexpr int kLipWaves = kLipThreads / 64;
constexpr int kLipDefaultTop = 4, kLipMaxTop = 16;
constexpr int kLipDefaultEval = 200, kLipMaxEval = 2000;
constexpr double kLipDefaultTol = 1e-9;
constexpr size_t kLipLds = 144 * 1024;           // LDS tier of k_lipschitz: X_norm and one output's alpha fit in this many bytes

struct LipArgs {
  ModelConst mc;
  int a_ld, top, max_eval, mask;             // mask: bit o = output o is bounded
  long long nS, nP;                          // seeds; solver problems q d 2 top (problem p's final iterate is point nS + p)
  double tol;
  double lo[kMaxD], hi[kMaxD];
};

// ---- stage 1: the gradient at a list ---------------------------------------------------------------------------------------------
// A lane owns a point and walks the outputs one after the other, the observations j = 0 .. n - 1 in order: a point's sums do not
// depend on the launch shape or on the point's place in the list.  X_norm and alpha_o come from LDS in chunks (every lane of a
// wave reads the same word: a broadcast).  grad [N][q][d], inf [N][q] (either may be nullptr); pts [N][d].
template <int D>
__global__ __launch_bounds__(kLipThreads) void k_mean_grad(const LipArgs* __restrict__ Ap, const double* __restrict__ alpha,
                                                           const double* __restrict__ Xn, const double* __restrict__ pts, long long N,
                                                           double* __restrict__ grad, double* __restrict__ inf) {
  __shared__ double sX[kLipChunk * D], sA[kLipChunk];
  const ModelConst& mc = Ap->mc;
  const int n = mc.n, d = mc.d, q = mc.q, tid = threadIdx.x;
  for (long long base = (long long)blockIdx.x * kLipThreads; base < N; base += (long long)gridDim.x * kLipThreads) {
    const long long i = base + tid;
    const bool on = i < N;
    double xn[D];
#pragma unroll
    for (int a = 0; a < D; ++a) xn[a] = (on && a < d) ? (pts[(size_t)i * d + a] - mc.X_mean[a]) / mc.X_std[a] : 0.0;
    for (int o = 0; o < q; ++o) {
      const double* al = alpha + (size_t)o * Ap->a_ld;
      const double sf2 = mc.sf2[o];
      double ie[D], acc[D];
#pragma unroll
      for (int a = 0; a < D; ++a) {
        ie[a] = a < d ? mc.inv_ell[o][a] : 0.0;
        acc[a] = 0.0;
      }
      for (int j0 = 0; j0 < n; j0 += kLipChunk) {
        const int cnt = min(kLipChunk, n - j0);
        __syncthreads();                              // (the chunk before this one has been read)
        for (int t = tid; t < cnt * D; t += kLipThreads) sX[t] = Xn[(size_t)j0 * D + t];
        for (int t = tid; t < cnt; t += kLipThreads) sA[t] = al[j0 + t];
        __syncthreads();
        if (on)
          for (int j = 0; j < cnt; ++j) {
            double diff[D], dist = 0.0;
#pragma unroll
            for (int a = 0; a < D; ++a) {
              diff[a] = a < d ? sX[j * D + a] - xn[a] : 0.0;
              dist += diff[a] * diff[a] * ie[a];
            }
            const double ak = sA[j] * (sf2 * exp(-0.5 * dist));
#pragma unroll
            for (int a = 0; a < D; ++a) acc[a] += ak * diff[a] * ie[a];
          }
      }
      if (on) {
        double m = 0.0;
#pragma unroll
        for (int a = 0; a < D; ++a)
          if (a < d) {
            const double g = mc.Y_std[o] * acc[a] / mc.X_std[a];
            if (grad) grad[((size_t)i * q + o) * d + a] = g;
            m = fmax(m, fabs(g));
          }
        if (inf) inf[(size_t)i * q + o] = m;
      }
    }
  }
}

// ---- which seeds are usable: finite and inside the box (not clipped) ---------------------------------------------------------------
__global__ void k_lip_flag(const LipArgs* __restrict__ Ap, const double* __restrict__ pts, int* __restrict__ use,
                           unsigned long long* __restrict__ count) {
  const LipArgs& A = *Ap;
  const int d = A.mc.d;
  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < A.nS; s += (long long)gridDim.x * blockDim.x) {
    bool ok = true;
    for (int a = 0; a < d; ++a) {
      const double v = pts[(size_t)s * d + a];
      ok = ok && isfinite(v) && v >= A.lo[a] && v <= A.hi[a];
    }
    use[s] = ok;
    if (ok) atomicAdd(count, 1ull);
  }
}

// ---- the `top` seeds of largest s g_a per (output, axis, sign), ties to the lowest seed -> pick[((o d + a) 2 + sg) top + t] -------
// One workgroup per (o, a, sg); round t takes the best seed behind round t - 1's in the order (value descending, index ascending).
// (The arg-max is arg_take / arg_block_best_all of device_common.hpp, the seed as the key: selects on plain scalars -- a comparator
// with early returns over a struct of (value, axis, sign, entry) came out of the compiler without the update of the value.)
__global__ __launch_bounds__(kLipThreads) void k_lip_top(const LipArgs* __restrict__ Ap, const double* __restrict__ grad,
                                                         const int* __restrict__ use, int* __restrict__ pick) {
  __shared__ double sv[kLipWaves];
  __shared__ long long sk[kLipWaves];
  const LipArgs& A = *Ap;
  const int d = A.mc.d, q = A.mc.q, tid = threadIdx.x;
  const int sg = blockIdx.x & 1, a = (blockIdx.x >> 1) % d, o = (blockIdx.x >> 1) / d;
  int* out = pick + (size_t)blockIdx.x * A.top;
  const bool asked = ((A.mask >> o) & 1) && A.hi[a] - A.lo[a] > 0.0;
  const double sgn = sg ? -1.0 : 1.0;
  bool more = asked;
  double lastv = 0.0;                                 // the pick of the round before
  long long lasti = -1;
  for (int t = 0; t < A.top; ++t) {
    if (!more) {                                      // (the same for the whole workgroup)
      if (tid == 0) out[t] = -1;
      continue;
    }
    double bv = 0.0;
    long long bk = kArgNone;
    for (long long s = tid; s < A.nS; s += kLipThreads) {
      const double v = sgn * grad[((size_t)s * q + o) * d + a];
      const bool open = use[s] != 0 && v == v && (t == 0 || v < lastv || (v == lastv && s > lasti));
      arg_take(bv, bk, v, open ? s : kArgNone);
    }
    arg_block_best_all(bv, bk, sv, sk);
    more = bk != kArgNone;
    if (tid == 0) out[t] = more ? (int)bk : -1;
    lastv = bv;
    lasti = bk;
  }
}

// ---- largest |g_a| of output o over the usable entries [0, E), all axes: ties to the lowest axis, then sign +, then the lowest entry
// (seeds stand before the iterates).  The order behind the value is one key: (2 axis + (sign < 0)) << 40 | entry ----------------------
struct LipBest {
  double v;
  long long key;             // kArgNone: none
};
__device__ __forceinline__ int lip_key_axis(long long key) { return (int)(key >> 41); }
__device__ __forceinline__ int lip_key_neg(long long key) { return (int)((key >> 40) & 1); }
__device__ __forceinline__ long long lip_key_entry(long long key) { return key & ((1LL << 40) - 1); }
__device__ LipBest lip_argmax(const LipArgs& A, int o, long long E, const double* grad, const int* use, double* sv, long long* sk) {
  const int d = A.mc.d, q = A.mc.q;
  double bv = 0.0;
  long long bk = kArgNone;
  for (long long e = threadIdx.x; e < E; e += kLipThreads) {
    const bool on = use[e] != 0;
    for (int a = 0; a < d; ++a) {
      const double g = grad[((size_t)e * q + o) * d + a];
      const double v = fabs(g);
      const long long key = ((long long)(2 * a + (g < 0.0 ? 1 : 0)) << 40) | e;
      arg_take(bv, bk, v, (on && v == v) ? key : kArgNone);      // (a NaN is never taken)
    }
  }
  arg_block_best_all(bv, bk, sv, sk);
  return LipBest{bv, bk};
}

// one workgroup per output: L_seed over the seeds
__global__ __launch_bounds__(kLipThreads) void k_lip_seedmax(const LipArgs* __restrict__ Ap, const double* __restrict__ grad,
                                                             const int* __restrict__ use, double* __restrict__ Lseed) {
  __shared__ double sv[kLipWaves];
  __shared__ long long sk[kLipWaves];
  const LipArgs& A = *Ap;
  const int o = blockIdx.x;
  if (!((A.mask >> o) & 1)) {
    if (threadIdx.x == 0) Lseed[o] = 0.0;
    return;
  }
  const LipBest b = lip_argmax(A, o, A.nS, grad, use, sv, sk);
  if (threadIdx.x == 0) Lseed[o] = b.key != kArgNone ? b.v : 0.0;
}

// one workgroup per output: the result over seeds and final iterates; workgroup 0 also sums the solver's counters
__global__ __launch_bounds__(kLipThreads) void k_lip_final(const LipArgs* __restrict__ Ap, const double* __restrict__ pts,
                                                           const double* __restrict__ grad, const int* __restrict__ use,
                                                           const double* __restrict__ Lseed, const int* __restrict__ nev,
                                                           const int* __restrict__ conv, const unsigned long long* __restrict__ count,
                                                           sbo_lipschitz_result* __restrict__ res) {
  __shared__ double sv[kLipWaves];
  __shared__ long long sk[kLipWaves];
  const LipArgs& A = *Ap;
  const int o = blockIdx.x, d = A.mc.d;
  if (o == 0 && threadIdx.x == 0) {
    long long ev = 0;
    int np = 0, nc = 0;
    for (long long p = 0; p < A.nP; ++p)
      if (use[A.nS + p]) {
        ++np;
        ev += nev[p];
        nc += conv[p];
      }
    res->seeds_used = (long long)*count;
    res->evaluations = ev;
    res->problems = np;
    res->converged = nc;
  }
  if (!((A.mask >> o) & 1)) return;               // (the block was cleared: L, L_seed, x, axis, sign stay 0)
  const LipBest b = lip_argmax(A, o, A.nS + A.nP, grad, use, sv, sk);
  if (threadIdx.x == 0) {
    res->L_seed[o] = Lseed[o];
    if (b.key != kArgNone) {
      res->L[o] = b.v;
      res->axis[o] = lip_key_axis(b.key);
      res->sign[o] = lip_key_neg(b.key) ? -1 : 1;
      for (int a = 0; a < d; ++a) res->x[o][a] = pts[(size_t)lip_key_entry(b.key) * d + a];
    }
  }
}

// ---- stage 2: maximise s g_a over the box from one seed --------------------------------------------------------------------------
struct LipState {
  PbfgsState<kMaxD> s;
  double D2[kMaxD], span[kMaxD];
  double f;
  int started, nev, conv;
};

// The next search direction at the accepted point: false when the projected gradient is within tol (converged), or when the step
// that led here gained nothing beyond rounding (stalled: as a failed search)
__device__ bool lip_new_iteration(LipState& S, const PbfgsBox& bx, int d, double tol, double* trial, bool stalled = false) {
  if (pbfgs_pgnorm(S.s, bx, d) <= tol) {
    S.conv = 1;
    return false;
  }
  if (stalled) return false;
  pbfgs_direction(S.s, bx, d, trial);
  return true;
}

// consume the evaluation (F, gF) of `trial`; true when `trial` holds the next point to evaluate
__device__ __noinline__ bool lip_advance(LipState& S, const LipArgs& A, double F, const double* gF, double* trial) {
  const int d = A.mc.d;
  const PbfgsBox bx{A.lo, A.hi, S.D2, S.span, 0.1};
  bool ok = isfinite(F);
  for (int a = 0; a < d; ++a) ok = ok && isfinite(gF[a]);
  ++S.nev;
  if (!S.started) {
    if (!ok) return false;                            // the seed stands as the final point
    S.started = 1;
    S.f = F;
    for (int a = 0; a < d; ++a) S.s.g[a] = gF[a];
    if (S.nev >= A.max_eval) return false;
    return lip_new_iteration(S, bx, d, A.tol, trial);
  }
  bool moved;
  if (pbfgs_armijo(S.s, d, trial, ok, F, S.f, moved)) {
    pbfgs_update(S.s, bx, d, trial, gF);
    const double fprev = S.f;
    S.f = F;
    if (S.nev >= A.max_eval) return false;
    return lip_new_iteration(S, bx, d, A.tol, trial, fabs(fprev - F) <= 1e-15 * (1.0 + fabs(fprev)));
  }
  if (S.nev >= A.max_eval) return false;
  if (pbfgs_backtrack(S.s, bx, d, moved, trial)) return true;
  if (S.s.h_identity) return false;                   // steepest descent found no Armijo point either: the end
  pbfgs_reset_h(S.s, bx, d);                          // the quasi-Newton direction failed: one steepest-descent try
  return lip_new_iteration(S, bx, d, A.tol, trial);
}

// One workgroup per problem p = ((o d + a) 2 + sg) top + t, from seed pick[p] (-1: no problem).  F = -s g_a / L_seed[o]; an
// evaluation is d + 1 workgroup sums over the observations (lane-serial partials, block_sum_cols).  kLds: X_norm and alpha_o are
// staged in LDS first; the arithmetic is the same either way.  The final iterate goes to pts[nS + p], its usability to use[nS + p].
template <bool kLds>
__global__ __launch_bounds__(kLipThreads) void k_lipschitz(const LipArgs* __restrict__ Ap, const double* __restrict__ alpha,
                                                           const double* __restrict__ Xn, double* __restrict__ pts,
                                                           const int* __restrict__ pick, const double* __restrict__ Lseed,
                                                           int* __restrict__ use, int* __restrict__ nev_out, int* __restrict__ conv_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ LipState R;
  __shared__ double trial[kMaxD], red[kMaxD + 1];
  __shared__ double part[kLipWaves][kMaxD + 1];
  __shared__ int go;
  const LipArgs& A = *Ap;
  const ModelConst& mc = A.mc;
  const int n = mc.n, d = mc.d, dp = mc.dpad, tid = threadIdx.x;
  const long long p = blockIdx.x;
  const int sg = (int)((p / A.top) & 1), ax = (int)((p / A.top / 2) % d), o = (int)(p / A.top / 2 / d);
  const int seed = pick[p];
  if (seed < 0) {                                     // (the same for the whole workgroup)
    if (tid == 0) {
      for (int a = 0; a < d; ++a) pts[(size_t)(A.nS + p) * d + a] = A.lo[a];
      use[A.nS + p] = 0;
      nev_out[p] = 0;
      conv_out[p] = 0;
    }
    return;
  }
  const double* Xs = Xn;
  const double* as = alpha + (size_t)o * A.a_ld;
  if (kLds) {
    double* lX = reinterpret_cast<double*>(smem);     // [n][dp]
    double* lA = lX + (size_t)n * dp;                 // [n]
    for (int t = tid; t < n * dp; t += kLipThreads) lX[t] = Xn[t];
    for (int t = tid; t < n; t += kLipThreads) lA[t] = as[t];
    Xs = lX;
    as = lA;
  }
  if (tid == 0) {
    for (int a = 0; a < d; ++a) {
      trial[a] = pts[(size_t)seed * d + a];
      R.s.x[a] = trial[a];
      R.span[a] = A.hi[a] - A.lo[a];
      R.D2[a] = R.span[a] * R.span[a];
    }
    R.started = R.nev = R.conv = 0;
    R.f = 0.0;
    pbfgs_reset_h(R.s, PbfgsBox{A.lo, A.hi, R.D2, R.span, 0.1}, d);
    go = 1;
  }
  __syncthreads();
  const double sf2 = mc.sf2[o], ls = Lseed[o];
  const double scale = (sg ? 1.0 : -1.0) / (ls > 0.0 && isfinite(ls) ? ls : 1.0);   // F = scale g_a
  double ie[kMaxD];
#pragma unroll
  for (int a = 0; a < kMaxD; ++a) ie[a] = a < d ? mc.inv_ell[o][a] : 0.0;
  while (go) {
    double xn[kMaxD];
#pragma unroll
    for (int a = 0; a < kMaxD; ++a) xn[a] = a < d ? (trial[a] - mc.X_mean[a]) / mc.X_std[a] : 0.0;
    double acc[kMaxD + 1];
#pragma unroll
    for (int a = 0; a < kMaxD + 1; ++a) acc[a] = 0.0;
    for (int j = tid; j < n; j += kLipThreads) {
      double diff[kMaxD], dist = 0.0, da = 0.0;
#pragma unroll
      for (int a = 0; a < kMaxD; ++a) {
        diff[a] = a < d ? Xs[(size_t)j * dp + a] - xn[a] : 0.0;
        dist += diff[a] * diff[a] * ie[a];
        if (a == ax) da = diff[a];
      }
      const double ak = as[j] * (sf2 * exp(-0.5 * dist));
      acc[0] += ak * da;
#pragma unroll
      for (int b = 0; b < kMaxD; ++b)
        if (b < d) acc[1 + b] += ak * (da * diff[b] * ie[b] - (b == ax ? 1.0 : 0.0));
    }
    block_sum_cols(acc, d + 1, part, red);
    if (tid == 0) {
      const double Ca = mc.Y_std[o] * mc.inv_ell[o][ax] / mc.X_std[ax];
      double gF[kMaxD];
      for (int b = 0; b < d; ++b) gF[b] = scale * (Ca * red[1 + b] / mc.X_std[b]);
      go = lip_advance(R, A, scale * (Ca * red[0]), gF, trial);
    }
    __syncthreads();
  }
  if (tid == 0) {
    for (int a = 0; a < d; ++a) pts[(size_t)(A.nS + p) * d + a] = R.s.x[a];
    use[A.nS + p] = 1;
    nev_out[p] = R.nev;
    conv_out[p] = R.conv;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static int lip_launch_grad(sbo_ctx* c, const LipArgs* dA, const double* pts, long long N, double* grad, double* inf) {
  if (N <= 0) return SBO_OK;
  const unsigned nb = (unsigned)std::min<long long>((N + kLipThreads - 1) / kLipThreads, 8192);
  const double *al = c->factor.alpha(), *Xn = (const double*)c->Xn.p;
  with_dpad(c->mc.dpad, [&](auto D) {
    hipLaunchKernelGGL(k_mean_grad<D()>, dim3(nb), dim3(kLipThreads), 0, c->stream, dA, al, Xn, pts, N, grad, inf);
  });
  SBO_HIP(hipGetLastError());
  return SBO_OK;
}

template <bool kLds>
static int lip_launch_solver(sbo_ctx* c, size_t lds, long long P, const LipArgs* dA, double* pts, const int* pick, const double* Lseed,
                             int* use, int* nev, int* conv) {
  SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_lipschitz<kLds>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_lipschitz<kLds>), dim3((unsigned)P), dim3(kLipThreads), lds, c->stream, dA, c->factor.alpha(),
                     (const double*)c->Xn.p, pts, pick, Lseed, use, nev, conv);
  SBO_HIP(hipGetLastError());
  return SBO_OK;
}

}  // namespace sbo

using namespace sbo;

extern "C" int sbo_mean_grad(sbo_ctx* c, int64_t n_points, const double* points, double* grad_out, double* infnorm_out) {
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (!points || (!grad_out && !infnorm_out)) return fail(SBO_E_INVALID, "NULL argument");
  if (n_points < 1 || n_points > (1LL << 28)) return fail(SBO_E_INVALID, "n_points out of range");
  int rc;
  if ((rc = model_reader_begin(c, "sbo_mean_grad", true))) return rc;
  const int d = c->mc.d, q = c->mc.q;
  const size_t N = (size_t)n_points;
  LipArgs A{};
  A.mc = c->mc;
  A.a_ld = c->factor.a_ld();
  LipArgs* dA;
  double *dpts, *dgrad, *dinf;
  auto layout = [&](Carve cv) {
    cv.take(dA, 1);
    cv.take(dpts, N * d);
    cv.take(dgrad, grad_out ? N * q * d : 0);
    cv.take(dinf, infnorm_out ? N * q : 0);
    return cv.off;
  };
  if ((rc = carve(c->lipbuf, layout, 256))) return rc;
  SBO_HIP(hipMemcpyAsync(dA, &A, sizeof(A), hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dpts, points, sizeof(double) * N * d, hipMemcpyHostToDevice, c->stream));
  if ((rc = lip_launch_grad(c, dA, dpts, n_points, grad_out ? dgrad : nullptr, infnorm_out ? dinf : nullptr))) return rc;
  if (grad_out) SBO_HIP(hipMemcpyAsync(grad_out, dgrad, sizeof(double) * N * q * d, hipMemcpyDeviceToHost, c->stream));
  if (infnorm_out) SBO_HIP(hipMemcpyAsync(infnorm_out, dinf, sizeof(double) * N * q, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipStreamSynchronize(c->stream));
  return SBO_OK;
}

extern "C" int sbo_lipschitz(sbo_ctx* c, const sbo_lipschitz_opts* opts, int64_t n_seeds, const double* seeds,
                             sbo_lipschitz_result* result) {
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (!opts || !seeds || !result) return fail(SBO_E_INVALID, "NULL argument");
  int rc;
  if ((rc = model_reader_check(c, "sbo_lipschitz", true))) return rc;   // (d and q, which the checks below need)
  const int d = c->mc.d, q = c->mc.q;
  if (n_seeds < 1 || n_seeds > (1LL << 24)) return fail(SBO_E_INVALID, "n_seeds out of range");
  if (opts->top > kLipMaxTop) return fail(SBO_E_INVALID, "top must be at most 16");
  if (opts->max_eval > kLipMaxEval) return fail(SBO_E_INVALID, "max_eval must be at most 2000");
  if (std::isnan(opts->tol)) return fail(SBO_E_INVALID, "tol is NaN");
  if (q < 32 && (opts->output_mask >> q) != 0) return fail(SBO_E_INVALID, "output_mask: no bit may reach q");
  for (int a = 0; a < d; ++a)
    if (!std::isfinite(opts->lo[a]) || !std::isfinite(opts->hi[a]) || !(opts->lo[a] <= opts->hi[a]))
      return fail(SBO_E_INVALID, "box needs finite lo <= hi");
  if ((rc = model_reader_begin(c, "sbo_lipschitz", true))) return rc;
  LipArgs A{};
  A.mc = c->mc;
  A.a_ld = c->factor.a_ld();
  A.top = opts->top > 0 ? opts->top : kLipDefaultTop;
  A.max_eval = opts->max_eval > 0 ? opts->max_eval : kLipDefaultEval;
  A.mask = opts->output_mask ? (int)opts->output_mask : (1 << q) - 1;
  A.tol = opts->tol > 0.0 ? opts->tol : kLipDefaultTol;
  A.nS = n_seeds;
  A.nP = (long long)q * d * 2 * A.top;
  for (int a = 0; a < d; ++a) {
    A.lo[a] = opts->lo[a];
    A.hi[a] = opts->hi[a];
  }
  // scratch: arguments | points [nS + nP][d] (seeds, then the problems' final iterates) | grad [nS + nP][q][d] | usable [nS + nP] |
  // pick, evaluations, converged [nP] | L_seed [q] | seed count | the result block
  const size_t E = (size_t)(A.nS + A.nP);
  LipArgs* dA;
  double *dpts, *dgrad, *dLs;
  int *duse, *dpick, *dnev, *dconv;
  unsigned long long* dcount;
  sbo_lipschitz_result* dres;
  auto layout = [&](Carve cv) {
    cv.take(dA, 1);
    cv.take(dpts, E * d);
    cv.take(dgrad, E * q * d);
    cv.take(duse, E);
    cv.take(dpick, A.nP);
    cv.take(dnev, A.nP);
    cv.take(dconv, A.nP);
    cv.take(dLs, kMaxQ);
    cv.take(dcount, 1);
    cv.take(dres, 1);
    return cv.off;
  };
  if ((rc = carve(c->lipbuf, layout, 256))) return rc;
  hipStream_t st = c->stream;
  SBO_HIP(hipMemcpyAsync(dA, &A, sizeof(A), hipMemcpyHostToDevice, st));
  SBO_HIP(hipMemcpyAsync(dpts, seeds, sizeof(double) * (size_t)A.nS * d, hipMemcpyHostToDevice, st));
  SBO_HIP(hipMemsetAsync(dcount, 0, sizeof(*dcount), st));
  SBO_HIP(hipMemsetAsync(dres, 0, sizeof(*dres), st));
  const unsigned nbs = (unsigned)std::min<long long>((A.nS + 255) / 256, 4096);
  hipLaunchKernelGGL(k_lip_flag, dim3(nbs), dim3(256), 0, st, (const LipArgs*)dA, (const double*)dpts, duse, dcount);
  SBO_HIP(hipGetLastError());
  if ((rc = lip_launch_grad(c, dA, dpts, A.nS, dgrad, nullptr))) return rc;
  hipLaunchKernelGGL(k_lip_seedmax, dim3(q), dim3(kLipThreads), 0, st, (const LipArgs*)dA, (const double*)dgrad, (const int*)duse, dLs);
  SBO_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_lip_top, dim3(q * d * 2), dim3(kLipThreads), 0, st, (const LipArgs*)dA, (const double*)dgrad, (const int*)duse, dpick);
  SBO_HIP(hipGetLastError());
  const size_t lds = sizeof(double) * (size_t)c->mc.n * (c->mc.dpad + 1);
  if (c->opt.lipschitz_lds && lds <= kLipLds)
    rc = lip_launch_solver<true>(c, lds, A.nP, dA, dpts, dpick, dLs, duse, dnev, dconv);
  else
    rc = lip_launch_solver<false>(c, 0, A.nP, dA, dpts, dpick, dLs, duse, dnev, dconv);
  if (rc) return rc;
  if ((rc = lip_launch_grad(c, dA, dpts + (size_t)A.nS * d, A.nP, dgrad + (size_t)A.nS * q * d, nullptr))) return rc;
  hipLaunchKernelGGL(k_lip_final, dim3(q), dim3(kLipThreads), 0, st, (const LipArgs*)dA, (const double*)dpts, (const double*)dgrad,
                     (const int*)duse, (const double*)dLs, (const int*)dnev, (const int*)dconv, (const unsigned long long*)dcount, dres);
  SBO_HIP(hipGetLastError());
  sbo_lipschitz_result res;
  SBO_HIP(hipMemcpyAsync(&res, dres, sizeof(res), hipMemcpyDeviceToHost, st));
  SBO_HIP(hipStreamSynchronize(st));
  if (res.seeds_used < 1) return fail(SBO_E_INVALID, "no seed is finite and inside the box");
  *result = res;
  return SBO_OK;
}
