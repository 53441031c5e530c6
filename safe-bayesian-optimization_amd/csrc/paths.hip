// paths.hip -- sbo_sample_paths: posterior sample paths by pathwise conditioning (Matheron's rule).
//
// A path is a function: a random-feature draw from the prior plus an update that depends on the data,
//   f_s(p) = mp + sum_f B[f][s] cos(omega_f . u(p) + phase_f) + sum_j k(X_j, p) c_s[j],   B[f][s] = sqrt(2 sf2 / F) weights[s][f],
//   c_s = M^T (M r_s),   r_s[j] = (y_j - mp) - prior_s(X_j) - sqrt(sn2) noise[s][j]   (M^T M = inv(K + sn2 I), the resident fp64 factor)
// which is ONE matrix product per point tile: the A operand [point][F + n] is generated on the fly (cos features, then RBF columns),
// the B operand [F + n][S] (scaled weights, then c) is small and lives in L2.
//   k_obs_prep     (through ObsResident, slab_tiles.hpp) the observations in the output's scaled coordinates and their squares
//   k_path_bw      the feature rows of B
//   k_path_main    the hot path on the matrix cores: a workgroup owns kPathTile points x all Spad paths, wave w points 32 w .. + 31 as
//                  2 x Spad / 16 accumulators of MM<double> (v_mfma_f64_4x4x4, four per step).  The K axis is the F features rounded up
//                  to a slab, then the n observations rounded up to a slab; per slab of kSlabK columns every thread generates 16
//                  elements of the A image (a column's value at a point is computed once and used by every path) and tile128_step
//                  (slab_tiles.hpp) stages the [32][Spad] slab of B beside it.  Epilogue (tile128_arg_best): un-normalise, store [m][S]
//                  where asked, a running arg-best per path.  A bounded grid walks the tiles; one partial per (workgroup, path).
//                  The prior at the data is THIS kernel with the observations as the points and no observation slabs: no second
//                  feature evaluator exists that could round differently.
//   k_path_solve   per path: r, w = M r (factor_lower_mv, whiten.hpp), c = M^T w (factor_upper_mv) into the observation rows of B
//   k_path_bt      the packed per-path image [S][F + n] of B's columns, for sbo_refine_paths' one-point evaluator (refine.hip)
//   k_path_finish  the partials of the workgroups -> the result block (partials_merge, slab_tiles.hpp)
// Every sum over features and observations runs in an order fixed by (F, n) alone, (value, index) reductions are arg_take's total
// order, there are no atomics: the value of (point, path) does not depend on m, on the point's place or on the other paths, and two
// calls return the same bits.  One read-back, one host wait; nothing resident is written.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include "slab_tiles.hpp"

namespace sbo {

constexpr int kPathTile = 128;                   // points of one workgroup tile of k_path_main (4 waves x 32 points)
constexpr int kPathThreads = 256;                // k_path_main
constexpr int kPathGridTiles = 1024;             // workgroups k_path_main aims at: min(point tiles, kPathGridTiles); each walks its tiles
static_assert(kPathTile == kTile128 && kPathThreads == kTileThreads, "k_path_main: tile128_step's tile and workgroup");
static_assert(SBO_MAX_PATHS == 64, "k_path_main is instantiated for 16, 32 and 64 padded paths");

struct PathArgs {                                // by value (kernarg segment)
  int n, d, ld, q;                               // observations, input dimension, leading dimension of the resident factor, outputs
  int F, S, Spad, o;                             // features, paths, paths rounded up to 16 | 32 | 64, the output
  int KF, KN, maximize, pad;                     // F and n rounded up to kSlabK (KN = 0: no observation part)
  long long m;                                   // points
  OutParams op;                                  // the output
  double ymean, ystd, fscale;                    // fscale = sqrt(2 sf2 / F)
};

struct PathBufs {
  ObsResident obs;                               // (without w)
  double *om, *ph, *wt, *nz, *B, *prior, *pts, *vals, *pval, *Bt;
  long long* pidx;
  sbo_paths_result* res;
};

// ---- the feature rows of B: B [f][s] = fscale weights[s][f] (the buffer was zeroed: rows from F on and columns from S on stay zero) ---
__global__ __launch_bounds__(256) void k_path_bw(const PathArgs A, const double* __restrict__ wt /* [S][F] */, double* __restrict__ B) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)A.F * A.S) return;
  const int s = (int)(e / A.F), f = (int)(e - (long long)s * A.F);
  B[(size_t)f * A.Spad + s] = A.fscale * wt[e];
}

// ---- the hot path -------------------------------------------------------------------------------------------------------------------
// Thread t generates, per slab, columns tile128_k() .. + 15 of point tile128_row() of the tile (the column is wave-uniform: its omega
// row or observation is read once per wave).  The tile of slab_tiles.hpp: the points are the rows, the paths the columns.  Points past
// m generate zeros and are never stored or taken.
// `pts` holds rows of d coordinates x with u = ((x - X_mean) / X_std) vinv: the raw points, or -- with X_mean = 0, X_std = 1, both exact
// -- the normalised observations.  The value is ymean + ystd (mp + sum): the caller's units, or -- with 0, 1, 0, all exact -- the sum.
template <int D, int SB>
__global__ __launch_bounds__(kPathThreads, 2) void k_path_main(const PathArgs A, long long ntiles, const double* __restrict__ pts,
                                                              const double* __restrict__ om /* [KF][D] */, const double* __restrict__ ph /* [KF] */,
                                                              const double* __restrict__ As, const double* __restrict__ sq,
                                                              const double* __restrict__ B /* [KF + KN][Spad] */, double* __restrict__ vals /* [m][S] or null */,
                                                              double* __restrict__ pval, long long* __restrict__ pidx /* [grid][Spad] or null */) {
  constexpr int SP = 16 * SB;
  __shared__ __attribute__((aligned(32))) Tile128Lds<SB> lds;
  const int gp = tile128_row(), gk = tile128_k();     // generation: this thread's point of the tile and its first column of the slab
  const int n = A.n, F = A.F;
  long long run_idx = kArgNone;                   // threads 0 .. SP - 1: path tid over this workgroup's tiles
  double run_val = 0.0;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long p0 = tile * kPathTile;
    const bool on = p0 + gp < A.m;
    double u[D];
    const double usq = rbf_scale<D>(A.op, pts + (size_t)(on ? p0 + gp : 0) * A.d, on, u);
    d4_t acc[2][SB];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int c = 0; c < SB; ++c) acc[a][c] = d4_t{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < A.KF + A.KN; k0 += kSlabK) {
      double g[16];
      if (k0 < A.KF) {                              // features: cos(omega_f . u + phase_f)
        const int f0 = __builtin_amdgcn_readfirstlane(k0 + gk);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int f = f0 + e;
          double arg = 0.0;
#pragma unroll
          for (int a = 0; a < D; ++a) arg += om[(size_t)f * D + a] * u[a];
          arg += ph[f];
          g[e] = (on && f < F) ? cos(arg) : 0.0;
        }
      } else {                                      // observations: rbf_k, their coordinates read from global memory
        const int j0 = __builtin_amdgcn_readfirstlane(k0 - A.KF + gk);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int j = j0 + e, jj = j < n ? j : n - 1;
          const double kv = rbf_k<D>(A.op.sf2, As + (size_t)jj * D, sq[jj], u, usq);
          g[e] = (on && j < n) ? kv : 0.0;
        }
      }
      tile128_step(lds, g, B + (size_t)k0 * SP, acc);
    }
    // epilogue: the values in the caller's units, and per path the arg-best over this tile's points
    tile128_arg_best(lds, acc, p0, A.m, A.S, A.maximize, vals, [&](long long, double x) { return A.ymean + A.ystd * (A.op.mp + x); }, run_val, run_idx);
  }
  tile128_store_partial<SB>(pval, pidx, run_val, run_idx);
}

// ---- per path: the residual, w = M r, c = M^T w -> B [KF + j][s] --------------------------------------------------------------------
// One workgroup per path; both orders depend on n alone.
__global__ __launch_bounds__(1024) void k_path_solve(const PathArgs A, const double* __restrict__ Yn /* [n][q] */, const double* __restrict__ prior /* [n][S] */,
                                                     const double* __restrict__ nz /* [S][n] */, const double* __restrict__ Fm, double* __restrict__ B) {
  static_assert(kFactorMvThreads == 1024, "k_path_solve is launched with the workgroup of factor_lower_mv / factor_upper_mv");
  __shared__ double sr[SBO_MAX_N], sw[SBO_MAX_N];
  const int n = A.n, ld = A.ld, s = blockIdx.x;
  const double* M = Fm + (size_t)A.o * ld * ld;
  const double sn = sqrt(A.op.sn2);
  for (int j = threadIdx.x; j < n; j += 1024) sr[j] = ((Yn[(size_t)j * A.q + A.o] - A.op.mp) - prior[(size_t)j * A.S + s]) - sn * nz[(size_t)s * n + j];
  __syncthreads();
  factor_lower_mv(M, ld, n, sr, sw, n);
  __syncthreads();
  factor_upper_mv(M, ld, n, sw, [&](int j, double t) { B[(size_t)(A.KF + j) * A.Spad + s] = t; });
}

// ---- per path: the workgroups' partials -> the result block ---------------------------------------------------------------------------
__global__ __launch_bounds__(kMergeThreads) void k_path_finish(const PathArgs A, int nwg, const double* __restrict__ pval,
                                                               const long long* __restrict__ pidx, sbo_paths_result* __restrict__ res) {
  partials_merge(A.S, A.Spad, A.maximize, nwg, pval, pidx, res->index, res->value);
}

// ---- per path: the packed image Bt [s][F + n] = B's feature rows, then its observation rows, of column s -------------------------------
// (what a one-point evaluator of path s reads front to back: sbo_refine_paths' solver)
__global__ __launch_bounds__(256) void k_path_bt(const PathArgs A, const double* __restrict__ B, double* __restrict__ Bt) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int w = A.F + A.n;
  if (e >= (long long)A.S * w) return;
  const int s = (int)(e / w), k = (int)(e - (long long)s * w);
  Bt[e] = B[(size_t)(k < A.F ? k : A.KF + (k - A.F)) * A.Spad + s];
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// the argument block of a call on c's model: S paths of F features of output o at m points
static PathArgs path_args(const sbo_ctx* c, int o, int S, int F, int maximize, long long m) {
  const ModelConst& mc = c->mc;
  PathArgs A{};
  A.n = mc.n;
  A.d = mc.d;
  A.q = mc.q;
  A.ld = c->factor.ld();
  A.F = F;
  A.S = S;
  A.Spad = spad_of(S);
  A.o = o;
  A.KF = (F + kSlabK - 1) / kSlabK * kSlabK;
  A.KN = (mc.n + kSlabK - 1) / kSlabK * kSlabK;
  A.maximize = maximize;
  A.m = m;
  A.op = out_params(mc, o);
  A.ymean = mc.Y_mean[o];
  A.ystd = mc.Y_std[o];
  A.fscale = std::sqrt(2.0 * mc.sf2[o] / (double)F);
  return A;
}

// scratch: X_norm [n][d] | Y_norm [n][q] | scaled observations [n][dpad], their squares | omega [KF][dpad], phase [KF] (zero rows behind
// F) | weights [S][F] | noise [S][n] | B [KF + KN][Spad] | the prior at the data [n][S] | the points | the values [m][S] where asked |
// sbo_sample_paths: the partials [nwg][Spad], the result block | a caller that evaluates paths itself (image): Bt [S][F + n]
static size_t paths_layout(Carve cv, const ModelConst& mc, const PathArgs& A, bool vals, int nwg, bool image, PathBufs& Bf) {
  const size_t KF = (size_t)A.KF, Sp = (size_t)A.Spad;
  Bf.obs.take(cv, mc, 1, 0);
  cv.take(Bf.om, KF * mc.dpad);
  cv.take(Bf.ph, KF);
  cv.take(Bf.wt, (size_t)A.S * A.F);
  cv.take(Bf.nz, (size_t)A.S * A.n);
  cv.take(Bf.B, (KF + (size_t)A.KN) * Sp);
  cv.take(Bf.prior, (size_t)A.n * A.S);
  cv.take(Bf.pts, (size_t)A.m * A.d);
  cv.take(Bf.vals, vals ? (size_t)A.m * A.S : 0);
  cv.take(Bf.pval, (size_t)nwg * Sp);
  cv.take(Bf.pidx, (size_t)nwg * Sp);
  cv.take(Bf.res, image ? 0 : 1);
  cv.take(Bf.Bt, image ? (size_t)A.S * (A.F + A.n) : 0);
  return cv.off;
}

// the draws and the observations on their way to the device; dr.omega_padded: omega in padded lanes [KF][dpad], zero behind d and behind
// F (a host block the copy reads: the caller waits for the stream before it lets go of dr)
static hipError_t paths_upload(sbo_ctx* c, const PathArgs& A, const PathBufs& Bf, PathDraws& dr) {
  hipStream_t st = c->stream;
  const int D = c->mc.dpad, d = A.d, F = A.F, S = A.S, n = A.n;
  const size_t KF = (size_t)A.KF, Sp = (size_t)A.Spad;
  dr.omega_padded.assign(KF * D, 0.0);
  for (int f = 0; f < F; ++f)
    for (int a = 0; a < d; ++a) dr.omega_padded[(size_t)f * D + a] = dr.omega[(size_t)f * d + a];
  hipError_t e = hipMemsetAsync(Bf.ph, 0, sizeof(double) * KF, st);
  if (e == hipSuccess) e = hipMemsetAsync(Bf.B, 0, sizeof(double) * (KF + (size_t)A.KN) * Sp, st);
  if (e == hipSuccess) e = hipMemcpyAsync(Bf.om, dr.omega_padded.data(), sizeof(double) * KF * D, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(Bf.ph, dr.phase, sizeof(double) * (size_t)F, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(Bf.wt, dr.weights, sizeof(double) * (size_t)S * F, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(Bf.nz, dr.noise, sizeof(double) * (size_t)S * n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = Bf.obs.upload(c, st);
  return e;
}

// prepare: the scaled observations, the feature rows of B, the prior at the data, the observation rows of B
template <int D, int SB>
static int paths_prepare(sbo_ctx* c, const PathArgs& A, const PathBufs& Bf) {
  hipStream_t st = c->stream;
  const int n = A.n;
  if (int rc = Bf.obs.prepare<D>(c, st, &A.op, &A.o, 1, 0)) return rc;
  hipLaunchKernelGGL(k_path_bw, dim3((unsigned)(((long long)A.F * A.S + 255) / 256)), dim3(256), 0, st, A, (const double*)Bf.wt, Bf.B);
  SBO_HIP(hipGetLastError());
  // the prior at the data: the observations as the points (already normalised: X_mean = 0, X_std = 1), no observation part, the bare sum
  PathArgs P = A;
  P.m = n;
  P.KN = 0;
  P.op.mp = 0.0;
  P.ymean = 0.0;
  P.ystd = 1.0;
  for (int a = 0; a < kMaxD; ++a) {
    P.op.X_mean[a] = 0.0;
    P.op.X_std[a] = 1.0;
  }
  const long long ptiles = ((long long)n + kPathTile - 1) / kPathTile;
  hipLaunchKernelGGL((k_path_main<D, SB>), dim3((unsigned)ptiles), dim3(kPathThreads), 0, st, P, ptiles, (const double*)Bf.obs.Xn, (const double*)Bf.om,
                     (const double*)Bf.ph, (const double*)Bf.obs.As, (const double*)Bf.obs.sq, (const double*)Bf.B, Bf.prior, (double*)nullptr,
                     (long long*)nullptr);
  SBO_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_path_solve, dim3((unsigned)A.S), dim3(1024), 0, st, A, (const double*)Bf.obs.Yn, (const double*)Bf.prior, (const double*)Bf.nz,
                     c->factor.F(), Bf.B);
  SBO_HIP(hipGetLastError());
  return SBO_OK;
}

// evaluate a point list: pts [A.m][d] -> vals, and per (workgroup, path) the arg-best partials where pval / pidx are given
template <int D, int SB>
static int paths_evaluate(sbo_ctx* c, const PathArgs& A, int nwg, long long ntiles, const double* pts, const double* om, const double* ph,
                          const double* As, const double* sq, const double* B, double* vals, double* pval, long long* pidx) {
  hipLaunchKernelGGL((k_path_main<D, SB>), dim3((unsigned)nwg), dim3(kPathThreads), 0, c->stream, A, ntiles, pts, om, ph, As, sq, B, vals, pval, pidx);
  SBO_HIP(hipGetLastError());
  return SBO_OK;
}

static long long path_tiles(long long m) { return (m + kPathTile - 1) / kPathTile; }

int paths_check_draws(const sbo_ctx* c, const PathDraws& dr) {
  const ModelConst& mc = c->mc;
  if (dr.S < 1 || dr.S > SBO_MAX_PATHS) return fail(SBO_E_INVALID, "n_paths must be in [1, SBO_MAX_PATHS]");
  if (dr.F < 1 || dr.F > SBO_MAX_FEATURES) return fail(SBO_E_INVALID, "n_features must be in [1, SBO_MAX_FEATURES]");
  if (dr.output < 0 || dr.output >= mc.q) return fail(SBO_E_INVALID, "output out of range [0, q)");
  if (!all_finite(dr.omega, (size_t)dr.F * mc.d) || !all_finite(dr.phase, (size_t)dr.F) || !all_finite(dr.weights, (size_t)dr.S * dr.F) ||
      !all_finite(dr.noise, (size_t)dr.S * mc.n))
    return fail(SBO_E_INVALID, "omega, phase, weights or noise holds a non-finite entry");
  return SBO_OK;
}

int paths_prepare_list(sbo_ctx* c, PathDraws& dr, long long m, PathImage* img) {
  const ModelConst& mc = c->mc;
  const PathArgs A = path_args(c, dr.output, dr.S, dr.F, 0, m);
  PathBufs Bf;
  int rc;
  if ((rc = carve(c->pathbuf, [&](Carve cv) { return paths_layout(cv, mc, A, true, 0, true, Bf); }, 256))) return rc;
  SBO_HIP(paths_upload(c, A, Bf, dr));
  if ((rc = with_dpad(mc.dpad, [&](auto DD) { return with_spad(A.Spad, [&](auto SB) { return paths_prepare<DD(), SB()>(c, A, Bf); }); }))) return rc;
  hipLaunchKernelGGL(k_path_bt, dim3((unsigned)(((long long)A.S * (A.F + A.n) + 255) / 256)), dim3(256), 0, c->stream, A, (const double*)Bf.B, Bf.Bt);
  SBO_HIP(hipGetLastError());
  *img = PathImage{Bf.Bt, Bf.om, Bf.ph, Bf.B, Bf.obs.As, Bf.obs.sq, Bf.pts, Bf.vals, dr.F, dr.S, dr.output, m};
  return SBO_OK;
}

int paths_eval_list(sbo_ctx* c, const PathImage& img) {
  const PathArgs A = path_args(c, img.output, img.S, img.F, 0, img.m);
  const long long ntiles = path_tiles(img.m);
  const int nwg = (int)std::min<long long>(ntiles, kPathGridTiles);
  return with_dpad(c->mc.dpad, [&](auto DD) {
    return with_spad(A.Spad, [&](auto SB) {
      return paths_evaluate<DD(), SB()>(c, A, nwg, ntiles, img.pts, img.om, img.ph, img.As, img.sq, img.B, img.vals, nullptr, nullptr);
    });
  });
}

}  // namespace sbo

using namespace sbo;

extern "C" int sbo_sample_paths(sbo_ctx* c, const sbo_paths_opts* opts, const double* omega, const double* phase, const double* weights,
                                const double* noise, int64_t m, const double* points, double* values_out, sbo_paths_result* result) {
  if (result) clear_index_value(result->index, result->value);
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (!opts || !omega || !phase || !weights || !noise || !points || !result) return fail(SBO_E_INVALID, "NULL argument");
  if (m < 1 || m > SBO_PATHS_MAX_POINTS) return fail(SBO_E_INVALID, "1 <= m <= SBO_PATHS_MAX_POINTS is required");
  if (opts->n_paths < 1 || opts->n_paths > SBO_MAX_PATHS) return fail(SBO_E_INVALID, "n_paths must be in [1, SBO_MAX_PATHS]");
  if (opts->n_features < 1 || opts->n_features > SBO_MAX_FEATURES) return fail(SBO_E_INVALID, "n_features must be in [1, SBO_MAX_FEATURES]");
  if (opts->maximize != 0 && opts->maximize != 1) return fail(SBO_E_INVALID, "maximize must be 0 or 1");
  int rc;
  if ((rc = model_reader_check(c, "sbo_sample_paths", false))) return rc;        // (d and q, which the checks below need)
  const ModelConst& mc = c->mc;
  const int d = mc.d, S = opts->n_paths;
  PathDraws dr{opts->output, S, opts->n_features, omega, phase, weights, noise, {}};
  if (dr.output < 0 || dr.output >= mc.q) return fail(SBO_E_INVALID, "output out of range [0, q)");
  if (values_out && (unsigned long long)m * (unsigned long long)S * sizeof(double) > SBO_PATHS_MAX_VALUES)
    return fail(SBO_E_UNSUPPORTED, "sbo_sample_paths: values_out needs more than SBO_PATHS_MAX_VALUES bytes");
  if ((rc = paths_check_draws(c, dr))) return rc;
  if (!all_finite(points, (size_t)m * d)) return fail(SBO_E_INVALID, "points holds a non-finite coordinate");
  if ((rc = model_reader_begin(c, "sbo_sample_paths", false))) return rc;
  const PathArgs A = path_args(c, dr.output, S, dr.F, opts->maximize, m);
  const long long ntiles = path_tiles(m);
  const int nwg = (int)std::min<long long>(ntiles, kPathGridTiles);
  PathBufs Bf;
  if ((rc = carve(c->pathbuf, [&](Carve cv) { return paths_layout(cv, mc, A, values_out != nullptr, nwg, false, Bf); }, 256))) return rc;
  if (!values_out) Bf.vals = nullptr;
  hipStream_t st = c->stream;
  hipError_t e = paths_upload(c, A, Bf, dr);
  if (e == hipSuccess) e = hipMemcpyAsync(Bf.pts, points, sizeof(double) * (size_t)m * d, hipMemcpyHostToDevice, st);
  auto enqueue = [&](auto DD) {
    return with_spad(A.Spad, [&](auto SB) {
      if (int r = paths_prepare<DD(), SB()>(c, A, Bf)) return r;
      return paths_evaluate<DD(), SB()>(c, A, nwg, ntiles, Bf.pts, Bf.om, Bf.ph, Bf.obs.As, Bf.obs.sq, Bf.B, Bf.vals, Bf.pval, Bf.pidx);
    });
  };
  rc = e == hipSuccess ? with_dpad(mc.dpad, enqueue) : SBO_OK;
  if (e == hipSuccess && !rc) {
    hipLaunchKernelGGL(k_path_finish, dim3(1), dim3(kMergeThreads), 0, st, A, nwg, (const double*)Bf.pval, (const long long*)Bf.pidx, Bf.res);
    e = hipGetLastError();
  }
  if (e != hipSuccess || rc) {
    (void)hipStreamSynchronize(st);                     // (nothing of the call may still read the caller's arrays or the padded omega)
    SBO_HIP(e);
    return rc;
  }
  // the one read-back (every refusal of the contract lies above: from here on only the runtime itself can fail)
  sbo_paths_result out;
  e = hipMemcpyAsync(&out, Bf.res, sizeof(out), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && values_out) e = hipMemcpyAsync(values_out, Bf.vals, sizeof(double) * (size_t)m * S, hipMemcpyDeviceToHost, st);
  const hipError_t ew = stream_wait(c, st);
  SBO_HIP(e);
  SBO_HIP(ew);
  *result = out;
  return SBO_OK;
}
