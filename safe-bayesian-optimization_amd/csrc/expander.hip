// expander.hip -- sbo_expander_gain: expanders by hallucinated optimistic observations (the SafeOpt paper's G_t).
//
// A source g is an expander when, were it measured at its optimistic value ucb_c(g), the GP would certify some target x that is not
// safe today.  One more observation changes the posterior of x by a rank-one step that needs a single number beyond the two points' own
// posteriors, the posterior covariance cov_c(x, g) = k_c(x, g) - t_x . t_g of the whitened vectors t_p = M_c k_c(X, p) (M_c^T M_c =
// inv(K_c + sn2_c I), the resident fp64 factor):
//   s = v_c(g) + sn2_c,   mu' = mu_c(x) + cov b sqrt(max(0, v_c(g))) / s,   v' = v_c(x) - cov^2 / s,
//   z_c(x | g) = mu' - b sqrt(max(0, v')) + Y_mean[c] / Y_std[c],   Z(x | g) = min over the masked constraints of z_c(x | g)
// and per source count = #{x : Z >= 0}, margin = max_x Z, witness = its index (lowest on a tie).
//   k_obs_prep, k_whiten_resid   (through ObsResident, slab_tiles.hpp) the observations in the scaled coordinates of every masked constraint
//                 and the whitened residuals w = M_c (y_c - mp_c): mu_c(p) = mp_c + k_c(X, p) . alpha_c = mp_c + t_p . w
//   k_exp_stage1  per (constraint, point): t_p [point][ldt] (zero beyond n), mu, v and the point's scaled coordinates; whiten_stage1
//                 (slab_tiles.hpp) on a padded LDS image, O((ms + mt) n^2) on the vector units
//   k_exp_pairs   the hot path, O(ms mt n) per constraint on the matrix cores: a workgroup owns a 64 x 64 (source x target) tile, a wave
//                 32 x 32 of it as 2 x 2 accumulators of MM<double> (v_mfma_f64_4x4x4, four per step); per constraint tile64_product
//                 (slab_tiles.hpp) runs over LDS-staged slabs of t, the epilogue turns t_x . t_g into z_c and keeps the running Z in registers; behind the last
//                 constraint a count and an arg-best per source row; the target tiles are split over the grid, one partial per
//                 (split, source).  No [ms][mt] array exists.
//   k_exp_finish  per source: the counts summed and the arg-best taken over the splits in order
// Sums over the observations run in a fixed order that depends on n alone, (value, index) reductions are arg_take's total order, there
// are no atomics: two calls return the same bits.  One read-back, one host wait; nothing resident is written.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include "slab_tiles.hpp"

namespace sbo {

constexpr int kExpTile = 64;                     // sources x targets of one workgroup tile of k_exp_pairs (2 x 2 waves of 32 x 32)
constexpr int kExpThreads = 256;                 // k_exp_pairs / k_exp_finish
constexpr int kExpGridTiles = 1024;              // workgroups k_exp_pairs aims at: target splits = min(target tiles, kExpGridTiles / source tiles)
static_assert(kExpTile == 64 && kExpThreads == kTileThreads, "k_exp_pairs: tile64_product's tile and workgroup");

struct ExpArgs {                                 // by value (kernarg segment)
  int n, d, ld, pad0;                            // observations, input dimension, leading dimension of the resident factor
  int ldt, nc, q, pad;                           // leading dimension of t (n rounded up to kSlabK), masked constraints, outputs of the model
  long long ms, mt;
  int out[kMaxQ];                                // [slot]: the output a masked constraint is
  OutParams op[kMaxQ];                           // [slot]
  double shift[kMaxQ];                           // [slot]: Y_mean / Y_std
  double b;
};

struct ExpState {                                // device: the verdict of stage 1
  int bad, pad;                                  // some source has s = v + sn2 <= 0 on some constraint
};

struct ExpBufs {
  ObsResident obs;
  double *pts, *T, *mu, *v, *bs, *bsq, *pval, *margin;
  long long *pcount, *pidx, *count, *witness;
  ExpState* st;
};

// ---- stage 1: t = M k_p, mu = mp + t . w, v = sf2 - ||t||^2 per (slot, point) ---------------------------------------------------
// whiten_stage1 (slab_tiles.hpp) over the list sources | targets; this kernel's own: one thread per point adds the squares and the products
// with w in row order.
template <int D>
__global__ __launch_bounds__(kWhitenThreads) void k_exp_stage1(const ExpArgs A, int P, const double* __restrict__ As, const double* __restrict__ sq,
                                                               const double* __restrict__ F, const double* __restrict__ w,
                                                               const double* __restrict__ pts, double* __restrict__ T, double* __restrict__ mu,
                                                               double* __restrict__ v, double* __restrict__ bs, double* __restrict__ bsq_out,
                                                               ExpState* __restrict__ st) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* sK = reinterpret_cast<double*>(smem);             // [n][P + 1]
  const int n = A.n, ld = A.ld, slot = blockIdx.y, o = A.out[slot], ldk = P + 1;
  const OutParams& op = A.op[slot];
  const long long m = A.ms + A.mt;
  const double* wo = w + (size_t)slot * A.ldt;
  whiten_stage1<D>(sK, P, n, op, As + (size_t)slot * n * D, sq + (size_t)slot * n, F + (size_t)o * ld * ld, ld, pts, m, (size_t)slot * m, T, A.ldt, bs,
                   bsq_out, [&](size_t rec, long long i, int col) {
                     double s = 0.0, dot = 0.0;
                     for (int j = 0; j < n; ++j) {
                       const double t = sK[j * ldk + col];
                       s += t * t;
                       dot = fma(t, wo[j], dot);
                     }
                     const double vv = op.sf2 - s;
                     v[rec] = vv;
                     mu[rec] = op.mp + dot;
                     if (i < A.ms && !(vv + op.sn2 > 0.0)) st->bad = 1;      // (every writer stores the same value)
                   });
}

// ---- stage 2: the pair tiles ----------------------------------------------------------------------------------------------------------
// Workgroup (bx, by): source tile bx, target tiles by, by + nsplit, ..  Wave w owns sources 32 (w >> 1) .. + 31 and targets 32 (w & 1) ..
// + 31 of the tile: acc[a][c][t] is the pair (source tile64_row(a, t), target tile64_col(c)) (slab_tiles.hpp); the sources are the A
// side of tile64_product, the targets the B side.  Rows past ms / mt are staged as zeros and never counted.
template <int D>
__global__ __launch_bounds__(kExpThreads, 2) void k_exp_pairs(const ExpArgs A, int nsplit, long long ntt, const double* __restrict__ T,
                                                           const double* __restrict__ mu, const double* __restrict__ v,
                                                           const double* __restrict__ bs, const double* __restrict__ bsq,
                                                           long long* __restrict__ pcount, double* __restrict__ pval, long long* __restrict__ pidx) {
  constexpr int LB = D + 1;                              // leading dimension of the coordinate images (targets are read 16 rows at a time)
  __shared__ __attribute__((aligned(32))) double sA[kExpTile * kSlabK], sB[kExpTile * kSlabK];
  __shared__ double gS[kExpTile], gCoef[kExpTile], gSq[kExpTile], gB[kExpTile * LB];      // sources: s, b sqrt(max(0, v)) / s, |.|^2, coordinates
  __shared__ double xMu[kExpTile], xV[kExpTile], xSq[kExpTile], xB[kExpTile * LB];        // targets
  __shared__ long long rCnt[4][32], rIdx[4][32];
  __shared__ double rVal[4][32];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long m = A.ms + A.mt, g0 = (long long)blockIdx.x * kExpTile;
  const int ldt = A.ldt, srow = tile64_stage_row();       // staging: this thread's point of the tile
  long long run_cnt = 0, run_idx = kArgNone;              // threads 0 .. 63: source g0 + tid over this workgroup's target tiles
  double run_val = 0.0;
  for (long long tt = blockIdx.y; tt < ntt; tt += nsplit) {
    const long long x0 = tt * kExpTile;
    double Z[2][2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int t = 0; t < 4; ++t) Z[a][c][t] = __builtin_huge_val();
    for (int slot = 0; slot < A.nc; ++slot) {
      const size_t base = (size_t)slot * m;
      __syncthreads();                                    // (the epilogue before this one has read the point images)
      if (tid < kExpTile) {
        const bool on = g0 + tid < A.ms;
        const size_t rec = base + (size_t)(on ? g0 + tid : 0);
        const double vg = on ? v[rec] : 0.0, s = on ? vg + A.op[slot].sn2 : 1.0;
        gS[tid] = s;
        gCoef[tid] = on ? A.b * sqrt(fmax(0.0, vg)) / s : 0.0;
        point_image<D>(gSq, gB, tid, bsq, bs, rec, on);
      } else if (tid < 2 * kExpTile) {
        const int c = tid - kExpTile;
        const bool on = x0 + c < A.mt;
        const size_t rec = base + (size_t)A.ms + (size_t)(on ? x0 + c : 0);
        xMu[c] = on ? mu[rec] : 0.0;
        xV[c] = on ? v[rec] : 0.0;
        point_image<D>(xSq, xB, c, bsq, bs, rec, on);
      }
      d4_t acc[2][2];
      const bool son = g0 + srow < A.ms, ton = x0 + srow < A.mt;
      tile64_product(sA, sB, T + (base + (size_t)(son ? g0 + srow : 0)) * ldt, son,
                     T + (base + (size_t)A.ms + (size_t)(ton ? x0 + srow : 0)) * ldt, ton, ldt, acc);
      // epilogue of this constraint: t_x . t_g -> z_c(x | g), the running minimum (a NaN stays)
      const double sf2 = A.op[slot].sf2, shift = A.shift[slot], bb = A.b;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int col = tile64_col(c);
        double xb[D];
#pragma unroll
        for (int t = 0; t < D; ++t) xb[t] = xB[col * LB + t];
        const double xsq = xSq[col], xmu = xMu[col], xv = xV[col];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int row = tile64_row(a, t);
            const double cov = rbf_k<D>(sf2, gB + row * LB, gSq[row], xb, xsq) - acc[a][c][t];
            const double m1 = xmu + cov * gCoef[row], v1 = xv - cov * cov / gS[row];
            const double z = (m1 - bb * sqrt(fmax(0.0, v1))) + shift;
            const double zo = Z[a][c][t];
            Z[a][c][t] = (z < zo || z != z) ? z : zo;
            __builtin_amdgcn_sched_barrier(0);            // (one pair at a time: sixteen interleaved exp chains cost a hundred registers)
          }
      }
    }
    // per source row of the tile: the count and the arg-best over this tile's targets
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        long long cnt = 0, bk = kArgNone;
        double bv = 0.0;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const long long x = x0 + tile64_col(c);
          const double z = Z[a][c][t];
          const bool on = x < A.mt;
          cnt += (on && z >= 0.0) ? 1 : 0;
          arg_take(bv, bk, z, (on && z == z) ? x : kArgNone);      // (a NaN is never taken)
        }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
          cnt += __shfl_xor(cnt, off);
          const double ov = __shfl_xor(bv, off);
          const long long ok = __shfl_xor(bk, off);
          arg_take(bv, bk, ov, ok);
        }
        if ((lane & 15) == 0) {
          const int row = tile64_row(a, t) & 31;           // of the wave's 32 sources
          rCnt[w][row] = cnt;
          rVal[w][row] = bv;
          rIdx[w][row] = bk;
        }
      }
    __syncthreads();
    if (tid < kExpTile) {                                  // the two waves of a source row, lower targets first
      const int wa = (tid >> 5) * 2, row = tid & 31;
      run_cnt += rCnt[wa][row] + rCnt[wa + 1][row];
      arg_take(run_val, run_idx, rVal[wa][row], rIdx[wa][row]);
      arg_take(run_val, run_idx, rVal[wa + 1][row], rIdx[wa + 1][row]);
    }
  }
  if (tid < kExpTile && g0 + tid < A.ms) {
    const size_t e = (size_t)blockIdx.y * (size_t)A.ms + (size_t)(g0 + tid);
    pcount[e] = run_cnt;
    pval[e] = run_val;
    pidx[e] = run_idx;
  }
}

// ---- per source: the splits in order ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kExpThreads) void k_exp_finish(long long ms, int nsplit, const long long* __restrict__ pcount,
                                                            const double* __restrict__ pval, const long long* __restrict__ pidx,
                                                            long long* __restrict__ count, double* __restrict__ margin, long long* __restrict__ witness) {
  const long long g = (long long)blockIdx.x * kExpThreads + threadIdx.x;
  if (g >= ms) return;
  long long cnt = 0, bk = kArgNone;
  double bv = 0.0;
  for (int s = 0; s < nsplit; ++s) {
    const size_t e = (size_t)s * (size_t)ms + (size_t)g;
    cnt += pcount[e];
    arg_take(bv, bk, pval[e], pidx[e]);
  }
  count[g] = cnt;
  margin[g] = bk == kArgNone ? __builtin_nan("") : bv;
  witness[g] = bk == kArgNone ? -1 : bk;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
template <int D>
static int expander_enqueue(sbo_ctx* c, const ExpArgs& A, const ExpBufs& B, int nsplit, long long ntt) {
  hipStream_t st = c->stream;
  const int n = A.n;
  const long long m = A.ms + A.mt;
  if (int rc = B.obs.prepare<D>(c, st, A.op, A.out, A.nc, A.ldt)) return rc;
  Stage1Launch S1;
  if (int rc = whiten_stage1_launch(k_exp_stage1<D>, "sbo_expander_gain", n, m, S1)) return rc;
  hipLaunchKernelGGL((k_exp_stage1<D>), dim3(S1.blocks, (unsigned)A.nc), dim3(kWhitenThreads), S1.lds, st, A, S1.P, (const double*)B.obs.As,
                     (const double*)B.obs.sq, c->factor.F(), (const double*)B.obs.w, (const double*)B.pts, B.T, B.mu, B.v, B.bs, B.bsq, B.st);
  SBO_HIP(hipGetLastError());
  const long long nst = (A.ms + kExpTile - 1) / kExpTile;
  hipLaunchKernelGGL((k_exp_pairs<D>), dim3((unsigned)nst, (unsigned)nsplit), dim3(kExpThreads), 0, st, A, nsplit, ntt, (const double*)B.T,
                     (const double*)B.mu, (const double*)B.v, (const double*)B.bs, (const double*)B.bsq, B.pcount, B.pval, B.pidx);
  SBO_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_exp_finish, dim3((unsigned)((A.ms + kExpThreads - 1) / kExpThreads)), dim3(kExpThreads), 0, st, A.ms, nsplit,
                     (const long long*)B.pcount, (const double*)B.pval, (const long long*)B.pidx, B.count, B.margin, B.witness);
  SBO_HIP(hipGetLastError());
  return SBO_OK;
}

static void expander_clear(int64_t ms, int64_t* count, double* margin, int64_t* witness) {
  for (int64_t g = 0; g < ms; ++g) {
    if (count) count[g] = 0;
    if (margin) margin[g] = std::numeric_limits<double>::quiet_NaN();
    if (witness) witness[g] = -1;
  }
}

}  // namespace sbo

using namespace sbo;

extern "C" int sbo_expander_gain(sbo_ctx* c, const sbo_expander_opts* opts, int64_t ms, const double* sources, int64_t mt,
                                 const double* targets, int64_t* count_out, double* margin_out, int64_t* witness_out) {
  expander_clear(ms, count_out, margin_out, witness_out);
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (!opts || !sources || !targets || !count_out) return fail(SBO_E_INVALID, "NULL argument");
  if (ms < 1 || mt < 1) return fail(SBO_E_INVALID, "ms >= 1 and mt >= 1 are required");
  if (!std::isfinite(opts->b) || opts->b < 0.0) return fail(SBO_E_INVALID, "b must be finite and >= 0");
  int rc;
  if ((rc = model_reader_check(c, "sbo_expander_gain", false))) return rc;       // (d and q, which the checks below need)
  const ModelConst& mc = c->mc;
  const int n = mc.n, d = mc.d, q = mc.q;
  if (q < 2) return fail(SBO_E_INVALID, "sbo_expander_gain needs a model with a constraint (q >= 2)");
  const uint32_t all = ((q >= 32 ? 0u : (1u << q)) - 1u) & ~1u;                    // bits 1 .. q - 1
  if (opts->constraint_mask & ~all) return fail(SBO_E_INVALID, "constraint_mask names bit 0 or a bit at or above q");
  const uint32_t mask = opts->constraint_mask ? opts->constraint_mask : all;
  if (ms > SBO_EXPANDER_MAX_POINTS || mt > SBO_EXPANDER_MAX_POINTS)
    return fail(SBO_E_UNSUPPORTED, "sbo_expander_gain: more than SBO_EXPANDER_MAX_POINTS sources or targets");
  ExpArgs A{};
  A.n = n;
  A.d = d;
  A.q = q;
  A.ldt = (n + kSlabK - 1) / kSlabK * kSlabK;
  A.ms = ms;
  A.mt = mt;
  A.b = opts->b;
  for (int o = 1; o < q; ++o)
    if (mask >> o & 1u) {
      const int s = A.nc++;
      A.out[s] = o;
      A.op[s] = out_params(mc, o);
      A.shift[s] = mc.Y_mean[o] / mc.Y_std[o];
    }
  const size_t m = (size_t)ms + (size_t)mt;
  if (m * (size_t)A.ldt * (size_t)A.nc * sizeof(double) > SBO_EXPANDER_MAX_SCRATCH)
    return fail(SBO_E_UNSUPPORTED, "sbo_expander_gain: the whitened vectors need more than SBO_EXPANDER_MAX_SCRATCH bytes");
  if (!all_finite(sources, (size_t)ms * d)) return fail(SBO_E_INVALID, "sources holds a non-finite coordinate");
  if (!all_finite(targets, (size_t)mt * d)) return fail(SBO_E_INVALID, "targets holds a non-finite coordinate");
  if ((rc = model_reader_begin(c, "sbo_expander_gain", false))) return rc;
  A.ld = c->factor.ld();
  const long long ntt = ((long long)mt + kExpTile - 1) / kExpTile, nst = ((long long)ms + kExpTile - 1) / kExpTile;
  const int nsplit = (int)std::min<long long>(ntt, std::max<long long>(1, kExpGridTiles / nst));
  // scratch: X_norm [n][d] | Y_norm [n][q] | scaled observations [nc][n][dpad], their squares, w [nc][ldt] | the points, sources first | t [nc][ms + mt][ldt] |
  // mu, v, |.|^2 [nc][ms + mt] and scaled coordinates [nc][ms + mt][dpad] | the partials [nsplit][ms] | the results [ms] | the state block
  const int D = mc.dpad;
  const size_t nc = (size_t)A.nc;
  ExpBufs B;
  auto layout = [&](Carve cv) {
    B.obs.take(cv, mc, nc, A.ldt);
    cv.take(B.pts, m * d);
    cv.take(B.T, nc * m * A.ldt);
    cv.take(B.mu, nc * m);
    cv.take(B.v, nc * m);
    cv.take(B.bs, nc * m * D);
    cv.take(B.bsq, nc * m);
    cv.take(B.pcount, (size_t)nsplit * ms);
    cv.take(B.pval, (size_t)nsplit * ms);
    cv.take(B.pidx, (size_t)nsplit * ms);
    cv.take(B.count, (size_t)ms);
    cv.take(B.margin, (size_t)ms);
    cv.take(B.witness, (size_t)ms);
    cv.take(B.st, 1);
    return cv.off;
  };
  if ((rc = carve(c->expbuf, layout, 256))) return rc;
  hipStream_t st = c->stream;
  const ExpState init{};
  SBO_HIP(hipMemcpyAsync(B.st, &init, sizeof(init), hipMemcpyHostToDevice, st));
  SBO_HIP(B.obs.upload(c, st));
  SBO_HIP(hipMemcpyAsync(B.pts, sources, sizeof(double) * (size_t)ms * d, hipMemcpyHostToDevice, st));
  SBO_HIP(hipMemcpyAsync(B.pts + (size_t)ms * d, targets, sizeof(double) * (size_t)mt * d, hipMemcpyHostToDevice, st));
  rc = with_dpad(D, [&](auto DD) { return expander_enqueue<DD()>(c, A, B, nsplit, ntt); });
  if (rc) {
    (void)hipStreamSynchronize(st);                     // (nothing of the call may still read the caller's arrays)
    return rc;
  }
  static_assert(sizeof(long long) == sizeof(int64_t), "the results are copied out as they are");
  ExpState out;
  hipError_t e = hipMemcpyAsync(&out, B.st, sizeof(out), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(count_out, B.count, sizeof(int64_t) * (size_t)ms, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && margin_out) e = hipMemcpyAsync(margin_out, B.margin, sizeof(double) * (size_t)ms, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && witness_out) e = hipMemcpyAsync(witness_out, B.witness, sizeof(int64_t) * (size_t)ms, hipMemcpyDeviceToHost, st);
  const hipError_t ew = stream_wait(c, st);
  if (e != hipSuccess || ew != hipSuccess || out.bad) expander_clear(ms, count_out, margin_out, witness_out);
  SBO_HIP(e);
  SBO_HIP(ew);
  if (out.bad) return fail(SBO_E_INVALID, "a source has s = v + sn2 <= 0 on a masked constraint");
  return SBO_OK;
}
