// joint.hip -- sbo_posterior_joint: the posterior of a point list as a multivariate normal.
//
// Mean vector, full covariance and exact draws through the covariance's Cholesky factor, for m <= SBO_JOINT_MAX_POINTS points of one
// output.  Normalised units, t_p = M k(X, p) the whitened vectors (M^T M = inv(K + sn2 I), the resident fp64 factor):
//   mu(p) = mp + t_p . (M (y - mp)),   C(p, p') = k(p, p') - t_p . t_p',   A = C + (noise sn2 + jitter sf2) I = L L^T,   f_s = mu + L z_s.
// The images that leave the device are un-normalised, and it is the un-normalised matrix that is factored: cov = Y_std^2 (C + noise
// sn2 I) is formed once per element, A' = cov + Y_std^2 (jitter sf2) I is factored as A' = L' L'^T, and chol_out is L' = Y_std L with no
// scaling behind the factorisation (the factor of a one-point list is then the correctly rounded square root of the entry returned in
// cov_out plus the jitter).  The pivot threshold is relative, so the scale does not enter it.
//   k_obs_prep, k_whiten_resid   (through ObsResident, slab_tiles.hpp) the observations in the output's scaled coordinates and their
//                   squares; the whitened residuals w = M (y - mp)
//   k_joint_stage1  per point: t_p [point][ldt] (zero beyond n), mu, the mean in the caller's units, the scaled coordinates;
//                   whiten_stage1 (slab_tiles.hpp)
//   k_joint_cov     C = Kpp - T T^T in 64 x 64 tiles of the lower triangle on the matrix cores (tile64_product, slab_tiles.hpp, K in
//                   slabs of 32 over ldt); the epilogue takes k(p, p') with the smaller of the two squared norms first -- the expanded
//                   distance is not symmetric in its rounding, the ordered one is --, subtracts the accumulator and stores the element
//                   and its mirror from one register; the matrix to factor gets the same value plus the jitter on its diagonal
//   k_joint_diag    blocked right-looking Cholesky, panels of 64 columns: the diagonal block by one workgroup in LDS, pivots checked
//                   against 2^-40 of their diagonal entry, the relative minimum and its row into the state block
//   k_joint_panel   L21 = A21 L11^-T, a workgroup per block of 64 rows, a row per lane
//   k_joint_update  A22 -= L21 L21^T as lower-triangle tiles on the matrix cores over the whole chip (tile64_product)
//   k_joint_draw    F = L' Z^T per tile of 128 points x Spad draws (tile128_step, slab_tiles.hpp), the slabs above the diagonal skipped;
//                   epilogue (tile128_arg_best): Y_mean + (Y_std mu + acc), stored [m][S] where asked, the arg-best per draw as
//                   workgroup partials
//   k_joint_finish  the partials of the workgroups (partials_merge) and the pivot record -> the result block
//   k_joint_lower   the factor in full, zeros above the diagonal
// Every sum runs in an order fixed by the element's (row, column) and n alone: C(i, j) depends on the two points and the model, rows
// 0 .. r of L on the first r + 1 points, and two calls return the same bits.  No atomics.  One host wait; nothing resident is written.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>
#include "slab_tiles.hpp"

namespace sbo {

constexpr int kJointTile = 64;                   // rows x columns of one workgroup tile of k_joint_cov / k_joint_update; the panel width
constexpr int kJointThreads = 256;               // every kernel of the factorisation and the two products
constexpr int kJointDrawTile = 128;              // points of one workgroup tile of k_joint_draw (4 waves x 32 points)
constexpr double kJointPivotRel = 0x1p-40;       // a pivot must exceed this times its diagonal entry of A
static_assert(kJointTile == 64 && kJointThreads == kTileThreads && kJointTile == 2 * kSlabK, "tile64_product's tile and workgroup; panels of two slabs");
static_assert(kJointDrawTile == kTile128, "k_joint_draw: tile128_step's tile");
static_assert(SBO_MAX_PATHS == 64, "k_joint_draw is instantiated for 16, 32 and 64 padded draws");
static_assert(SBO_JOINT_MAX_POINTS % kJointDrawTile == 0, "the padded order of the images is a multiple of both tiles");

struct JointArgs {                               // by value (kernarg segment)
  int n, d, ld, q;                               // observations, input dimension, leading dimension of the resident factor, outputs
  int ldt, o, S, Spad;                           // leading dimension of t (n rounded up to kSlabK), the output, draws, draws rounded up to 16 | 32 | 64
  int m, lda, maximize, pad;                     // points, leading dimension of the matrix to factor (m rounded up to kJointDrawTile)
  OutParams op;
  double ymean, ystd, ys2;                       // ys2 = Y_std^2
  double dnoise, djit;                           // noise sn2 (normalised, inside cov) and Y_std^2 (jitter sf2) (only in the matrix that is factored)
};

struct JointState {                              // device: the record of the factorisation
  double pmin;                                   // smallest pivot / diagonal entry so far (+inf: none)
  long long prow, bad_row;                       // its row; the first row whose pivot failed (-1: none)
};

struct JointBufs {
  ObsResident obs;
  double *pts, *T, *mu, *mean, *bs, *bsq, *cov, *A, *dg, *rinv, *Lout, *Zt, *draws, *pval;
  long long* pidx;
  JointState* st;
  sbo_joint_result* res;
};

// tile b of the lower triangle in row-major order: (ti, tj), tj <= ti
__device__ __forceinline__ void joint_tile(int b, int& ti, int& tj) {
  ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= b) ++ti;
  tj = b - ti * (ti + 1) / 2;
}

// ---- stage 1: t = M k_p, mu = mp + t . w per point (whiten_stage1, slab_tiles.hpp; one output) -------------------------------------
template <int D>
__global__ __launch_bounds__(kWhitenThreads) void k_joint_stage1(const JointArgs A, int P, const double* __restrict__ As, const double* __restrict__ sq,
                                                                 const double* __restrict__ F, const double* __restrict__ w,
                                                                 const double* __restrict__ pts, double* __restrict__ T, double* __restrict__ mu,
                                                                 double* __restrict__ mean, double* __restrict__ bs, double* __restrict__ bsq_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* sK = reinterpret_cast<double*>(smem);             // [n][P + 1]
  const int n = A.n, ld = A.ld, ldk = P + 1;
  whiten_stage1<D>(sK, P, n, A.op, As, sq, F + (size_t)A.o * ld * ld, ld, pts, A.m, 0, T, A.ldt, bs, bsq_out, [&](size_t rec, long long, int col) {
    double dot = 0.0;
    for (int j = 0; j < n; ++j) dot = fma(sK[j * ldk + col], w[j], dot);
    const double mv = A.op.mp + dot;
    mu[rec] = mv;
    mean[rec] = A.ymean + A.ystd * mv;
  });
}

// ---- C = Kpp - T T^T: the tiles of the lower triangle ----------------------------------------------------------------------------------
// Workgroup b owns tile (ti, tj): rows 64 ti .. + 63 are the A side of tile64_product, columns 64 tj .. + 63 the B side; acc[a][c][t]
// is the element (tile64_row(a, t), tile64_col(c)) of the tile (slab_tiles.hpp).  Rows past m are staged as zeros and never stored.
// Only elements with column <= row are stored, each with its mirror.
template <int D>
__global__ __launch_bounds__(kJointThreads, 2) void k_joint_cov(const JointArgs A, const double* __restrict__ T, const double* __restrict__ bs,
                                                                const double* __restrict__ bsq, double* __restrict__ cov /* [m][m] or null */,
                                                                double* __restrict__ Aw /* [lda][lda] or null */, double* __restrict__ dg) {
  constexpr int LB = D + 1;
  __shared__ __attribute__((aligned(32))) double sA[kJointTile * kSlabK], sB[kJointTile * kSlabK];
  __shared__ double gSq[kJointTile], gB[kJointTile * LB], xSq[kJointTile], xB[kJointTile * LB];
  const int tid = threadIdx.x;
  int ti, tj;
  joint_tile((int)blockIdx.x, ti, tj);
  const int i0 = ti * kJointTile, j0 = tj * kJointTile, m = A.m, ldt = A.ldt;
  if (tid < kJointTile) {
    const bool on = i0 + tid < m;
    point_image<D>(gSq, gB, tid, bsq, bs, (size_t)(on ? i0 + tid : 0), on);
  } else if (tid < 2 * kJointTile) {
    const int c = tid - kJointTile;
    const bool on = j0 + c < m;
    point_image<D>(xSq, xB, c, bsq, bs, (size_t)(on ? j0 + c : 0), on);
  }
  const int srow = tile64_stage_row();
  const bool son = i0 + srow < m, ton = j0 + srow < m;
  d4_t acc[2][2];
  tile64_product(sA, sB, T + (size_t)(son ? i0 + srow : 0) * ldt, son, T + (size_t)(ton ? j0 + srow : 0) * ldt, ton, ldt, acc);
  const double sf2 = A.op.sf2;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int col = tile64_col(c), j = j0 + col;
    double xb[D];
#pragma unroll
    for (int t = 0; t < D; ++t) xb[t] = xB[col * LB + t];
    const double xsq = xSq[col];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int row = tile64_row(a, t), i = i0 + row;
        const double gsq = gSq[row];
        // the smaller squared norm first: the value is that of the pair, whichever of the two is the row
        const double cn = rbf_k<D>(sf2, gB + row * LB, fmin(gsq, xsq), xb, fmax(gsq, xsq)) - acc[a][c][t];
        if (i < m && j <= i) {
          const bool diag = i == j;
          const double cu = A.ys2 * (diag ? cn + A.dnoise : cn);
          if (cov) {
            cov[(size_t)i * m + j] = cu;
            cov[(size_t)j * m + i] = cu;
          }
          if (Aw) {
            const double av = diag ? cu + A.djit : cu;
            Aw[(size_t)i * A.lda + j] = av;
            if (diag) dg[i] = av;
          }
        }
        __builtin_amdgcn_sched_barrier(0);            // (one pair at a time, as k_exp_pairs)
      }
  }
}

// ---- Cholesky: the diagonal block of panel kb ------------------------------------------------------------------------------------------
// One workgroup; the block's lower triangle in LDS, thread (cc, r0) = (tid & 63, tid >> 6) owns column cc of rows r0, r0 + 4, ..  Per
// pivot j: the trailing elements take -(D[i][j] rv) (D[cc][j] rv), rv = 1 / sqrt(pivot), one barrier, then column j is scaled by the
// same products.  Rows past m are zeros and are not pivots.
__global__ __launch_bounds__(kJointThreads) void k_joint_diag(const JointArgs A, int kb, double* __restrict__ Aw, const double* __restrict__ dg,
                                                              double* __restrict__ rinv, JointState* __restrict__ st) {
  __shared__ double Dm[kJointTile][kJointTile + 1];
  __shared__ double sdg[kJointTile], srv[kJointTile];
  const int tid = threadIdx.x, lda = A.lda, kw = min(kJointTile, A.m - kb);
  for (int idx = tid; idx < kJointTile * kJointTile; idx += kJointThreads) {
    const int r = idx >> 6, c = idx & 63;
    Dm[r][c] = (r < kw && c <= r) ? Aw[(size_t)(kb + r) * lda + kb + c] : 0.0;
  }
  if (tid < kJointTile) {
    sdg[tid] = tid < kw ? dg[kb + tid] : 1.0;
    srv[tid] = 1.0;
  }
  __syncthreads();
  const int cc = tid & 63, r0 = tid >> 6;
  double pmin = __builtin_huge_val();
  long long prow = -1, bad = -1;
  for (int j = 0; j < kw; ++j) {
    const double piv = Dm[j][j], dj = sdg[j];
    const bool ok = piv > 0.0 && piv > kJointPivotRel * dj;
    if (tid == 0) {                                   // (the record is thread 0's)
      const double rel = piv / dj;
      if (!ok && bad < 0) bad = kb + j;
      if (ok && rel < pmin) {
        pmin = rel;
        prow = kb + j;
      }
    }
    const double ljj = sqrt_rn(ok ? piv : 1.0), rv = 1.0 / ljj;
    if (cc > j) {
      const double lc = Dm[cc][j] * rv;
#pragma unroll 4
      for (int mm = 0; mm < kJointTile / 4; ++mm) {
        const int i = r0 + 4 * mm;
        if (i >= cc) Dm[i][cc] -= (Dm[i][j] * rv) * lc;
      }
    }
    __syncthreads();                                  // (column j has been read by everybody; the update of column j + 1 is complete)
    if (cc == j) {
#pragma unroll 4
      for (int mm = 0; mm < kJointTile / 4; ++mm) {
        const int i = r0 + 4 * mm;
        if (i > j) Dm[i][j] = Dm[i][j] * rv;
        if (i == j) {
          Dm[j][j] = ljj;
          srv[j] = rv;
        }
      }
    }
  }
  __syncthreads();
  for (int idx = tid; idx < kJointTile * kJointTile; idx += kJointThreads) {
    const int r = idx >> 6, c = idx & 63;
    if (r < kw && c <= r) Aw[(size_t)(kb + r) * lda + kb + c] = Dm[r][c];
  }
  if (tid < kJointTile) rinv[kb + tid] = srv[tid];
  if (tid == 0) {                                     // (the panels run one after the other on one stream: a plain read-modify-write)
    if (bad >= 0 && st->bad_row < 0) st->bad_row = bad;
    if (pmin < st->pmin) {
      st->pmin = pmin;
      st->prow = prow;
    }
  }
}

// ---- Cholesky: L21 = A21 L11^-T, a workgroup per block of 64 rows below the diagonal block -------------------------------------------
// Lane r of wave 0 solves row r: x_c = (a_c - sum_{t < c} x_t L11[c][t]) rv_c, t ascending.  Only full panels have rows below them.
__global__ __launch_bounds__(kJointThreads) void k_joint_panel(const JointArgs A, int kb, double* __restrict__ Aw, const double* __restrict__ rinv) {
  __shared__ double sL[kJointTile * (kJointTile + 1) / 2];      // L11's lower triangle, packed by rows (every lane reads the same entry)
  __shared__ double sX[kJointTile][kJointTile + 1];
  __shared__ double srv[kJointTile];
  const int tid = threadIdx.x, lda = A.lda, m = A.m, r0 = kb + kJointTile * (1 + (int)blockIdx.x);
  for (int idx = tid; idx < kJointTile * kJointTile; idx += kJointThreads) {
    const int r = idx >> 6, c = idx & 63;
    if (c <= r) sL[r * (r + 1) / 2 + c] = Aw[(size_t)(kb + r) * lda + kb + c];
    sX[r][c] = r0 + r < m ? Aw[(size_t)(r0 + r) * lda + kb + c] : 0.0;
  }
  if (tid < kJointTile) srv[tid] = rinv[kb + tid];
  __syncthreads();
  if (tid < kJointTile) {
    const int r = tid;
    for (int c = 0; c < kJointTile; ++c) {
      double s = sX[r][c];
      const double* Lc = sL + c * (c + 1) / 2;
      for (int t = 0; t < c; ++t) s = fma(-sX[r][t], Lc[t], s);
      sX[r][c] = s * srv[c];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < kJointTile * kJointTile; idx += kJointThreads) {
    const int r = idx >> 6, c = idx & 63;
    if (r0 + r < m) Aw[(size_t)(r0 + r) * lda + kb + c] = sX[r][c];
  }
}

// ---- Cholesky: A22 -= L21 L21^T, the tiles of the lower triangle behind panel kb ------------------------------------------------------
// tile64_product as in k_joint_cov; both operands are rows of the panel's 64 columns (two slabs).
__global__ __launch_bounds__(kJointThreads, 2) void k_joint_update(const JointArgs A, int kb, double* __restrict__ Aw) {
  __shared__ __attribute__((aligned(32))) double sA[kJointTile * kSlabK], sB[kJointTile * kSlabK];
  int ti, tj;
  joint_tile((int)blockIdx.x, ti, tj);
  const int base = kb + kJointTile, i0 = base + ti * kJointTile, j0 = base + tj * kJointTile, m = A.m, lda = A.lda;
  const int srow = tile64_stage_row();
  const bool son = i0 + srow < m, ton = j0 + srow < m;
  d4_t acc[2][2];
  tile64_product(sA, sB, Aw + (size_t)(son ? i0 + srow : 0) * lda + kb, son, Aw + (size_t)(ton ? j0 + srow : 0) * lda + kb, ton, kJointTile, acc);
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int j = j0 + tile64_col(c);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = i0 + tile64_row(a, t);
        if (i < m && j <= i) Aw[(size_t)i * lda + j] -= acc[a][c][t];
      }
  }
}

// ---- the draws: F = L Z^T ------------------------------------------------------------------------------------------------------------
// A workgroup owns kJointDrawTile points x all Spad draws (the tile of slab_tiles.hpp: the points are the rows, the draws the columns);
// a thread stages columns tile128_k() .. + 15 of row tile128_row() per slab, zeros right of the diagonal (the image's upper triangle is
// not the factor's).  The slabs from the tile's last row on are skipped.  Zt [lda][Spad]: the caller's z transposed, zeros behind m and S.
template <int SB>
__global__ __launch_bounds__(kJointThreads, 2) void k_joint_draw(const JointArgs A, const double* __restrict__ L, const double* __restrict__ Zt,
                                                                 const double* __restrict__ mu, double* __restrict__ draws /* [m][S] or null */,
                                                                 double* __restrict__ pval, long long* __restrict__ pidx /* [grid][Spad] */) {
  constexpr int SP = 16 * SB;
  __shared__ __attribute__((aligned(32))) Tile128Lds<SB> lds;
  const int m = A.m, gp = tile128_row(), gk = tile128_k();
  const int p0 = (int)blockIdx.x * kJointDrawTile, pr = p0 + gp;
  const bool on = pr < m;
  const double* row = L + (size_t)(on ? pr : 0) * A.lda;
  const int kend = min(p0 + kJointDrawTile, A.lda);
  d4_t acc[2][SB];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < SB; ++c) acc[a][c] = d4_t{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < kend; k0 += kSlabK) {
    double g[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int k = k0 + gk + e;
      g[e] = (on && k <= pr) ? row[k] : 0.0;
    }
    tile128_step(lds, g, Zt + (size_t)k0 * SP, acc);
  }
  long long run_idx = kArgNone;
  double run_val = 0.0;
  tile128_arg_best(lds, acc, p0, m, A.S, A.maximize, draws, [&](long long p, double x) { return A.ymean + (A.ystd * mu[p < m ? p : 0] + x); }, run_val,
                   run_idx);
  tile128_store_partial<SB>(pval, pidx, run_val, run_idx);
}

// ---- the partials of the workgroups and the pivot record -> the result block -----------------------------------------------------------
__global__ __launch_bounds__(kMergeThreads) void k_joint_finish(const JointArgs A, int nwg, const double* __restrict__ pval,
                                                                const long long* __restrict__ pidx, const JointState* __restrict__ st,
                                                                sbo_joint_result* __restrict__ res) {
  if (threadIdx.x == 0) {
    res->pivot_min = st->prow < 0 ? __builtin_nan("") : st->pmin;
    res->pivot_row = st->prow;
  }
  partials_merge(A.S, A.Spad, A.maximize, nwg, pval, pidx, res->index, res->value);
}

// ---- the factor in full: zeros above the diagonal ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kJointThreads) void k_joint_lower(const JointArgs A, const double* __restrict__ L, double* __restrict__ out /* [m][m] */) {
  const long long e = (long long)blockIdx.x * kJointThreads + threadIdx.x;
  if (e >= (long long)A.m * A.m) return;
  const int i = (int)(e / A.m), j = (int)(e - (long long)i * A.m);
  out[e] = j <= i ? L[(size_t)i * A.lda + j] : 0.0;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
template <int D>
static int joint_enqueue(sbo_ctx* c, const JointArgs& A, const JointBufs& B, bool want_cov, bool factorise, bool want_chol, int nwg) {
  hipStream_t st = c->stream;
  const int n = A.n, m = A.m;
  if (int rc = B.obs.prepare<D>(c, st, &A.op, &A.o, 1, A.ldt)) return rc;
  Stage1Launch S1;
  if (int rc = whiten_stage1_launch(k_joint_stage1<D>, "sbo_posterior_joint", n, m, S1)) return rc;
  hipLaunchKernelGGL((k_joint_stage1<D>), dim3(S1.blocks), dim3(kWhitenThreads), S1.lds, st, A, S1.P, (const double*)B.obs.As, (const double*)B.obs.sq,
                     c->factor.F(), (const double*)B.obs.w, (const double*)B.pts, B.T, B.mu, B.mean, B.bs, B.bsq);
  SBO_HIP(hipGetLastError());
  const int nt = (m + kJointTile - 1) / kJointTile;          // tiles of 64 rows that hold a point
  if (want_cov || factorise) {
    hipLaunchKernelGGL((k_joint_cov<D>), dim3((unsigned)(nt * (nt + 1) / 2)), dim3(kJointThreads), 0, st, A, (const double*)B.T, (const double*)B.bs,
                       (const double*)B.bsq, want_cov ? B.cov : nullptr, factorise ? B.A : nullptr, B.dg);
    SBO_HIP(hipGetLastError());
  }
  if (!factorise) return SBO_OK;
  for (int p = 0; p < nt; ++p) {
    const int kb = p * kJointTile, below = nt - p - 1;
    hipLaunchKernelGGL(k_joint_diag, dim3(1), dim3(kJointThreads), 0, st, A, kb, B.A, (const double*)B.dg, B.rinv, B.st);
    SBO_HIP(hipGetLastError());
    if (!below) break;
    hipLaunchKernelGGL(k_joint_panel, dim3((unsigned)below), dim3(kJointThreads), 0, st, A, kb, B.A, (const double*)B.rinv);
    SBO_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_joint_update, dim3((unsigned)(below * (below + 1) / 2)), dim3(kJointThreads), 0, st, A, kb, B.A);
    SBO_HIP(hipGetLastError());
  }
  if (A.S > 0) {
    with_spad(A.Spad, [&](auto SB) {
      hipLaunchKernelGGL((k_joint_draw<SB()>), dim3((unsigned)nwg), dim3(kJointThreads), 0, st, A, (const double*)B.A, (const double*)B.Zt,
                         (const double*)B.mu, B.draws, B.pval, B.pidx);
    });
    SBO_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_joint_finish, dim3(1), dim3(kMergeThreads), 0, st, A, A.S > 0 ? nwg : 0, (const double*)B.pval, (const long long*)B.pidx,
                     (const JointState*)B.st, B.res);
  SBO_HIP(hipGetLastError());
  if (want_chol) {
    hipLaunchKernelGGL(k_joint_lower, dim3((unsigned)(((long long)m * m + kJointThreads - 1) / kJointThreads)), dim3(kJointThreads), 0, st, A,
                       (const double*)B.A, B.Lout);
    SBO_HIP(hipGetLastError());
  }
  return SBO_OK;
}

static void joint_clear(sbo_joint_result* r) {
  if (!r) return;
  clear_index_value(r->index, r->value);
  r->pivot_min = std::numeric_limits<double>::quiet_NaN();
  r->pivot_row = -1;
}

}  // namespace sbo

using namespace sbo;

extern "C" int sbo_posterior_joint(sbo_ctx* c, const sbo_joint_opts* opts, int64_t m64, const double* points, const double* z, double* mean_out,
                                   double* cov_out, double* chol_out, double* draws_out, sbo_joint_result* result) {
  joint_clear(result);
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (!opts || !points || !result) return fail(SBO_E_INVALID, "NULL argument");
  if (m64 < 1) return fail(SBO_E_INVALID, "m >= 1 is required");
  if (opts->n_draws < 0 || opts->n_draws > SBO_MAX_PATHS) return fail(SBO_E_INVALID, "n_draws must be in [0, SBO_MAX_PATHS]");
  if (opts->noise != 0 && opts->noise != 1) return fail(SBO_E_INVALID, "noise must be 0 or 1");
  if (opts->maximize != 0 && opts->maximize != 1) return fail(SBO_E_INVALID, "maximize must be 0 or 1");
  if (!std::isfinite(opts->jitter) || opts->jitter < 0.0) return fail(SBO_E_INVALID, "jitter must be finite and >= 0");
  const int S = opts->n_draws;
  if ((S > 0) != (z != nullptr)) return fail(SBO_E_INVALID, "z must be given exactly when n_draws > 0");
  int rc;
  if ((rc = model_reader_check(c, "sbo_posterior_joint", false))) return rc;     // (d and q, which the checks below need)
  const ModelConst& mc = c->mc;
  const int n = mc.n, d = mc.d, q = mc.q, o = opts->output;
  if (o < 0 || o >= q) return fail(SBO_E_INVALID, "output out of range [0, q)");
  if (m64 > SBO_JOINT_MAX_POINTS) return fail(SBO_E_UNSUPPORTED, "sbo_posterior_joint: more than SBO_JOINT_MAX_POINTS points");
  const int m = (int)m64;
  if (!all_finite(points, (size_t)m * d)) return fail(SBO_E_INVALID, "points holds a non-finite coordinate");
  if (S > 0 && !all_finite(z, (size_t)S * m)) return fail(SBO_E_INVALID, "z holds a non-finite entry");
  if ((rc = model_reader_begin(c, "sbo_posterior_joint", false))) return rc;
  const bool factorise = S > 0 || chol_out, want_cov = cov_out != nullptr, want_chol = chol_out != nullptr, want_draws = draws_out && S > 0;
  JointArgs A{};
  A.n = n;
  A.d = d;
  A.q = q;
  A.ld = c->factor.ld();
  A.ldt = (n + kSlabK - 1) / kSlabK * kSlabK;
  A.o = o;
  A.S = S;
  A.Spad = spad_of(S);
  A.m = m;
  A.lda = (m + kJointDrawTile - 1) / kJointDrawTile * kJointDrawTile;
  A.maximize = opts->maximize;
  A.op = out_params(mc, o);
  A.ymean = mc.Y_mean[o];
  A.ystd = mc.Y_std[o];
  A.ys2 = A.ystd * A.ystd;
  A.dnoise = opts->noise ? A.op.sn2 : 0.0;
  A.djit = A.ys2 * (opts->jitter * A.op.sf2);
  const int nwg = (m + kJointDrawTile - 1) / kJointDrawTile;
  // scratch: X_norm [n][d] | Y_norm [n][q] | scaled observations [n][dpad], their squares, w [ldt] | the points | t [m][ldt] | mu, the
  // mean, |.|^2 [m] and scaled coordinates [m][dpad] | cov [m][m] where asked | where a factor is needed: the matrix [lda][lda], its
  // diagonal and the reciprocal pivots [lda], the factor in full [m][m] where asked, z transposed [lda][Spad], the draws [m][S] where
  // asked, the partials [nwg][Spad] | the state block | the result block
  const int D = mc.dpad;
  const size_t lda = (size_t)A.lda, Sp = (size_t)A.Spad, mm = (size_t)m;
  JointBufs B;
  auto layout = [&](Carve cv) {
    B.obs.take(cv, mc, 1, A.ldt);
    cv.take(B.pts, mm * d);
    cv.take(B.T, mm * A.ldt);
    cv.take(B.mu, mm);
    cv.take(B.mean, mm);
    cv.take(B.bs, mm * D);
    cv.take(B.bsq, mm);
    cv.take(B.cov, want_cov ? mm * mm : 0);
    cv.take(B.A, factorise ? lda * lda : 0);
    cv.take(B.dg, factorise ? lda : 0);
    cv.take(B.rinv, factorise ? lda : 0);
    cv.take(B.Lout, want_chol ? mm * mm : 0);
    cv.take(B.Zt, S > 0 ? lda * Sp : 0);
    cv.take(B.draws, want_draws ? mm * S : 0);
    cv.take(B.pval, S > 0 ? (size_t)nwg * Sp : 0);
    cv.take(B.pidx, S > 0 ? (size_t)nwg * Sp : 0);
    cv.take(B.st, 1);
    cv.take(B.res, 1);
    return cv.off;
  };
  if ((rc = carve(c->jointbuf, layout, 256))) return rc;
  if (!want_draws) B.draws = nullptr;
  hipStream_t st = c->stream;
  // z transposed and padded (the host block is read by the copy before the call returns: it is waited for)
  std::vector<double> zt;
  if (S > 0) {
    zt.assign(lda * Sp, 0.0);
    for (int s = 0; s < S; ++s)
      for (int k = 0; k < m; ++k) zt[(size_t)k * Sp + s] = z[(size_t)s * m + k];
  }
  const JointState init{std::numeric_limits<double>::infinity(), -1, -1};
  sbo_joint_result cleared;
  joint_clear(&cleared);
  sbo_joint_result out = cleared;
  hipError_t e = hipMemcpyAsync(B.st, &init, sizeof(init), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(B.res, &cleared, sizeof(cleared), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = B.obs.upload(c, st);
  if (e == hipSuccess) e = hipMemcpyAsync(B.pts, points, sizeof(double) * mm * d, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && S > 0) e = hipMemcpyAsync(B.Zt, zt.data(), sizeof(double) * lda * Sp, hipMemcpyHostToDevice, st);
  rc = e == hipSuccess ? with_dpad(D, [&](auto DD) { return joint_enqueue<DD()>(c, A, B, want_cov, factorise, want_chol, nwg); }) : SBO_OK;
  if (e != hipSuccess || rc) {
    (void)hipStreamSynchronize(st);                     // (nothing of the call may still read the caller's arrays or `zt`)
    SBO_HIP(e);
    return rc;
  }
  // The one read-back.  Without a factorisation every refusal of the contract lies above and the arrays go straight to the caller.
  // With one, the verdict on the pivots arrives in the same wait and a refused call writes no output array: the arrays are read into
  // blocks of the call's own and handed over behind the verdict.
  JointState state = init;
  std::vector<double> h_mean, h_cov, h_chol, h_draws;
  auto back = [&](double* dst, std::vector<double>& hold, const double* src, size_t count) {
    if (!dst || e != hipSuccess) return;
    if (factorise) hold.resize(count);
    e = hipMemcpyAsync(factorise ? hold.data() : dst, src, sizeof(double) * count, hipMemcpyDeviceToHost, st);
  };
  e = hipMemcpyAsync(&state, B.st, sizeof(state), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && factorise) e = hipMemcpyAsync(&out, B.res, sizeof(out), hipMemcpyDeviceToHost, st);
  back(mean_out, h_mean, B.mean, mm);
  back(cov_out, h_cov, B.cov, mm * mm);
  back(chol_out, h_chol, B.Lout, mm * mm);
  if (want_draws) back(draws_out, h_draws, B.draws, mm * S);
  const hipError_t ew = stream_wait(c, st);
  SBO_HIP(e);
  SBO_HIP(ew);
  if (state.bad_row >= 0)
    return fail(SBO_E_INVALID, "sbo_posterior_joint: the pivot of row " + std::to_string(state.bad_row) +
                                   " is not above 2^-40 of its diagonal entry (a larger jitter or noise = 1 makes the matrix definite)");
  if (factorise) {
    if (mean_out) std::memcpy(mean_out, h_mean.data(), sizeof(double) * mm);
    if (cov_out) std::memcpy(cov_out, h_cov.data(), sizeof(double) * mm * mm);
    if (chol_out) std::memcpy(chol_out, h_chol.data(), sizeof(double) * mm * mm);
    if (want_draws) std::memcpy(draws_out, h_draws.data(), sizeof(double) * mm * S);
  }
  *result = out;
  return SBO_OK;
}
