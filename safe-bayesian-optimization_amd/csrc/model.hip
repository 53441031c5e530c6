// model.hip -- SURVEY.md section 8(f) rank 1 (model build): the per-model factorisation on the device.
//
// What models/GP_Safe.py:229-245 leaves in `inference_datasets` is invK (or, when the caller passes none, the
// hyper-parameters to build K = sf2 exp(-1/2 D) + (sn2 + float32 eps) I from).  The sweep kernels contract with a
// LOWER-triangular M, M^T M = invK (K1g / K1c / K1, and the table build of K1b), and the mean uses
// alpha = invK (Y_norm - mp).  Here, one workgroup per output:
//   invK given : alpha = invK rhs with the matrix exactly as passed; M from the "UL" factorisation of the symmetrised
//                invK: reverse both index orders, factor J invK J = U~^T U~ (U~ upper), M = J U~ J.
//   invK absent: K from the expanded distance (models/GP_Safe.py:119), K = U^T U, M = L^-1 = U^-T by row-wise
//                substitution, alpha = M^T (M rhs).
// The factor is then packed into the matrix-core fragment images every K1 kernel reads (Fpk).  Small models (n < kBlockedFrom =
// 96) run in one workgroup per output; from there on the blocked multi-workgroup form below is used (n = 512: 1.4 ms, n = 2048:
// 9 ms per model, against ~95 ms / seconds of host Cholesky).
#include <cmath>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>
#include "device_common.hpp"

namespace sbo {

// In-place K = U^T U on the upper triangle of a row-major n x n matrix, one workgroup (the loop of fit.hip without the
// right-hand side).  `bad` is set when a pivot is not positive.  With E != nullptr (zero-initialised, row-major) the
// identity rides along as n extra right-hand sides, exactly as y does in fit.hip, and E ends up as L^-1 (L = U^T).
__device__ void factor_utu(double* __restrict__ U, int n, int* bad, double* sh_piv, double* __restrict__ E = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  for (int j = 0; j < n; ++j) {
    if (tid == 0) {
      const double piv = U[(size_t)j * n + j];
      if (!(piv > 0.0)) *bad = 1;
      *sh_piv = piv > 0.0 ? sqrt(piv) : 1.0;
    }
    __syncthreads();
    const double ljj = *sh_piv;
    double* uj = U + (size_t)j * n;
    for (int i = j + 1 + tid; i < n; i += blockDim.x) uj[i] /= ljj;
    if (tid == 0) uj[j] = ljj;
    double* ej = E ? E + (size_t)j * n : nullptr;
    if (E) {
      for (int cidx = tid; cidx < j; cidx += blockDim.x) ej[cidx] /= ljj;
      if (tid == 0) ej[j] = 1.0 / ljj;
    }
    __syncthreads();
    // trailing update, row k from column k on; a wave keeps two rows in flight (the loop is bound by memory latency)
    for (int k = j + 1 + wave; k < n; k += 2 * nw) {
      const int k2 = k + nw;
      const double f = uj[k];
      double* uk = U + (size_t)k * n;
      if (k2 < n) {
        const double f2 = uj[k2];
        double* uk2 = U + (size_t)k2 * n;
        for (int i = k + lane; i < n; i += 64) {
          const double v = uj[i];
          uk[i] -= f * v;
          if (i >= k2) uk2[i] -= f2 * v;
        }
      } else {
        for (int i = k + lane; i < n; i += 64) uk[i] -= f * uj[i];
      }
      if (E) {                                  // rows k (and k2) of the inverse, columns 0..j
        double* ek = E + (size_t)k * n;
        for (int cidx = lane; cidx <= j; cidx += 64) ek[cidx] -= f * ej[cidx];
        if (k2 < n) {
          const double f2 = uj[k2];
          double* ek2 = E + (size_t)k2 * n;
          for (int cidx = lane; cidx <= j; cidx += 64) ek2[cidx] -= f2 * ej[cidx];
        }
      }
    }
    __syncthreads();
  }
}

// mode 0: W = invK [q][n][n] given.  mode 1: build K from As / sqA.  Outputs: F [q][n][n] lower triangle (row-major),
// alpha [q][npad], bad[q].  `work` [q][n][n] scratch.
__global__ __launch_bounds__(1024) void k_model_build(int mode, int n, int npad, int dpad, int d, const double* __restrict__ W,
                                                     const double* __restrict__ As, const double* __restrict__ sqA,
                                                     const double* __restrict__ rhs, const ModelConst mc, double* __restrict__ work,
                                                     double* __restrict__ F, double* __restrict__ alpha, int* __restrict__ bad) {
  __shared__ double sh_piv;
  __shared__ int sh_bad;
  const int o = blockIdx.x, tid = threadIdx.x;
  double* U = work + (size_t)o * n * n;
  double* Fo = F + (size_t)o * n * n;
  const double* r = rhs + (size_t)o * n;
  if (tid == 0) sh_bad = 0;
  __syncthreads();
  if (mode == 0) {
    const double* Wo = W + (size_t)o * n * n;
    // alpha straight from the caller's inverse (GP_Safe.py:342)
    for (int i = tid; i < n; i += blockDim.x) {
      double s = 0.0;
      for (int j = 0; j < n; ++j) s += Wo[(size_t)i * n + j] * r[j];
      alpha[(size_t)o * npad + i] = s;
    }
    // reversed, symmetrised copy (upper triangle)
    for (long long idx = tid; idx < (long long)n * n; idx += blockDim.x) {
      const int i = (int)(idx / n), k = (int)(idx % n);
      if (k < i) continue;
      const int ri = n - 1 - i, rk = n - 1 - k;
      U[idx] = 0.5 * (Wo[(size_t)ri * n + rk] + Wo[(size_t)rk * n + ri]);
    }
    __syncthreads();
    factor_utu(U, n, &sh_bad, &sh_piv);
    // M = J U~ J  (lower triangular):  M[i][j] = U~[n-1-i][n-1-j], j <= i
    for (long long idx = tid; idx < (long long)n * n; idx += blockDim.x) {
      const int i = (int)(idx / n), j = (int)(idx % n);
      Fo[idx] = j <= i ? U[(size_t)(n - 1 - i) * n + (n - 1 - j)] : 0.0;
    }
  } else {
    const double sf2 = mc.sf2[o], sn2 = mc.sn2[o];
    const double* Ao = As + (size_t)o * npad * dpad;
    const double* so = sqA + (size_t)o * npad;
    // K[i][k] = sf2 exp(-1/2 dist(i, k)) + sn2 [i == k], dist as GP_Safe.py:119 evaluates it; the lower element (i >= k)
    // is the one a lower Cholesky reads, stored here at the transposed (upper) position
    for (long long idx = tid; idx < (long long)n * n; idx += blockDim.x) {
      const int k = (int)(idx / n), i = (int)(idx % n);      // upper position (k, i), k <= i
      if (i < k) continue;
      double dot = 0.0;
      for (int a = 0; a < d; ++a) dot += Ao[(size_t)i * dpad + a] * Ao[(size_t)k * dpad + a];
      const double dist = (-2.0 * dot + so[i]) + so[k];
      U[idx] = sf2 * exp(-0.5 * dist) + (i == k ? sn2 : 0.0);
    }
    for (long long idx = tid; idx < (long long)n * n; idx += blockDim.x) Fo[idx] = 0.0;
    __syncthreads();
    factor_utu(U, n, &sh_bad, &sh_piv, Fo);       // Fo = L^-1 = M
    // alpha = M^T (M rhs)
    double* t = U;                                            // scratch: the factor is no longer needed
    for (int i = tid; i < n; i += blockDim.x) {
      double s = 0.0;
      for (int j = 0; j <= i; ++j) s += Fo[(size_t)i * n + j] * r[j];
      t[i] = s;
    }
    __syncthreads();
    for (int j = tid; j < n; j += blockDim.x) {
      double s = 0.0;
      for (int i = j; i < n; ++i) s += Fo[(size_t)i * n + j] * t[i];
      alpha[(size_t)o * npad + j] = s;
    }
  }
  __syncthreads();
  if (tid == 0) bad[o] = sh_bad;
}

// ---- blocked, multi-workgroup form of the same factorisation (n >= kBlockedFrom) ---------------------------------------------
// Right-looking U^T U with panels of kPB rows; per panel two kinds of launches, every output (blockIdx.y) at once:
//   k_chol_panel : every workgroup factors the kPB x kPB diagonal block in LDS (redundantly: it is tiny), then applies
//                  Ukk^-T to its share of the columns to the right (the panel rows of U) and, with E, to the columns of
//                  the inverse companion left of and inside the panel (E = L^-1 rides along exactly as in factor_utu);
//   k_chol_update: rank-kPB update of the trailing matrix (upper triangle) and of the trailing rows of E, tiled 32 x 32.
constexpr int kPB = 32;

__device__ __forceinline__ double readlane_f64(double v, int l) {      // l: wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}
constexpr int kBlockedFrom = 96;   // smallest n factorised by the blocked form (below: one workgroup does everything)

// mode 0 front end, coalesced (the all-in-one k_chol_prep below reads invK by columns: 133 us at n = 512):
//   k_invk_alpha: alpha = invK rhs with the caller's matrix as given (GP_Safe.py:342), one wave per row;
//   k_invk_reverse: U = upper triangle of J sym(invK) J in 32 x 32 tiles, the transposed partner of a tile through LDS
__global__ __launch_bounds__(256) void k_invk_alpha(int n, int npad, const double* __restrict__ W, const double* __restrict__ rhs,
                                                    double* __restrict__ alpha) {
  const int o = blockIdx.y, lane = threadIdx.x & 63;
  const double* Wo = W + (size_t)o * n * n;
  const double* r = rhs + (size_t)o * n;
  for (int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += (gridDim.x * blockDim.x) >> 6) {
    double s = 0.0;
    for (int j = lane; j < n; j += 64) s += Wo[(size_t)i * n + j] * r[j];
    s = wave_sum(s);
    if (lane == 0) alpha[(size_t)o * npad + i] = s;
  }
}
__global__ __launch_bounds__(256) void k_invk_reverse(int n, const double* __restrict__ W, double* __restrict__ work) {
  __shared__ double Ta[32][33], Tb[32][33];
  const int o = blockIdx.z, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const double* Wo = W + (size_t)o * n * n;
  double* U = work + (size_t)o * n * n;
  const int i0 = blockIdx.y * 32, k0 = blockIdx.x * 32;
  if (k0 + 31 < i0) {                                   // tile entirely below the diagonal: zeros
    for (int rr = ty; rr < 32; rr += 8)
      if (i0 + rr < n && k0 + tx < n) U[(size_t)(i0 + rr) * n + k0 + tx] = 0.0;
    return;
  }
  // element (i, k) of the tile needs W[n-1-i][n-1-k] and W[n-1-k][n-1-i]: the blocks W[R..][C..] and W[C..][R..] with
  // R = n-1-i0-31, C = n-1-k0-31 (rows / columns clipped at 0), read row-wise
  const int R = n - 1 - i0 - 31, Cc = n - 1 - k0 - 31;
  for (int rr = ty; rr < 32; rr += 8) {
    const int ra = R + rr, ca = Cc + tx;
    Ta[rr][tx] = (ra >= 0 && ra < n && ca >= 0 && ca < n) ? Wo[(size_t)ra * n + ca] : 0.0;
    const int rb = Cc + rr, cb = R + tx;
    Tb[rr][tx] = (rb >= 0 && rb < n && cb >= 0 && cb < n) ? Wo[(size_t)rb * n + cb] : 0.0;
  }
  __syncthreads();
  for (int rr = ty; rr < 32; rr += 8) {
    const int i = i0 + rr, k = k0 + tx;
    if (i < n && k < n) {
      // W[n-1-i][n-1-k] = Ta[31 - rr][31 - tx];  W[n-1-k][n-1-i] = Tb[31 - tx][31 - rr]
      U[(size_t)i * n + k] = k >= i ? 0.5 * (Ta[31 - rr][31 - tx] + Tb[31 - tx][31 - rr]) : 0.0;
    }
  }
}

__global__ __launch_bounds__(256) void k_chol_prep(int mode, int n, int npad, int dpad, int d, const double* __restrict__ W,
                                                   const double* __restrict__ As, const double* __restrict__ sqA,
                                                   const double* __restrict__ rhs, const ModelConst mc, double* __restrict__ work,
                                                   double* __restrict__ F, double* __restrict__ alpha) {
  const int o = blockIdx.y;
  double* U = work + (size_t)o * n * n;
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x, gstride = (long long)gridDim.x * blockDim.x;
  if (mode == 0) {
    const double* Wo = W + (size_t)o * n * n;
    const double* r = rhs + (size_t)o * n;
    for (long long i = gid; i < n; i += gstride) {                       // alpha from the caller's inverse as given
      double s = 0.0;
      for (int j = 0; j < n; ++j) s += Wo[(size_t)i * n + j] * r[j];
      alpha[(size_t)o * npad + i] = s;
    }
    for (long long idx = gid; idx < (long long)n * n; idx += gstride) { // reversed, symmetrised copy (upper triangle)
      const int i = (int)(idx / n), k = (int)(idx % n);
      const int ri = n - 1 - i, rk = n - 1 - k;
      U[idx] = k >= i ? 0.5 * (Wo[(size_t)ri * n + rk] + Wo[(size_t)rk * n + ri]) : 0.0;
    }
  } else {
    const double sf2 = mc.sf2[o], sn2 = mc.sn2[o];
    const double* Ao = As + (size_t)o * npad * dpad;
    const double* so = sqA + (size_t)o * npad;
    double* Fo = F + (size_t)o * n * n;
    for (long long idx = gid; idx < (long long)n * n; idx += gstride) {
      const int k = (int)(idx / n), i = (int)(idx % n);                  // upper position (k, i)
      double v = 0.0;
      if (i >= k) {
        double dot = 0.0;
        for (int a = 0; a < d; ++a) dot += Ao[(size_t)i * dpad + a] * Ao[(size_t)k * dpad + a];
        v = sf2 * exp(-0.5 * ((-2.0 * dot + so[i]) + so[k])) + (i == k ? sn2 : 0.0);
      }
      U[idx] = v;
      Fo[idx] = 0.0;                                                     // E starts empty (its unit diagonal is implicit)
    }
  }
}

// ---- r03: one launch per panel ------------------------------------------------------------------------------------------
// The two-launch form of round 2 (a panel kernel + a trailing update, removed in r04) took 16 x (19-25 + 7-10) us at n = 512, and what a panel
// launch waits for is the pivot chain of its 32 x 32 diagonal block: IEEE sqrt + IEEE division per pivot and ~90 lane
// broadcasts per step on ONE wave).  k_chol_step is the same right-looking factorisation with the trailing update one
// launch late ("look-ahead"): the launch of panel kb
//   role A (workgroups [0, nA)): applies the PENDING rank-32 update of panel kb - 32 to the diagonal block and to its own
//          columns of the panel rows, factors the block with all four waves in LDS (four elements per thread, one barrier
//          per pivot; the pivot's reciprocal square root by v_rsq_f64 + two Newton steps instead of sqrt and division),
//          then the forward substitution of its columns, a row per lane, multiplying by the stored reciprocals;
//   role B (the rest): the pending update of panel kb - 32 on the rows BELOW the current panel (k_chol_update's tiles).
// Every element receives the same updates in the same order as before (sum over a panel's 32 rows, then one subtraction);
// the factors differ from the two-launch form only through the reciprocal pivots (a few ulp).
__device__ __forceinline__ double rsqrt_nr(double x) {
  double r = __builtin_amdgcn_rsq(x);                       // v_rsq_f64: ~2^-23 relative
  const double h = 0.5 * x;
  r = fma(r, fma(-h * r, r, 0.5), r);                       // r (1.5 - h r^2), twice: ~2^-45, then rounding
  r = fma(r, fma(-h * r, r, 0.5), r);
  return r;
}

__global__ __launch_bounds__(256) void k_chol_step(double* __restrict__ work, double* __restrict__ F, int with_E, int n, int kb, int nA,
                                                   int ti, int* __restrict__ bad, double* __restrict__ Dg) {
  __shared__ double D[kPB][kPB + 1];      // role A: working copy of the diagonal block (upper triangle)
  __shared__ double Uf[kPB][kPB + 1];     // role A: its factor
  __shared__ double P[kPB][kPB + 1];      // role A: P[t][r] = U[kbp + t][kb + r];  role B: the tile's rows of the pending panel
  __shared__ double Qx[kPB][kPB + 1];     // role B: the tile's columns of the pending panel
  __shared__ double rinv_sh[kPB];
  const int o = blockIdx.y, tid = threadIdx.x, bid = blockIdx.x;
  double* U = work + (size_t)o * n * n;
  double* E = F + (size_t)o * n * n;
  const int kw = n - kb < kPB ? n - kb : kPB;
  const int kbp = kb - kPB;                                  // the pending panel (kb > 0): always a full one
  if (bid >= nA) {
    // ---- role B: pending update of panel kbp on rows >= kb + kw (k_chol_update's arithmetic) ----
    int b = bid - nA, part = 0;
    if (b >= ti * ti) { b -= ti * ti; part = 1; }
    const int bx = part == 0 ? b % ti : b / ti, by = part == 0 ? b / ti : b % ti;
    const int i0 = kb + kw + by * 32;
    const int x0 = part == 0 ? kb + kw + bx * 32 : bx * 32;
    if (i0 >= n) return;
    if (part == 0 && x0 + 31 < i0) return;                   // tile entirely below the diagonal
    const double* Q = part == 0 ? U : E;
    for (int idx = tid; idx < kPB * 32; idx += blockDim.x) {
      const int r = idx / 32, t = idx % 32;
      P[r][t] = i0 + t < n ? U[(size_t)(kbp + r) * n + i0 + t] : 0.0;
      const int xc = x0 + t;
      const bool xin = part == 0 ? xc < n : xc < kb;
      // rows of E inside a panel are lower triangular: entries right of their diagonal are zero
      Qx[r][t] = (xin && (part == 0 || xc <= kbp + r)) ? Q[(size_t)(kbp + r) * n + xc] : 0.0;
    }
    __syncthreads();
    const int tx = tid % 32, ty = tid / 32;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int il = ty + 8 * rr, i = i0 + il, xc = x0 + tx;
      if (i >= n) continue;
      if (part == 0 ? (xc >= n || xc < i) : (xc >= kb)) continue;
      double acc = 0.0;
#pragma unroll
      for (int r = 0; r < kPB; ++r) acc += P[r][il] * Qx[r][tx];
      double* dst = (part == 0 ? U : E) + (size_t)i * n + xc;
      *dst -= acc;
    }
    return;
  }
  // ---- role A ----
  for (int idx = tid; idx < kPB * kPB; idx += blockDim.x) {
    const int r = idx / kPB, cc = idx % kPB;
    D[r][cc] = (r < kw && cc < kw && cc >= r) ? U[(size_t)(kb + r) * n + kb + cc] : 0.0;
    P[r][cc] = (kb > 0 && cc < kw) ? U[(size_t)(kbp + r) * n + kb + cc] : 0.0;
  }
  __syncthreads();
  const int cc = tid & 31, r0 = tid >> 5;                    // this thread's four elements: column cc, rows r0 + 8 m
  if (kb > 0) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int r = r0 + 8 * m;
      if (r <= cc && cc < kw) {
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < kPB; ++t) acc += P[t][r] * P[t][cc];
        D[r][cc] -= acc;
      }
    }
    __syncthreads();
  }
  bool notpd = false;
  for (int j = 0; j < kw; ++j) {
    const double piv = D[j][j];
    notpd = notpd || !(piv > 0.0);
    const double x = piv > 0.0 ? piv : 1.0;
    const double rv = rsqrt_nr(x);
    double ljj = x * rv;
    ljj = fma(0.5 * rv, fma(-ljj, ljj, x), ljj);             // one correction step: sqrt(x) to ~1 ulp
    const double ujc = D[j][cc] * rv;                        // entry of the scaled pivot row in this thread's column
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int r = r0 + 8 * m;
      if (r > j && cc >= r) D[r][cc] -= (D[j][r] * rv) * ujc;
      if (r == j) Uf[j][cc] = cc > j ? ujc : (cc == j ? ljj : 0.0);
    }
    if (tid == 0) rinv_sh[j] = rv;
    __syncthreads();
  }
  for (int idx = tid; idx < kPB * kPB; idx += blockDim.x)     // rows / columns beyond a short last panel
    if (idx / kPB >= kw || idx % kPB >= kw) Uf[idx / kPB][idx % kPB] = 0.0;
  if (tid >= kw && tid < kPB) rinv_sh[tid] = 1.0;
  if (tid == 0 && notpd) bad[o] = 1;
  __syncthreads();
  // the factored block goes to the side array k_chol_finish reads (never back into U: see k_chol_panel)
  if (bid == 0) {
    double* dg = Dg + ((size_t)o * ((n + kPB - 1) / kPB) + kb / kPB) * (kPB * kPB);
    for (int idx = tid; idx < kPB * kPB; idx += blockDim.x) dg[idx] = Uf[idx / kPB][idx % kPB];
  }
  // columns [kb + kw, n) of U, then (with E) [0, kb + kw) of E: a column per half wave, a row per lane
  const int nright = n - kb - kw;
  const int ncols = nright + (with_E ? kb + kw : 0);
  const int lane = tid & 63, r = lane & 31, half = lane >> 5;
  double dcol[kPB];
#pragma unroll
  for (int t = 0; t < kPB; ++t) dcol[t] = Uf[t][r];
  const double myrinv = rinv_sh[r];
  const int pairs_total = (ncols + 1) / 2;
  for (int pr = bid * (blockDim.x >> 6) + (tid >> 6); pr < pairs_total; pr += nA * (blockDim.x >> 6)) {
    const int xcol = 2 * pr + half;
    const bool live = xcol < ncols && r < kw;
    const bool isU = xcol < nright;
    const int col = isU ? kb + kw + xcol : xcol - nright;
    double* base = isU ? U : E;
    double acc = 0.0;
    if (live) acc = (!isU && col >= kb) ? (col - kb == r ? 1.0 : 0.0) : base[(size_t)(kb + r) * n + col];
    if (kb > 0) {
      // pending update: acc -= sum_t P[t][r] X[kbp + t][col]; lane t of a half fetches X[kbp + t][col] (rows of E inside the
      // pending panel are zero right of their diagonal, and so for every column of the current panel's own block)
      double xr = 0.0;
      if (xcol < ncols && (isU || col <= kbp + r)) xr = base[(size_t)(kbp + r) * n + col];
      double pend = 0.0;
#pragma unroll
      for (int t = 0; t < kPB; ++t) {
        const double x0 = readlane_f64(xr, t), x1 = readlane_f64(xr, 32 + t);
        pend += P[t][r] * (half ? x1 : x0);
      }
      if (live && (isU || col < kb)) acc -= pend;
    }
#pragma unroll
    for (int t = 0; t < kPB; ++t) {
      if (t < kw) {
        if (r == t) acc = acc * myrinv;
        const double v0 = readlane_f64(acc, t), v1 = readlane_f64(acc, 32 + t);
        const double vt = half ? v1 : v0;
        if (r > t) acc -= dcol[t] * vt;
      }
    }
    if (live && (isU || col <= kb + r)) base[(size_t)(kb + r) * n + col] = acc;
  }
}

__global__ __launch_bounds__(256) void k_chol_finish(int mode, int n, int npad, const double* __restrict__ rhs,
                                                     double* __restrict__ work, double* __restrict__ F, double* __restrict__ alpha,
                                                     const double* __restrict__ Dg) {
  const int o = blockIdx.y;
  double* U = work + (size_t)o * n * n;
  double* Fo = F + (size_t)o * n * n;
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x, gstride = (long long)gridDim.x * blockDim.x;
  if (mode == 0) {
    for (long long idx = gid; idx < (long long)n * n; idx += gstride) {   // M = J U~ J
      const int i = (int)(idx / n), j = (int)(idx % n);
      const int ur = n - 1 - i, uc = n - 1 - j;                           // position in U~ (diagonal blocks: the side array)
      double v = 0.0;
      if (j <= i)
        v = ur / kPB == uc / kPB ? Dg[((size_t)o * ((n + kPB - 1) / kPB) + ur / kPB) * (kPB * kPB) + (ur % kPB) * kPB + uc % kPB]
                                 : U[(size_t)ur * n + uc];
      Fo[idx] = v;
    }
  } else {
    // alpha = M^T (M rhs), M = Fo (lower).  t = M rhs goes through the (now free) first row of `work`
    const double* r = rhs + (size_t)o * n;
    if (blockIdx.x == 0) {
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        double s = 0.0;
        for (int j = 0; j <= i; ++j) s += Fo[(size_t)i * n + j] * r[j];
        U[i] = s;
      }
      __syncthreads();
      for (int j = threadIdx.x; j < n; j += blockDim.x) {
        double s = 0.0;
        for (int i = j; i < n; ++i) s += Fo[(size_t)i * n + j] * U[i];
        alpha[(size_t)o * npad + j] = s;
      }
    }
  }
}

// lower-triangular factor [q][n][n] -> matrix-core A-fragment images [q][tri(I, J)][256] in the model dtype
template <typename T>
__global__ __launch_bounds__(256) void k_pack_factor(const double* __restrict__ F, int n, int ld, size_t ostride, int nb,
                                                     size_t fpk_stride, T* __restrict__ Fpk) {
  const int o = blockIdx.y;
  const size_t ntri = (size_t)nb * (nb + 1) / 2;
  const double* Fo = F + (size_t)o * ostride;
  T* dst = Fpk + (size_t)o * fpk_stride;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < ntri * 256; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t blk = idx >> 8;
    const int e = (int)(idx & 255);
    // block (I, J) of the triangle from its linear index
    int I = (int)((sqrt(8.0 * (double)blk + 1.0) - 1.0) * 0.5);
    while ((size_t)(I + 1) * (I + 2) / 2 <= blk) ++I;
    while ((size_t)I * (I + 1) / 2 > blk) --I;
    const int J = (int)(blk - (size_t)I * (I + 1) / 2);
    int r, k, kk;
    MM<T>::unpack_pos(e, r, k, kk);
    const int row = 16 * I + r, col = 16 * J + MM<T>::jslot(kk, k);
    dst[idx] = (row < n && col < n && col <= row) ? (T)Fo[(size_t)row * ld + col] : T(0);
  }
}

// the caller's invK [q][n][n] (row-major, as given) -> full A images [q][nb][nb][256] for the table GEMM of the K1b plan
__global__ __launch_bounds__(256) void k_pack_full(const double* __restrict__ W, int n, int nb, double* __restrict__ img) {
  const int o = blockIdx.y;
  const double* Wo = W + (size_t)o * n * n;
  double* dst = img + (size_t)o * nb * nb * 256;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < (size_t)nb * nb * 256; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t blk = idx >> 8;
    const int e = (int)(idx & 255), I = (int)(blk / nb), J = (int)(blk % nb);
    int r, k, kk;
    MM<double>::unpack_pos(e, r, k, kk);
    const int row = 16 * I + r, col = 16 * J + MM<double>::jslot(kk, k);
    dst[idx] = (row < n && col < n) ? Wo[(size_t)row * n + col] : 0.0;
  }
}

// alpha [q][sstride] fp64 -> [q][dstride] in the model dtype (first n entries of each output, zero padding)
template <typename T>
__global__ void k_cast_alpha(const double* __restrict__ src, int sstride, int n, int q, int dstride, T* __restrict__ dst) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < q * dstride; i += gridDim.x * blockDim.x) {
    const int o = i / dstride, j = i % dstride;
    dst[i] = j < n ? (T)src[(size_t)o * sstride + j] : T(0);
  }
}

// One more observation with frozen hyper-parameters and normalisation.  With k = K(X, x_new),
// kappa = sf2 + sn2 and u = invK k = M^T (M k), s = kappa - k.u, the inverse of the bordered matrix is
// [[invK + u u^T / s, -u / s], [-u^T / s, 1 / s]]: the lower factor simply gains the row (-u^T / sqrt(s), 1 / sqrt(s)),
// and alpha_new = (alpha + u (k.alpha - rho) / s, (rho - k.alpha) / s).  O(n^2), one workgroup per output, in two launches:
// k_model_append computes u, s and k.alpha into scratch and flags s <= 0; k_model_append_commit writes the factor's new row and
// alpha -- launched only once the host has seen no output flagged, so that a refused append leaves the model as it was.
__global__ __launch_bounds__(1024) void k_model_append(int n, int ld, const double* __restrict__ F, const double* __restrict__ alpha,
                                                       const double* __restrict__ kvec, const double* __restrict__ kappa,
                                                       double* __restrict__ scratch, double* __restrict__ sk, int* __restrict__ bad) {
  __shared__ double red[32];
  const int o = blockIdx.x, tid = threadIdx.x;
  const double* M = F + (size_t)o * ld * ld;
  const double* al = alpha + (size_t)o * ld;
  const double* k = kvec + (size_t)o * n;
  double* t = scratch + (size_t)o * 2 * ld;
  double* u = t + ld;
  for (int i = tid; i < n; i += blockDim.x) {            // t = M k
    double s = 0.0;
    for (int j = 0; j <= i; ++j) s += M[(size_t)i * ld + j] * k[j];
    t[i] = s;
  }
  __syncthreads();
  double ku = 0.0, ka = 0.0;
  for (int j = tid; j < n; j += blockDim.x) {            // u = M^T t ;  partial sums of k.u and k.alpha
    double s = 0.0;
    for (int i = j; i < n; ++i) s += M[(size_t)i * ld + j] * t[i];
    u[j] = s;
    ku += k[j] * s;
    ka += k[j] * al[j];
  }
  auto block_sum = [&](double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
    return s;
  };
  ku = block_sum(ku);
  ka = block_sum(ka);
  if (tid == 0) {
    const double s = kappa[o] - ku;
    if (!(s > 0.0)) bad[o] = 1;
    sk[2 * o] = s;
    sk[2 * o + 1] = ka;
  }
}
__global__ __launch_bounds__(1024) void k_model_append_commit(int n, int ld, double* __restrict__ F, double* __restrict__ alpha,
                                                              const double* __restrict__ rho, const double* __restrict__ scratch,
                                                              const double* __restrict__ sk) {
  const int o = blockIdx.x, tid = threadIdx.x;
  double* M = F + (size_t)o * ld * ld;
  double* al = alpha + (size_t)o * ld;
  const double* u = scratch + (size_t)o * 2 * ld + ld;
  const double s = sk[2 * o], ka = sk[2 * o + 1], rs = 1.0 / sqrt(s), coef = (ka - rho[o]) / s;
  for (int j = tid; j < n; j += blockDim.x) {
    M[(size_t)n * ld + j] = -u[j] * rs;
    al[j] += u[j] * coef;
  }
  if (tid == 0) {
    M[(size_t)n * ld + n] = rs;
    al[n] = (rho[o] - ka) / s;
  }
  for (int j = n + 1 + tid; j < ld; j += blockDim.x) M[(size_t)n * ld + j] = 0.0;
}

// k observations in one block update.  With B = K(X, X_new) [n][k], Z = K(X_new, X_new) + sn2 I, rho = y_new - mp:
//   T = M B,  U = M^T T (= invK B),  S = Z - B^T U,  g = B^T alpha,  S = R R^T,  G = R^-1,  w = G^T G (g - rho);
//   rows n + r of M: -(G U^T)[r] | G[r][0..r] | 0;   alpha[0..n) += U w,  alpha[n..n+k) = -w
// -- the factor k calls of k_model_append would leave (a lower factor with positive diagonal is unique), with the two triangular
// products as block products over the whole chip.  The block's columns are padded to kp = a multiple of kAppColBlock; the padding
// columns of B are zero and stay zero through T and U, so that no kernel needs a column guard.  Launches, fp64 throughout:
//   k_append_cross : B [q][n][kp] (column c of the block contiguous: a wave reads <= 512 contiguous bytes per row) and Z [q][kp][kp]
//                    from the fp64 observations with the expanded distance; Z[r][c] is formed once for r < c and mirrored;
//   k_append_t     : T = M B.  A wave owns kAppRows rows of M, lanes along the block's columns: M[i][j] is wave-uniform, rows of B and T
//                    are coalesced; the sum of (i, c) runs over j = 0 .. i in index order in one accumulator;
//   k_append_u     : U = M^T T.  A wave owns a strip of 64 columns j of M (lanes along them: a row segment is one coalesced load, as
//                    k_model_remove) and kAppColBlock columns of the block; T[i][c] is a broadcast read; the sum of (j, c) runs over
//                    i = j .. n - 1 in index order in one accumulator;
//   k_append_s     : S = Z - B^T U, a wave per kAppSRows rows of S, lanes along its columns, and g = B^T alpha in one more wave;
//                    every sum over j = 0 .. n - 1 in index order in one accumulator;
//   k_append_chol  : one workgroup per output: the lower Cholesky of S in LDS (IEEE sqrt and division; a pivot that is not > 0 flags
//                    bad[o] = 1 + its row), G = R^-1, w;
//   k_append_commit: once the host has seen every output accepted: the k new rows (lanes along the columns, coalesced writes; the sum
//                    over c <= r of G[r][c] U[j][c] in index order), zeros right of the diagonal up to ld, alpha.
// Nothing above the diagonal of the resident factor is read (a build leaves scratch there), no kernel but the last writes the factor
// or alpha, no atomics, and no sum depends on the launch shape.
constexpr int kAppRows = 4;          // k_append_t: rows of M per wave
constexpr int kAppWaves = 4;         // ... waves per workgroup
constexpr int kAppColBlock = 8;      // k_append_u: columns of the block per wave; the block's padded width is a multiple of it
constexpr int kAppSRows = 4;         // k_append_s: rows of S per wave
static_assert(SBO_MAX_APPEND == 64 && SBO_MAX_APPEND % kAppColBlock == 0 && kAppColBlock % kAppSRows == 0, "the block is one wave wide");

template <int D>
__global__ __launch_bounds__(256) void k_append_cross(const ModelConst mc, int n, int k, int kp, const double* __restrict__ Xall /* [n + k][d] */,
                                                      double* __restrict__ B, double* __restrict__ Z) {
  const int o = blockIdx.y, d = mc.d;
  const double sf2 = mc.sf2[o], sn2 = mc.sn2[o];
  double* Bo = B + (size_t)o * n * kp;
  double* Zo = Z + (size_t)o * kp * kp;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < (long long)(n + kp) * kp; idx += (long long)gridDim.x * blockDim.x) {
    const int row = (int)(idx / kp), c = (int)(idx % kp);
    const int r = row - n;                                   // row of Z (row >= n)
    double v = 0.0;
    if (c < k && r < k) {
      // the older observation is `a` of the expanded distance, as in a row-by-row append
      const int ia = r < 0 ? row : n + min(r, c), ib = r < 0 ? n + c : n + max(r, c);
      if (r == c) {
        v = sf2 + sn2;                                       // kappa, as sbo_model_append sets it
      } else {
        double dot = 0.0, asq = 0.0, bsq = 0.0;
#pragma unroll
        for (int a = 0; a < D; ++a) {
          if (a < d) {
            const double va = Xall[(size_t)ia * d + a] * mc.vinv[o][a], vb = Xall[(size_t)ib * d + a] * mc.vinv[o][a];
            dot += va * vb;
            asq += va * va;
            bsq += vb * vb;
          }
        }
        v = sf2 * exp(-0.5 * ((-2.0 * dot + asq) + bsq));
      }
    }
    if (r < 0) Bo[(size_t)row * kp + c] = v;
    else Zo[(size_t)r * kp + c] = v;
  }
}

// Steps of kAppStep columns: the wave fetches the rows' segments M[i][j0 .. j0 + 63] (one coalesced load per row, zero right of a
// row's diagonal; the next step's segments are requested before this step's arithmetic), every lane its 64 values of B, all in
// flight at once; M[i][j] then reaches the multiply as a wave-uniform operand (readlane).  The terms right of the diagonal are +0
// and leave the sum as it is.
constexpr int kAppStep = 64;
__global__ __launch_bounds__(64 * kAppWaves) void k_append_t(int n, int ld, int kp, const double* __restrict__ F, const double* __restrict__ B,
                                                             double* __restrict__ T) {
  const int o = blockIdx.y, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int i0 = ((int)blockIdx.x * kAppWaves + wave) * kAppRows;
  if (i0 >= n) return;
  const int c = min(lane, kp - 1);                           // (lanes past the block's width repeat its last column and store nothing)
  const double* M = F + (size_t)o * ld * ld;
  const double* Bo = B + (size_t)o * n * kp + c;
  const int ilast = min(i0 + kAppRows, n) - 1;
  double acc[kAppRows], m[kAppRows], mnext[kAppRows];
#pragma unroll
  for (int u = 0; u < kAppRows; ++u) {
    acc[u] = 0.0;
    m[u] = (i0 + u < n && lane <= i0 + u) ? M[(size_t)(i0 + u) * ld + lane] : 0.0;
  }
  for (int j0 = 0; j0 <= ilast; j0 += kAppStep) {
    double b[kAppStep];
    const int jn = j0 + kAppStep + lane;
#pragma unroll
    for (int u = 0; u < kAppRows; ++u) mnext[u] = (i0 + u < n && jn <= i0 + u) ? M[(size_t)(i0 + u) * ld + jn] : 0.0;
#pragma unroll
    for (int t = 0; t < kAppStep; ++t) b[t] = Bo[(size_t)min(j0 + t, n - 1) * kp];      // (past the last row: any finite value, its factor is 0)
#pragma unroll
    for (int t = 0; t < kAppStep; ++t) {
#pragma unroll
      for (int u = 0; u < kAppRows; ++u) acc[u] = fma(readlane_f64(m[u], t), b[t], acc[u]);
    }
#pragma unroll
    for (int u = 0; u < kAppRows; ++u) m[u] = mnext[u];
  }
  if (lane < kp) {
    double* To = T + (size_t)o * n * kp + lane;
#pragma unroll
    for (int u = 0; u < kAppRows; ++u)
      if (i0 + u < n) To[(size_t)(i0 + u) * kp] = acc[u];
  }
}

// Steps of kAppURows rows: every lane fetches its column's 128 values of M (coalesced row segments, zero above the diagonal) and two
// rows of the step's [128][kAppColBlock] tile of T, all in flight at once -- the walk down a strip is bound by the latency of these
// loads, so as many as the registers hold --; the tile goes through LDS, from where T[i][c] is a broadcast read.
constexpr int kAppURows = 128;
__global__ __launch_bounds__(64) void k_append_u(int n, int ld, int kp, const double* __restrict__ F, const double* __restrict__ T,
                                                 double* __restrict__ U) {
  static_assert(kAppURows == 2 * 64, "two rows of the tile per lane");
  __shared__ __attribute__((aligned(32))) double sT[kAppURows][kAppColBlock];
  const int o = blockIdx.z, c0 = (int)blockIdx.y * kAppColBlock, j0 = (int)blockIdx.x * 64, lane = threadIdx.x, j = j0 + lane;
  const double* M = F + (size_t)o * ld * ld;
  const double* To = T + (size_t)o * n * kp + c0;
  double acc[kAppColBlock];
#pragma unroll
  for (int cc = 0; cc < kAppColBlock; ++cc) acc[cc] = 0.0;
  for (int i0 = j0; i0 < n; i0 += kAppURows) {
    double x[kAppURows];
#pragma unroll
    for (int u = 0; u < kAppURows; ++u) {
      const int i = i0 + u;
      x[u] = (i < n && j <= i) ? M[(size_t)i * ld + j] : 0.0;          // (j <= i < n: inside the triangle)
    }
    double tv[2][kAppColBlock];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int e = 0; e < kAppColBlock; ++e) tv[h][e] = i0 + 64 * h + lane < n ? To[(size_t)(i0 + 64 * h + lane) * kp + e] : 0.0;
    }
    __syncthreads();                                         // (the previous step's reads of the tile are done)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int e = 0; e < kAppColBlock; ++e) sT[64 * h + lane][e] = tv[h][e];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kAppURows; ++u) {
#pragma unroll
      for (int cc = 0; cc < kAppColBlock; ++cc) acc[cc] = fma(x[u], sT[u][cc], acc[cc]);      // (rows above the lane's diagonal and past n add +0)
    }
  }
  if (j < n) {
    double* dst = U + ((size_t)o * n + j) * kp + c0;
#pragma unroll
    for (int cc = 0; cc < kAppColBlock; ++cc) dst[cc] = acc[cc];
  }
}

// blockIdx.x < kp / kAppSRows: rows of S;  the last workgroup: g.  Steps of kAppStep rows j: every lane fetches its column's 64 values
// of U and one row of the step's [64][kAppSRows] tile of B, all in flight at once; the tile goes through LDS, from where B[j][r] is a
// broadcast read (g: alpha[j] by readlane).
__global__ __launch_bounds__(64) void k_append_s(int n, int a_ld, int kp, const double* __restrict__ B, const double* __restrict__ U,
                                                 const double* __restrict__ Z, const double* __restrict__ alpha, double* __restrict__ S,
                                                 double* __restrict__ g) {
  static_assert(kAppStep == 64, "one row of the tile per lane");
  __shared__ __attribute__((aligned(32))) double sB[kAppStep][kAppSRows];
  const int o = blockIdx.y, lane = threadIdx.x, c = min(lane, kp - 1);
  const double* Bo = B + (size_t)o * n * kp;
  if ((int)blockIdx.x == kp / kAppSRows) {
    const double* al = alpha + (size_t)o * a_ld;
    double s = 0.0;
    for (int j0 = 0; j0 < n; j0 += kAppStep) {
      double b[kAppStep];
      const double av = j0 + lane < n ? al[j0 + lane] : 0.0;
#pragma unroll
      for (int t = 0; t < kAppStep; ++t) b[t] = Bo[(size_t)min(j0 + t, n - 1) * kp + c];
#pragma unroll
      for (int t = 0; t < kAppStep; ++t) s = fma(b[t], readlane_f64(av, t), s);
    }
    if (lane < kp) g[(size_t)o * kp + lane] = s;
    return;
  }
  const int r0 = (int)blockIdx.x * kAppSRows;
  const double* Uo = U + (size_t)o * n * kp + c;
  double acc[kAppSRows];
#pragma unroll
  for (int u = 0; u < kAppSRows; ++u) acc[u] = 0.0;
  for (int j0 = 0; j0 < n; j0 += kAppStep) {
    double uv[kAppStep], bv[kAppSRows];
#pragma unroll
    for (int u = 0; u < kAppSRows; ++u) bv[u] = j0 + lane < n ? Bo[(size_t)(j0 + lane) * kp + r0 + u] : 0.0;
#pragma unroll
    for (int t = 0; t < kAppStep; ++t) uv[t] = Uo[(size_t)min(j0 + t, n - 1) * kp];      // (past the last row: its factor is 0)
    __syncthreads();                                         // (the previous step's reads of the tile are done)
#pragma unroll
    for (int u = 0; u < kAppSRows; ++u) sB[lane][u] = bv[u];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kAppStep; ++t) {
#pragma unroll
      for (int u = 0; u < kAppSRows; ++u) acc[u] = fma(sB[t][u], uv[t], acc[u]);
    }
  }
  if (lane < kp) {
#pragma unroll
    for (int u = 0; u < kAppSRows; ++u) S[((size_t)o * kp + r0 + u) * kp + lane] = Z[((size_t)o * kp + r0 + u) * kp + lane] - acc[u];
  }
}

__global__ __launch_bounds__(256) void k_append_chol(int k, int kp, const double* __restrict__ S, const double* __restrict__ g,
                                                     const double* __restrict__ rho, double* __restrict__ G, double* __restrict__ w,
                                                     int* __restrict__ bad) {
  // A: below the diagonal R; above it, transposed, first the running sums and then the entries of G = R^-1 (A[c][r] <-> G[r][c],
  // r > c); the diagonals of R and G in dg and ginv.  One array: two would not fit 64 KiB.
  constexpr int K = SBO_MAX_APPEND;
  __shared__ double A[K][K + 1];
  __shared__ double dg[K], ginv[K], e[K], v[K];
  __shared__ int sh_bad;
  const int o = blockIdx.x, tid = threadIdx.x;
  const double* So = S + (size_t)o * kp * kp;
  if (tid == 0) sh_bad = 0;
  for (int idx = tid; idx < K * K; idx += blockDim.x) {
    const int r = idx / K, c = idx % K;
    A[r][c] = (r < k && c <= r) ? So[(size_t)r * kp + c] : 0.0;      // (the lower triangle is the one that is factored)
  }
  __syncthreads();
  // S = R R^T, right-looking: every element receives its updates in the order of the pivots
  for (int jj = 0; jj < k; ++jj) {
    const double piv = A[jj][jj];                            // (nobody writes the diagonal)
    if (tid == 0 && !(piv > 0.0) && sh_bad == 0) sh_bad = 1 + jj;
    const double rjj = sqrt(piv > 0.0 ? piv : 1.0);
    if (tid > jj && tid < k) A[tid][jj] = A[tid][jj] / rjj;
    if (tid == jj) dg[jj] = rjj;
    __syncthreads();
    {                                                        // column c = tid % K, rows r = tid / K + 4 s: operands first, then the stores
      const int c = tid & (K - 1), rb = tid >> 6;
      const double lc = A[c][jj];
      double a[K / 4], lr[K / 4];
#pragma unroll
      for (int s = 0; s < K / 4; ++s) {
        a[s] = A[rb + 4 * s][c];
        lr[s] = A[rb + 4 * s][jj];
      }
#pragma unroll
      for (int s = 0; s < K / 4; ++s) {
        const int r = rb + 4 * s;
        if (c > jj && c <= r && r < k) A[r][c] = a[s] - lr[s] * lc;
      }
    }
    __syncthreads();
  }
  // G = R^-1, right-looking as well: G[t][c] = (delta_tc - sum_{t' < t} R[t][t'] G[t'][c]) / R[t][t], the sum of (r, c) growing by
  // the term of t once row t of G is known -- in the order of t
  for (int t = 0; t < k; ++t) {
    if (tid < t) A[tid][t] = -A[tid][t] / dg[t];
    if (tid == t) ginv[t] = 1.0 / dg[t];
    __syncthreads();
    {                                                        // row r = tid % K of R, columns c = tid / K + 4 s of G: operands first
      const int r = tid & (K - 1), cb = tid >> 6;
      const double rt = A[r][t], gt = ginv[t];
      double a[K / 4], gc[K / 4];
#pragma unroll
      for (int s = 0; s < K / 4; ++s) {
        a[s] = A[cb + 4 * s][r];
        gc[s] = A[cb + 4 * s][t];
      }
#pragma unroll
      for (int s = 0; s < K / 4; ++s) {
        const int c = cb + 4 * s;
        if (c <= t && r > t && r < k) A[c][r] = fma(rt, c == t ? gt : gc[s], a[s]);
      }
    }
    __syncthreads();
  }
  if (tid < k) e[tid] = g[(size_t)o * kp + tid] - rho[(size_t)o * kp + tid];
  __syncthreads();
  if (tid < k) {                                             // v = G e
    double s = 0.0;
    for (int c = 0; c < tid; ++c) s = fma(A[c][tid], e[c], s);
    v[tid] = fma(ginv[tid], e[tid], s);
  }
  __syncthreads();
  if (tid < kp) {                                            // w = G^T v  (padding columns: 0)
    double s = 0.0;
    if (tid < k) {
      s = ginv[tid] * v[tid];
      for (int r = tid + 1; r < k; ++r) s = fma(A[tid][r], v[r], s);
    }
    w[(size_t)o * kp + tid] = s;
  }
  for (int idx = tid; idx < kp * kp; idx += blockDim.x) {
    const int r = idx / kp, c = idx % kp;
    G[(size_t)o * kp * kp + idx] = (r < k && c <= r) ? (c == r ? ginv[r] : A[c][r]) : 0.0;
  }
  if (tid == 0) bad[o] = sh_bad;
}

// A wave per 64 columns of the new rows.  Left of column n a lane keeps its row of U in registers and walks the rows of G (LDS,
// broadcast reads; the entries right of G's diagonal and in the padding are zero and leave the sum as it is).
__global__ __launch_bounds__(64) void k_append_commit(int n, int ld, int a_ld, int k, int kp, double* __restrict__ F, double* __restrict__ alpha,
                                                      const double* __restrict__ U, const double* __restrict__ G, const double* __restrict__ w) {
  constexpr int K = SBO_MAX_APPEND;
  __shared__ double sG[K][K];
  __shared__ double sw[K];
  const int o = blockIdx.y, lane = threadIdx.x, j0 = (int)blockIdx.x * 64, j = j0 + lane;
  double* M = F + (size_t)o * ld * ld;
  if (j0 >= n + k) {                                         // right of the new diagonal block: zeros
    if (j < ld)
      for (int r = 0; r < k; ++r) M[(size_t)(n + r) * ld + j] = 0.0;
    return;
  }
  for (int idx = lane; idx < K * K; idx += 64) {
    const int r = idx / K, c = idx % K;
    sG[r][c] = (r < kp && c < kp) ? G[((size_t)o * kp + r) * kp + c] : 0.0;
  }
  sw[lane] = lane < kp ? w[(size_t)o * kp + lane] : 0.0;
  double u[K];
#pragma unroll
  for (int c = 0; c < K; ++c) u[c] = (j < n && c < kp) ? U[((size_t)o * n + j) * kp + c] : 0.0;
  __syncthreads();
  if (j >= ld) return;
  for (int r = 0; r < k; ++r) {
    double val = 0.0;
    if (j < n) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < K; ++c) s = fma(sG[r][c], u[c], s);
      val = -s;
    } else if (j - n <= r) {
      val = sG[r][j - n];
    }
    M[(size_t)(n + r) * ld + j] = val;                       // (right of the diagonal: 0)
  }
  double* al = alpha + (size_t)o * a_ld;
  if (j < n) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < K; ++c) s = fma(u[c], sw[c], s);
    al[j] += s;
  } else if (j < n + k) {
    al[j] = -sw[j - n];
  }
}

// One observation less.  With m = column j of M (zero above row j, m[j] > 0), M~ = M without column j,
// r_i = sqrt(sum_{t=j..i} m[t]^2) and the running sum W_i = sum_{t=j..i} m[t] row_t(M~), the Givens rotations that turn m into
// r_{n-1} e_j leave rows 0 .. j-1 of M~ as they are and give, for i = j+1 .. n-1,
//   new row i-1 = (r_{i-1} / r_i) row_i(M~) - (m[i] / (r_i r_{i-1})) W_{i-1};
// the rotated row j is dropped.  N^T N is the Schur complement invK_-j-j - p p^T / P_jj with p = M~^T m = W_{n-1} and
// P_jj = r_{n-1}^2, the exact inverse of K without row and column j, and alpha' = alpha_-j - p alpha_j / P_jj.  Two launches:
//   k_model_remove_coef: one workgroup per output reads column j once and writes what every strip needs per row -- m[i],
//                        a[i] = r_{i-1} / r_i, b[i] = m[i] / (r_i r_{i-1}) -- and alpha_j / P_jj (IEEE sqrt and division);
//   k_model_remove     : one wave per strip of kRemoveStrip new columns and output, lanes along the columns (the row-major
//                        factor is read and written coalesced), down the rows with W in a register.
// New column c comes from old column c (c < j) or c + 1 and new row i - 1 from old row i, so the result goes to a second, zeroed
// buffer (no strip reads what another writes); nothing above the diagonal of the old factor is read (a build leaves scratch there).
constexpr int kRemoveStrip = 64;
__global__ __launch_bounds__(256) void k_model_remove_coef(int n, int ld, int a_ld, int j, const double* __restrict__ F,
                                                           const double* __restrict__ alpha, double* __restrict__ coef) {
  __shared__ double mv[SBO_MAX_N], sq[SBO_MAX_N];
  __shared__ double part[256];
  const int o = blockIdx.x, tid = threadIdx.x, len = n - j;
  const double* M = F + (size_t)o * ld * ld;
  double* cm = coef + (size_t)o * (3 * (size_t)ld + 1);
  double* ca = cm + ld;
  double* cb = ca + ld;
  for (int k = tid; k < len; k += 256) {
    const double v = M[(size_t)(j + k) * ld + j];
    cm[j + k] = v;
    mv[k] = v;
    sq[k] = v * v;
  }
  __syncthreads();
  // inclusive prefix sums of m^2: a contiguous chunk per thread, the chunks before it summed in order
  const int chunk = (len + 255) / 256, k0 = tid * chunk, k1 = min(len, k0 + chunk);
  double s = 0.0;
  for (int k = k0; k < k1; ++k) s += sq[k];
  part[tid] = s;
  __syncthreads();
  double acc = 0.0;
  for (int t = 0; t < tid; ++t) acc += part[t];
  for (int k = k0; k < k1; ++k) {
    const double prev = acc;
    acc += sq[k];
    if (k > 0) {
      const double r = sqrt(acc), rp = sqrt(prev);
      ca[j + k] = rp / r;
      cb[j + k] = mv[k] / (r * rp);
    }
    if (k == len - 1) cb[ld + 0] = alpha[(size_t)o * a_ld + j] / acc;       // alpha_j / P_jj
  }
}
__global__ __launch_bounds__(64) void k_model_remove(int n, int ld, int a_ld, int j, const double* __restrict__ F,
                                                     const double* __restrict__ alpha, const double* __restrict__ coef,
                                                     double* __restrict__ F2, double* __restrict__ alpha2) {
  constexpr int kU = 8;                      // rows in flight per wave
  const int o = blockIdx.y, c0 = blockIdx.x * kRemoveStrip, cn = c0 + (int)threadIdx.x;
  const bool active = cn < n - 1;
  const int co = cn < j ? cn : cn + 1;       // the old column of new column cn
  const double* M = F + (size_t)o * ld * ld;
  double* N = F2 + (size_t)o * ld * ld;
  const double* cm = coef + (size_t)o * (3 * (size_t)ld + 1);
  const double* ca = cm + ld;
  const double* cb = ca + ld;
  // rows above j: as they were (their columns lie left of j)
  for (int i0 = c0; i0 < j; i0 += kU) {
    double x[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int i = i0 + u;
      x[u] = (active && i < j && cn <= i) ? M[(size_t)i * ld + cn] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int i = i0 + u;
      if (active && i < j && cn <= i) N[(size_t)i * ld + cn] = x[u];
    }
  }
  // rows j .. n-1 (a strip right of j starts at its own diagonal: the rows above hold nothing of its columns)
  double W = 0.0;
  for (int i0 = max(j, c0); i0 < n; i0 += kU) {
    double x[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int i = i0 + u;
      x[u] = (active && i < n && co <= i) ? M[(size_t)i * ld + co] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int i = i0 + u;
      if (i < n) {
        if (i > j && active && cn <= i - 1) N[(size_t)(i - 1) * ld + cn] = ca[i] * x[u] - cb[i] * W;
        W += cm[i] * x[u];
      }
    }
  }
  if (active) alpha2[(size_t)o * a_ld + cn] = alpha[(size_t)o * a_ld + co] - W * cb[ld];
}

// Leave-one-out diagnostics of the resident model.  With P = invK = M^T M the leave-one-out prediction of
// observation i has the residual e_i = y_i - mu_-i = alpha_i / P_ii and the variance v_i = 1 / P_ii (noise included), and
// P_ii = sum_{t >= i} M[t][i]^2 is a column sum of squares of the lower factor; log det(K + sn2 I) = -2 sum_i log M[i][i].
// Read-only, two launches:
//   k_model_loo_colsq : one wave per strip of kLooStrip columns, chunk of kLooRows rows and output, lanes along the columns (a row
//                       segment is one coalesced load, kU rows in flight), the running sum in a register, rows in ascending order;
//                       the partial sum of chunk k goes to part[o][k][column].  Nothing above the diagonal is read (a build leaves
//                       scratch there) and no row >= n (a grown factor has ld > n).  A chunk that lies above the strip's diagonal
//                       block has no rows: its wave leaves at once and its partials are never read.
//   k_model_loo_finish: one workgroup per output adds the partials of a column in chunk order (from the chunk that holds the
//                       diagonal on), forms e, v, z = e / sqrt(v) (IEEE division and sqrt) and reduces logdet, lpd, max |z| with
//                       its lowest index and #{|z| > b} in LDS.
// No atomics and one summation order: the same model gives the same bits whatever was called before.
constexpr int kLooStrip = 64;
constexpr int kLooRows = 64;
__global__ __launch_bounds__(64) void k_model_loo_colsq(int n, int ld, int chunks, const double* __restrict__ F, double* __restrict__ part) {
  constexpr int kU = 16;                     // rows in flight per wave
  const int o = blockIdx.z, k = blockIdx.y, c0 = blockIdx.x * kLooStrip, cn = c0 + (int)threadIdx.x;
  const int r0 = max(k * kLooRows, c0), r1 = min(n, (k + 1) * kLooRows);
  if (r1 <= r0) return;
  const double* M = F + (size_t)o * ld * ld;
  double s = 0.0;
  for (int i0 = r0; i0 < r1; i0 += kU) {
    double x[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int i = i0 + u;
      x[u] = (i < r1 && cn <= i) ? M[(size_t)i * ld + cn] : 0.0;      // (cn <= i < n: inside the triangle)
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) s += x[u] * x[u];
  }
  if (cn < n) part[((size_t)o * chunks + k) * ld + cn] = s;
}
__global__ __launch_bounds__(1024) void k_model_loo_finish(int n, int q, int ld, int a_ld, int chunks, double b, const double* __restrict__ F,
                                                           const double* __restrict__ alpha, const double* __restrict__ part,
                                                           double* __restrict__ resid /* [n][q] or nullptr */,
                                                           double* __restrict__ var /* [n][q] or nullptr */, LooSummary* __restrict__ sum) {
  __shared__ double s_ld[1024], s_lp[1024], s_z[1024];
  __shared__ int s_i[1024], s_c[1024];
  constexpr int kU = 8;
  const int o = blockIdx.x, tid = threadIdx.x;
  const double* M = F + (size_t)o * ld * ld;
  double ldsum = 0.0, lpsum = 0.0, zm = -1.0;
  int zi = 0x7fffffff, cnt = 0;
  for (int i = tid; i < n; i += 1024) {
    double P = 0.0;
    for (int k0 = i / kLooRows; k0 < chunks; k0 += kU) {      // (chunk order; kU partials in flight, the missing ones add +0)
      double x[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) x[u] = k0 + u < chunks ? part[((size_t)o * chunks + k0 + u) * ld + i] : 0.0;
#pragma unroll
      for (int u = 0; u < kU; ++u) P += x[u];
    }
    const double a = alpha[(size_t)o * a_ld + i];
    const double v = 1.0 / P, e = a / P;
    const double az = fabs(e / sqrt(v));
    if (resid) resid[(size_t)i * q + o] = e;
    if (var) var[(size_t)i * q + o] = v;
    ldsum += log(M[(size_t)i * ld + i]);
    lpsum += log(6.283185307179586476925 * v) + e * e / v;
    if (az > zm) { zm = az; zi = i; }        // (ascending i: the lowest index of a tie stays)
    cnt += az > b ? 1 : 0;
  }
  s_ld[tid] = ldsum, s_lp[tid] = lpsum, s_z[tid] = zm, s_i[tid] = zi, s_c[tid] = cnt;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if (tid < w) {
      s_ld[tid] += s_ld[tid + w];
      s_lp[tid] += s_lp[tid + w];
      s_c[tid] += s_c[tid + w];
      const double z2 = s_z[tid + w];
      const int i2 = s_i[tid + w];
      if (z2 > s_z[tid] || (z2 == s_z[tid] && i2 < s_i[tid])) { s_z[tid] = z2; s_i[tid] = i2; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    LooSummary r;
    r.logdet = -2.0 * s_ld[0];
    r.lpd = -0.5 * s_lp[0];
    r.z_max = s_z[0];
    r.z_argmax = s_i[0];
    r.outside = s_c[0];
    sum[o] = r;
  }
}

// Derived model arrays from the uploaded X_norm [n][d] / Y_norm [n][q] (models/GP_Safe.py:112-116, 331-342):
//   As[o][j][a] = X_norm[j][a] ell_a^-1/2, sqA[o][j] = sum_a As^2 (model dtype for the K1 kernels, fp64 for the build),
//   Xn[j][a] (model dtype, for the mean gradient), rhs[o][j] = Y_norm[j][o] - mp_o (fp64, only with Y_norm).
// Rows j >= n of the padded arrays are zero.
template <typename T>
__global__ __launch_bounds__(256) void k_model_prep(const ModelConst mc, const double* __restrict__ Xh, const double* __restrict__ Yh,
                                                    T* __restrict__ As, T* __restrict__ sqA, T* __restrict__ Xn, double* __restrict__ As64,
                                                    double* __restrict__ sq64, double* __restrict__ rhs) {
  const int n = mc.n, npad = mc.npad, d = mc.d, D = mc.dpad, q = mc.q;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < q * npad; i += gridDim.x * blockDim.x) {
    const int o = i / npad, j = i - o * npad;
    double s_ = 0.0;
    for (int a = 0; a < D; ++a) {
      double v = 0.0, x = 0.0;
      if (j < n && a < d) {
        x = Xh[(size_t)j * d + a];
        v = x * mc.vinv[o][a];                                          // GP_Safe.py:115
        s_ += v * v;
      }
      As[(size_t)i * D + a] = (T)v;
      As64[(size_t)i * D + a] = v;
      if (o == 0) Xn[(size_t)j * D + a] = (T)x;
    }
    sqA[i] = (T)s_;
    sq64[i] = s_;
    if (Yh && j < n) rhs[(size_t)o * n + j] = Yh[(size_t)j * q + o] - mc.mp[o];
  }
}

// Upload X_norm (and Y_norm) through the pinned staging area and derive the model arrays on the device.  Layout of
// c->mwork (doubles): XY [n d + n q] | As64 | sq64 | rhs | sf2 sn2 | W | work | Dg | bad (ints)
struct ModelWork {
  double *XY, *As64, *sq64, *rhs, *sfsn, *W, *work, *Dg;
  int* bad;
};
static int model_work(sbo_ctx* c, bool with_W, ModelWork& w) {
  const ModelConst& mc = c->mc;
  const size_t n = mc.n, q = mc.q, npad = mc.npad, nn = n * n;
  const size_t nXY = n * mc.d + n * q, nAs = q * npad * mc.dpad, nsq = q * npad, nrhs = q * n;
  const size_t ndiag = q * ((n + kPB - 1) / kPB) * (kPB * kPB);
  return carve(c->mwork, [&](Carve cv) {
    cv.take(w.XY, nXY); cv.take(w.As64, nAs); cv.take(w.sq64, nsq); cv.take(w.rhs, nrhs);
    cv.take(w.sfsn, 2 * q); cv.take(w.W, with_W ? q * nn : 0); cv.take(w.work, q * nn); cv.take(w.Dg, ndiag);
    cv.take(w.bad, q);
    return cv.off;
  });
}
static int stage_ensure(sbo_ctx* c, size_t bytes) {
  if (c->h_stage.bytes >= bytes) return SBO_OK;
  c->h_stage.reset();
  const size_t want = bytes + bytes / 2 + 4096;
  if (hipHostMalloc(&c->h_stage.p, want, hipHostMallocDefault) != hipSuccess) return fail(SBO_E_HIP, "hipHostMalloc (model staging)");
  c->h_stage.bytes = want;
  return SBO_OK;
}
template <typename T>
static int model_prep_t(sbo_ctx* c, const double* X_norm, const double* Y_norm, const ModelWork& w) {
  const ModelConst& mc = c->mc;
  const size_t n = mc.n, q = mc.q, npad = mc.npad;
  int rc;
  if ((rc = stage_ensure(c, sizeof(double) * (n * mc.d + n * q + 2 * q)))) return rc;
  double* hs = (double*)c->h_stage.p;
  std::memcpy(hs, X_norm, sizeof(double) * n * mc.d);
  if (Y_norm) std::memcpy(hs + n * mc.d, Y_norm, sizeof(double) * n * q);
  SBO_HIP(hipMemcpyAsync(w.XY, hs, sizeof(double) * (n * mc.d + (Y_norm ? n * q : 0)), hipMemcpyHostToDevice, c->stream));
  if ((rc = ensure(c->As, sizeof(T) * q * npad * mc.dpad))) return rc;
  if ((rc = ensure(c->sqA, sizeof(T) * q * npad))) return rc;
  if ((rc = ensure(c->Xn, sizeof(T) * npad * mc.dpad))) return rc;
  hipLaunchKernelGGL((k_model_prep<T>), dim3((unsigned)((q * npad + 255) / 256)), dim3(256), 0, c->stream, mc, (const double*)w.XY,
                     Y_norm ? (const double*)(w.XY + n * mc.d) : (const double*)nullptr, (T*)c->As.p, (T*)c->sqA.p, (T*)c->Xn.p, w.As64,
                     w.sq64, w.rhs);
  SBO_HIP(hipGetLastError());
  return SBO_OK;
}
int model_prep(sbo_ctx* c, const double* X_norm) {         // (after an append: the derived arrays with the new row)
  ModelWork w;
  int rc = model_work(c, false, w);
  if (rc) return rc;
  rc = c->dtype == SBO_F64 ? model_prep_t<double>(c, X_norm, nullptr, w) : model_prep_t<float>(c, X_norm, nullptr, w);
  if (rc) return rc;
  SBO_HIP(hipStreamSynchronize(c->stream));                 // (the staging area is free again)
  return SBO_OK;
}

// The factorisation proper on stream `fs`: front end (mode 0: reversed symmetrised copy of invK -- alpha is made by the caller of
// this function from the matrix as given --; mode 1: K from the expanded distance), the panels, the finish, the fragment images.
template <typename T>
static int factor_chain_enqueue(sbo_ctx* c, const ModelWork& w, int mode, hipStream_t fs) {
  const ModelConst& mc = c->mc;
  const int n = mc.n, npad = mc.npad, q = mc.q, nb = npad / 16;
  const size_t nn = (size_t)n * n;
  double* dF = c->factor.F_mut();
  double* dalpha = c->factor.alpha_mut();
  if (n >= kBlockedFrom) {
    // blocked multi-workgroup factorisation: the single-workgroup loop is bound by the latency of its own updates
    if (mode == 0) {
      hipLaunchKernelGGL(k_invk_reverse, dim3((unsigned)((n + 31) / 32), (unsigned)((n + 31) / 32), q), dim3(256), 0, fs, n,
                         (const double*)w.W, w.work);
    } else {
      hipLaunchKernelGGL(k_chol_prep, dim3(256, q), dim3(256), 0, fs, mode, n, npad, mc.dpad, mc.d, (const double*)w.W,
                         (const double*)w.As64, (const double*)w.sq64, (const double*)w.rhs, mc, w.work, dF, dalpha);
    }
    {
      // one launch per panel: the pending update of the previous panel rides in the panel's own launch (k_chol_step)
      for (int kb = 0; kb < n; kb += kPB) {
        const int kw = std::min(kPB, n - kb);
        const int ncols = (n - kb - kw) + (mode ? kb + kw : 0);
        const int nA = std::max(1, ((ncols + 1) / 2 + 3) / 4);
        const int ti = kb > 0 ? (n - kb - kw + 31) / 32 : 0;
        const int nB = ti * ti + (mode && kb > 0 ? ((kb + 31) / 32) * ti : 0);
        hipLaunchKernelGGL(k_chol_step, dim3((unsigned)(nA + nB), q), dim3(256), 0, fs, w.work, dF, mode, n, kb, nA, ti, w.bad, w.Dg);
      }
    }
    hipLaunchKernelGGL(k_chol_finish, dim3(256, q), dim3(256), 0, fs, mode, n, npad, (const double*)w.rhs, w.work, dF, dalpha,
                       (const double*)w.Dg);
  } else {
    hipLaunchKernelGGL(k_model_build, dim3(q), dim3(1024), 0, fs, mode, n, npad, mc.dpad, mc.d, (const double*)w.W,
                       (const double*)w.As64, (const double*)w.sq64, (const double*)w.rhs, mc, w.work, dF, dalpha, w.bad);
  }
  const size_t ntri = (size_t)nb * (nb + 1) / 2;
  // (k_pack_factor writes every element of the images, zeros included; only the over-read padding needs clearing)
  SBO_HIP(hipMemsetAsync((T*)c->Fpk.p + (size_t)q * c->fpk_stride, 0, sizeof(T) * 512, fs));
  hipLaunchKernelGGL((k_pack_factor<T>), dim3((unsigned)std::min<size_t>((ntri * 256 + 255) / 256, 4096), q), dim3(256), 0, fs,
                     (const double*)dF, n, n, nn, nb, c->fpk_stride, (T*)c->Fpk.p);
  SBO_HIP(hipGetLastError());
  return SBO_OK;
}

// Device side of sbo_model_set.  host_invK may be NULL (the library factors K itself).  On success Fpk (dtype T), alpha
// (dtype T), the derived arrays As / sqA / Xn and the fp64 factor / alpha (sbo_ctx::factor: leading dimension n / npad
// until an append grows them) are in place.  One host synchronisation, at the end (the positive-definiteness verdict);
// when a K1b-capable grid is resident the axis bases of the new model are built meanwhile on the second stream.
template <typename T>
static int model_build_t(sbo_ctx* c, const double* const* host_invK /* q matrices, or nullptr */, const double* X_norm, const double* Y_norm) {
  const ModelConst& mc = c->mc;
  const int n = mc.n, npad = mc.npad, q = mc.q, nb = npad / 16;
  const size_t nn = (size_t)n * n;
  int rc;
  if (c->factor_pending) {                // (the previous model's deferred factor chain works in the buffers reused below)
    SBO_HIP(hipEventSynchronize(c->ev_factor));
    c->factor_pending = false;
  }
  c->invk_img_valid = false;
  c->invk_w_valid = false;
  c->factor_todo = false;
  ModelWork w;
  if ((rc = model_work(c, host_invK != nullptr, w))) return rc;
  if ((rc = c->factor.build(n, npad, q))) return rc;
  double* dalpha = c->factor.alpha_mut();
  if ((rc = model_prep_t<T>(c, X_norm, Y_norm, w))) return rc;
  bool eager_basis = false;
  // (r04) a caller's invK on a K1b-capable grid: the model's first sweep runs on interpolated node values (K1i, bilinear.hip), which
  // needs no bases -- they are made when the model is swept a second time
  const bool interp_first = bilinear_applicable(c) && c->opt.bilinear == 1 && host_invK != nullptr && n >= kBlockedFrom && c->opt.chol_async &&
                            !c->is_shadow && c->stream4 && std::is_same<T, double>::value && c->mc.npad % 16 == 0;
  if (bilinear_applicable(c) && !interp_first) {
    // the bases need X_norm only: next to the factorisation, on the second stream -- and ahead of the upload of invK
    // (4 MB at n = 512, ~0.15 ms of pageable copies the host sits in): their pivot loop is the longest chain of a model change
    SBO_HIP(hipEventRecord(c->ev[6], c->stream));
    SBO_HIP(hipStreamWaitEvent(c->stream2, c->ev[6], 0));
    if ((rc = bilinear_basis_enqueue(c, c->stream2, false))) return rc;
    eager_basis = true;
  }
  if (host_invK) {                        // (the reference keeps them as a list of q arrays: one copy each, no stacking on the host)
    for (int o = 0; o < q; ++o)
      SBO_HIP(hipMemcpyAsync(w.W + (size_t)o * nn, host_invK[o], sizeof(double) * nn, hipMemcpyHostToDevice, c->stream));
    c->invk_w_valid = std::is_same<T, double>::value && !c->is_shadow;
    c->invk_plain = w.W;
  }
  SBO_HIP(hipMemsetAsync(dalpha, 0, sizeof(double) * (size_t)q * npad, c->stream));
  SBO_HIP(hipMemsetAsync(w.bad, 0, sizeof(int) * q, c->stream));
  const int mode = host_invK ? 0 : 1;
  // A caller's invK on a K1b-capable grid: the GEMM posterior's tables take invK itself (k_pack_full), so the reverse
  // Cholesky factor is only needed by the O(n^2) kernels and by sbo_model_append -- it is built on stream4 and nobody waits
  // for it here (n = 512: 16 dependent panel launches, ~0.43 ms off the critical path of a model change).  Its launches are
  // not even enqueued here (the host needs ~0.1 ms for them): the next sweep does that while it waits for its own result
  // (model_factor_enqueue), a consumer of the factor before that enqueues and waits (factor_sync), and a model replaced
  // before anyone asked never factors at all.
  const bool deferred = mode == 0 && n >= kBlockedFrom && c->opt.chol_async && !c->is_shadow && (eager_basis || interp_first) && c->stream4 &&
                        std::is_same<T, double>::value;
  const size_t ntri = (size_t)nb * (nb + 1) / 2;
  c->fpk_stride = ntri * 4 * 64;
  if ((rc = ensure(c->Fpk, sizeof(T) * ((size_t)q * c->fpk_stride + 512)))) return rc;   // + padding: the K1g pipeline over-reads
  if ((rc = ensure(c->alpha, sizeof(T) * (size_t)q * npad))) return rc;
  if (n >= kBlockedFrom && mode == 0) {
    hipLaunchKernelGGL(k_invk_alpha, dim3((unsigned)((n + 3) / 4), q), dim3(256), 0, c->stream, n, npad, (const double*)w.W,
                       (const double*)w.rhs, dalpha);
    if (deferred) {
      if ((rc = ensure(c->invk_img, sizeof(double) * (size_t)q * npad * npad))) return rc;
      hipLaunchKernelGGL(k_pack_full, dim3((unsigned)std::min<size_t>(((size_t)nb * nb * 256 + 255) / 256, 4096), q), dim3(256), 0, c->stream,
                         (const double*)w.W, n, nb, (double*)c->invk_img.p);
      c->invk_img_valid = true;
      SBO_HIP(hipEventRecord(c->ev_w, c->stream));
      hipLaunchKernelGGL((k_cast_alpha<T>), dim3(16), dim3(256), 0, c->stream, (const double*)dalpha, npad, n, q, npad, (T*)c->alpha.p);
      SBO_HIP(hipGetLastError());
      c->factor_todo = true;
      // (the bases' records come back with this synchronisation; a K1i-first model has none to wait for -- r05: the host goes straight on
      // to enqueue the plan while these kernels run, ~30 us of a model change)
      if (eager_basis) {
        SBO_HIP(stream_wait(c, c->stream));
        SBO_HIP(stream_wait(c, c->stream2));
      }
      return SBO_OK;                      // (the verdict on invK comes with the factor: factor_sync)
    }
  }
  if ((rc = factor_chain_enqueue<T>(c, w, mode, c->stream))) return rc;
  hipLaunchKernelGGL((k_cast_alpha<T>), dim3(16), dim3(256), 0, c->stream, (const double*)dalpha, npad, n, q, npad, (T*)c->alpha.p);
  SBO_HIP(hipGetLastError());
  int* hbad = c->h_back->build_bad;
  SBO_HIP(hipMemcpyAsync(hbad, w.bad, sizeof(int) * q, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(stream_wait(c, c->stream));
  if (eager_basis) SBO_HIP(stream_wait(c, c->stream2));
  for (int o = 0; o < q; ++o)
    if (hbad[o]) return fail(SBO_E_INVALID, host_invK ? "invK is not positive definite" : "K + sn2 I is not positive definite");
  return SBO_OK;
}

// A grid that arrived after the model: the images of the caller's invK for the K1b tables are packed now, from the upload that
// still sits in the build workspace -- so that the GEMM posterior contracts with invK as given whatever the order of the calls.
int model_pack_invk(sbo_ctx* c) {
  if (c->invk_img_valid) return SBO_OK;
  if (!c->invk_w_valid) return fail(SBO_E_INVALID, "internal: the uploaded invK is gone");
  ModelWork w;
  int rc = model_work(c, true, w);
  if (rc) return rc;
  const int n = c->mc.n, npad = c->mc.npad, q = c->mc.q, nb = npad / 16;
  if ((rc = ensure(c->invk_img, sizeof(double) * (size_t)q * npad * npad))) return rc;
  hipLaunchKernelGGL(k_pack_full, dim3((unsigned)std::min<size_t>(((size_t)nb * nb * 256 + 255) / 256, 4096), q), dim3(256), 0, c->stream,
                     (const double*)w.W, n, nb, (double*)c->invk_img.p);
  SBO_HIP(hipGetLastError());
  c->invk_img_valid = true;
  return SBO_OK;
}

// The deferred factor chain of a caller's invK (see model_build_t): enqueued on stream4 behind the upload of invK (ev_w),
// ended by ev_factor; the positive-definiteness flags land in the pinned block for factor_sync.
int model_factor_enqueue(sbo_ctx* c) {
  if (!c->factor_todo) return SBO_OK;
  c->factor_todo = false;
  ModelWork w;
  int rc = model_work(c, true, w);
  if (rc) return rc;
  SBO_HIP(hipStreamWaitEvent(c->stream4, c->ev_w, 0));
  if ((rc = factor_chain_enqueue<double>(c, w, 0, c->stream4))) return rc;
  SBO_HIP(hipMemcpyAsync(c->h_back->factor_bad, w.bad, sizeof(int) * c->mc.q, hipMemcpyDeviceToHost, c->stream4));
  SBO_HIP(hipEventRecord(c->ev_factor, c->stream4));
  c->factor_pending = true;
  return SBO_OK;
}

// Re-pack Fpk / alpha of the model dtype from the resident fp64 factor (after an append; mc.n, mc.npad already updated).
template <typename T>
static int model_repack_t(sbo_ctx* c) {
  const ModelConst& mc = c->mc;
  const int n = mc.n, npad = mc.npad, q = mc.q, nb = npad / 16, cap = c->factor.ld();
  const size_t ntri = (size_t)nb * (nb + 1) / 2;
  int rc;
  c->fpk_stride = ntri * 4 * 64;
  if ((rc = ensure(c->Fpk, sizeof(T) * ((size_t)q * c->fpk_stride + 512)))) return rc;
  SBO_HIP(hipMemsetAsync(c->Fpk.p, 0, sizeof(T) * ((size_t)q * c->fpk_stride + 512), c->stream));
  hipLaunchKernelGGL((k_pack_factor<T>), dim3((unsigned)std::min<size_t>((ntri * 256 + 255) / 256, 4096), q), dim3(256), 0, c->stream,
                     c->factor.F(), n, cap, (size_t)cap * cap, nb, c->fpk_stride, (T*)c->Fpk.p);
  if ((rc = ensure(c->alpha, sizeof(T) * (size_t)q * npad))) return rc;
  hipLaunchKernelGGL((k_cast_alpha<T>), dim3(16), dim3(256), 0, c->stream, c->factor.alpha(), c->factor.a_ld(), n, q, npad, (T*)c->alpha.p);
  SBO_HIP(hipGetLastError());
  SBO_HIP(hipStreamSynchronize(c->stream));
  return SBO_OK;
}
int model_repack(sbo_ctx* c) { return c->dtype == SBO_F64 ? model_repack_t<double>(c) : model_repack_t<float>(c); }

// c->appendbuf: kvec [q][n] | kappa [q] | rho [q] | scratch [q][2 cap] | (s, k.alpha) [q][2] | bad [q]
struct AppendWork {
  double *k, *kappa, *rho, *scratch, *sk;
  int* bad;
};
static size_t append_layout(Carve cv, int n, int q, int cap, AppendWork& w) {
  cv.take(w.k, (size_t)q * n); cv.take(w.kappa, q); cv.take(w.rho, q);
  cv.take(w.scratch, 2 * (size_t)q * cap); cv.take(w.sk, 2 * (size_t)q);
  cv.take(w.bad, q);
  return cv.off;
}

int ResidentFactor::build(int n, int npad, int q) {
  ld_ = n, a_ld_ = npad;
  if (const int rc = ensure(F_, sizeof(double) * (size_t)q * n * n)) return rc;
  return ensure(alpha_, sizeof(double) * (size_t)q * npad);
}

int ResidentFactor::reserve(sbo_ctx* c, int rows) {
  const int n = c->mc.n, q = c->mc.q;
  if (n + rows <= ld_ && a_ld_ == ld_) return SBO_OK;
  int rc;
  const int cap = std::min(SBO_MAX_N, std::max((c->mc.npad + 256 + 127) / 128 * 128, (n + rows + 127) / 128 * 128));
  if (n + rows > cap) return fail(SBO_E_UNSUPPORTED, "model is at its capacity: rebuild it with sbo_model_set");
  DevBuf F2, a2;
  if ((rc = ensure(F2, sizeof(double) * (size_t)q * cap * cap))) return rc;
  if ((rc = ensure(a2, sizeof(double) * (size_t)q * cap))) return rc;
  hipError_t e = hipMemsetAsync(F2.p, 0, sizeof(double) * (size_t)q * cap * cap, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(a2.p, 0, sizeof(double) * (size_t)q * cap, c->stream);
  for (int o = 0; o < q && e == hipSuccess; ++o) {
    e = hipMemcpy2DAsync((double*)F2.p + (size_t)o * cap * cap, sizeof(double) * cap, F() + (size_t)o * ld_ * ld_, sizeof(double) * ld_,
                         sizeof(double) * n, n, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync((double*)a2.p + (size_t)o * cap, alpha() + (size_t)o * a_ld_, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return hip_fail(e, "growing the resident factor");
  F_ = std::move(F2);
  alpha_ = std::move(a2);
  ld_ = a_ld_ = cap;
  return SBO_OK;
}

int ResidentFactor::spare_ensure_zeroed(sbo_ctx* c) {
  const size_t fbytes = sizeof(double) * (size_t)c->mc.q * ld_ * ld_, abytes = sizeof(double) * (size_t)c->mc.q * a_ld_;
  if (const int rc = ensure(Fspare_, fbytes)) return rc;
  if (const int rc = ensure(aspare_, abytes)) return rc;
  SBO_HIP(hipMemsetAsync(Fspare_.p, 0, fbytes, c->stream));
  SBO_HIP(hipMemsetAsync(aspare_.p, 0, abytes, c->stream));
  return SBO_OK;
}

// The verdict of a staged append (its one host wait): the first output whose flag in `dbad` [q] is set names the error, msg(o, flag).
template <class Msg>
static int append_verdict(sbo_ctx* c, const int* dbad, Msg&& msg) {
  const int q = c->mc.q;
  int hbad[kMaxQ] = {};
  SBO_HIP(hipMemcpyAsync(hbad, dbad, sizeof(int) * q, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipStreamSynchronize(c->stream));
  for (int o = 0; o < q; ++o)
    if (hbad[o]) return fail(SBO_E_INVALID, msg(o, hbad[o]));
  return SBO_OK;
}
ModelUpdate model_update_staged(const sbo_ctx* c, int rows, int index) {
  ModelUpdate u;
  u.rows = rows, u.index = index, u.ld = c->factor.ld(), u.serial = c->model_serial;
  return u;
}

int model_append_stage(sbo_ctx* c, const double* x_norm_new, const double* y_norm_new, ModelUpdate& u) {
  const ModelConst& mc = c->mc;
  const int n = mc.n, d = mc.d, q = mc.q;
  // cross-covariances of the new point with the expanded distance of the reference (GP_Safe.py:115-119, 166)
  std::vector<double> kvec((size_t)q * n);
  double kappa[kMaxQ], rho[kMaxQ];
  for (int o = 0; o < q; ++o) {
    double bsq = 0.0, bvec[kMaxD];
    for (int a = 0; a < d; ++a) { bvec[a] = x_norm_new[a] * mc.vinv[o][a]; bsq += bvec[a] * bvec[a]; }
    for (int j = 0; j < n; ++j) {
      double dot = 0.0, asq = 0.0;
      for (int a = 0; a < d; ++a) {
        const double v = c->h_Xnorm[(size_t)j * d + a] * mc.vinv[o][a];
        dot += v * bvec[a];
        asq += v * v;
      }
      kvec[(size_t)o * n + j] = mc.sf2[o] * std::exp(-0.5 * ((-2.0 * dot + asq) + bsq));
    }
    kappa[o] = mc.sf2[o] + mc.sn2[o];
    rho[o] = y_norm_new[o] - mc.mp[o];
  }
  int rc;
  if ((rc = c->factor.reserve(c, 1))) return rc;
  const int cap = c->factor.ld();
  AppendWork w;
  if ((rc = carve(c->appendbuf, [&](Carve cv) { return append_layout(cv, n, q, cap, w); }))) return rc;
  SBO_HIP(hipMemcpyAsync(w.k, kvec.data(), sizeof(double) * (size_t)q * n, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(w.kappa, kappa, sizeof(double) * q, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(w.rho, rho, sizeof(double) * q, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemsetAsync(w.bad, 0, sizeof(int) * q, c->stream));
  hipLaunchKernelGGL(k_model_append, dim3(q), dim3(1024), 0, c->stream, n, cap, c->factor.F(), c->factor.alpha(), (const double*)w.k,
                     (const double*)w.kappa, w.scratch, w.sk, w.bad);
  SBO_HIP(hipGetLastError());
  if ((rc = append_verdict(c, w.bad, [](int, int) { return "appended observation makes K singular (duplicate point without noise?)"; }))) return rc;
  u = model_update_staged(c, 1);
  u.rho = w.rho; u.scratch = w.scratch; u.sk = w.sk;
  return SBO_OK;
}

// c->appendbuf for a block of k rows (kp = k rounded up to kAppColBlock):
//   Xall [n + k][d] | rho [q][kp] | B, T, U [q][n][kp] | Z, S, G [q][kp][kp] | g, w [q][kp] | bad [q]
struct AppendBlockWork {
  double *Xall, *rho, *B, *T, *U, *Z, *S, *G, *g, *w;
  int* bad;
};
static size_t append_block_layout(Carve cv, int n, int d, int q, int k, int kp, AppendBlockWork& w) {
  const size_t nk = (size_t)q * n * kp, kk = (size_t)q * kp * kp;
  cv.take(w.Xall, (size_t)(n + k) * d); cv.take(w.rho, (size_t)q * kp);
  cv.take(w.B, nk); cv.take(w.T, nk); cv.take(w.U, nk);
  cv.take(w.Z, kk); cv.take(w.S, kk); cv.take(w.G, kk);
  cv.take(w.g, (size_t)q * kp); cv.take(w.w, (size_t)q * kp);
  cv.take(w.bad, q);
  return cv.off;
}
static inline int append_block_kp(int k) { return (k + kAppColBlock - 1) / kAppColBlock * kAppColBlock; }

// Rows n .. n + k - 1: Xall holds the model's observations followed by the k new rows (normalised, fp64), rho [q][kp] = y_norm_new - mp.
int model_append_block_stage(sbo_ctx* c, int k, const double* x_norm_new, const double* y_norm_new, ModelUpdate& u) {
  const ModelConst& mc = c->mc;
  const int n = mc.n, d = mc.d, q = mc.q, kp = append_block_kp(k);
  int rc;
  if ((rc = c->factor.reserve(c, k))) return rc;
  const int cap = c->factor.ld();
  AppendBlockWork w;
  if ((rc = carve(c->appendbuf, [&](Carve cv) { return append_block_layout(cv, n, d, q, k, kp, w); }))) return rc;
  std::vector<double> hrho((size_t)q * kp, 0.0);
  for (int o = 0; o < q; ++o)
    for (int r = 0; r < k; ++r) hrho[(size_t)o * kp + r] = y_norm_new[(size_t)r * q + o] - mc.mp[o];
  SBO_HIP(hipMemcpyAsync(w.Xall, c->h_Xnorm.data(), sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(w.Xall + (size_t)n * d, x_norm_new, sizeof(double) * (size_t)k * d, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(w.rho, hrho.data(), sizeof(double) * (size_t)q * kp, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemsetAsync(w.bad, 0, sizeof(int) * q, c->stream));
  const double* dF = c->factor.F();
  const long long cells = (long long)(n + kp) * kp;
  with_dpad(mc.dpad, [&](auto D) {
    hipLaunchKernelGGL((k_append_cross<D()>), dim3((unsigned)std::min<long long>((cells + 255) / 256, 1024), q), dim3(256), 0, c->stream, mc, n, k,
                       kp, (const double*)w.Xall, w.B, w.Z);
  });
  hipLaunchKernelGGL(k_append_t, dim3((unsigned)((n + kAppWaves * kAppRows - 1) / (kAppWaves * kAppRows)), q), dim3(64 * kAppWaves), 0, c->stream,
                     n, cap, kp, dF, (const double*)w.B, w.T);
  hipLaunchKernelGGL(k_append_u, dim3((unsigned)((n + 63) / 64), (unsigned)(kp / kAppColBlock), q), dim3(64), 0, c->stream, n, cap, kp, dF,
                     (const double*)w.T, w.U);
  hipLaunchKernelGGL(k_append_s, dim3((unsigned)(kp / kAppSRows + 1), q), dim3(64), 0, c->stream, n, c->factor.a_ld(), kp, (const double*)w.B,
                     (const double*)w.U, (const double*)w.Z, c->factor.alpha(), w.S, w.g);
  hipLaunchKernelGGL(k_append_chol, dim3(q), dim3(256), 0, c->stream, k, kp, (const double*)w.S, (const double*)w.g, (const double*)w.rho, w.G,
                     w.w, w.bad);
  SBO_HIP(hipGetLastError());
  rc = append_verdict(c, w.bad, [](int o, int flag) {
    return "appended block makes K singular: output " + std::to_string(o) + ", row " + std::to_string(flag - 1) +
           " of the block has a Schur pivot that is not > 0 (duplicate point without noise?)";
  });
  if (rc) return rc;
  u = model_update_staged(c, k);
  u.U = w.U; u.G = w.G; u.w = w.w;
  return SBO_OK;
}

// A removal writes the factor and alpha without observation `index` into the zeroed spare pair (the padding and everything right of the
// diagonal stay zero), which is adopted once every launch has been accepted -- until then nothing of the model has changed.
int model_update_commit(sbo_ctx* c, const ModelUpdate& u) {
  ResidentFactor& f = c->factor;
  if (u.serial != c->model_serial || u.ld != f.ld() || u.rows == 0)
    return fail(SBO_E_INVALID, "internal: the model changed between the staging of an update and its commit");
  const int n = c->mc.n, q = c->mc.q, cap = f.ld(), a_ld = f.a_ld();
  if (u.rows < 0) {
    if (const int rc = f.spare_ensure_zeroed(c)) return rc;
    if (const int rc = ensure(c->removebuf, sizeof(double) * (size_t)q * (3 * (size_t)cap + 1))) return rc;
    hipLaunchKernelGGL(k_model_remove_coef, dim3(q), dim3(256), 0, c->stream, n, cap, a_ld, u.index, f.F(), f.alpha(), (double*)c->removebuf.p);
    hipLaunchKernelGGL(k_model_remove, dim3((unsigned)((n - 1 + kRemoveStrip - 1) / kRemoveStrip), q), dim3(64), 0, c->stream, n, cap, a_ld,
                       u.index, f.F(), f.alpha(), (const double*)c->removebuf.p, f.spare_F(), f.spare_alpha());
  } else if (u.U) {
    const int k = u.rows, kp = append_block_kp(k);
    hipLaunchKernelGGL(k_append_commit, dim3((unsigned)((cap + 63) / 64), q), dim3(64), 0, c->stream, n, cap, a_ld, k, kp, f.F_mut(), f.alpha_mut(),
                       u.U, u.G, u.w);
  } else {
    hipLaunchKernelGGL(k_model_append_commit, dim3(q), dim3(1024), 0, c->stream, n, cap, f.F_mut(), f.alpha_mut(), u.rho, u.scratch, u.sk);
  }
  SBO_HIP(hipGetLastError());
  if (u.rows < 0) f.adopt_spare();
  c->invk_img_valid = false;                                   // (the images of the caller's invK follow no update)
  c->invk_w_valid = false;
  return SBO_OK;
}

// sbo_model_loo's device side: the two launches, one copy into the pinned landing area, one wait.  Nothing of the model, the plans
// or the caches is written; the scratch is kept for the next call (a grown factor grows it).
int model_loo(sbo_ctx* c, double b, bool arrays, const unsigned char** host) {
  const int n = c->mc.n, q = c->mc.q, cap = c->factor.ld(), a_ld = c->factor.a_ld();
  const int chunks = (n + kLooRows - 1) / kLooRows, strips = (n + kLooStrip - 1) / kLooStrip;
  const size_t head = sizeof(LooSummary) * kMaxQ, nq = sizeof(double) * (size_t)n * q;
  const size_t bytes = head + (arrays ? 2 * nq : 0);
  int rc;
  if ((rc = ensure(c->loo.part, sizeof(double) * (size_t)q * ((cap + kLooRows - 1) / kLooRows) * cap))) return rc;
  if ((rc = ensure(c->loo.out, head + 2 * sizeof(double) * (size_t)cap * q))) return rc;
  if (c->loo.h_out.bytes < bytes) {
    c->loo.h_out.reset();
    const size_t want = head + 2 * sizeof(double) * (size_t)cap * q;
    if (hipHostMalloc(&c->loo.h_out.p, want, hipHostMallocDefault) != hipSuccess) return fail(SBO_E_HIP, "hipHostMalloc (leave-one-out results)");
    c->loo.h_out.bytes = want;
  }
  unsigned char* dout = (unsigned char*)c->loo.out.p;
  hipLaunchKernelGGL(k_model_loo_colsq, dim3((unsigned)strips, (unsigned)chunks, (unsigned)q), dim3(64), 0, c->stream, n, cap, chunks,
                     c->factor.F(), (double*)c->loo.part.p);
  hipLaunchKernelGGL(k_model_loo_finish, dim3(q), dim3(1024), 0, c->stream, n, q, cap, a_ld, chunks, b, c->factor.F(),
                     c->factor.alpha(), (const double*)c->loo.part.p, arrays ? (double*)(dout + head) : (double*)nullptr,
                     arrays ? (double*)(dout + head + nq) : (double*)nullptr, (LooSummary*)dout);
  SBO_HIP(hipGetLastError());
  SBO_HIP(hipMemcpyAsync(c->loo.h_out.p, dout, bytes, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(stream_wait(c, c->stream));
  *host = (const unsigned char*)c->loo.h_out.p;
  return SBO_OK;
}

int model_build(sbo_ctx* c, const double* const* host_invK, const double* X_norm, const double* Y_norm) {
  const int rc = c->dtype == SBO_F64 ? model_build_t<double>(c, host_invK, X_norm, Y_norm) : model_build_t<float>(c, host_invK, X_norm, Y_norm);
  if (rc != SBO_OK) drain_streams(c);     // (the bases may still be running on the second stream)
  return rc;
}

}  // namespace sbo
