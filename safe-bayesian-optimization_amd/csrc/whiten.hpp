// whiten.hpp -- what the point calls on the resident fp64 factor M (M^T M = inv(K + sn2 I)) share: sbo_batch_select (batch.hip),
// sbo_expander_gain (expander.hip), sbo_sample_paths (paths.hip), sbo_posterior_joint (joint.hip).  They promise the same bits from call
// to call and across the model's history; every rounding sequence they have in common is stated here once.
//   OutParams, out_params      the constants of one output, by value inside the callers' argument blocks
//   rbf_scale, rbf_k           a raw point in the output's scaled coordinates; the kernel with the reference's expanded distance
//   k_obs_prep                 the observations in the scaled coordinates of gridDim.y slots
//   whiten_tile                t = M k_x for P points of a workgroup, in an LDS image
//   factor_lower_mv / _upper_mv   M x and M^T t by one workgroup
// What only the three calls with a matrix-core stage share -- the residual kernel, the stage-1 body, their resident observations and the
// tile steps on the whitened vectors -- is in slab_tiles.hpp.
// k_model_append (model.hip) sums with s += a * b, not fma, and guard.hip, lipschitz.hip, refine.hip and sets_recheck.inc.hpp keep the
// data in other layouts: they share the kernel expression, not these sequences, and have pins of their own.
#pragma once
#include "internal.hpp"
#include "device_common.hpp"

namespace sbo {

constexpr int kWhitenThreads = 1024;             // whiten_tile: P points x 1024 / P row lanes
constexpr int kWhitenRows = 4;                   // ... rows of M per row lane and step
constexpr int kFactorMvThreads = 1024;           // factor_lower_mv / factor_upper_mv: the workgroup they are written for

// points per workgroup of whiten_tile: the image [n][P (+ 1)] stays within 128 (144) KiB up to SBO_MAX_N
inline int whiten_tier(int n) { return n <= 512 ? 32 : n <= 1024 ? 16 : 8; }

struct OutParams {                               // one output of the model, by value (kernarg segment)
  int d, pad;
  double X_mean[kMaxD], X_std[kMaxD], vinv[kMaxD];     // axes >= d: 0, 1, 0 (never read)
  double sf2, sn2, mp;
};
inline OutParams out_params(const ModelConst& mc, int o) {
  OutParams p{};
  p.d = mc.d;
  for (int a = 0; a < kMaxD; ++a) {
    p.X_mean[a] = a < mc.d ? mc.X_mean[a] : 0.0;
    p.X_std[a] = a < mc.d ? mc.X_std[a] : 1.0;
    p.vinv[a] = a < mc.d ? mc.vinv[o][a] : 0.0;
  }
  p.sf2 = mc.sf2[o];
  p.sn2 = mc.sn2[o];
  p.mp = mc.mp[o];
  return p;
}

// scaled coordinates b = ((x - X_mean) / X_std) ell^-1/2 of a raw point and their sum of squares, axis order (GP_Safe.py:115-116)
template <int D>
__device__ __forceinline__ double rbf_scale(const OutParams& op, const double* __restrict__ raw, bool on, double* b) {
  double bsq = 0.0;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    b[a] = (on && a < op.d) ? ((raw[a] - op.X_mean[a]) / op.X_std[a]) * op.vinv[a] : 0.0;
    bsq += b[a] * b[a];
  }
  return bsq;
}
// sf2 exp(-1/2 dist) with the expanded distance (-2 a.b + |a|^2) + |b|^2 of the reference (GP_Safe.py:119), as sbo_model_append forms
// it; a: the observation (registers, LDS or global memory)
template <int D>
__device__ __forceinline__ double rbf_k(double sf2, const double* a, double asq, const double* b, double bsq) {
  double dot = 0.0;
#pragma unroll
  for (int t = 0; t < D; ++t) dot += a[t] * b[t];
  return sf2 * exp(-0.5 * ((-2.0 * dot + asq) + bsq));
}

// ---- the observations in the scaled coordinates of every slot: As [slot][n][D], sq [slot][n] ------------------------------------------
// (static: each file that includes this header instantiates and registers a copy of its own)
struct PrepArgs {                                // by value (kernarg segment)
  int n, d;
  double vinv[kMaxQ][kMaxD];                     // [slot]
};
template <int D>
static __global__ __launch_bounds__(256) void k_obs_prep(const PrepArgs A, const double* __restrict__ Xn /* [n][d] */, double* __restrict__ As,
                                                         double* __restrict__ sq) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, slot = blockIdx.y;
  if (i >= A.n) return;
  double s = 0.0;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const double v = a < A.d ? Xn[(size_t)i * A.d + a] * A.vinv[slot][a] : 0.0;
    As[((size_t)slot * A.n + i) * D + a] = v;
    s += v * v;
  }
  sq[(size_t)slot * A.n + i] = s;
}
template <int D>
inline hipError_t obs_prep(hipStream_t st, int n, const OutParams* op, int slots, const double* Xn, double* As, double* sq) {
  PrepArgs P{};
  P.n = n;
  P.d = op[0].d;
  for (int s = 0; s < slots; ++s)
    for (int a = 0; a < kMaxD; ++a) P.vinv[s][a] = op[s].vinv[a];
  hipLaunchKernelGGL((k_obs_prep<D>), dim3((unsigned)((n + 255) / 256), (unsigned)slots), dim3(256), 0, st, P, Xn, As, sq);
  return hipGetLastError();
}

// ---- t = M k_x for the P points of a workgroup of kWhitenThreads threads --------------------------------------------------------------
// Thread (p, r) = (tid mod P, tid / P); b, bsq: point p in scaled coordinates (rbf_scale), `on`: it exists.  K(X, tile) is formed once
// into LDS as sK[j * ldk + p] (ldk >= P); the rows of t = M k_x are taken in blocks of (1024 / P) kWhitenRows rows from the bottom up, a
// thread owning kWhitenRows consecutive rows of its point -- row i needs k[0 .. i] only, so a finished block's t overwrites the k entries
// nobody reads any more --, every row sum in column order.  Nothing above the diagonal of M is read.  On return (behind a barrier)
// sK[j * ldk + p] = t_p[j], j < n; zeros for a point that does not exist.
template <int D>
__device__ __forceinline__ void whiten_tile(double* sK, int ldk, int P, int n, double sf2, const double* As, const double* sq,
                                            const double* M, int ld, const double* b, double bsq, bool on) {
  const int tid = threadIdx.x, p = tid % P, r = tid / P, R = kWhitenThreads / P;
  for (int j = r; j < n; j += R) {
    double a[D];
#pragma unroll
    for (int t = 0; t < D; ++t) a[t] = As[(size_t)j * D + t];
    sK[j * ldk + p] = on ? rbf_k<D>(sf2, a, sq[j], b, bsq) : 0.0;
  }
  __syncthreads();
  const int RB = R * kWhitenRows;
  for (int blk = (n + RB - 1) / RB - 1; blk >= 0; --blk) {
    const int i0 = blk * RB + r * kWhitenRows, cnt = min(kWhitenRows, n - i0);      // this thread's rows i0 .. i0 + cnt - 1 (cnt <= 0: none)
    double t[kWhitenRows];
#pragma unroll
    for (int u = 0; u < kWhitenRows; ++u) t[u] = 0.0;
    if (cnt > 0) {
      const double* row[kWhitenRows];
#pragma unroll
      for (int u = 0; u < kWhitenRows; ++u) row[u] = M + (size_t)min(i0 + u, n - 1) * ld;    // (a missing row reads the last one; its sum is dropped)
#pragma unroll 4
      for (int j = 0; j <= i0; ++j) {
        const double kj = sK[j * ldk + p];
#pragma unroll
        for (int u = 0; u < kWhitenRows; ++u) t[u] = fma(row[u][j], kj, t[u]);
      }
#pragma unroll
      for (int u = 1; u < kWhitenRows; ++u)
        if (u < cnt)
          for (int j = i0 + 1; j <= i0 + u; ++j) t[u] = fma(row[u][j], sK[j * ldk + p], t[u]);
    }
    __syncthreads();                                    // (every k entry of this block of rows has been read)
#pragma unroll
    for (int u = 0; u < kWhitenRows; ++u)
      if (u < cnt) sK[(i0 + u) * ldk + p] = t[u];
  }
  __syncthreads();
}

// ---- M x and M^T t by one workgroup of kFactorMvThreads threads; both orders depend on n alone ----------------------------------------
// out[i] = sum_{j <= i} M[i][j] x[j], i < n: a wave per row, lanes along the row, butterfly.  Rows n .. rows - 1 of out become zeros.
__device__ __forceinline__ void factor_lower_mv(const double* M, int ld, int n, const double* x, double* out, int rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < rows; i += kFactorMvThreads / 64) {
    double s = 0.0;
    if (i < n)
      for (int j = lane; j <= i; j += 64) s = fma(M[(size_t)i * ld + j], x[j], s);
    s = wave_sum(s);
    if (lane == 0) out[i] = s;
  }
}
// out(j, sum_{i >= j} M[i][j] t[i]), j < n: a thread per column, the rows i = j .. n - 1 in order (lanes read consecutive columns of a row)
template <class Out>
__device__ __forceinline__ void factor_upper_mv(const double* M, int ld, int n, const double* t, Out&& out) {
  for (int j = threadIdx.x; j < n; j += kFactorMvThreads) {
    double s = 0.0;
#pragma unroll 8
    for (int i = j; i < n; ++i) s = fma(M[(size_t)i * ld + j], t[i], s);
    out(j, s);
  }
}

}  // namespace sbo
