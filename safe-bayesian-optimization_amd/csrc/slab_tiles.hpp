// slab_tiles.hpp -- what sbo_expander_gain (expander.hip), sbo_sample_paths (paths.hip) and sbo_posterior_joint (joint.hip) share beyond
// whiten.hpp: the three calls stage rows in LDS slabs and multiply them with MM<double>.  Each step is stated here once; a caller
// brings what is its own as an argument or a callable, and no step asks which call it serves.  sbo_batch_select has none of these
// stages and does not include this header (k_whiten_resid has internal linkage: every file that includes it compiles a copy).
//   k_whiten_resid           the whitened residuals w = M (y - mp) of gridDim.x slots
//   whiten_stage1, whiten_stage1_launch
//                            the body of a stage-1 kernel around its own per-point sums (k_exp_stage1, k_joint_stage1), and its launch
//   ObsResident              the observations of a call in its scratch: the carve entries, the uploads, k_obs_prep and k_whiten_resid
//   kSlabK, slab_pos_a / _b, slab_col, slab_mfma   the LDS images of a K-slab of MM<double> operands and the multiply step over one
//   tile64_product, tile64_row / _col / _stage_row, point_image
//                            the 64 x 64 tile of a product of rows of two row-major matrices (k_exp_pairs, k_joint_cov, k_joint_update),
//                            where an accumulator element lies in it, and the |.|^2 / coordinates image of a tile's points
//   Tile128Lds, tile128_step, tile128_arg_best, tile128_store_partial
//                            the 128 rows x Spad columns tile (k_path_main, k_joint_draw): one slab, the per-column arg-best of a tile
//   partials_merge           the (workgroup, column) partials -> index[] / value[] (k_path_finish, k_joint_finish)
//   clear_index_value        the host's cleared index / value pair
// (spad_of and with_spad stand beside with_dpad in internal.hpp.)
#pragma once
#include <limits>
#include <string>
#include "whiten.hpp"

namespace sbo {

constexpr int kSlabK = 32;                       // columns of the K axis of one LDS slab
constexpr int kSlabBlk = 16 * kSlabK;            // doubles of one 16-row block of a slab image
constexpr int kSlabBlkA = kSlabBlk + 16;         // ... and the distance between two blocks of the 128-row tile's A image (the four
                                                 // blocks a wave writes at once land in two bank halves)
constexpr int kTileThreads = 256;                // the workgroup both tiles are written for: 4 waves
constexpr int kMergeThreads = 1024;              // partials_merge: SBO_MAX_PATHS columns x 16 parts of the workgroups
static_assert(kSlabK == 32 && kTileThreads == 256, "a 64-row tile is staged 8 columns per thread, a 128-row tile 16 columns per thread");

// ---- the whitened residuals w = M (y - mp) of gridDim.x slots: w [slot][ldt] -------------------------------------------------------------
// One workgroup per slot (factor_lower_mv), zeros from n to ldt.  With t_p = M k_p the mean is mp + k_p . alpha = mp + t_p . w (alpha =
// M^T M (y - mp)): a call rests on the factor and the data alone, so whatever leaves the first n rows of the factor as they are -- an
// append and the removal of that row -- leaves the call's bits as they are.
struct ResidArgs {                               // by value (kernarg segment)
  int n, ld, ldt, q;                             // observations, leading dimension of the factor, of w, outputs of the model
  int out[kMaxQ];                                // [slot]: the output
  double mp[kMaxQ];                              // [slot]
};
static __global__ __launch_bounds__(kFactorMvThreads) void k_whiten_resid(const ResidArgs A, const double* __restrict__ Yn /* [n][q] */,
                                                                          const double* __restrict__ F, double* __restrict__ w) {
  __shared__ double sy[SBO_MAX_N];
  const int n = A.n, ld = A.ld, slot = blockIdx.x, o = A.out[slot];
  for (int j = threadIdx.x; j < n; j += kFactorMvThreads) sy[j] = Yn[(size_t)j * A.q + o] - A.mp[slot];
  __syncthreads();
  factor_lower_mv(F + (size_t)o * ld * ld, ld, n, sy, w + (size_t)slot * A.ldt, A.ldt);
}

// ---- stage 1 of a call that multiplies whitened vectors: t = M k_p per point, written out as rows -------------------------------------
// A workgroup of kWhitenThreads threads owns P points of a list of m (whiten_tile on an image sK [n][P + 1]: the write-out below reads
// columns).  Of point i, record rec0 + i: the scaled coordinates and their squares go to bs / bsq_out; behind whiten_tile one thread
// per point runs per_point(rec, i, column) for the caller's own sums down its column sK[j * (P + 1) + column], j < n; the image is
// then written out as T [rec][ldt], lanes along a row, zeros from n to ldt.
template <int D, class PerPoint>
__device__ __forceinline__ void whiten_stage1(double* sK, int P, int n, const OutParams& op, const double* As, const double* sq, const double* M,
                                              int ld, const double* __restrict__ pts, long long m, size_t rec0, double* __restrict__ T, int ldt,
                                              double* __restrict__ bs, double* __restrict__ bsq_out, PerPoint&& per_point) {
  const int tid = threadIdx.x, ldk = P + 1;
  const long long i = (long long)blockIdx.x * P + tid % P;
  const bool on = i < m;
  const size_t rec = rec0 + (size_t)(on ? i : 0);
  double b[D];
  const double bsq = rbf_scale<D>(op, pts + (size_t)(on ? i : 0) * op.d, on, b);
  if (tid < P && on) {                                  // (tid % P == tid)
    bsq_out[rec] = bsq;
#pragma unroll
    for (int t = 0; t < D; ++t) bs[rec * D + t] = b[t];
  }
  whiten_tile<D>(sK, ldk, P, n, op.sf2, As, sq, M, ld, b, bsq, on);
  if (tid < P && on) per_point(rec, i, tid);
  for (int e = tid; e < P * ldt; e += kWhitenThreads) {
    const int pp = e / ldt, j = e - pp * ldt;
    const long long ii = (long long)blockIdx.x * P + pp;
    if (ii < m) T[(rec0 + (size_t)ii) * ldt + j] = j < n ? sK[j * ldk + pp] : 0.0;
  }
}
// the launch of a stage-1 kernel over m points: P = whiten_tier(n) points per workgroup, the dynamic LDS of its image
constexpr size_t kWhitenS1Lds = 144 * 1024;      // whiten_tile's image [n][P + 1], P = whiten_tier(n): full at SBO_MAX_N
struct Stage1Launch {
  int P;
  unsigned blocks;
  size_t lds;
};
template <class Kernel>
inline int whiten_stage1_launch(Kernel* kernel, const char* call, int n, long long m, Stage1Launch& L) {
  const int P = whiten_tier(n);
  L = Stage1Launch{P, (unsigned)((m + P - 1) / P), sizeof(double) * (size_t)n * (P + 1)};
  if (L.lds > kWhitenS1Lds) return fail(SBO_E_UNSUPPORTED, std::string(call) + ": the model is too large");      // (n <= SBO_MAX_N: never)
  SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWhitenS1Lds));
  return SBO_OK;
}

// ---- the observations of a call, resident in its scratch -------------------------------------------------------------------------------
// X_norm [n][d] | Y_norm [n][q] | the scaled observations As [slots][n][D] and their squares sq [slots][n] | w [slots][ldt] (ldt = 0:
// the call has no w).  take() inside the caller's Carve layout; upload() the two copies from the context's host blocks; prepare() the
// kernels behind them.
struct ObsResident {
  double *Xn, *Yn, *As, *sq, *w;
  void take(Carve& cv, const ModelConst& mc, size_t slots, int ldt) {
    cv.take(Xn, (size_t)mc.n * mc.d);
    cv.take(Yn, (size_t)mc.n * mc.q);
    cv.take(As, slots * mc.n * mc.dpad);
    cv.take(sq, slots * mc.n);
    cv.take(w, slots * ldt);
  }
  hipError_t upload(sbo_ctx* c, hipStream_t st) const {
    const ModelConst& mc = c->mc;
    const hipError_t e = hipMemcpyAsync(Xn, c->h_Xnorm.data(), sizeof(double) * (size_t)mc.n * mc.d, hipMemcpyHostToDevice, st);
    return e != hipSuccess ? e : hipMemcpyAsync(Yn, c->h_Ynorm.data(), sizeof(double) * (size_t)mc.n * mc.q, hipMemcpyHostToDevice, st);
  }
  // As, sq of every slot (op [slots]) and, for a call with w, w of the slots' outputs out [slots]
  template <int D>
  int prepare(sbo_ctx* c, hipStream_t st, const OutParams* op, const int* out, int slots, int ldt) const {
    const ModelConst& mc = c->mc;
    SBO_HIP(obs_prep<D>(st, mc.n, op, slots, Xn, As, sq));
    if (!ldt) return SBO_OK;
    ResidArgs R{};
    R.n = mc.n;
    R.ld = c->factor.ld();
    R.ldt = ldt;
    R.q = mc.q;
    for (int s = 0; s < slots; ++s) {
      R.out[s] = out[s];
      R.mp[s] = op[s].mp;
    }
    hipLaunchKernelGGL(k_whiten_resid, dim3((unsigned)slots), dim3(kFactorMvThreads), 0, st, R, (const double*)Yn, c->factor.F(), w);
    SBO_HIP(hipGetLastError());
    return SBO_OK;
  }
};

// ---- a K-slab of MM<double> operands in LDS ----------------------------------------------------------------------------------------
// Per block of 16 rows (points, or paths) and k-step of 4 columns: the A side in MM<double>'s packed order (a lane's four row groups
// contiguous: one 32-byte read), the B side as [k-slot][row] (lane l reads element l).  Where column k of row r goes inside its block's
// image -- on the A side MM<double>::pack_pos(r & 15, k & 3, k >> 2) --, and how far column k + e, e < 16, lies behind a k that is a
// multiple of 4.
__device__ __forceinline__ int slab_pos_a(int r, int k) { return (k >> 2) * 64 + (k & 3) * 16 + (r & 3) * 4 + ((r & 15) >> 2); }
__device__ __forceinline__ int slab_pos_b(int r, int k) { return (k >> 2) * 64 + (k & 3) * 16 + (r & 15); }
__device__ __forceinline__ constexpr int slab_col(int e) { return (e >> 2) * 64 + (e & 3) * 16; }
// acc[a][c] += (block a of sA) x (block c of sB) over the slab; strideA / strideB: doubles between two blocks of an image
template <int NA, int NB>
__device__ __forceinline__ void slab_mfma(const double* sA, int strideA, const double* sB, int strideB, int lane, d4_t (&acc)[NA][NB]) {
#pragma unroll
  for (int kk = 0; kk < kSlabK / 4; ++kk) {
    d4_t fa[NA];
    double fb[NB];
#pragma unroll
    for (int a = 0; a < NA; ++a) fa[a] = MM<double>::load_a(sA + a * strideA, lane, kk);
#pragma unroll
    for (int c = 0; c < NB; ++c) fb[c] = sB[c * strideB + kk * 64 + lane];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int c = 0; c < NB; ++c) acc[a][c] = MM<double>::mfma(fa[a], fb[c], acc[a][c]);
  }
}

// ---- the 64 x 64 tile of (rows of one matrix) . (rows of another), kTileThreads threads ------------------------------------------------
// The A side's rows are the tile's rows, the B side's its columns.  Wave w owns rows 32 (w >> 1) .. + 31 and columns 32 (w & 1) .. + 31
// as 2 x 2 accumulators: acc[a][c][t] of lane l is the element (tile64_row(a, t), tile64_col(c)), the D layout of the 4x4x4 form
// (device_common.hpp).  Thread t stages columns 8 (t & 3) .. + 7 of row tile64_stage_row() of either side per slab.
__device__ __forceinline__ int tile64_row(int a, int t) { return 32 * ((int)threadIdx.x >> 7) + 16 * a + 4 * t + (((int)threadIdx.x & 63) >> 4); }
__device__ __forceinline__ int tile64_col(int c) { return 32 * (((int)threadIdx.x >> 6) & 1) + 16 * c + ((int)threadIdx.x & 15); }
__device__ __forceinline__ int tile64_stage_row() { return (int)threadIdx.x >> 2; }
// acc = the tile over columns 0 .. K - 1 (K a multiple of kSlabK) in slabs.  ra / rb: row tile64_stage_row() of the A / B side, 32-byte
// aligned; aon / bon: the row exists (one that does not is staged as zeros and its pointer is not read).  The first barrier of a slab stands behind whatever the caller wrote
// to LDS before the call; K >= kSlabK.
__device__ __forceinline__ void tile64_product(double* sA, double* sB /* [64 * kSlabK] each, 32-byte aligned */, const double* ra, bool aon, const double* rb, bool bon,
                                               int K, d4_t (&acc)[2][2]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int srow = tid >> 2, sk = (tid & 3) * 8;
  // where column sk of row srow goes in the two images; column sk + e, e = 0 .. 7: slab_col(e) behind it
  const int posA = (srow >> 4) * kSlabBlk + slab_pos_a(srow, sk), posB = (srow >> 4) * kSlabBlk + slab_pos_b(srow, sk);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[a][c] = d4_t{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < K; k0 += kSlabK) {
    d4_t s0, s1, t0, t1;
    s0 = s1 = t0 = t1 = d4_t{0.0, 0.0, 0.0, 0.0};
    if (aon) {
      s0 = *reinterpret_cast<const d4_t*>(ra + sk + k0);
      s1 = *reinterpret_cast<const d4_t*>(ra + sk + k0 + 4);
    }
    if (bon) {
      t0 = *reinterpret_cast<const d4_t*>(rb + sk + k0);
      t1 = *reinterpret_cast<const d4_t*>(rb + sk + k0 + 4);
    }
    __syncthreads();                                  // (the slab before this one has been read)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sA[posA + slab_col(e)] = s0[e];
      sA[posA + slab_col(4 + e)] = s1[e];
      sB[posB + slab_col(e)] = t0[e];
      sB[posB + slab_col(4 + e)] = t1[e];
    }
    __syncthreads();
    slab_mfma<2, 2>(sA + 2 * (w >> 1) * kSlabBlk, kSlabBlk, sB + 2 * (w & 1) * kSlabBlk, kSlabBlk, lane, acc);
  }
}
// entry e of a tile's point image: |.|^2 and the D scaled coordinates (leading dimension D + 1: the columns are read 16 rows at a
// time) of record rec; zeros for a point that does not exist
template <int D>
__device__ __forceinline__ void point_image(double* iSq, double* iB, int e, const double* __restrict__ bsq, const double* __restrict__ bs,
                                            size_t rec, bool on) {
  iSq[e] = on ? bsq[rec] : 0.0;
#pragma unroll
  for (int t = 0; t < D; ++t) iB[e * (D + 1) + t] = on ? bs[rec * D + t] : 0.0;
}

// ---- the tile of 128 rows x SP = 16 SB columns, kTileThreads threads -----------------------------------------------------------------
// Wave w owns rows 32 w .. + 31 as 2 x SB accumulators: acc[a][c][t] of lane l is (row 32 w + 16 a + 4 t + (l >> 4), column 16 c +
// (l & 15)).  Thread t brings columns 16 (t >> 7) .. + 15 of row t & 127 of the A side per slab (tile128_row / tile128_k); the B side
// is a [kSlabK][SP] row-major slab in global memory.
constexpr int kTile128 = 128;
template <int SB>
struct Tile128Lds {
  double sA[(kTile128 / 16) * kSlabBlkA], sB[SB * kSlabBlk];
  double rVal[4][16 * SB];
  long long rIdx[4][16 * SB];
};
__device__ __forceinline__ int tile128_row() { return (int)threadIdx.x & (kTile128 - 1); }
__device__ __forceinline__ int tile128_k() { return ((int)threadIdx.x >> 7) * 16; }
// acc += one slab: g = this thread's 16 elements of the A side, Bslab the slab of the B side
template <int SB>
__device__ __forceinline__ void tile128_step(Tile128Lds<SB>& L, const double (&g)[16], const double* __restrict__ Bslab, d4_t (&acc)[2][SB]) {
  constexpr int SP = 16 * SB;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int gp = tile128_row(), gk = tile128_k();
  const int posA = (gp >> 4) * kSlabBlkA + slab_pos_a(gp, gk);      // column gk + e, e = 0 .. 15: slab_col(e) behind it
  double bv[SB * 2];                                // [32][SP] row-major = 32 SP consecutive doubles
#pragma unroll
  for (int i = 0; i < SB * 2; ++i) bv[i] = Bslab[i * kTileThreads + tid];
  __syncthreads();                                  // (the slab before this one has been read)
#pragma unroll
  for (int e = 0; e < 16; ++e) L.sA[posA + slab_col(e)] = g[e];
#pragma unroll
  for (int i = 0; i < SB * 2; ++i) {
    const int idx = i * kTileThreads + tid, k = idx / SP, s = idx - k * SP;
    L.sB[(s >> 4) * kSlabBlk + slab_pos_b(s, k)] = bv[i];
  }
  __syncthreads();
  slab_mfma<2, SB>(L.sA + 2 * w * kSlabBlkA, kSlabBlkA, L.sB, kSlabBlk, lane, acc);
}
// The epilogue of a tile whose first row is p0: v = form(p, acc element) is the value of (row p, column s); it is stored to out [m][S]
// where out is given, and thread s < SP takes the column's arg-best over the tile's rows into (run_val, run_idx): per wave over its
// 2 x 4 register entries and the lanes 16 and 32 apart, then the four waves in order.  maximize: the largest value, else the smallest;
// ties to the lowest row, a NaN is never taken.  (The first barrier of the next step stands between these reads and the next
// epilogue's writes.)
template <int SB, class Form>
__device__ __forceinline__ void tile128_arg_best(Tile128Lds<SB>& L, const d4_t (&acc)[2][SB], long long p0, long long m, int S, int maximize,
                                                 double* __restrict__ out, Form&& form, double& run_val, long long& run_idx) {
  constexpr int SP = 16 * SB;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int c = 0; c < SB; ++c) {
    const int s = 16 * c + (lane & 15);
    long long bk = kArgNone;
    double bvv = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const long long p = p0 + 32 * w + 16 * a + 4 * t + (lane >> 4);
        const double v = form(p, acc[a][c][t]);
        const bool in = p < m && s < S;
        if (out && in) out[(size_t)p * S + s] = v;
        arg_take(bvv, bk, maximize ? v : -v, (in && v == v) ? p : kArgNone);
      }
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) {
      const double ov = __shfl_xor(bvv, off);
      const long long ok = __shfl_xor(bk, off);
      arg_take(bvv, bk, ov, ok);
    }
    if (lane < 16) {
      L.rVal[w][s] = bvv;
      L.rIdx[w][s] = bk;
    }
  }
  __syncthreads();
  if (tid < SP)
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) arg_take(run_val, run_idx, L.rVal[ww][tid], L.rIdx[ww][tid]);
}
// the workgroup's partial of column tid -> pval / pidx [grid][SP] (null: not wanted)
template <int SB>
__device__ __forceinline__ void tile128_store_partial(double* __restrict__ pval, long long* __restrict__ pidx, double run_val, long long run_idx) {
  if (pidx && threadIdx.x < 16 * SB) {
    pval[(size_t)blockIdx.x * (16 * SB) + threadIdx.x] = run_val;
    pidx[(size_t)blockIdx.x * (16 * SB) + threadIdx.x] = run_idx;
  }
}

// ---- the partials [nwg][Spad] of such tiles -> index [SBO_MAX_PATHS] / value [SBO_MAX_PATHS] -----------------------------------------
// One workgroup of kMergeThreads threads: thread (s, part) = (tid & 63, tid >> 6) takes workgroups part, part + 16, .. of column s, then
// thread s the 16 parts in order (arg_take's order is total: the winner is that of the workgroups taken one by one).  Columns from S
// on and columns without an entry: -1 / NaN.  The values were negated for an arg-min.
__device__ __forceinline__ void partials_merge(int S, int Spad, int maximize, int nwg, const double* __restrict__ pval,
                                               const long long* __restrict__ pidx, int64_t* __restrict__ index, double* __restrict__ value) {
  constexpr int kParts = kMergeThreads / SBO_MAX_PATHS;
  __shared__ double sv[kParts][SBO_MAX_PATHS];
  __shared__ long long sk[kParts][SBO_MAX_PATHS];
  const int s = threadIdx.x & (SBO_MAX_PATHS - 1), part = threadIdx.x / SBO_MAX_PATHS;
  long long bk = kArgNone;
  double bv = 0.0;
  if (s < S)
    for (int g = part; g < nwg; g += kParts) arg_take(bv, bk, pval[(size_t)g * Spad + s], pidx[(size_t)g * Spad + s]);
  sv[part][s] = bv;
  sk[part][s] = bk;
  __syncthreads();
  if (part) return;
  for (int p = 1; p < kParts; ++p) arg_take(bv, bk, sv[p][s], sk[p][s]);
  index[s] = bk == kArgNone ? -1 : bk;
  value[s] = bk == kArgNone ? __builtin_nan("") : (maximize ? bv : -bv);
}

// the host's cleared pair: what a refused call leaves, and what the device block starts from
inline void clear_index_value(int64_t (&index)[SBO_MAX_PATHS], double (&value)[SBO_MAX_PATHS]) {
  for (int s = 0; s < SBO_MAX_PATHS; ++s) {
    index[s] = -1;
    value[s] = std::numeric_limits<double>::quiet_NaN();
  }
}

}  // namespace sbo
