// bilinear.hip -- K1b: GP posterior on 2-D tensor grids as two dense fp64 GEMMs (gfx950).
//
// Reference arithmetic replaced: GP.GP_inference, models/GP_Safe.py:326-347, evaluated at every point of a
// linspace x linspace grid (test/test_SafeOpt.py:324-345).  The math and the host-side construction of the bases are
// in bilinear_host.hpp; this file holds the plan (device tables) and the kernels, with two parts of the same translation unit:
// bilinear_post.inc.hpp (stage 2 and the launch of both stages) and bilinear_interp.inc.hpp (K1i's plan):
//
//   stage 1 (k_bstage1) Bt[x1, k0]  = sum_k1 P1[k1, x1] T4qq[k0, k1]        (lines of the grid  x  pair index of axis 0)
//   stage 2 (k_bpost)  quad[x1,x0] = sum_k0 Bt[x1, k0] P0[k0, x0]   ->  var = max(0, sf2 - quad) Y_std^2
//                      m[x1, x0]   = sum_p  V0[p, x1] S0[p, x0]     (and the two gradient sums, same shape)
//
// Both GEMMs run on the matrix cores with the fragment conventions of device_common.hpp (four v_mfma_f64_4x4x4 per
// 16x16x4 step): A operands are stored as packed 16x16 block images, B operands in fragment order, so every operand
// load is one contiguous 512-byte (B) or 2-KiB (A) wave access.  Inner dimensions: K0 = r0 (r0 + 1) / 2 ~ 280 for the
// reference's length-scales, whatever n is.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>
#include <type_traits>
#include <hip/hip_ext.h>
#include "device_common.hpp"

namespace sbo {

// Plain GEMM on the matrix cores.  OUT[rows x cols] = A[rows x K] B[K x cols];  A: packed 16 x 16 block images, Bf:
// [ncs][KB * 4][64] fragments.  A wave owns 16 rows x (16 S) columns; the four waves of a workgroup take four
// consecutive row blocks.  Used for the per-model build of T4 (stage 1 of a posterior launch has its own kernel below).
//   TRI   0: A images [nrb][KB][256];  1: lower-triangular images [tri(rb, kb)][256] (the model's factor M as K1g keeps
//            it), only k-blocks <= rb exist and are run
//   OMODE 0: OUT as packed block images [nrb][ncs][256] (the A operand of a following GEMM with K = cols)
//         1: OUT both as B fragments [ncs][nrb * 4][64] (K = rows) and, transposed, as A images [ncs][nrb][256]
//         2: OUT row-major with leading dimension ld
template <int S, int TRI, int OMODE>
__global__ __launch_bounds__(256) void k_bgemm(const double* __restrict__ A, size_t a_stride_o, const double* __restrict__ Bf,
                                               size_t b_stride_o, int KB, int nrb, int ncs, double* __restrict__ out,
                                               size_t out_stride_o, double* __restrict__ out2, long long ld) {
  const int o = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rb = blockIdx.y * 4 + wave;
  if (rb >= nrb) return;                       // (no barriers in this kernel)
  const int cs0 = blockIdx.x * S;
  const double* Ablk = A + (size_t)o * a_stride_o + (TRI ? (size_t)rb * (rb + 1) / 2 : (size_t)rb * KB) * 256;
  const double* Bo = Bf + (size_t)o * b_stride_o;
  const int kend = TRI ? rb + 1 : KB;
  size_t boff[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int cs = cs0 + s < ncs ? cs0 + s : ncs - 1;
    boff[s] = (size_t)cs * KB * 4 * 64 + lane;
  }
  d4_t acc[S];
#pragma unroll
  for (int s = 0; s < S; ++s) acc[s] = d4_t{0.0, 0.0, 0.0, 0.0};
  // operands of k-block kb + 1 are loaded while kb is multiplied: with two to three waves per SIMD nothing else hides
  // the L2 latency of the fragment loads
  d4_t a[2][4];
  double b[2][4][S];
  auto load_kb = [&](int kb, d4_t (&aa)[4], double (&bb)[4][S]) {
    MM<double>::load_a4(Ablk + (size_t)kb * 256, lane, aa);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int s = 0; s < S; ++s) bb[kk][s] = Bo[boff[s] + (size_t)(kb * 4 + kk) * 64];
  };
  auto mul_kb = [&](const d4_t (&aa)[4], const double (&bb)[4][S]) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int s = 0; s < S; ++s) acc[s] = MM<double>::mfma(aa[kk], bb[kk][s], acc[s]);
  };
  load_kb(0, a[0], b[0]);
  for (int kb = 0; kb < kend; kb += 2) {
    if (kb + 1 < kend) load_kb(kb + 1, a[1], b[1]);
    mul_kb(a[0], b[0]);
    if (kb + 1 < kend) {
      if (kb + 2 < kend) load_kb(kb + 2, a[0], b[0]);
      mul_kb(a[1], b[1]);
    }
  }
  // accumulator element t of lane l: row 4 t + (l >> 4), column l & 15 of the 16 x 16 tile
  const int col_in = lane & 15, row_in = lane >> 4;
  out += (size_t)o * out_stride_o;
  if (OMODE == 1) out2 += (size_t)o * out_stride_o;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (cs0 + s >= ncs) continue;
    if (OMODE == 0) {
      double* blk = out + ((size_t)rb * ncs + (cs0 + s)) * 256;
#pragma unroll
      for (int t = 0; t < 4; ++t) blk[MM<double>::pack_pos(4 * t + row_in, col_in & 3, col_in >> 2)] = acc[s][t];
    } else if (OMODE == 1) {
      // as B fragments: k = row = rb * 16 + 4 t + row_in  ->  k-step rb * 4 + t, slot row_in: the lane's own position
      double* fr = out + ((size_t)(cs0 + s) * nrb * 4 + (size_t)rb * 4) * 64 + lane;
      // transposed as A images: row = column index, k = rb * 16 + 4 t + row_in
      double* img = out2 + ((size_t)(cs0 + s) * nrb + rb) * 256;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        fr[(size_t)t * 64] = acc[s][t];
        img[MM<double>::pack_pos(col_in, row_in, t)] = acc[s][t];
      }
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        out[(size_t)(rb * 16 + 4 * t + row_in) * ld + (size_t)(cs0 + s) * 16 + col_in] = acc[s][t];
    }
  }
}

typedef double d2_t __attribute__((ext_vector_type(2)));

// Stage 1 of every posterior launch (OUT as packed block images, the OMODE 0 of k_bgemm): the four waves of a workgroup
// own four row blocks and share S column strips, so the strips' B fragments are staged once per workgroup through LDS
// (double-buffered, one barrier per k-block) instead of once per wave from L2 -- with K ~ 290 and only 16 x 16 S outputs
// per wave the plain kernel is bound by L2 bandwidth (~110 KB of operands per wave), not by the matrix cores.
template <int S>
__global__ __launch_bounds__(256) void k_bstage1(const double* __restrict__ A, size_t a_stride_o, const double* __restrict__ Bf,
                                                 size_t b_stride_o, int KB, int nrb, int ncs, double* __restrict__ out,
                                                 size_t out_stride_o, const int* __restrict__ eff /* nullptr, or the Chebyshev core's
                                                 per-output counts: [4 o + 1] strips to produce, [4 o + 2] k-blocks to run */) {
  __shared__ double Bs[2][4 * S * 64];          // [buffer][(kk S + s) 64 + lane]
  // A: a wave's 16 x 16 block image goes through LDS too.  Read straight from memory, a fragment load has the four
  // lanes of a quad fetch the same 32 bytes (8 KB of lane traffic for a 2 KB image per k-block, which is what the
  // texture path then limits); here a lane fetches 32 bytes once and the replicated reads are LDS broadcasts.  Layout per
  // k-step as in k_bpost: the first 16-byte halves of the 16 chunks, then the second halves (conflict-free b128 reads).
  __shared__ __attribute__((aligned(16))) double As[2][4][256];   // [buffer][wave][image]
  const int o = blockIdx.z, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int rb = blockIdx.y * 4 + wave, rbl = rb < nrb ? rb : nrb - 1;
  const int cs0 = blockIdx.x * S;
  const int KBrun = eff ? eff[4 * o + 2] : KB;            // (KB stays the layout's stride)
  if (eff && cs0 >= eff[4 * o + 1]) return;               // strips behind the last degree that matters: never read
  const double* Ablk = A + (size_t)o * a_stride_o + (size_t)rbl * KB * 256 + lane * 4;   // this lane's 32 bytes of an image
  const double* Bo = Bf + (size_t)o * b_stride_o;
  // staging role: element e = tid + 256 j (j < S) of the k-block's [4][S][64] fragment set
  size_t goff[S];
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const int e = tid + 256 * j, l = e & 63, ks = e >> 6, s_ = ks % S, kk = ks / S;
    const int cs = cs0 + s_ < ncs ? cs0 + s_ : ncs - 1;
    goff[j] = ((size_t)cs * KB * 4 + kk) * 64 + l;
  }
  const int a_st = (lane >> 4) * 64 + (lane & 15) * 2;                        // where this lane's 32 bytes go (two halves)
  const int a_rd = (((lane >> 4) << 2) + (lane & 3)) * 2;                     // the chunk its fragment reads
  d4_t acc[S];
#pragma unroll
  for (int s_ = 0; s_ < S; ++s_) acc[s_] = d4_t{0.0, 0.0, 0.0, 0.0};
  double breg[S];
  d4_t areg = *reinterpret_cast<const d4_t*>(Ablk);
#pragma unroll
  for (int j = 0; j < S; ++j) Bs[0][tid + 256 * j] = Bo[goff[j]];
  *reinterpret_cast<d2_t*>(&As[0][wave][a_st]) = d2_t{areg[0], areg[1]};
  *reinterpret_cast<d2_t*>(&As[0][wave][a_st + 32]) = d2_t{areg[2], areg[3]};
  __syncthreads();
  // one k-block: prefetch block kb + 1 (registers), multiply block kb out of LDS buffer CUR, park the prefetch in the
  // other buffer (its last readers passed the previous barrier).  Written twice so that the buffers are compile-time names.
  auto step = [&](int kb, const double* bs_cur, double* bs_nxt, const double* as_cur, double* as_nxt) {
    const bool more = kb + 1 < KBrun;
    if (more) {
#pragma unroll
      for (int j = 0; j < S; ++j) breg[j] = Bo[goff[j] + (size_t)(kb + 1) * 256];
      areg = *reinterpret_cast<const d4_t*>(Ablk + (size_t)(kb + 1) * 256);
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const d2_t lo = *reinterpret_cast<const d2_t*>(as_cur + kk * 64 + a_rd), hi = *reinterpret_cast<const d2_t*>(as_cur + kk * 64 + 32 + a_rd);
      const d4_t af = d4_t{lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
      for (int s_ = 0; s_ < S; ++s_) acc[s_] = MM<double>::mfma(af, bs_cur[(kk * S + s_) * 64 + lane], acc[s_]);
    }
    if (more) {
#pragma unroll
      for (int j = 0; j < S; ++j) bs_nxt[tid + 256 * j] = breg[j];
      *reinterpret_cast<d2_t*>(as_nxt + a_st) = d2_t{areg[0], areg[1]};
      *reinterpret_cast<d2_t*>(as_nxt + a_st + 32) = d2_t{areg[2], areg[3]};
    }
    __syncthreads();
  };
  for (int kb = 0; kb < KBrun; kb += 2) {
    step(kb, Bs[0], Bs[1], As[0][wave], As[1][wave]);
    if (kb + 1 < KBrun) step(kb + 1, Bs[1], Bs[0], As[1][wave], As[0][wave]);
  }
  if (rb >= nrb) return;
  const int col_in = lane & 15, row_in = lane >> 4;
#pragma unroll
  for (int s_ = 0; s_ < S; ++s_) {
    if (cs0 + s_ >= ncs) continue;
    double* blk = out + (size_t)o * out_stride_o + ((size_t)rb * ncs + (cs0 + s_)) * 256;
#pragma unroll
    for (int t = 0; t < 4; ++t) blk[MM<double>::pack_pos(4 * t + row_in, col_in & 3, col_in >> 2)] = acc[s_][t];
  }
}

// ---- per-model plan build, all on the device ------------------------------------------------------------------------------
// A model change costs: the 2 q axis bases (k_bl_basis, one workgroup each), then a dozen launches batched over the outputs
// (blockIdx.y / .z = output) that turn the bases into the operand tables of the two GEMMs.  The host only reads the bases'
// ranks back (to size the GEMMs) -- no host numerics, no staging upload.
constexpr int kBlMaxR = 64;             // largest rank of an axis basis
constexpr int kBlMaxRc = 128;           // largest Chebyshev degree of an axis family
static inline int pair_count(int r) { return r * (r + 1) / 2; }

struct BlDims {                          // plan dimensions, by value
  int q, n, KBn;
  int r0[kMaxQ], r1[kMaxQ], rc0[kMaxQ], rc1[kMaxQ];
  int r0u, r1u, r0p, KB0, KB1, KBm, KBm2, ncs0, nrb, ncsR;
  int K0m, K1m;                          // largest pair counts over the outputs (Chebyshev core: rows of the pair-coefficient matrices)
  int D0m, D1m;                          // Chebyshev core: padded degrees (16 KB0, 16 KB1)
  long long cnt0, nlines;
  double a[2], b[2];                     // interval of each axis in normalised coordinates
  double sf2[kMaxQ];
};

// pair index k -> (p <= p'), pairs enumerated row by row : row p starts at p (2 r - p + 1) / 2
__device__ __forceinline__ void pair_of(int k, int r, int& p, int& pp) {
  const double t = 2.0 * r + 1.0;
  int g = (int)((t - sqrt(t * t - 8.0 * k)) * 0.5);
  g = g < 0 ? 0 : (g > r - 1 ? r - 1 : g);
  while (g > 0 && g * (2 * r - g + 1) / 2 > k) --g;
  while (g + 1 < r && (g + 1) * (2 * r - g) / 2 <= k) ++g;
  p = g;
  pp = g + (k - g * (2 * r - g + 1) / 2);
}

// normalised positions of the grid axes: xn0[cnt0] (all of axis 0), xn1[nlines] (the local lines of axis 1) -- the
// arithmetic of cand_coords and models/GP_Safe.py:326
__global__ __launch_bounds__(256) void k_bl_axes(const ModelConst mc, const CandSpec cs, long long cnt0, long long line0, long long nlines,
                                                 double* __restrict__ xn0, double* __restrict__ xn1) {
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < cnt0 + nlines; t += (long long)gridDim.x * blockDim.x) {
    const int a = t < cnt0 ? 0 : 1;
    const long long i = a == 0 ? t : line0 + (t - cnt0), tot = cs.count[a];
    const double x = (i == tot - 1 && tot > 1) ? cs.hi[a] : __dadd_rn(cs.lo[a], __dmul_rn((double)i, cs.step[a]));
    const double v = (x - mc.X_mean[a]) / mc.X_std[a];
    if (a == 0) xn0[t] = v; else xn1[t - cnt0] = v;
  }
}

// Basis of one axis family f_j(x) = exp(-1/2 (x vinv - A_j)^2), j < n, on the interval [a, b] (normalised coordinates),
// one workgroup per (output, axis):
//   1. Chebyshev interpolant of every f_j (degree raised 32 -> 128 until the last four coefficients are < 1e-14),
//      coefficient rows c_j in R^rc by the discrete cosine sum;
//   2. column-pivoted Gram-Schmidt on the rows (largest residual first, every direction re-orthogonalised twice against
//      the ones before): directions q_0 .. q_{r-1}, stopped when the largest residual row is below 2e-16 ||coef||_F --
//      the rank a singular value decomposition finds (or one less), at a fraction of its sequential depth (r steps instead
//      of several hundred rounds of rotations);
//   3. U_jp = c_j . q_p, taken from the loop itself (the residual of row j is c_j minus its components along the earlier,
//      orthogonal directions), so that f_j(x) = sum_p U_jp S_p(x), S_p = sum_c Q_pc T_c(xi(x)).
// Outputs: U [r][n], Vs = Q [r][rc], sig = 1, info = (ok, r, rc).  ok = 0: the interpolant did not converge or the rank
// exceeds kBlMaxR -- the caller keeps the separable-table kernel; ok = 2: the small form ran out of LDS (degree > 64), the
// caller runs the big one.
// The pivot loop is a chain of short dependent phases, so operand latency is its duration: small problems (n <= 128: NT =
// 256 threads, LDSRES) keep samples / residual rows in LDS, every problem keeps the directions there when rc <= 64.
struct BlJobs {
  int n, dpad;
  double vinv[2 * kMaxQ], a[2], b[2];
};
constexpr int kBasisQLds = 64 * 64;          // doubles of LDS for the directions (used when rc <= 64, row stride rc)
constexpr int kBasisResLds = 64 * 128;       // doubles of LDS for samples / residual rows of the small variant

template <int NT>
__device__ __forceinline__ double bl_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) s += red[w];
  return s;                                             // (same order in every thread: deterministic)
}

// the pivot loop; res [rc][n] and Q [..][rc] may live in LDS (pointers derived from the dynamic LDS block at the call site)
template <int NT, typename Stamp>
__device__ __forceinline__ int basis_pivot_loop(int n, int rc, double* res, double* Q, double* __restrict__ U, double tol2, double* nrm2,
                                                double* qv, double* cf, double* red, int* redi, bool& too_large, Stamp stamp, double& res2_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rmax = rc < n ? rc : n;
  int r = 0;
  too_large = false;
  // pivot of the first step: the row with the largest norm (ties -> lowest row)
  double bv = -1.0;
  int bi = 0x7fffffff;
  for (int j = tid; j < n; j += NT)
    if (nrm2[j] > bv) { bv = nrm2[j]; bi = j; }
  for (;;) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double yv = __shfl_xor(bv, o);
      const int yi = __shfl_xor(bi, o);
      if (yv > bv || (yv == bv && yi < bi)) { bv = yv; bi = yi; }
    }
    if (lane == 0) { red[wave] = bv; redi[wave] = bi; }
    __syncthreads();
    bv = red[0];
    bi = redi[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w)
      if (red[w] > bv || (red[w] == bv && redi[w] < bi)) { bv = red[w]; bi = redi[w]; }
    if (!(bv > tol2) || r >= rmax) break;
    if (r >= kBlMaxR) { too_large = true; break; }
    const double inv0 = 1.0 / sqrt(bv);
    if (tid < rc) qv[tid] = res[(size_t)tid * n + bi] * inv0;
    __syncthreads();
    // twice: remove what is left along the previous directions (the residual rows are only orthogonal to them to the
    // rounding of the ORIGINAL rows, which is not small against a residual of 1e-12)
    double mine = 0.0, nq = 1.0;
    for (int pass = 0; pass < 2; ++pass) {
      for (int i = tid >> 4; i < r; i += NT / 16) {              // 16 lanes per previous direction
        double s_ = 0.0;
        for (int cidx = tid & 15; cidx < rc; cidx += 16) s_ += Q[(size_t)i * rc + cidx] * qv[cidx];
        s_ += __shfl_xor(s_, 8);
        s_ += __shfl_xor(s_, 4);
        s_ += __shfl_xor(s_, 2);
        s_ += __shfl_xor(s_, 1);
        if ((tid & 15) == 0) cf[i] = s_;
      }
      __syncthreads();
      if (tid < rc) {
        // (four partial sums: the chain of dependent multiply-adds, not their count, is what a step waits for)
        double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
        int i = 0;
        for (; i + 3 < r; i += 4) {
          p0 += cf[i] * Q[(size_t)i * rc + tid];
          p1 += cf[i + 1] * Q[(size_t)(i + 1) * rc + tid];
          p2 += cf[i + 2] * Q[(size_t)(i + 2) * rc + tid];
          p3 += cf[i + 3] * Q[(size_t)(i + 3) * rc + tid];
        }
        for (; i < r; ++i) p0 += cf[i] * Q[(size_t)i * rc + tid];
        mine = qv[tid] - ((p0 + p1) + (p2 + p3));
      }
      if (pass == 0) {
        if (tid < rc) qv[tid] = mine;
        __syncthreads();
      } else {
        nq = bl_block_sum<NT>(tid < rc ? mine * mine : 0.0, red);
      }
    }
    if (nq < 0.25) break;                                  // mostly rounding of rows already covered: nothing left to add
    if (tid < rc) {
      mine /= sqrt(nq);
      qv[tid] = mine;
      Q[(size_t)r * rc + tid] = mine;
    }
    __syncthreads();
    // residual rows: d_j = res_j . q (= U_j,r), res_j -= d_j q, norms recomputed from the updated rows, next pivot
    bv = -1.0;
    bi = 0x7fffffff;
    for (int j = tid; j < n; j += NT) {
      double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;         // (rc is a multiple of 16)
      for (int cidx = 0; cidx < rc; cidx += 4) {
        d0 += res[(size_t)cidx * n + j] * qv[cidx];
        d1 += res[(size_t)(cidx + 1) * n + j] * qv[cidx + 1];
        d2 += res[(size_t)(cidx + 2) * n + j] * qv[cidx + 2];
        d3 += res[(size_t)(cidx + 3) * n + j] * qv[cidx + 3];
      }
      const double d_ = (d0 + d1) + (d2 + d3);
      U[(size_t)r * n + j] = d_;
      double n0 = 0.0, n1 = 0.0, n2 = 0.0, n3 = 0.0;
      for (int cidx = 0; cidx < rc; cidx += 4) {
        const double v0 = res[(size_t)cidx * n + j] - d_ * qv[cidx], v1 = res[(size_t)(cidx + 1) * n + j] - d_ * qv[cidx + 1];
        const double v2 = res[(size_t)(cidx + 2) * n + j] - d_ * qv[cidx + 2], v3 = res[(size_t)(cidx + 3) * n + j] - d_ * qv[cidx + 3];
        res[(size_t)cidx * n + j] = v0;
        res[(size_t)(cidx + 1) * n + j] = v1;
        res[(size_t)(cidx + 2) * n + j] = v2;
        res[(size_t)(cidx + 3) * n + j] = v3;
        n0 += v0 * v0; n1 += v1 * v1; n2 += v2 * v2; n3 += v3 * v3;
      }
      const double nn = (n0 + n1) + (n2 + n3);
      if (nn > bv) { bv = nn; bi = j; }
    }
    ++r;
    __syncthreads();                                       // (red / redi / qv are rewritten by the next step)
    stamp();
  }
  res2_out = bv > 0.0 ? bv : 0.0;          // (the block's largest residual row norm^2 at every way out of the loop)
  return r;
}

// The same loop with the residual rows in REGISTERS (r03): two threads per row, each holding half of its rc coefficients
// (rc = 32 / 48 / 64, n <= NT / 2).  A step of the loop above re-reads and re-writes every residual row through LDS (n <= 128)
// or global memory (n > 128: 13 us per step at n = 512, 22 steps); here the pivot row is published once to LDS and every
// thread updates its own registers -- the step is left with the barriers of the re-orthogonalisation.  Same algorithm and
// stopping rules; sums are grouped differently (per half row), which moves U by a few ulp.
template <int NT, int RCH>
__device__ __forceinline__ int basis_pivot_loop_reg(int n, const double* __restrict__ resG, double* Q, double* __restrict__ U, double* qv, double* cf,
                                                    double* red, int* redi, bool& too_large, double& fro2_out, double& res2_out) {
  constexpr int rc = 2 * RCH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = tid >> 1, half = tid & 1;
  const bool row = j < n;
  double rr[RCH];
#pragma unroll
  for (int k = 0; k < RCH; ++k) rr[k] = row ? resG[(size_t)(half * RCH + k) * n + j] : 0.0;
  auto row_norm = [&]() {
    double n0 = 0.0, n1 = 0.0, n2 = 0.0, n3 = 0.0;
#pragma unroll
    for (int k = 0; k < RCH; k += 4) { n0 += rr[k] * rr[k]; n1 += rr[k + 1] * rr[k + 1]; n2 += rr[k + 2] * rr[k + 2]; n3 += rr[k + 3] * rr[k + 3]; }
    double nn = (n0 + n1) + (n2 + n3);
    nn += __shfl_xor(nn, 1);
    return nn;
  };
  double nn = row_norm();
  const double fro2 = bl_block_sum<NT>((row && half == 0) ? nn : 0.0, red);
  fro2_out = fro2;
  __syncthreads();
  const double tol2 = (2e-16 * 2e-16) * fro2;
  const int rmax = rc < n ? rc : n;
  int r = 0;
  too_large = false;
  double bv = (row && half == 0) ? nn : -1.0;
  int bi = (row && half == 0) ? j : 0x7fffffff;
  for (;;) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double yv = __shfl_xor(bv, o);
      const int yi = __shfl_xor(bi, o);
      if (yv > bv || (yv == bv && yi < bi)) { bv = yv; bi = yi; }
    }
    if (lane == 0) { red[wave] = bv; redi[wave] = bi; }
    __syncthreads();
    bv = red[0];
    bi = redi[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w)
      if (red[w] > bv || (red[w] == bv && redi[w] < bi)) { bv = red[w]; bi = redi[w]; }
    if (!(bv > tol2) || r >= rmax) break;
    if (r >= kBlMaxR) { too_large = true; break; }
    const double inv0 = 1.0 / sqrt(bv);
    if (j == bi) {
#pragma unroll
      for (int k = 0; k < RCH; ++k) qv[half * RCH + k] = rr[k] * inv0;
    }
    __syncthreads();
    double mine = 0.0, nq = 1.0;
    for (int pass = 0; pass < 2; ++pass) {
      for (int i = tid >> 4; i < r; i += NT / 16) {              // 16 lanes per previous direction
        double s_ = 0.0;
        for (int cidx = tid & 15; cidx < rc; cidx += 16) s_ += Q[(size_t)i * rc + cidx] * qv[cidx];
        s_ += __shfl_xor(s_, 8);
        s_ += __shfl_xor(s_, 4);
        s_ += __shfl_xor(s_, 2);
        s_ += __shfl_xor(s_, 1);
        if ((tid & 15) == 0) cf[i] = s_;
      }
      __syncthreads();
      if (tid < rc) {
        double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
        int i = 0;
        for (; i + 3 < r; i += 4) {
          p0 += cf[i] * Q[(size_t)i * rc + tid];
          p1 += cf[i + 1] * Q[(size_t)(i + 1) * rc + tid];
          p2 += cf[i + 2] * Q[(size_t)(i + 2) * rc + tid];
          p3 += cf[i + 3] * Q[(size_t)(i + 3) * rc + tid];
        }
        for (; i < r; ++i) p0 += cf[i] * Q[(size_t)i * rc + tid];
        mine = qv[tid] - ((p0 + p1) + (p2 + p3));
      }
      if (pass == 0) {
        __syncthreads();                                         // (everyone has read qv / cf of this pass)
        if (tid < rc) qv[tid] = mine;
        __syncthreads();
      } else {
        nq = bl_block_sum<NT>(tid < rc ? mine * mine : 0.0, red);
      }
    }
    if (nq < 0.25) break;                                  // mostly rounding of rows already covered: nothing left to add
    if (tid < rc) {
      mine /= sqrt(nq);
      qv[tid] = mine;
      Q[(size_t)r * rc + tid] = mine;
    }
    __syncthreads();
    // residual rows in registers: d_j = res_j . q (= U_j,r), res_j -= d_j q, norms recomputed from the updated rows
    double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
    const double* qh = qv + half * RCH;
#pragma unroll
    for (int k = 0; k < RCH; k += 4) {
      d0 += rr[k] * qh[k];
      d1 += rr[k + 1] * qh[k + 1];
      d2 += rr[k + 2] * qh[k + 2];
      d3 += rr[k + 3] * qh[k + 3];
    }
    double d_ = (d0 + d1) + (d2 + d3);
    d_ += __shfl_xor(d_, 1);
    if (row && half == 0) U[(size_t)r * n + j] = d_;
#pragma unroll
    for (int k = 0; k < RCH; ++k) rr[k] -= d_ * qh[k];
    nn = row_norm();
    bv = (row && half == 0) ? nn : -1.0;
    bi = (row && half == 0) ? j : 0x7fffffff;
    ++r;
    __syncthreads();                                       // (red / redi / qv are rewritten by the next step)
  }
  res2_out = bv > 0.0 ? bv : 0.0;          // (the block's largest residual row norm^2 at every way out of the loop)
  return r;
}

// ---- front end of the bases, spread over the chip -------------------------------------------------------------------------
// k_bl_basis is one workgroup per (output, axis): its pivot loop is sequential by nature, but the two passes in front of it
// (Chebyshev samples + degree test, all coefficients) are not, and on a single CU they took 54 of config B's 182 us and 184
// of H's 520.  k_bl_degree finds the smallest degree of the ladder 32 / 48 / 64 / 96 / 128 whose last four coefficients are
// below 1e-14 for every row (a thread per row, the ladder walked per workgroup, one atomicMax per workgroup and job);
// k_bl_coef writes the coefficient rows of that degree straight into the job's residual-row workspace (a workgroup per 32
// rows: its samples in LDS, the sums in the order the single-workgroup pass uses -- the same values bit for bit).
constexpr int kCoefRows = 32;
__device__ __forceinline__ int bl_degree_of(int trial) { return trial == 0 ? 32 : (trial == 1 ? 48 : (trial == 2 ? 64 : (trial == 3 ? 96 : kBlMaxRc))); }

__global__ __launch_bounds__(256) void k_bl_degree(const BlJobs jb, const double* __restrict__ Xn, int* __restrict__ rc_job) {
  // four lanes per row (64 rows per workgroup): each takes every fourth sample -- a thread alone walks up to 80 exp() before
  // the ladder stops at degree 48
  __shared__ double ct[4 * kBlMaxRc];
  __shared__ double red[4];
  const int job = blockIdx.y, axis = job & 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = jb.n, j = blockIdx.x * 64 + (tid >> 2), sub = tid & 3;
  const double vinv = jb.vinv[job], a = jb.a[axis], b = jb.b[axis];
  const double xj = j < n ? Xn[(size_t)j * jb.dpad + axis] * vinv : 0.0;
  int pass = 0;                                                    // 0: no degree of the ladder is enough
  for (int trial = 0; trial < 5; ++trial) {
    const int rc = bl_degree_of(trial);
    __syncthreads();
    for (int m = tid; m < 4 * rc; m += 256) ct[m] = cospi((double)m / (2.0 * rc));
    __syncthreads();
    double s_[4] = {0.0, 0.0, 0.0, 0.0};
    if (j < n) {
      int m_[4], st_[4];                                           // angle index p (2 k + 1) mod 4 rc and its step for k += 4
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int pq = rc - 4 + u;
        m_[u] = (pq * (2 * sub + 1)) % (4 * rc);
        st_[u] = (pq * 8) % (4 * rc);
      }
      for (int k = sub; k < rc; k += 4) {
        const double x = 0.5 * (ct[2 * k + 1] * (b - a) + (a + b));
        const double df = x * vinv - xj;
        const double f = exp(-0.5 * (df * df));
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          s_[u] += f * ct[m_[u]];
          m_[u] += st_[u];
          if (m_[u] >= 4 * rc) m_[u] -= 4 * rc;
        }
      }
    }
    double tail = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      double v = s_[u];
      v += __shfl_xor(v, 1);
      v += __shfl_xor(v, 2);
      const double t_ = fabs(v * (2.0 / rc));
      tail = t_ > tail ? t_ : tail;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const double y = __shfl_xor(tail, o); tail = y > tail ? y : tail; }
    __syncthreads();
    if (lane == 0) red[wave] = tail;
    __syncthreads();
    tail = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    if (tail <= 1e-14) { pass = rc; break; }                       // (uniform: every thread sees the same maximum)
  }
  if (tid == 0) atomicMax(&rc_job[job], pass ? pass : 0x7fffffff);
}

__global__ __launch_bounds__(256) void k_bl_coef(const BlJobs jb, const double* __restrict__ Xn, const int* __restrict__ rc_job,
                                                 double* __restrict__ work, size_t work_stride, double* __restrict__ axis_eps) {
  __shared__ double ct[4 * kBlMaxRc];
  __shared__ double fs[kBlMaxRc * kCoefRows];                       // samples [k][row of the tile]
  const int job = blockIdx.y, axis = job & 1, tid = threadIdx.x;
  const int n = jb.n, rc = rc_job[job];
  if (rc <= 0 || rc > kBlMaxRc) return;                             // no degree qualified: k_bl_basis reports it
  const int j0 = blockIdx.x * kCoefRows;
  const double vinv = jb.vinv[job], a = jb.a[axis], b = jb.b[axis];
  double* res = work + (size_t)job * work_stride + (size_t)n * kBlMaxRc;   // the job's residual rows (resG of k_bl_basis)
  for (int m = tid; m < 4 * rc; m += 256) ct[m] = cospi((double)m / (2.0 * rc));
  __syncthreads();
  for (int w = tid; w < rc * kCoefRows; w += 256) {
    const int k = w / kCoefRows, jl = w % kCoefRows, j = j0 + jl;
    double f = 0.0;
    if (j < n) {
      const double x = 0.5 * (ct[2 * k + 1] * (b - a) + (a + b));
      const double df = x * vinv - Xn[(size_t)j * jb.dpad + axis] * vinv;
      f = exp(-0.5 * (df * df));
    }
    fs[w] = f;
  }
  __syncthreads();
  double t4 = 0.0;
  for (int w = tid; w < rc * kCoefRows; w += 256) {
    const int p = w / kCoefRows, jl = w % kCoefRows, j = j0 + jl;
    if (j >= n) continue;
    double s_ = 0.0;
    int m = p;
    for (int k = 0; k < rc; ++k) {
      s_ += fs[k * kCoefRows + jl] * ct[m];
      m += 2 * p;
      if (m >= 4 * rc) m -= 4 * rc;
    }
    const double cv = s_ * ((p == 0 ? 1.0 : 2.0) / rc);
    res[(size_t)p * n + j] = cv;
    if (p >= rc - 4) t4 = fmax(t4, fabs(cv));
  }
  // the largest of the last four coefficients at the degree chosen: what the guard band extrapolates the dropped tail from
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t4 = fmax(t4, __shfl_xor(t4, o));
  if ((tid & 63) == 0 && t4 > 0.0 && axis_eps)
    atomicMax(reinterpret_cast<unsigned long long*>(axis_eps + 2 * job), (unsigned long long)__double_as_longlong(t4));
}

template <int NT, bool LDSRES>
__global__ __launch_bounds__(NT) void k_bl_basis(const BlJobs jb, const double* __restrict__ Xn, double* __restrict__ work,
                                                 size_t work_stride, double* __restrict__ Uout, double* __restrict__ Vsout,
                                                 double* __restrict__ sigout, int* __restrict__ info,
                                                 long long* __restrict__ dbg /* nullptr, or 80 time stamps of job 0 */,
                                                 const int* __restrict__ rc_pre /* nullptr, or the degree per job from k_bl_degree
                                                                                    (its coefficient rows are in the workspace) */,
                                                 int no_reg /* 1: never the register form of the pivot loop (A/B) */, double* __restrict__ axis_eps) {
  extern __shared__ double bl_dyn[];          // [kBasisQLds directions | kBasisResLds samples / residual rows (LDSRES)]
  __shared__ double ct[4 * kBlMaxRc];        // cos(pi m / (2 rc)), m < 4 rc
  __shared__ double qv[kBlMaxRc];            // the direction being built
  __shared__ double cf[kBlMaxR];             // its coefficients along the previous directions
  __shared__ double nrm2[SBO_MAX_N];         // squared norm of every row
  __shared__ double red[NT / 64];
  __shared__ int redi[NT / 64];
  const int job = blockIdx.x, axis = job & 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = jb.n;
  const double vinv = jb.vinv[job], a = jb.a[axis], b = jb.b[axis];
  double* wk = work + (size_t)job * work_stride;
  double* fnT = LDSRES ? bl_dyn + kBasisQLds : wk;                          // [k][j] samples
  double* resG = wk + (size_t)n * kBlMaxRc;                                // [p][j] residual rows (global form)
  double* QG = resG + (size_t)n * kBlMaxRc;                                // directions (global form, rc > 64)
  int* inf = info + 4 * job;
  int rc = 0;
  bool ok = false, out_of_lds = false, regpath = false;
  int ndbg = 0;
  auto stamp = [&]() { if (dbg && job == 0 && tid == 0 && ndbg < 80) dbg[ndbg++] = wall_clock64(); };
  stamp();
  if (rc_pre) {
    rc = rc_pre[job];
    ok = rc > 0 && rc <= kBlMaxRc;
    // rows in registers, two threads per row (the 1024-thread form has 128 registers per thread: degree 64 would spill)
    regpath = ok && n <= NT / 2 && (rc == 32 || rc == 48 || (rc == 64 && NT <= 256)) && !no_reg;
    if (ok && LDSRES && !regpath && rc * n > kBasisResLds) { ok = false; out_of_lds = true; }
    if (ok && LDSRES && !regpath) {                                // the rows move from the workspace into LDS
      for (int w = tid; w < rc * n; w += NT) (bl_dyn + kBasisQLds)[w] = resG[w];
    }
    __syncthreads();
  }
  for (int trial = 0; trial < 5 && !ok && !rc_pre; ++trial) {
    rc = trial == 0 ? 32 : (trial == 1 ? 48 : (trial == 2 ? 64 : (trial == 3 ? 96 : kBlMaxRc)));
    if (LDSRES && rc * n > kBasisResLds) { out_of_lds = true; break; }
    __syncthreads();
    for (int m = tid; m < 4 * rc; m += NT) ct[m] = cospi((double)m / (2.0 * rc));
    __syncthreads();
    // samples at the Chebyshev points of the first kind, theta_k = pi (k + 1/2) / rc
    for (int w = tid; w < rc * n; w += NT) {
      const int k = w / n, j = w - k * n;
      const double x = 0.5 * (ct[2 * k + 1] * (b - a) + (a + b));
      const double df = x * vinv - Xn[(size_t)j * jb.dpad + axis] * vinv;
      fnT[w] = exp(-0.5 * (df * df));
    }
    __syncthreads();
    // the last four coefficients decide whether this degree is enough
    double tail = 0.0;
    for (int w = tid; w < 4 * n; w += NT) {
      const int p = rc - 4 + w / n, j = w % n;
      double s_ = 0.0;
      int m = p;
      for (int k = 0; k < rc; ++k) {
        s_ += fnT[(size_t)k * n + j] * ct[m];
        m += 2 * p;
        if (m >= 4 * rc) m -= 4 * rc;
      }
      s_ = fabs(s_ * (2.0 / rc));
      tail = s_ > tail ? s_ : tail;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const double y = __shfl_xor(tail, o); tail = y > tail ? y : tail; }
    __syncthreads();
    if (lane == 0) red[wave] = tail;
    __syncthreads();
    tail = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) tail = red[w] > tail ? red[w] : tail;
    ok = tail <= 1e-14;
  }
  if (!ok) {
    if (tid == 0) { inf[0] = out_of_lds ? 2 : 0; inf[1] = 0; inf[2] = rc; inf[3] = 0; }
    return;
  }
  stamp();
  // all coefficients: coef[j][p] = w_p / rc sum_k f_j(x_k) cos(p theta_k), straight into the residual rows.  The small
  // variant reuses the samples' LDS: every thread holds its coefficients in registers until all sums are done.
  double* res = LDSRES ? bl_dyn + kBasisQLds : resG;
  constexpr int kKeep = LDSRES ? kBasisResLds / NT : 1;
  double keep[kKeep];
  if (rc_pre) {
    // (the coefficient rows were written by k_bl_coef)
  } else if (LDSRES) {
#pragma unroll
    for (int it = 0; it < kKeep; ++it) {
      const int w = tid + it * NT;
      double s_ = 0.0;
      if (w < rc * n) {
        const int p = w / n, j = w - p * n;
        int m = p;
        for (int k = 0; k < rc; ++k) {
          s_ += fnT[(size_t)k * n + j] * ct[m];
          m += 2 * p;
          if (m >= 4 * rc) m -= 4 * rc;
        }
        s_ *= (p == 0 ? 1.0 : 2.0) / rc;
      }
      keep[it] = s_;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kKeep; ++it) {
      const int w = tid + it * NT;
      if (w < rc * n) res[w] = keep[it];
    }
  } else {
    for (int w = tid; w < rc * n; w += NT) {
      const int p = w / n, j = w - p * n;
      double s_ = 0.0;
      int m = p;
      for (int k = 0; k < rc; ++k) {
        s_ += fnT[(size_t)k * n + j] * ct[m];
        m += 2 * p;
        if (m >= 4 * rc) m -= 4 * rc;
      }
      res[w] = s_ * ((p == 0 ? 1.0 : 2.0) / rc);
    }
  }
  __syncthreads();
  double* U = Uout + (size_t)job * kBlMaxR * n;
  bool too_large = false;
  int r;
  double res2 = 0.0;
  if (regpath) {
    double fro2r = 0.0;
    if (rc == 32) r = basis_pivot_loop_reg<NT, 16>(n, resG, bl_dyn, U, qv, cf, red, redi, too_large, fro2r, res2);
    else if (rc == 48) r = basis_pivot_loop_reg<NT, 24>(n, resG, bl_dyn, U, qv, cf, red, redi, too_large, fro2r, res2);
    else if constexpr (NT <= 256) r = basis_pivot_loop_reg<NT, 32>(n, resG, bl_dyn, U, qv, cf, red, redi, too_large, fro2r, res2);
    else r = 0;
    stamp();
  } else {
  double fro2 = 0.0;
  for (int j = tid; j < n; j += NT) {
    double s_ = 0.0;
    for (int p = 0; p < rc; ++p) { const double v = res[(size_t)p * n + j]; s_ += v * v; }
    nrm2[j] = s_;
    fro2 += s_;
  }
  fro2 = bl_block_sum<NT>(fro2, red);
  __syncthreads();
  const double tol2 = (2e-16 * 2e-16) * fro2;
  stamp();
  if (rc <= 64)
    r = basis_pivot_loop<NT>(n, rc, res, bl_dyn, U, tol2, nrm2, qv, cf, red, redi, too_large, stamp, res2);
  else
    r = basis_pivot_loop<NT>(n, rc, res, QG, U, tol2, nrm2, qv, cf, red, redi, too_large, stamp, res2);
  }
  if (too_large || r < 1) {
    if (tid == 0) { inf[0] = 0; inf[1] = r; inf[2] = rc; inf[3] = 0; }
    return;
  }
  __syncthreads();
  const double* Q = rc <= 64 ? bl_dyn : QG;
  double* Vs = Vsout + (size_t)job * kBlMaxR * kBlMaxRc;
  for (int w = tid; w < r * rc; w += NT) Vs[w] = Q[w];
  if (tid < r) sigout[(size_t)job * kBlMaxR + tid] = 1.0;
  if (tid == 0) { inf[0] = 1; inf[1] = r; inf[2] = rc; inf[3] = 0; }
  // what the rank cut leaves of any factor, as a function on the axis: |sum_p R_jp T_p| <= ||R_j||_1 <= sqrt(rc) ||R_j||_2
  if (tid == 0 && axis_eps) axis_eps[2 * job + 1] = sqrt((double)rc * res2);
  __syncthreads();
  stamp();
  if (dbg && job == 0 && tid == 0) dbg[80] = ndbg;
}

// Axis tables S[p][i] = sig_p sum_c Vs[p][c] T_c(xi_i) from the Chebyshev series of the bases (three-term recurrence, sum
// in ascending c, one thread per entry); blockIdx.y = 2 o + axis
__global__ __launch_bounds__(256) void k_bl_stab(const BlDims dm, const double* __restrict__ Vsall, const double* __restrict__ sigall,
                                                 const double* __restrict__ xn0, const double* __restrict__ xn1, double* __restrict__ S0all,
                                                 double* __restrict__ S1all) {
  const int job = blockIdx.y, o = job >> 1, axis = job & 1;
  const int r = axis ? dm.r1[o] : dm.r0[o], rc = axis ? dm.rc1[o] : dm.rc0[o];
  const long long count = axis ? dm.nlines : dm.cnt0;
  const double a = dm.a[axis], b = dm.b[axis];
  const double* Vs = Vsall + (size_t)job * kBlMaxR * kBlMaxRc;
  const double* sig = sigall + (size_t)job * kBlMaxR;
  const double* xn = axis ? xn1 : xn0;
  double* S = axis ? S1all + (size_t)o * dm.r1u * dm.nlines : S0all + (size_t)o * dm.r0u * dm.cnt0;
  const long long total = (long long)r * count;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int p = (int)(idx / count);
    const long long i = idx % count;
    double xi = (2.0 * xn[i] - (a + b)) / (b - a);
    xi = xi < 1.0 ? xi : 1.0;
    xi = xi > -1.0 ? xi : -1.0;
    const double* v = Vs + (size_t)p * rc;
    double t0 = 1.0, t1 = xi, s_ = 0.0;
    s_ += v[0] * t0;
    if (rc > 1) s_ += v[1] * t1;
    for (int c2 = 2; c2 < rc; ++c2) {
      const double t = 2.0 * xi * t1 - t0;
      s_ += v[c2] * t;
      t0 = t1;
      t1 = t;
    }
    S[idx] = sig[p] * s_;
  }
}

// Z_j,(p,s) = U0_jp U1_js as B fragments [ncsR][KBn * 4][64] (k = observation j, column c = p r1 + s); blockIdx.y = o
__global__ __launch_bounds__(256) void k_bl_zf(const BlDims dm, const double* __restrict__ Uall, size_t nZf, double* __restrict__ Zfall) {
  const int o = blockIdx.y, n = dm.n, r0 = dm.r0[o], r1 = dm.r1[o], KBn = dm.KBn;
  const double* U0 = Uall + (size_t)(2 * o) * kBlMaxR * n;
  const double* U1 = Uall + (size_t)(2 * o + 1) * kBlMaxR * n;
  double* Zf = Zfall + (size_t)o * nZf;
  const long long total = (long long)dm.ncsR * KBn * 4 * 64;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int l = (int)(i & 63);
    const long long fr = i >> 6;
    const int ks = (int)(fr % (KBn * 4)), cs = (int)(fr / (KBn * 4));
    const int j = (ks >> 2) * 16 + MM<double>::jslot(ks & 3, l >> 4);
    const int cidx = cs * 16 + (l & 15);
    double v = 0.0;
    if (j < n && cidx < r0 * r1) v = U0[(size_t)(cidx / r1) * n + j] * U1[(size_t)(cidx % r1) * n + j];
    Zf[i] = v;
  }
}
// T4qq^T as B fragments over the columns k0: [KB0][KB1 * 4][64], element (k1, k0) = sf2^2 / 2 (G[(p,s),(p',s')] + G[(p',s),(p,s')])
// (sym: G is symmetric only up to rounding -- the form with a caller's invK -- and both transposed entries are averaged in)
__global__ __launch_bounds__(256) void k_bl_t4f(const BlDims dm, const double* __restrict__ Gall, long long ldg, size_t sT4f,
                                                double* __restrict__ T4fall, int sym) {
  const int o = blockIdx.y, r0 = dm.r0[o], r1 = dm.r1[o], KB0 = dm.KB0, KB1 = dm.KB1;
  const int K0 = r0 * (r0 + 1) / 2, K1 = r1 * (r1 + 1) / 2;
  const double* G = Gall + (size_t)o * ldg * ldg;
  double* T4f = T4fall + (size_t)o * sT4f;
  const double scale = dm.sf2[o] * dm.sf2[o];
  const long long total = (long long)KB0 * KB1 * 4 * 64;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int l = (int)(i & 63);
    const long long fr = i >> 6;
    const int ks = (int)(fr % (KB1 * 4)), cs = (int)(fr / (KB1 * 4));
    const int k1 = (ks >> 2) * 16 + MM<double>::jslot(ks & 3, l >> 4);
    const int k0 = cs * 16 + (l & 15);
    double v = 0.0;
    if (k0 < K0 && k1 < K1) {
      int p, pp, s1, ss;
      pair_of(k0, r0, p, pp);
      pair_of(k1, r1, s1, ss);
      const size_t a1 = (size_t)(p * r1 + s1), b1 = (size_t)(pp * r1 + ss), a2 = (size_t)(pp * r1 + s1), b2 = (size_t)(p * r1 + ss);
      v = sym ? scale * 0.25 * ((G[a1 * ldg + b1] + G[b1 * ldg + a1]) + (G[a2 * ldg + b2] + G[b2 * ldg + a2]))
              : scale * 0.5 * (G[a1 * ldg + b1] + G[a2 * ldg + b2]);
    }
    T4f[i] = v;
  }
}
// ---- mean-phase operands -------------------------------------------------------------------------------------------------
// Mb[o][b][p r1 + s] = sf2 sum_j beta_b[j] U0_jp U1_js, beta = (alpha, alpha Xn_0, alpha Xn_1): the bilinear forms of the
// mean and of its two gradient sums.  One wave per (b, p, s), lanes over the observations; blockIdx.y = o
__global__ __launch_bounds__(256) void k_bl_mb(const BlDims dm, const double* __restrict__ Uall, const double* __restrict__ alpha, int ald,
                                               const double* __restrict__ Xn, int dpad, double* __restrict__ Mball) {
  const int o = blockIdx.y, n = dm.n, r0 = dm.r0[o], r1 = dm.r1[o];
  const double* U0 = Uall + (size_t)(2 * o) * kBlMaxR * n;
  const double* U1 = Uall + (size_t)(2 * o + 1) * kBlMaxR * n;
  const double* al = alpha + (size_t)o * ald;
  double* Mb = Mball + (size_t)o * 3 * dm.r0u * dm.r1u;
  const int lane = threadIdx.x & 63, total = 3 * r0 * r1;
  for (int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < total; i += (gridDim.x * blockDim.x) >> 6) {
    const int s_ = i % r1, p = (i / r1) % r0, b = i / (r0 * r1);
    const double *u0 = U0 + (size_t)p * n, *u1 = U1 + (size_t)s_ * n;
    double acc = 0.0;
    for (int j = lane; j < n; j += 64) {
      const double be = b == 0 ? al[j] : al[j] * Xn[(size_t)j * dpad + (b - 1)];
      acc += be * u0[j] * u1[j];
    }
    acc = wave_sum(acc);
    if (lane == 0) Mb[i] = dm.sf2[o] * acc;
  }
}
// Vb[o][b][p][line] = sum_s Mb[b][p, s] S1[s][line]
__global__ __launch_bounds__(256) void k_bl_vb(const BlDims dm, const double* __restrict__ Mball, const double* __restrict__ S1all,
                                               double* __restrict__ Vball) {
  const int o = blockIdx.y, r0 = dm.r0[o], r1 = dm.r1[o], r0u = dm.r0u;
  const long long nlines = dm.nlines;
  const double* Mb = Mball + (size_t)o * 3 * dm.r0u * dm.r1u;
  const double* S1 = S1all + (size_t)o * dm.r1u * nlines;
  double* Vb = Vball + (size_t)o * 3 * r0u * nlines;
  const long long total = 3ll * r0 * nlines;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long l = i % nlines;
    const int p = (int)((i / nlines) % r0), b = (int)(i / (nlines * r0));
    double acc = 0.0;
    for (int s_ = 0; s_ < r1; ++s_) acc += Mb[((size_t)b * r0 + p) * r1 + s_] * S1[(size_t)s_ * nlines + l];
    Vb[((size_t)b * r0u + p) * nlines + l] = acc;
  }
}
// A images of the mean phases, three sets:  V0 (K = 16 KBm) | [V1; V0] (K = 16 KBm2, V0 from k = r0p) | V1x = V2 - xn1 V0
__global__ __launch_bounds__(256) void k_bl_va(const BlDims dm, const double* __restrict__ Vball, const double* __restrict__ xn1, size_t sVA,
                                               double* __restrict__ outall) {
  const int o = blockIdx.y, nrb = dm.nrb, KBm = dm.KBm, KBm2 = dm.KBm2, r0 = dm.r0[o], r0p = dm.r0p, r0u = dm.r0u;
  const long long nlines = dm.nlines;
  const double* Vb = Vball + (size_t)o * 3 * r0u * nlines;
  double* out = outall + (size_t)o * sVA;
  const long long set = (long long)nrb * KBm * 256, set2 = (long long)nrb * KBm2 * 256, total = 2 * set + set2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int which = i < set ? 0 : (i < set + set2 ? 1 : 2);
    const long long li = which == 0 ? i : (which == 1 ? i - set : i - set - set2);
    const int KBx = which == 1 ? KBm2 : KBm;
    // invert pack_pos(r, slot, kk) = kk * 64 + (slot * 4 + (r & 3)) * 4 + (r >> 2)
    const int e = (int)(li & 255);
    const long long blk = li >> 8;
    const int kk = e >> 6, rem = e & 63, slot = rem >> 4, r = ((rem >> 2) & 3) + 4 * (rem & 3);
    const int k = (int)(blk % KBx) * 16 + MM<double>::jslot(kk, slot);
    const long long line = (blk / KBx) * 16 + r;
    double v = 0.0;
    if (line < nlines) {
      if (which == 0) {
        if (k < r0) v = Vb[((size_t)0 * r0u + k) * nlines + line];
      } else if (which == 1) {
        if (k < r0) v = Vb[((size_t)1 * r0u + k) * nlines + line];
        else if (k >= r0p && k < r0p + r0) v = Vb[((size_t)0 * r0u + (k - r0p)) * nlines + line];
      } else if (k < r0) {
        v = Vb[((size_t)2 * r0u + k) * nlines + line] - xn1[line] * Vb[((size_t)0 * r0u + k) * nlines + line];
      }
    }
    out[i] = v;
  }
}
// B fragments of the mean phases, two sets:  S0 (K = 16 KBm) | [S0; -xn0 S0] (K = 16 KBm2, second copy from k = r0p)
__global__ __launch_bounds__(256) void k_bl_sbf(const BlDims dm, const double* __restrict__ S0all, const double* __restrict__ xn0, size_t sSBf,
                                                double* __restrict__ outall) {
  const int o = blockIdx.y, ncs0 = dm.ncs0, KBm = dm.KBm, KBm2 = dm.KBm2, r0 = dm.r0[o], r0p = dm.r0p;
  const long long cnt0 = dm.cnt0;
  const double* S0 = S0all + (size_t)o * dm.r0u * cnt0;
  double* out = outall + (size_t)o * sSBf;
  const long long fset = (long long)ncs0 * KBm * 256, total = fset + (long long)ncs0 * KBm2 * 256;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int which = i < fset ? 0 : 1;
    const long long li = which ? i - fset : i;
    const int KBx = which ? KBm2 : KBm;
    const int l = (int)(li & 63);
    const long long fr = li >> 6;
    const int ks = (int)(fr % (KBx * 4));
    const int k = (ks >> 2) * 16 + MM<double>::jslot(ks & 3, l >> 4);
    const long long x = (fr / (KBx * 4)) * 16 + (l & 15);
    double v = 0.0;
    if (x < cnt0) {
      if (k < r0) v = S0[(size_t)k * cnt0 + x];
      else if (which == 1 && k >= r0p && k < r0p + r0) v = -xn0[x] * S0[(size_t)(k - r0p) * cnt0 + x];
    }
    out[i] = v;
  }
}

#include "bilinear_post.inc.hpp"

// ---- Chebyshev core of the variance phase (r03) ---------------------------------------------------------------------------
// The pair form above contracts  quad = sum_{k0, k1} T4[k0][k1] P0_k0(x0) P1_k1(x1)  over K = r (r + 1) / 2 ~ 276 pair products
// per axis.  But the pair products are not independent functions: S_p is a Chebyshev series of degree < rc on the axis, so
// every P_k = c S_p S_p' is a polynomial of degree <= 2 rc - 2, and quad is a polynomial of that degree in each variable --
//     quad(x0, x1) = sum_{a < D0, b < D1} Chat[a][b] T_a(xi0) T_b(xi1),      Chat = PC0^T T4 PC1,
// with PC[k][m] the Chebyshev coefficients of P_k (product formula T_a T_b = (T_{a+b} + T_|a-b|) / 2: exact, no sampling).
// The same two GEMMs then run with the Chebyshev polynomials of the grid positions as operand tables (no dependence on the
// data at all) and the inner dimensions D <= 2 rc - 1 = 95 instead of 276 -- and Chat decays: the variance surface of the
// BASELINE hyper-parameters needs degree ~50 for 1e-15, so the kernels stop at the degree behind which every coefficient is
// below 4e-15 of the largest (k_cheb_trunc writes the k-step / k-block counts per output; stage 1 and k_bpost read them from
// memory: no host round trip).  Where the coefficients do not decay that far -- ill-conditioned models, whose Chat carries the
// rounding of the reference formula itself -- nothing is dropped.
// PC[job][k][m] = Chebyshev coefficient m of P_k, job = 2 o + axis; rows k >= K and columns m >= 2 rc - 1 are zero.
// One workgroup per pair: the two coefficient rows go to LDS once, a thread per degree m sums its two convolutions from
// there (four independent partial sums each: read straight from memory, a thread waited out ~150 dependent loads, 21 us).
__global__ __launch_bounds__(256) void k_cheb_pairs(const BlDims dm, const double* __restrict__ Vsall, const double* __restrict__ sigall,
                                                    size_t sPC0, size_t sPC1, double* __restrict__ PC0all, double* __restrict__ PC1all) {
  __shared__ double va[kBlMaxRc], vb[kBlMaxRc];
  const int job = blockIdx.y, o = job >> 1, axis = job & 1, k = blockIdx.x, tid = threadIdx.x;
  const int r = axis ? dm.r1[o] : dm.r0[o], rc = axis ? dm.rc1[o] : dm.rc0[o];
  const int K = r * (r + 1) / 2, Km = axis ? dm.K1m : dm.K0m, Dm = axis ? dm.D1m : dm.D0m;
  if (k >= (Km + 15) / 16 * 16) return;
  // Output in the operand layouts of the two MFMA GEMMs that form Chat^T = (PC1^T T4^T) PC0:
  //   axis 1: A images of PC1^T  [D1m / 16][KBp][256]   (row = degree m, inner index = pair k)
  //   axis 0: B fragments of PC0 [D0m / 16][KBp * 4][64] (inner index = pair k, column = degree m)
  double* PC = axis ? PC1all + (size_t)o * sPC1 : PC0all + (size_t)o * sPC0;
  const int KBp = (Km + 15) / 16;
  auto put = [&](int m, double v) {
    const int kb = k >> 4, j = k & 15, kk = j >> 2, slot = j & 3;          // MM<double>::jslot(kk, slot) = 4 kk + slot
    if (axis) PC[(((size_t)(m >> 4) * KBp + kb) << 8) + (size_t)MM<double>::pack_pos(m & 15, slot, kk)] = v;
    else PC[(((size_t)(m >> 4) * (KBp * 4) + (size_t)(kb * 4 + kk)) << 6) + (size_t)(slot * 16 + (m & 15))] = v;
  };
  if (k >= K) {
    for (int m = tid; m < Dm; m += blockDim.x) put(m, 0.0);
    return;
  }
  const double* Vs = Vsall + (size_t)job * kBlMaxR * kBlMaxRc;
  const double* sig = sigall + (size_t)job * kBlMaxR;
  int p, pp;
  pair_of(k, r, p, pp);
  for (int a = tid; a < rc; a += blockDim.x) {
    va[a] = Vs[(size_t)p * rc + a];
    vb[a] = Vs[(size_t)pp * rc + a];
  }
  __syncthreads();
  const double scale = (p == pp ? 0.5 : 1.0) * (sig[p] * sig[pp]);       // (1 | 2) * 1/2
  for (int m = tid; m < Dm; m += blockDim.x) {
    double v = 0.0;
    if (m <= 2 * rc - 2) {
      // T_a T_b = (T_{a+b} + T_|a-b|) / 2
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
      const int a0 = m - rc + 1 > 0 ? m - rc + 1 : 0, a1 = m < rc - 1 ? m : rc - 1;      // a + b = m, both below rc
      int a = a0;
      for (; a + 3 <= a1; a += 4) {
        s0 += va[a] * vb[m - a];
        s1 += va[a + 1] * vb[m - a - 1];
        s2 += va[a + 2] * vb[m - a - 2];
        s3 += va[a + 3] * vb[m - a - 3];
      }
      for (; a <= a1; ++a) s0 += va[a] * vb[m - a];
      if (m == 0) {
        for (a = 0; a + 3 < rc; a += 4) {
          s0 += va[a] * vb[a];
          s1 += va[a + 1] * vb[a + 1];
          s2 += va[a + 2] * vb[a + 2];
          s3 += va[a + 3] * vb[a + 3];
        }
        for (; a < rc; ++a) s0 += va[a] * vb[a];
      } else {
        const int lim = rc - m;                                        // |a - b| = m
        for (a = 0; a + 1 < lim; a += 2) {
          s0 += va[a + m] * vb[a];
          s1 += va[a] * vb[a + m];
          s2 += va[a + 1 + m] * vb[a + 1];
          s3 += va[a + 1] * vb[a + 1 + m];
        }
        for (; a < lim; ++a) { s0 += va[a + m] * vb[a]; s1 += va[a] * vb[a + m]; }
      }
      v = scale * ((s0 + s1) + (s2 + s3));
    }
    put(m, v);
  }
}
// T4 as a plain matrix [K0m][K1m] (the entries k_bl_t4f gathers, same formula)
__global__ __launch_bounds__(256) void k_cheb_t4(const BlDims dm, const double* __restrict__ Gall, long long ldg, double* __restrict__ T4all,
                                                 int sym) {
  const int o = blockIdx.y, r0 = dm.r0[o], r1 = dm.r1[o];
  const int K0 = r0 * (r0 + 1) / 2, K1 = r1 * (r1 + 1) / 2;
  const double* G = Gall + (size_t)o * ldg * ldg;
  double* T4 = T4all + (size_t)o * dm.K0m * dm.K1m;
  const double scale = dm.sf2[o] * dm.sf2[o];
  const long long total = (long long)dm.K0m * dm.K1m;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int k0 = (int)(i / dm.K1m), k1 = (int)(i % dm.K1m);
    double v = 0.0;
    if (k0 < K0 && k1 < K1) {
      int p, pp, s1, ss;
      pair_of(k0, r0, p, pp);
      pair_of(k1, r1, s1, ss);
      const size_t a1 = (size_t)(p * r1 + s1), b1 = (size_t)(pp * r1 + ss), a2 = (size_t)(pp * r1 + s1), b2 = (size_t)(p * r1 + ss);
      v = sym ? scale * 0.25 * ((G[a1 * ldg + b1] + G[b1 * ldg + a1]) + (G[a2 * ldg + b2] + G[b2 * ldg + a2]))
              : scale * 0.5 * (G[a1 * ldg + b1] + G[a2 * ldg + b2]);
    }
    T4[i] = v;
  }
}
// C = A^T B for small matrices, A [K][M], B [K][N] row-major (k-major); 32 x 32 outputs per workgroup, 64-deep k tiles (the
// 16-deep form waited out 18 load -> barrier round trips for K = 276: 40 us), plain fp64 sums in ascending k.  TRANS: C stored
// transposed ([N][M]).  blockIdx.z = output.  rowmax / colmax (nullptr: none): max |C| of every row and column as bit
// patterns (non-negative doubles order like their bits), for k_cheb_trunc.
template <bool TRANS>
__global__ __launch_bounds__(256) void k_small_tn(const double* __restrict__ Aall, size_t sA, const double* __restrict__ Ball, size_t sB, int K,
                                                  int M, int N, double* __restrict__ Call, size_t sC, unsigned long long* __restrict__ rowmax,
                                                  unsigned long long* __restrict__ colmax) {
  constexpr int KT = 64;
  __shared__ double As[KT][33], Bs[KT][33];
  const int o = blockIdx.z, tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const double* A = Aall + (size_t)o * sA;
  const double* B = Ball + (size_t)o * sB;
  double* C = Call + (size_t)o * sC;
  const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < K; k0 += KT) {
    for (int e = tid; e < KT * 32; e += 256) {
      const int kk = e >> 5, c = e & 31;
      As[kk][c] = (k0 + kk < K && m0 + c < M) ? A[(size_t)(k0 + kk) * M + m0 + c] : 0.0;
      Bs[kk][c] = (k0 + kk < K && n0 + c < N) ? B[(size_t)(k0 + kk) * N + n0 + c] : 0.0;
    }
    __syncthreads();
#pragma unroll 16
    for (int kk = 0; kk < KT; ++kk) {
      const double b = Bs[kk][tx];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] += As[kk][ty + 8 * u] * b;
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int m = m0 + ty + 8 * u, n = n0 + tx;
    if (m < M && n < N) {
      C[TRANS ? (size_t)n * M + m : (size_t)m * N + n] = acc[u];
      if (rowmax) {
        const unsigned long long key = (unsigned long long)__double_as_longlong(fabs(acc[u]));
        atomicMax(&rowmax[(size_t)o * M + m], key);
        atomicMax(&colmax[(size_t)o * N + n], key);
      }
    }
  }
}
// degrees the kernels run to, per output: behind them every |Chat| is below thr of the largest.  ChatT [D1m][D0m] row-major
// (the GEMMs deliver the transpose).  eff[4 o + 0] = k-steps of the variance phase (axis 0, four degrees each), [1] = its
// 16-blocks (strips of stage 1), [2] = 16-blocks of axis 1 (inner dimension of stage 1), [3] = 0.  One workgroup of 1024.
// tail[o] (behind the q x 4 counts): the sum of |Chat| over the entries the kernels do NOT run -- a bound on what the truncation
// moves the quadratic form by (|T_a T_b| <= 1), part of K1b's guard band (guard.hip).
__global__ __launch_bounds__(1024) void k_cheb_trunc(const BlDims dm, const double* __restrict__ ChatT_all, double thr, int* __restrict__ eff) {
  __shared__ double red[16];
  __shared__ int redi[16][2];
  const int o = blockIdx.x, tid = threadIdx.x, D0 = dm.D0m, D1 = dm.D1m;
  const double* Ch = ChatT_all + (size_t)o * D0 * D1;
  double mx = 0.0;
  for (int i = tid; i < D0 * D1; i += 1024) { const double v = fabs(Ch[i]); mx = v > mx ? v : mx; }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const double y = __shfl_xor(mx, off); mx = y > mx ? y : mx; }
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = 0.0;
#pragma unroll
  for (int w = 0; w < 16; ++w) mx = red[w] > mx ? red[w] : mx;
  const double cut = thr * mx;
  int a_hi = 0, b_hi = 0;                          // 1 + largest index holding an entry above the cut
  for (int i = tid; i < D0 * D1; i += 1024) {
    if (fabs(Ch[i]) > cut) {
      const int b = i / D0, a = i % D0;            // ChatT[b][a]
      a_hi = a + 1 > a_hi ? a + 1 : a_hi;
      b_hi = b + 1 > b_hi ? b + 1 : b_hi;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int ya = __shfl_xor(a_hi, off), yb = __shfl_xor(b_hi, off);
    a_hi = ya > a_hi ? ya : a_hi;
    b_hi = yb > b_hi ? yb : b_hi;
  }
  if ((tid & 63) == 0) { redi[tid >> 6][0] = a_hi; redi[tid >> 6][1] = b_hi; }
  __syncthreads();
  __shared__ int run_ab[2];
  if (tid == 0) {
    for (int w = 1; w < 16; ++w) { a_hi = redi[w][0] > a_hi ? redi[w][0] : a_hi; b_hi = redi[w][1] > b_hi ? redi[w][1] : b_hi; }
    a_hi = a_hi < 1 ? 1 : a_hi;
    b_hi = b_hi < 1 ? 1 : b_hi;
    eff[4 * o + 0] = (a_hi + 3) / 4;
    eff[4 * o + 1] = (a_hi + 15) / 16;
    eff[4 * o + 2] = (b_hi + 15) / 16;
    eff[4 * o + 3] = 0;
    run_ab[0] = (a_hi + 3) / 4 * 4;              // degrees the two GEMMs run: axis 0 in k-steps of four, axis 1 in blocks of 16
    run_ab[1] = (b_hi + 15) / 16 * 16;
  }
  __syncthreads();
  double ts = 0.0, fs = 0.0;
  for (int i = tid; i < D0 * D1; i += 1024) {
    const int b = i / D0, a = i % D0;
    if (a >= run_ab[0] || b >= run_ab[1]) ts += fabs(Ch[i]);
    if (a >= D0 - 4 || b >= D1 - 4) fs += fabs(Ch[i]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { ts += __shfl_xor(ts, off); fs += __shfl_xor(fs, off); }
  __syncthreads();
  __shared__ double redf[16];
  if ((tid & 63) == 0) { red[tid >> 6] = ts; redf[tid >> 6] = fs; }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0, f = 0.0;
    for (int w = 0; w < 16; ++w) { s += red[w]; f += redf[w]; }
    reinterpret_cast<double*>(eff + 4 * dm.q)[o] = s;
    // frame[o] (behind the tails): the sum of |Chat| over the last four degrees of either axis -- for the series of an INTERPOLANT
    // (K1i: the coefficients beyond the node count are not zero, they alias into these) the figure its band extrapolates the
    // aliasing error from; K1b's core is the exact product of degree-(rc - 1) polynomials and holds zeros there
    reinterpret_cast<double*>(eff + 4 * dm.q)[gridDim.x + o] = f;
  }
}
// ChatT [D1m][D0m] -> the B fragments of stage 1 (T4f layout: k = axis-1 degree, column = axis-0 degree)
__global__ __launch_bounds__(256) void k_cheb_t4f(const BlDims dm, const double* __restrict__ Chat_all, size_t sT4f, double* __restrict__ T4fall) {
  const int o = blockIdx.y, KB0 = dm.KB0, KB1 = dm.KB1;
  const double* Ch = Chat_all + (size_t)o * dm.D0m * dm.D1m;
  double* T4f = T4fall + (size_t)o * sT4f;
  const long long total = (long long)KB0 * KB1 * 4 * 64;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int l = (int)(i & 63);
    const long long fr = i >> 6;
    const int ks = (int)(fr % (KB1 * 4)), cs = (int)(fr / (KB1 * 4));
    const int k1 = (ks >> 2) * 16 + MM<double>::jslot(ks & 3, l >> 4);
    const int k0 = cs * 16 + (l & 15);
    T4f[i] = Ch[(size_t)k1 * dm.D0m + k0];
  }
}
// Chebyshev polynomials of the grid positions in the operand layouts of the two GEMMs (k_bl_pairs' layouts): FRAG 1: B
// fragments [ncs0][KB0 * 4][64] of axis 0; FRAG 0: A images [nrb][KB1][256] of axis 1.  A thread per position walks the
// three-term recurrence once (the argument exactly as k_bl_stab forms it); the same table serves every output.
template <int FRAG>
__global__ __launch_bounds__(256) void k_cheb_tab(const BlDims dm, const double* __restrict__ xn, double* __restrict__ out) {
  const int KB = FRAG ? dm.KB0 : dm.KB1, nblk = FRAG ? dm.ncs0 : dm.nrb;
  const long long count = FRAG ? dm.cnt0 : dm.nlines;
  const double a = dm.a[FRAG ? 0 : 1], b = dm.b[FRAG ? 0 : 1];
  for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < (long long)nblk * 16; x += (long long)gridDim.x * blockDim.x) {
    double xi = 0.0;
    if (x < count) {
      xi = (2.0 * xn[x] - (a + b)) / (b - a);
      xi = xi < 1.0 ? xi : 1.0;
      xi = xi > -1.0 ? xi : -1.0;
    }
    double t0 = 1.0, t1 = xi;
    for (int k = 0; k < KB * 16; ++k) {
      double v = k == 0 ? t0 : t1;
      if (k >= 2) {
        v = 2.0 * xi * t1 - t0;
        t0 = t1;
        t1 = v;
      }
      if (x >= count) v = 0.0;
      size_t idx;
      if (FRAG) {
        // fragment (strip = x / 16, k-step ks = k / 4 ... ): element of k-block kb = k / 16 with jslot(kk, slot) = k % 16
        const int kb = k >> 4, j = k & 15, kk = j >> 2, slot = j & 3;      // MM<double>::jslot(kk, slot) = 4 kk + slot
        idx = (((size_t)(x >> 4) * (KB * 4) + (size_t)(kb * 4 + kk)) << 6) + (size_t)(slot * 16 + (x & 15));
      } else {
        const int kb = k >> 4, j = k & 15, kk = j >> 2, slot = j & 3;
        idx = (((size_t)(x >> 4) * KB + kb) << 8) + (size_t)MM<double>::pack_pos((int)(x & 15), slot, kk);
      }
      out[idx] = v;
    }
  }
}

// K1b's own representation at the probe points of its guard band (guard.hip), from the plan's tables -- the sums the two GEMMs
// of a posterior launch form, term by term in another order (the difference is their rounding, which the band's floor covers):
//   quad = sum_{a < A, b < B} ChatT[b][a] T_a(xi0) T_b(xi1)   over the degrees the kernels run (eff), T by the tables' recurrence
//   mean = mp + sum_p Vb0[p][line] S0[p][x0]
// A wave per (probe, output): lane l takes the rows b = l, l + 64, .. of ChatT (its T_b by the recurrence up to b, then the row's
// sum over a with T_a walked along), the lanes' shares meet in a wave sum.  (A thread per probe walked 2304 dependent steps: 105 us.)
__global__ __launch_bounds__(256) void k_gb_probe_k1b(const ModelConst mc, const CandSpec cs, const BlDims dm, const double* __restrict__ ChatT_all,
                                                      const int* __restrict__ eff, const double* __restrict__ xn0, const double* __restrict__ xn1,
                                                      const double* __restrict__ S0all, const double* __restrict__ Vball,
                                                      double* __restrict__ pm, double* __restrict__ pv) {
  const int o = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D0 = dm.D0m;
  const int p = blockIdx.x * 4 + wave;
  if (p >= kGbProbes) return;                      // (no barriers in this kernel)
  const int A = eff[4 * o] * 4, B = eff[4 * o + 2] * 16;
  const double* Ch = ChatT_all + (size_t)o * D0 * dm.D1m;
  long long x0, x1;
  gb_probe_xy(cs, dm.nlines, p, x0, x1);
  auto xi_of = [&](double xn, int axis) {
    double xi = (2.0 * xn - (dm.a[axis] + dm.b[axis])) / (dm.b[axis] - dm.a[axis]);
    xi = xi < 1.0 ? xi : 1.0;
    return xi > -1.0 ? xi : -1.0;
  };
  const double xi0 = xi_of(xn0[x0], 0), xi1 = xi_of(xn1[x1], 1);
  double quad = 0.0;
  for (int b = lane; b < B; b += 64) {
    double tb0 = 1.0, tb1 = xi1, tb = b == 0 ? 1.0 : xi1;
    for (int k = 2; k <= b; ++k) { tb = 2.0 * xi1 * tb1 - tb0; tb0 = tb1; tb1 = tb; }
    const double* rowp = Ch + (size_t)b * D0;
    double row = 0.0, ta0 = 1.0, ta1 = xi0;
    for (int a = 0; a < A; ++a) {
      double ta = a == 0 ? 1.0 : xi0;
      if (a >= 2) { ta = 2.0 * xi0 * ta1 - ta0; ta0 = ta1; ta1 = ta; }
      row = fma(rowp[a], ta, row);
    }
    quad = fma(row, tb, quad);
  }
  quad = wave_sum(quad);
  const int r0 = dm.r0[o];
  const double* S0 = S0all + (size_t)o * dm.r0u * dm.cnt0;
  const double* Vb = Vball + (size_t)o * 3 * dm.r0u * dm.nlines;
  double ms = 0.0;
  for (int pp = lane; pp < r0; pp += 64) ms = fma(Vb[(size_t)pp * dm.nlines + x1], S0[(size_t)pp * dm.cnt0 + x0], ms);
  ms = wave_sum(ms);
  if (lane == 0) {
    double var = mc.sf2[o] - quad;
    var = var > 0.0 ? var : 0.0;
    const double ys = mc.Y_std[o];
    pm[(size_t)o * kGbProbes + p] = (mc.mp[o] + ms) * ys + mc.Y_mean[o];
    pv[(size_t)o * kGbProbes + p] = var * (ys * ys);
  }
}

// ---- Lipschitz keys without the gradient phases on every tile (r04) ------------------------------------------------------------
// L_i = max over the grid of ||grad MEAN_i||_inf (models/SafeOpt.py:68-83) took two of k_bpost's four GEMM phases on EVERY tile
// -- ~90 of its 257 us on config H -- for two scalars per output.  The gradient sums are polynomials of the axes' Chebyshev
// variables (degree <= rc per axis, the degree of the bases), so:
//   (1) k_bl_gradw / k_bl_gradrow / k_bl_gradslack, per plan: the Chebyshev coefficients C[a][b] of g_0 = f_1 - xn0 f_0 and g_1 = f_2 - xn1 f_0 (f_b the
//       three bilinear forms of the mean phases) and from them sum |C| a^2, sum |C| b^2 >= max |dg / dxi| (|T_a'| <= a^2) -> a
//       bound `slack` on how far |g| can move over half a sampling cell;
//   (2) k_bl_gradcoarse, per plan: g at the centres of kGradStep x kGradStep cells of the grid (direct sums over the rank,
//       1 / 64 of the candidates) -> the largest sample of every k_bpost tile and of the whole grid;
//   (3) k_bpost runs a gradient phase only on the tiles whose largest sample + slack reaches the grid's largest sample: no
//       other tile can hold the maximum.  The key is still the maximum of the FINE-grid values of phases 2 / 3 (on those tiles),
//       i.e. the same number as before, to the last bit.  Config H: ~1-7 % of the tiles qualify.
constexpr int kGradStep = 8;
// coefficient bounds in three small launches (one workgroup per output took 0.21 ms of the plan build):
//   k_bl_gradw      W_b[p][c1] = sum_s Mb_b[p][s] sig1_s Vs1[s][c1]                       grid (3 r0u, q), a thread per c1
//   k_bl_gradrow    row a of the coefficient matrices C_b[a][c1] = sum_p sig0_p Vs0[p][a] W_b[p][c1] (C_0 also for a - 1, a + 1),
//                   the products with xn = mid + half xi by  xi T_0 = T_1, xi T_k = (T_{k+1} + T_{k-1}) / 2,  and the row's part
//                   of sum |C| a^2, sum |C| c1^2 for both gradient components                 grid (rc0m + 1, q)
//   k_bl_gradslack  the rows' parts summed in a fixed order -> slack[o][component]            grid (q)
__global__ __launch_bounds__(128) void k_bl_gradw(const BlDims dm, const double* __restrict__ Vsall, const double* __restrict__ sigall,
                                                  const double* __restrict__ Mball, double* __restrict__ Wscr /* [q][3][kBlMaxR][kBlMaxRc] */) {
  const int o = blockIdx.y, b = blockIdx.x / dm.r0u, p = blockIdx.x % dm.r0u, c1 = threadIdx.x;
  const int r0 = dm.r0[o], r1 = dm.r1[o], rc1 = dm.rc1[o];
  if (p >= r0 || c1 >= rc1) return;
  const double* Vs1 = Vsall + (size_t)(2 * o + 1) * kBlMaxR * kBlMaxRc;
  const double* sig1 = sigall + (size_t)(2 * o + 1) * kBlMaxR;
  const double* Mb = Mball + (size_t)o * 3 * dm.r0u * dm.r1u + ((size_t)b * r0 + p) * r1;
  double s = 0.0;
  for (int s_ = 0; s_ < r1; ++s_) s += Mb[s_] * (sig1[s_] * Vs1[(size_t)s_ * rc1 + c1]);
  Wscr[(((size_t)o * 3 + b) * kBlMaxR + p) * kBlMaxRc + c1] = s;
}
__global__ __launch_bounds__(256) void k_bl_gradrow(const BlDims dm, const double* __restrict__ Vsall, const double* __restrict__ sigall,
                                                    const double* __restrict__ Wscr, double* __restrict__ part /* [q][gridDim.x][4] */) {
  __shared__ double c0row[kBlMaxRc + 3];                 // C_0[a][-1 .. rc1 + 1] (zero outside the degrees)
  __shared__ double red[4][4];
  const int o = blockIdx.y, a = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c1 = tid;
  const int r0 = dm.r0[o], rc0 = dm.rc0[o], rc1 = dm.rc1[o];
  double b00 = 0.0, b01 = 0.0, b10 = 0.0, b11 = 0.0;       // [component][axis]: |coefficient| degree^2
  const bool row = a <= rc0;                               // (uniform: the products with xi reach one degree further)
  if (row) {
    const double* Vs0 = Vsall + (size_t)(2 * o) * kBlMaxR * kBlMaxRc;
    const double* sig0 = sigall + (size_t)(2 * o) * kBlMaxR;
    const double* W = Wscr + (size_t)o * 3 * kBlMaxR * kBlMaxRc;
    // C_0 at rows a - 1, a, a + 1, C_1 and C_2 at row a, column c1 of this thread
    double c0m = 0.0, c0 = 0.0, c0p = 0.0, c1v = 0.0, c2v = 0.0;
    if (c1 < rc1)
      for (int p = 0; p < r0; ++p) {
        const double w0 = W[((size_t)0 * kBlMaxR + p) * kBlMaxRc + c1], w1 = W[((size_t)1 * kBlMaxR + p) * kBlMaxRc + c1],
                     w2 = W[((size_t)2 * kBlMaxR + p) * kBlMaxRc + c1];
        const double* v = Vs0 + (size_t)p * rc0;
        const double sg = sig0[p];
        const double am = a >= 1 ? sg * v[a - 1] : 0.0, aa = a < rc0 ? sg * v[a] : 0.0, ap = a + 1 < rc0 ? sg * v[a + 1] : 0.0;
        c0m += am * w0;
        c0 += aa * w0;
        c0p += ap * w0;
        c1v += aa * w1;
        c2v += aa * w2;
      }
    if (c1 <= rc1 + 2) c0row[c1] = 0.0;
    __syncthreads();
    if (c1 < rc1) c0row[c1 + 1] = c0;
    __syncthreads();
    if (c1 <= rc1) {
      const double mid0 = 0.5 * (dm.a[0] + dm.b[0]), half0 = 0.5 * (dm.b[0] - dm.a[0]);
      const double mid1 = 0.5 * (dm.a[1] + dm.b[1]), half1 = 0.5 * (dm.b[1] - dm.a[1]);
      // (xi F)_a along the first index: D_0 = C_1 / 2, D_1 = C_0 + C_2 / 2, D_a = (C_{a-1} + C_{a+1}) / 2
      const double sh0 = a == 0 ? 0.5 * c0p : (a == 1 ? c0m + 0.5 * c0p : 0.5 * (c0m + c0p));
      const double lo = c0row[c1], hi = c0row[c1 + 2];     // C_0[a][c1 - 1], C_0[a][c1 + 1]
      const double sh1 = c1 == 0 ? 0.5 * hi : (c1 == 1 ? lo + 0.5 * hi : 0.5 * (lo + hi));
      const double g0c = c1v - mid0 * c0 - half0 * sh0;    // coefficient (a, c1) of g_0 = f_1 - xn0 f_0
      const double g1c = c2v - mid1 * c0 - half1 * sh1;    //                     of g_1 = f_2 - xn1 f_0
      const double a2 = (double)a * a, c2 = (double)c1 * c1;
      b00 = fabs(g0c) * a2;
      b01 = fabs(g0c) * c2;
      b10 = fabs(g1c) * a2;
      b11 = fabs(g1c) * c2;
    }
  }
  b00 = wave_sum(b00); b01 = wave_sum(b01); b10 = wave_sum(b10); b11 = wave_sum(b11);
  if (lane == 0) { red[wave][0] = b00; red[wave][1] = b01; red[wave][2] = b10; red[wave][3] = b11; }
  __syncthreads();
  if (tid < 4) part[((size_t)o * gridDim.x + a) * 4 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}
__global__ __launch_bounds__(64) void k_bl_gradslack(const double* __restrict__ part, int rows, double dxi0, double dxi1 /* half a sampling cell
                                                     in xi units */, double* __restrict__ slack /* [q][2] */) {
  const int o = blockIdx.x, k = threadIdx.x;
  if (k >= 4) return;
  double s = 0.0;
  for (int a = 0; a < rows; ++a) s += part[((size_t)o * rows + a) * 4 + k];
  // |g| moves by at most max |dg/dxi0| dxi0 + max |dg/dxi1| dxi1 between a candidate and the sample of its cell
  const double t = s * ((k & 1) ? dxi1 : dxi0);
  const double other = __shfl_xor(t, 1);
  if ((k & 1) == 0) slack[2 * o + (k >> 1)] = (t + other) * (1.0 + 1e-9);
}
// the gradient sums at the cell centres of one k_bpost tile (TL lines x 128 positions): a workgroup per (tile, output); the
// tile's columns of S0 and lines of Vb go through LDS (read straight from memory, strided by the cell: 0.11 ms on config H).
// tmax[(o 2 + comp) ntiles + tile] = the tile's largest |g_comp| sample, gkey[o 2 + comp] = the grid's (bit pattern: values >= 0)
constexpr int kGradTL = 64, kGradNpx = 128 / kGradStep, kGradNpl = kGradTL / kGradStep;
__global__ __launch_bounds__(128) void k_bl_gradcoarse(const BlDims dm, const double* __restrict__ S0all, const double* __restrict__ Vball,
                                                       const double* __restrict__ xn0, const double* __restrict__ xn1, int ntx,
                                                       double* __restrict__ tmax, unsigned long long* __restrict__ gkey) {
  __shared__ double sS[kBlMaxR][kGradNpx];
  __shared__ double sV[3][kBlMaxR][kGradNpl];
  __shared__ double red[2][2];
  const int o = blockIdx.y, tile = blockIdx.x, bx = tile % ntx, by = tile / ntx;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = dm.r0[o];
  const double* S0 = S0all + (size_t)o * dm.r0u * dm.cnt0;
  const double* Vb = Vball + (size_t)o * 3 * dm.r0u * dm.nlines;
  // the centre of the cell, or the last candidate of a cell the grid ends in: every candidate within kGradStep / 2 of a sample
  auto xs = [&](int i) { const long long x = (long long)bx * 128 + i * kGradStep; return x >= dm.cnt0 ? -1ll : (x + kGradStep / 2 < dm.cnt0 ? x + kGradStep / 2 : dm.cnt0 - 1); };
  auto ls = [&](int j) { const long long l = (long long)by * kGradTL + j * kGradStep; return l >= dm.nlines ? -1ll : (l + kGradStep / 2 < dm.nlines ? l + kGradStep / 2 : dm.nlines - 1); };
  for (int e = tid; e < r0 * kGradNpx; e += blockDim.x) {
    const int p = e / kGradNpx, i = e % kGradNpx;
    const long long x = xs(i);
    sS[p][i] = x >= 0 ? S0[(size_t)p * dm.cnt0 + x] : 0.0;
  }
  for (int e = tid; e < 3 * r0 * kGradNpl; e += blockDim.x) {
    const int j = e % kGradNpl, p = (e / kGradNpl) % r0, b = e / (kGradNpl * r0);
    const long long l = ls(j);
    sV[b][p][j] = l >= 0 ? Vb[((size_t)b * dm.r0u + p) * dm.nlines + l] : 0.0;
  }
  __syncthreads();
  double m0 = 0.0, m1 = 0.0;
  {
    const int i = tid % kGradNpx, j = tid / kGradNpx;      // 16 x 8 samples: one per thread
    const long long x = xs(i), l = ls(j);
    if (x >= 0 && l >= 0) {
      const double x0n = xn0[x], x1n = xn1[l];
      double g0 = 0.0, g1 = 0.0;
      for (int p = 0; p < r0; ++p) {
        const double s0 = sS[p][i], v0 = sV[0][p][j];
        g0 = fma(sV[1][p][j] - x0n * v0, s0, g0);
        g1 = fma(sV[2][p][j] - x1n * v0, s0, g1);
      }
      m0 = fabs(g0);
      m1 = fabs(g1);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    m0 = fmax(m0, __shfl_xor(m0, off));
    m1 = fmax(m1, __shfl_xor(m1, off));
  }
  if (lane == 0) { red[wave][0] = m0; red[wave][1] = m1; }
  __syncthreads();
  if (tid == 0) {
    m0 = fmax(m0, red[1][0]);
    m1 = fmax(m1, red[1][1]);
    const size_t nt = (size_t)gridDim.x;
    tmax[((size_t)o * 2 + 0) * nt + tile] = m0;
    tmax[((size_t)o * 2 + 1) * nt + tile] = m1;
    // (the grid's largest samples: k_bl_gradmax -- 4096 workgroups on four addresses queue their atomics up in L2)
  }
}
__global__ __launch_bounds__(256) void k_bl_gradmax(const double* __restrict__ tmax, int nt, unsigned long long* __restrict__ gkey) {
  __shared__ double red[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  double m = 0.0;
  for (int i = tid; i < nt; i += blockDim.x) m = fmax(m, tmax[(size_t)row * nt + i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) gkey[row] = (unsigned long long)__double_as_longlong(fmax(fmax(red[0], red[1]), fmax(red[2], red[3])));
}

// ---- plan ------------------------------------------------------------------------------------------------
static double axis_position(const sbo_ctx* c, int a, long long i) {
  const CandSpec& cs = c->cs;
  const long long tot = cs.count[a];
  const double x = (i == tot - 1 && tot > 1) ? cs.hi[a] : cs.lo[a] + (double)i * cs.step[a];
  return (x - c->mc.X_mean[a]) / c->mc.X_std[a];                                                  // GP_Safe.py:326
}

bool bilinear_applicable(const sbo_ctx* c) {
  const CandSpec& cs = c->cs;
  if (!c->opt.bilinear || c->dtype != SBO_F64 || !c->has_cand || cs.kind != 1 || cs.d != 2 || c->mc.d != 2) return false;
  const long long cnt0 = cs.count[0];
  if ((cs.n_local <= 0 && !(c->dist.sharded && c->dist.world > 1)) || cs.first % cnt0 != 0 || cs.n_local % cnt0 != 0) return false;
  // the bases pay off (and the interpolation interval is meaningful) only on real grids
  // (ranks > 1: ONE decision for all of them -- the recheck behind an approximating posterior contains collectives, so a rank that
  // took the exact kernel K1g for its 15-line shard would return while its 16-line neighbours wait for it there.  The shard sizes
  // are known to every rank: the smallest one decides.)
  long long min_lines = cs.n_local / cnt0;
  if (c->dist.sharded && c->dist.first_of.size() == (size_t)c->dist.world + 1)
    for (int r = 0; r < c->dist.world; ++r) min_lines = std::min(min_lines, (c->dist.first_of[r + 1] - c->dist.first_of[r]) / cnt0);
  // (a caller's matrix whose factor is deferred: the band's reference runs on the matrix itself and must fit its LDS budget)
  if (c->mc.factor == SBO_FACTOR_INVK && c->opt.chol_async && c->mc.npad > kGuardRefMaxNpad) return false;
  return cnt0 >= 64 && cs.count[1] >= 64 && min_lines >= 16 && c->factor.present() && c->factor.ld() >= c->mc.n;
}

// layout of bl_basis (doubles): U [2q][kBlMaxR][n] | Vs [2q][kBlMaxR][kBlMaxRc] | sig [2q][kBlMaxR] | info (ints, 2q x 4, in
// 4 q doubles) | rcjob | eps [2q][2] | work [2q][3 n kBlMaxRc + kBlMaxR kBlMaxRc]
struct BasisLayout {
  size_t U, Vs, sig, info, rcjob, eps, work, work_stride, total;
};
static BasisLayout basis_layout(int n, int q) {
  BasisLayout L;
  L.U = 0;
  L.Vs = L.U + (size_t)2 * q * kBlMaxR * n;
  L.sig = L.Vs + (size_t)2 * q * kBlMaxR * kBlMaxRc;
  L.info = L.sig + (size_t)2 * q * kBlMaxR;
  L.rcjob = L.info + (size_t)4 * q;                 // ints, 2 q (in q doubles): the degree k_bl_degree found per job
  L.eps = L.rcjob + (size_t)q;                      // [2 q][2]: truncation figures of the axis factors for the guard band (GbAnalytic)
  L.work = L.eps + (size_t)4 * q;
  L.work_stride = (size_t)3 * n * kBlMaxRc + (size_t)kBlMaxR * kBlMaxRc;
  L.total = L.work + (size_t)2 * q * L.work_stride;
  return L;
}

// The interval of each grid axis in normalised coordinates.  Axis 1 always spans the WHOLE axis, so that every rank of a
// sharded grid builds the same functions (shard results are bit-identical to the whole grid's).
static bool basis_intervals(const sbo_ctx* c, double (&ab)[4]) {
  for (int a = 0; a < 2; ++a) {
    const double x0 = axis_position(c, a, 0), x1 = axis_position(c, a, c->cs.count[a] - 1);
    ab[2 * a] = std::min(x0, x1);
    ab[2 * a + 1] = std::max(x0, x1);
    if (!(ab[2 * a + 1] > ab[2 * a])) return false;
  }
  return true;
}

// Enqueues the 2 q basis workgroups and the read-back of their (ok, r, rc) records on `st`; the caller synchronises.
// Used by bilinear_setup, and ahead of time by sbo_model_set (next to the factorisation, on a second stream) when a grid
// is already resident.
int bilinear_basis_enqueue(sbo_ctx* c, hipStream_t st, bool force_big) {
  const ModelConst& mc = c->mc;
  const int n = mc.n, q = mc.q;
  double ab[4];
  c->bl_basis_ok = false;
  if (!basis_intervals(c, ab)) return SBO_OK;
  const BasisLayout L = basis_layout(n, q);
  int rc;
  if ((rc = ensure(c->bl_basis, sizeof(double) * L.total))) return rc;
  double* base = (double*)c->bl_basis.p;
  {
    BlJobs jb;
    memset(&jb, 0, sizeof(jb));
    jb.n = n;
    jb.dpad = mc.dpad;
    for (int o = 0; o < q; ++o)
      for (int a = 0; a < 2; ++a) jb.vinv[2 * o + a] = mc.vinv[o][a];
    for (int a = 0; a < 2; ++a) { jb.a[a] = ab[2 * a]; jb.b[a] = ab[2 * a + 1]; }
    // n <= 128: 256 threads, samples / residual rows in LDS (degree <= 64 assumed: a larger one fails over to the big form)
    const bool small = !force_big && n <= kBasisResLds / 64;
    const size_t dyn = sizeof(double) * (kBasisQLds + (small ? kBasisResLds : 0));
    DevBuf dbgbuf;
    const bool phases = getenv("SBO_BL_TIMING") != nullptr;
    long long* dbg = phases && ensure(dbgbuf, sizeof(long long) * 81) == SBO_OK ? (long long*)dbgbuf.p : nullptr;
    // front end on the whole chip: degree per job, then its coefficient rows into the jobs' workspaces
    int* rcjob = (int*)(base + L.rcjob);
    SBO_HIP(hipMemsetAsync(rcjob, 0, sizeof(double) * 5 * q, st));          // (the degrees and, behind them, the truncation figures)
    hipLaunchKernelGGL(k_bl_degree, dim3((unsigned)((n + 63) / 64), (unsigned)(2 * q)), dim3(256), 0, st, jb, (const double*)c->Xn.p, rcjob);
    hipLaunchKernelGGL(k_bl_coef, dim3((unsigned)((n + kCoefRows - 1) / kCoefRows), (unsigned)(2 * q)), dim3(256), 0, st, jb,
                       (const double*)c->Xn.p, (const int*)rcjob, base + L.work, L.work_stride, base + L.eps);
    for (int rep = 0; rep < (dbg ? 2 : 1); ++rep) {       // (with SBO_BL_TIMING a second run records the phase stamps of job 0)
      long long* dg = rep ? dbg : nullptr;
      if (rep)      // (the pivot loop consumed the rows in place)
        hipLaunchKernelGGL(k_bl_coef, dim3((unsigned)((n + kCoefRows - 1) / kCoefRows), (unsigned)(2 * q)), dim3(256), 0, st, jb,
                           (const double*)c->Xn.p, (const int*)rcjob, base + L.work, L.work_stride, base + L.eps);
      if (small) {
        SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_bl_basis<256, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
        hipLaunchKernelGGL((k_bl_basis<256, true>), dim3((unsigned)(2 * q)), dim3(256), dyn, st, jb, (const double*)c->Xn.p, base + L.work,
                           L.work_stride, base + L.U, base + L.Vs, base + L.sig, (int*)(base + L.info), dg, (const int*)rcjob, 0, base + L.eps);
      } else {
        SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_bl_basis<1024, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
        hipLaunchKernelGGL((k_bl_basis<1024, false>), dim3((unsigned)(2 * q)), dim3(1024), dyn, st, jb, (const double*)c->Xn.p, base + L.work,
                           L.work_stride, base + L.U, base + L.Vs, base + L.sig, (int*)(base + L.info), dg, (const int*)rcjob, 0, base + L.eps);
      }
    }
    SBO_HIP(hipGetLastError());
    if (dbg) {
      long long h[81];
      if (hipMemcpyAsync(h, dbg, sizeof(h), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess) {
        fprintf(stderr, "[k_bl_basis] job 0 phases (us):");
        for (int i = 1; i < (int)h[80]; ++i) fprintf(stderr, " %.1f", (double)(h[i] - h[i - 1]) / 100.0);
        fprintf(stderr, "\n");
      }
    }
  }
  SBO_HIP(hipMemcpyAsync(c->h_back->basis_info, base + L.info, sizeof(int) * 8 * q, hipMemcpyDeviceToHost, st));
  for (int t = 0; t < 4; ++t) c->bl_basis_ab[t] = ab[t];
  c->bl_basis_serial = c->model_serial;
  c->bl_basis_ok = true;       // (enqueued: valid once `st` has drained)
  return SBO_OK;
}

static bool basis_current(const sbo_ctx* c) {
  double ab[4];
  if (!c->bl_basis_ok || c->bl_basis_serial != c->model_serial || !basis_intervals(c, ab)) return false;
  for (int t = 0; t < 4; ++t)
    if (ab[t] != c->bl_basis_ab[t]) return false;
  return true;
}

// Builds the device tables for the current (model, candidates).  Returns SBO_OK with plan.usable = false when the bases do
// not qualify (rank / interpolation limits): the caller then keeps the separable-table kernel.
int bilinear_setup(sbo_ctx* c) {
  BilinearPlan& pl = c->bl;
  pl.valid = true;
  pl.usable = false;
  pl.ops = GemmOps();
  GemmOps& g = pl.ops;
  pl.encl_ready = false;
  pl.lrows_ready = false;
  pl.omap_dirty = true;      // (a new plan: no tile of the objective holds its bits yet)
  pl.bt_ready = false;      // (new tables below: stage 1 runs again with the plan's first launch)
  pl.setup_ms = 0.0;
  const auto t_begin = std::chrono::steady_clock::now();
  const bool timing = getenv("SBO_BL_TIMING") != nullptr;
  auto lap = [&](const char* what) {
    if (timing) fprintf(stderr, "[K1b setup] %-12s %8.2f ms\n", what,
                        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
  };
  const ModelConst& mc = c->mc;
  const CandSpec& cs = c->cs;
  const int n = mc.n, q = mc.q;
  const long long cnt0 = cs.count[0], nlines = cs.n_local / cnt0, line0 = cs.first / cnt0;
  int rc;
  if (!basis_current(c)) {
    if ((rc = bilinear_basis_enqueue(c, c->stream, false))) return rc;
    if (!c->bl_basis_ok) return SBO_OK;
    SBO_HIP(hipStreamSynchronize(c->stream));
  }
  const int* inf = c->h_back->basis_info;
  for (int t = 0; t < 2 * q; ++t)
    if (inf[4 * t] == 2) {                 // the small form of the basis kernel needs more LDS than it has: the big form
      if ((rc = bilinear_basis_enqueue(c, c->stream, true))) return rc;
      SBO_HIP(hipStreamSynchronize(c->stream));
      break;
    }
  lap("bases");
  BlDims dm;
  memset(&dm, 0, sizeof(dm));
  int r0u = 0, r1u = 0, K0 = 0, K1 = 0, Rmax = 0, rc0m = 0, rc1m = 0;
  for (int o = 0; o < q; ++o) {
    if (inf[8 * o] != 1 || inf[8 * o + 4] != 1) return SBO_OK;    // a basis did not qualify
    dm.r0[o] = inf[8 * o + 1]; dm.rc0[o] = inf[8 * o + 2];
    dm.r1[o] = inf[8 * o + 5]; dm.rc1[o] = inf[8 * o + 6];
    if (dm.r0[o] < 1 || dm.r0[o] > kBlMaxR || dm.r1[o] < 1 || dm.r1[o] > kBlMaxR) return SBO_OK;
    r0u = std::max(r0u, dm.r0[o]);
    r1u = std::max(r1u, dm.r1[o]);
    K0 = std::max(K0, pair_count(dm.r0[o]));
    K1 = std::max(K1, pair_count(dm.r1[o]));
    Rmax = std::max(Rmax, dm.r0[o] * dm.r1[o]);
    rc0m = std::max(rc0m, dm.rc0[o]);
    rc1m = std::max(rc1m, dm.rc1[o]);
    dm.sf2[o] = mc.sf2[o];
    pl.r0[o] = dm.r0[o];
    pl.r1[o] = dm.r1[o];
    if (timing) fprintf(stderr, "[K1b setup] output %d: r0 %d (degree %d), r1 %d (degree %d)\n", o, dm.r0[o], dm.rc0[o], dm.r1[o], dm.rc1[o]);
  }
  // inner dimensions of the two GEMMs of the variance phase: the degrees of quad as a polynomial of the axis (D = 2 rc - 1, cut
  // on the device where its coefficients have decayed); K0m / K1m: the pair counts r (r + 1) / 2 the core is contracted from
  const int K0m = K0, K1m = K1;
  K0 = 2 * rc0m - 1;
  K1 = 2 * rc1m - 1;
  const int KB0 = (K0 + 15) / 16, KB1 = (K1 + 15) / 16;
  const int ncs0 = (int)((cnt0 + 15) / 16), nrb = (int)((nlines + 15) / 16);
  {
    // worth it only while the two GEMMs issue clearly fewer flops than the triangular contraction of K1g
    const double gemm = (double)nlines * KB0 * 16.0 * KB1 * 16.0 + (double)cs.n_local * (KB0 * 16.0 + 3.0 * r0u);
    const double tri = 0.5 * (double)mc.npad * (mc.npad + 16.0) * (double)cs.n_local;
    if (gemm > 0.7 * tri) return SBO_OK;
  }
  const long long nlines_pad = (long long)nrb * 16;
  pl.r0u = r0u; pl.nlines_pad = nlines_pad;
  g.KB0 = KB0; g.KB1 = KB1; g.ncs0 = ncs0; g.nrb = nrb;
  g.sP0f = g.sP1A = 0;                                     // (one table of Chebyshev polynomials for every output)
  const size_t nP0f = (size_t)ncs0 * KB0 * 4 * 64, nP1A = (size_t)nrb * KB1 * 256;
  g.sT4f = (size_t)KB0 * KB1 * 4 * 64;
  g.sBtA = g.sBt1 = (size_t)nrb * KB0 * 256;
  // mean phases: K = r0p (basis size rounded to whole k-steps); the axis-0 gradient phase concatenates two such operands
  const int r0p = (r0u + 3) / 4 * 4;
  const int KBm = (r0p + 15) / 16, KBm2 = (2 * r0p + 15) / 16;
  g.KBm = KBm; g.KBm2 = KBm2; g.KSm = r0p / 4; g.KS0 = KB0 * 4;
  g.sVA = (size_t)nrb * (2 * KBm + KBm2) * 256;     // image sets  V0 | [V1; V0] | V1x
  g.sSBf = (size_t)ncs0 * (KBm + KBm2) * 256;      // fragment sets  S0 | [S0; -xn0 S0]
  if ((rc = ensure(c->bl_P0f, sizeof(double) * nP0f))) return rc;
  if ((rc = ensure(c->bl_P1A, sizeof(double) * nP1A))) return rc;
  // Chebyshev core scratch: PC0 | PC1 | T4 plain | Y^T | Chat | eff (ints)
  const size_t D0m = (size_t)KB0 * 16, D1m = (size_t)KB1 * 16;
  // (PC0 as B fragments [D0m / 16][KBp0 * 4][64], PC1^T as A images [D1m / 16][KBp1][256], T4^T as B fragments [KBp0][KBp1 * 4][64],
  // Y' = PC1^T T4^T as A images [D1m / 16][KBp0][256], Chat^T [D1m][D0m] row-major)
  const int KBp0 = (K0m + 15) / 16, KBp1 = (K1m + 15) / 16;
  const size_t nPC0 = D0m * (size_t)KBp0 * 16, nPC1 = D1m * (size_t)KBp1 * 16, nT4p = (size_t)KBp0 * KBp1 * 256, nYt = D1m * (size_t)KBp0 * 16,
               nCh = D0m * D1m;
  if ((rc = ensure(c->bl_cheb, sizeof(double) * (size_t)q * (nPC0 + nPC1 + nT4p + nYt + nCh) + 256))) return rc;
  if ((rc = ensure(c->bl_T4f, sizeof(double) * g.sT4f * q))) return rc;
  if ((rc = ensure(c->bl_SBf, sizeof(double) * g.sSBf * q))) return rc;     // mean-phase B fragments
  if ((rc = ensure(c->bl_VA, sizeof(double) * g.sVA * q))) return rc;      // mean-phase A images
  if ((rc = ensure(c->bl_BtA, sizeof(double) * g.sBtA * q))) return rc;
  g.BtA = (double*)c->bl_BtA.p; g.P0f = (double*)c->bl_P0f.p; g.VA = (double*)c->bl_VA.p; g.SBf = (double*)c->bl_SBf.p;
  const int KBn = mc.npad / 16, ncsR = (Rmax + 15) / 16;
  const size_t nZf = (size_t)ncsR * KBn * 256;                // fragments of Z, of C, images of C^T: same size
  const size_t ldg = (size_t)ncsR * 16;
  if ((rc = ensure(c->bl_work, sizeof(double) * (size_t)q * (3 * nZf + ldg * ldg)))) return rc;
  // bl_small: xn0 | xn1 (local lines) | S0 | S1 | Mb | Vb  -- everything made on the device
  const size_t oS0 = (size_t)cnt0 + (size_t)nlines, oS1 = oS0 + (size_t)q * r0u * cnt0, oMb = oS1 + (size_t)q * r1u * nlines,
               oVb = oMb + (size_t)q * 3 * r0u * r1u, oEnd = oVb + (size_t)q * 3 * r0u * nlines;
  if ((rc = ensure(c->bl_small, sizeof(double) * oEnd))) return rc;
  dm.K0m = K0m; dm.K1m = K1m; dm.D0m = (int)D0m; dm.D1m = (int)D1m;
  dm.q = q; dm.n = n; dm.KBn = KBn;
  dm.r0u = r0u; dm.r1u = r1u; dm.r0p = r0p; dm.KB0 = KB0; dm.KB1 = KB1; dm.KBm = KBm; dm.KBm2 = KBm2;
  dm.ncs0 = ncs0; dm.nrb = nrb; dm.ncsR = ncsR; dm.cnt0 = cnt0; dm.nlines = nlines;
  for (int a = 0; a < 2; ++a) { dm.a[a] = c->bl_basis_ab[2 * a]; dm.b[a] = c->bl_basis_ab[2 * a + 1]; }
  const BasisLayout L = basis_layout(n, q);
  const double* bb = (const double*)c->bl_basis.p;
  const double *dU = bb + L.U, *dVs = bb + L.Vs, *dsig = bb + L.sig;
  double* dsm = (double*)c->bl_small.p;
  double *dxn0 = dsm, *dxn1 = dsm + cnt0, *dS0 = dsm + oS0, *dS1 = dsm + oS1, *dMb = dsm + oMb, *dVb = dsm + oVb;
  double* Zf = (double*)c->bl_work.p;
  double* Cf = Zf + (size_t)q * nZf;
  double* CtA = Cf + (size_t)q * nZf;
  double* G = CtA + (size_t)q * nZf;
  auto blocks = [&](size_t total, unsigned y) { return dim3((unsigned)std::min<size_t>((total + 255) / 256, 1u << 16), y); };
  const unsigned uq = (unsigned)q;
  // Two independent chains (r03): X = the form T4 of the variance phase (Z fragments -> two GEMMs -> gather: the long one,
  // ~0.11 ms on config H), Y = everything made from the axis tables (normalised axes, S0 / S1, their pair tables, the mean
  // phases' operands: eight small launches, ~0.09 ms).  Y runs on the second stream beside X and joins before stage 1.
  hipStream_t xs = c->stream, ys = (c->stream2 && !c->is_shadow) ? c->stream2 : c->stream;
  // (r04) Z = the guard band's reference values at the probe points (guard.hip: the reference formula itself, 0.12 ms on config
  // H and independent of everything here): a third stream, or Y -- now also carrying the gradient gate -- becomes the long chain
  hipStream_t zs = (ys != xs && c->stream3) ? c->stream3 : ys;
  if (ys != xs) {
    SBO_HIP(hipEventRecord(c->ev[7], xs));                 // (alpha, Xn and the bases are in place at this point of the main stream)
    SBO_HIP(hipStreamWaitEvent(ys, c->ev[7], 0));
    if (zs != ys) SBO_HIP(hipStreamWaitEvent(zs, c->ev[7], 0));
  }
  // (enqueue order: with a caller's invK the head of the long chain X goes first -- twelve short launches of Y ahead of it cost
  // X ~60 us of host time; with the library's own factor X starts with a host wait for the factorisation, and Y goes first)
  hipLaunchKernelGGL(k_bl_zf, blocks(nZf, uq), dim3(256), 0, xs, dm, dU, nZf, Zf);
  // G = Z^T invK Z.  With the library's own Cholesky factor (M = L^-1): C = M Z from the packed triangular images, written as
  // fragments (k = observation) and as images of C^T, then G = C^T C.  With a CALLER's invK (sbo_ctx::invk_img, r03): W =
  // invK Z with the matrix as given -- the contraction the reference itself performs, models/GP_Safe.py:341-343, no
  // factorisation of an ill-conditioned inverse in between --, then G^T = W^T Z; k_bl_t4f symmetrises what rounding leaves.
  if (mc.factor == SBO_FACTOR_INVK && c->opt.chol_async && !c->invk_img_valid && c->invk_w_valid && (rc = model_pack_invk(c))) return rc;
  const bool direct = mc.factor == SBO_FACTOR_INVK && c->opt.chol_async && c->invk_img_valid;
  auto x_head = [&]() -> int {
  if (!direct && (rc = factor_sync(c))) return rc;
  if (direct) {
    hipLaunchKernelGGL((k_bgemm<4, 0, 1>), dim3((unsigned)((ncsR + 3) / 4), (unsigned)((KBn + 3) / 4), uq), dim3(256), 0, c->stream,
                       (const double*)c->invk_img.p, (size_t)mc.npad * mc.npad, (const double*)Zf, nZf, KBn, KBn, ncsR, Cf, nZf, CtA, 0ll);
    hipLaunchKernelGGL((k_bgemm<4, 0, 2>), dim3((unsigned)((ncsR + 3) / 4), (unsigned)((ncsR + 3) / 4), uq), dim3(256), 0, c->stream,
                       (const double*)CtA, nZf, (const double*)Zf, nZf, KBn, ncsR, ncsR, G, ldg * ldg, (double*)nullptr, (long long)ldg);
  } else {
    hipLaunchKernelGGL((k_bgemm<4, 1, 1>), dim3((unsigned)((ncsR + 3) / 4), (unsigned)((KBn + 3) / 4), uq), dim3(256), 0, c->stream,
                       (const double*)c->Fpk.p, c->fpk_stride, (const double*)Zf, nZf, KBn, KBn, ncsR, Cf, nZf, CtA, 0ll);
    // G = C^T C  (R x R, row-major)
    hipLaunchKernelGGL((k_bgemm<4, 0, 2>), dim3((unsigned)((ncsR + 3) / 4), (unsigned)((ncsR + 3) / 4), uq), dim3(256), 0, c->stream,
                       (const double*)CtA, nZf, (const double*)Cf, nZf, KBn, ncsR, ncsR, G, ldg * ldg, (double*)nullptr, (long long)ldg);
  }
  return SBO_OK;
  };
  if (direct && (rc = x_head())) return rc;
  hipLaunchKernelGGL(k_bl_axes, dim3((unsigned)std::min<long long>((cnt0 + nlines + 255) / 256, 4096)), dim3(256), 0, ys, mc, cs,
                     cnt0, line0, nlines, dxn0, dxn1);
  hipLaunchKernelGGL(k_bl_stab, blocks((size_t)std::max(r0u * cnt0, r1u * nlines), 2 * uq), dim3(256), 0, ys, dm, dVs, dsig,
                     (const double*)dxn0, (const double*)dxn1, dS0, dS1);
  hipLaunchKernelGGL((k_cheb_tab<1>), dim3((unsigned)((ncs0 * 16 + 255) / 256)), dim3(256), 0, ys, dm, (const double*)dxn0, (double*)c->bl_P0f.p);
  hipLaunchKernelGGL((k_cheb_tab<0>), dim3((unsigned)((nrb * 16 + 255) / 256)), dim3(256), 0, ys, dm, (const double*)dxn1, (double*)c->bl_P1A.p);
  // mean phases: Mb (forms of alpha, alpha Xn_0, alpha Xn_1) -> Vb = Mb S1 -> A images [V0 | V1;V0 | V1x], B fragments
  // [S0 | S0;-xn0 S0]
  hipLaunchKernelGGL(k_bl_mb, blocks((size_t)3 * r0u * r1u * 64, uq), dim3(256), 0, ys, dm, dU, c->factor.alpha(),
                     c->factor.a_ld(), (const double*)c->Xn.p, mc.dpad, dMb);
  hipLaunchKernelGGL(k_bl_vb, blocks((size_t)3 * r0u * nlines, uq), dim3(256), 0, ys, dm, (const double*)dMb, (const double*)dS1, dVb);
  hipLaunchKernelGGL(k_bl_va, blocks(g.sVA, uq), dim3(256), 0, ys, dm, (const double*)dVb, (const double*)dxn1, g.sVA,
                     (double*)c->bl_VA.p);
  hipLaunchKernelGGL(k_bl_sbf, blocks(g.sSBf, uq), dim3(256), 0, ys, dm, (const double*)dS0, (const double*)dxn0, g.sSBf,
                     (double*)c->bl_SBf.p);
  // where the gradient phases of k_bpost have to run (k_bl_gradbound / k_bl_gradcoarse): [q][2][tiles] largest samples | [q][2]
  // slacks | [q][2] keys of the grid's largest samples | scratch of the coefficient kernel
  {
    static_assert(kGradNpx * kGradNpl == 128, "k_bl_gradcoarse: one sample per thread");
    const int ntx = (ncs0 + 7) / 8, nty = (nrb + 3) / 4;
    const size_t nt = (size_t)ntx * nty, head = (size_t)q * 2 * nt + 4 * (size_t)q;
    const int rows = std::max(rc0m, 1) + 1;                  // coefficient rows 0 .. largest degree + 1
    if ((rc = ensure(c->bl_grad, sizeof(double) * (head + (size_t)q * (3 * kBlMaxR * kBlMaxRc + 4 * (size_t)rows))))) return rc;
    double* gt = (double*)c->bl_grad.p;
    double* slack = gt + (size_t)q * 2 * nt;
    unsigned long long* gkey = (unsigned long long*)(slack + 2 * q);
    // half a sampling cell in the Chebyshev variable of each axis: kGradStep / 2 grid steps
    const double half0 = 0.5 * (dm.b[0] - dm.a[0]), half1 = 0.5 * (dm.b[1] - dm.a[1]);
    const double dxi0 = cs.count[0] > 1 ? 0.5 * kGradStep * std::fabs(cs.step[0] / mc.X_std[0]) / half0 : 0.0;
    const double dxi1 = cs.count[1] > 1 ? 0.5 * kGradStep * std::fabs(cs.step[1] / mc.X_std[1]) / half1 : 0.0;
    SBO_HIP(hipMemsetAsync(gkey, 0, sizeof(unsigned long long) * 2 * q, ys));
    double* Wscr = (double*)(gkey + 2 * q);
    double* part = Wscr + (size_t)q * 3 * kBlMaxR * kBlMaxRc;
    hipLaunchKernelGGL(k_bl_gradw, dim3((unsigned)(3 * r0u), uq), dim3(128), 0, ys, dm, dVs, dsig, (const double*)dMb, Wscr);
    hipLaunchKernelGGL(k_bl_gradrow, dim3((unsigned)rows, uq), dim3(256), 0, ys, dm, dVs, dsig, (const double*)Wscr, part);
    hipLaunchKernelGGL(k_bl_gradslack, dim3(uq), dim3(64), 0, ys, (const double*)part, rows, dxi0, dxi1, slack);
    hipLaunchKernelGGL(k_bl_gradcoarse, dim3((unsigned)nt, uq), dim3(128), 0, ys, dm, (const double*)dS0, (const double*)dVb, (const double*)dxn0,
                       (const double*)dxn1, ntx, gt, gkey);
    hipLaunchKernelGGL(k_bl_gradmax, dim3(2 * uq), dim3(256), 0, ys, (const double*)gt, (int)nt, gkey);
    if (std::isfinite(dxi0) && std::isfinite(dxi1)) {
      g.gtmax = gt;
      g.gkey = gkey;
    }
  }
  // guard band of this plan (guard.hip): the exact evaluator at the probe points runs here, beside the core's GEMM chain
  const bool band = c->opt.guard_band && !c->is_shadow;
  double *gref_m = nullptr, *gref_v = nullptr;
  if (band && (rc = guard_probe_reference(c, zs, &gref_m, &gref_v))) return rc;
  // (and the exact gradient components there: the scale the analytic band of the Lipschitz keys is taken relative to)
  double* gref_g = band ? gref_m + (4 * (size_t)q + 2) * kGbProbes : nullptr;
  if (band && (rc = guard_probe_gradients(c, zs, gref_m + 4 * (size_t)q * kGbProbes, gref_g, nullptr))) return rc;
  if (band && zs != ys) SBO_HIP(hipEventRecord(c->ev_join[6], zs));
  if (ys != xs) SBO_HIP(hipEventRecord(c->ev_join[3], ys));
  if (!direct && (rc = x_head())) return rc;
  {
    double* PC0 = (double*)c->bl_cheb.p;
    double* PC1 = PC0 + (size_t)q * nPC0;
    double* T4p = PC1 + (size_t)q * nPC1;
    double* Yt = T4p + (size_t)q * nT4p;
    double* Chat = Yt + (size_t)q * nYt;
    int* eff = (int*)(Chat + (size_t)q * nCh);
    // Chat^T = (PC1^T T4^T) PC0 on the matrix cores: PC1^T as A images and PC0 as B fragments straight out of k_cheb_pairs, T4^T
    // as B fragments -- which is what k_bl_t4f writes for the pair form --; Y' = PC1^T T4^T comes out as A images (k_bgemm OMODE 0)
    hipLaunchKernelGGL(k_cheb_pairs, dim3((unsigned)(std::max(KBp0, KBp1) * 16), 2 * uq), dim3(128), 0, xs, dm, dVs, dsig, nPC0, nPC1, PC0, PC1);
    {
      BlDims dp = dm;                    // (the pair form's block counts for the gather)
      dp.KB0 = KBp0;
      dp.KB1 = KBp1;
      hipLaunchKernelGGL(k_bl_t4f, blocks(nT4p, uq), dim3(256), 0, xs, dp, (const double*)G, (long long)ldg, nT4p, T4p, direct ? 1 : 0);
    }
    const int nrbD1 = (int)(D1m / 16), ncsD0 = (int)(D0m / 16);
    hipLaunchKernelGGL((k_bgemm<4, 0, 0>), dim3((unsigned)((KBp0 + 3) / 4), (unsigned)((nrbD1 + 3) / 4), uq), dim3(256), 0, xs, (const double*)PC1,
                       nPC1, (const double*)T4p, nT4p, KBp1, nrbD1, KBp0, Yt, nYt, (double*)nullptr, 0ll);
    hipLaunchKernelGGL((k_bgemm<4, 0, 2>), dim3((unsigned)((ncsD0 + 3) / 4), (unsigned)((nrbD1 + 3) / 4), uq), dim3(256), 0, xs, (const double*)Yt,
                       nYt, (const double*)PC0, nPC0, KBp0, nrbD1, ncsD0, Chat, nCh, (double*)nullptr, (long long)D0m);
    hipLaunchKernelGGL(k_cheb_trunc, dim3(uq), dim3(1024), 0, xs, dm, (const double*)Chat, c->opt.cheb_tol, eff);
    hipLaunchKernelGGL(k_cheb_t4f, blocks(g.sT4f, uq), dim3(256), 0, xs, dm, (const double*)Chat, g.sT4f, (double*)c->bl_T4f.p);
    // (the counts also travel to the host, unwaited: the profile's flop count reads them after the next sweep's own sync)
    SBO_HIP(hipMemcpyAsync(c->h_back->tile_eff, eff, sizeof(int) * 4 * q, hipMemcpyDeviceToHost, xs));
    g.eff = eff;
  }
  if (ys != xs) SBO_HIP(hipStreamWaitEvent(xs, c->ev_join[3], 0));
  if (band && zs != ys) SBO_HIP(hipStreamWaitEvent(xs, c->ev_join[6], 0));
  if (band) {
    // ... K1b's own values at the probes from the tables just made, and the band from the deviations: in place before the
    // plan's first posterior launch, whose fused classification reads it
    double* pm = gref_m + 2 * (size_t)q * kGbProbes;
    double* pv = pm + (size_t)q * kGbProbes;
    const double* Chat = (const double*)c->bl_cheb.p + (size_t)q * (nPC0 + nPC1 + nT4p + nYt);
    hipLaunchKernelGGL(k_gb_probe_k1b, dim3((unsigned)((kGbProbes + 3) / 4), uq), dim3(256), 0, xs, mc, cs, dm, Chat, (const int*)g.eff,
                       (const double*)dxn0, (const double*)dxn1, (const double*)dS0, (const double*)dVb, pm, pv);
    GbAnalytic an;
    memset(&an, 0, sizeof(an));
    an.axis_eps = bb + basis_layout(n, q).eps;
    an.alpha = c->factor.alpha();
    an.a_ld = c->factor.a_ld();
    an.n = n;
    for (int o = 0; o < q; ++o) { an.rc[o][0] = dm.rc0[o]; an.rc[o][1] = dm.rc1[o]; }
    an.Xn = (const double*)c->Xn.p;
    an.dpad = mc.dpad;
    for (int t = 0; t < 4; ++t) an.ab[t] = c->bl_basis_ab[t];
    an.ref_g = gref_g;
    if ((rc = guard_band_from_probes(c, pm, pv, gref_m, gref_v, reinterpret_cast<const double*>(g.eff + 4 * q), an))) return rc;
    g.band_ready = true;
  }
  SBO_HIP(hipGetLastError());
  lap("enqueue");
  if (timing && g.gtmax) {
    // (diagnostic: how many tiles keep their gradient phases)
    const int ntx = (ncs0 + 7) / 8, nty = (nrb + 3) / 4;
    const size_t nt = (size_t)ntx * nty;
    std::vector<double> h((size_t)q * 2 * nt + 4 * (size_t)q);
    SBO_HIP(hipStreamSynchronize(xs));
    SBO_HIP(hipMemcpy(h.data(), g.gtmax, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    const double* sl = h.data() + (size_t)q * 2 * nt;
    for (int o = 0; o < q; ++o)
      for (int k = 0; k < 2; ++k) {
        double G;
        memcpy(&G, sl + 2 * q + 2 * o + k, 8);
        size_t run = 0;
        for (size_t i = 0; i < nt; ++i) run += !(h[((size_t)o * 2 + k) * nt + i] + sl[2 * o + k] < G * (1.0 - 1e-12));
        fprintf(stderr, "[K1b setup] gradient phase %d of output %d: %zu of %zu tiles (largest sample %.6e, slack %.3e)\n", k, o, run, nt, G, sl[2 * o + k]);
      }
  }
  pl.usable = true;       // (nothing to wait for: the tables are made in stream order ahead of the posterior kernels)
  pl.setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return SBO_OK;
}


#include "bilinear_interp.inc.hpp"

}  // namespace sbo
