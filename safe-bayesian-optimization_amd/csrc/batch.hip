// batch.hip -- sbo_batch_select: a greedy batch of k pool points under hallucinated observations (GP-BUCB).
//
// A GP's posterior variance does not depend on the observed values, so the j-th point of a batch can maximise the variance of one
// output conditioned on the data AND on the j - 1 points already chosen before any of them is measured.  The picks act as
// observations n, n + 1, ..: a scratch copy of the selected output's lower factor M (M^T M = inv(K + sn2 I)) grows by one row per
// conditioned point -- k_model_append's bordered update, on scratch the context owns; the resident factor is only read.  With
//   v_0(x) = sf2 - ||M k_x||^2                                                  (k_batch_v0, the O(m n^2) part)
// conditioning on a point z is, for every pool point x,
//   u = M_aug^T (M_aug k_z),  s = (sf2 + sn2) - k_z . u                          (k_batch_u, one workgroup)
//   c(x) = k(x, z) - sum_i k(x, X_aug_i) u_i,   v(x) <- v(x) - c(x)^2 / s        (k_batch_pass, one lane per pool point)
// and the pass leaves per-workgroup (max v, lowest index) partials that k_batch_finish reduces to the next pick.  Every sum over the
// observations and the earlier picks runs in index order inside one lane, (value, index) reductions are selects on scalars under a
// total order, there are no atomics: the value of a pool point depends on its coordinates only, not on m or on its place in the list.
// The whole batch is enqueued without a host wait (a stop or a refused step turns the kernels behind it into no-ops through the
// state block); one read-back follows.  Nothing resident is written.
#include <algorithm>
#include <cmath>
#include <cstring>
#include "internal.hpp"
#include "device_common.hpp"

namespace sbo {

constexpr int kBatThreads = 256;                 // k_batch_pass / k_batch_finish
constexpr int kBatChunk = 512;                   // augmented observations of one LDS chunk of k_batch_pass (40 KiB at dpad = 8)
constexpr int kBatV0Threads = 1024;              // k_batch_v0: P points x 1024 / P row lanes
constexpr int kBatV0Rows = 4;                    // ... rows of M per row lane and step
constexpr size_t kBatV0Lds = 128 * 1024;         // ... its K(X, tile) image [n][P]: P = 32 up to n = 512, 16 up to 1024, 8 up to SBO_MAX_N
constexpr int kBatMaxAug = SBO_MAX_N + SBO_MAX_BATCH;

struct BatchArgs {                               // by value (kernarg segment)
  int n, d, ld;                                  // observations of the model, input dimension, leading dimension n + n_pending + k of the scratch factor
  int pad;
  double X_mean[kMaxD], X_std[kMaxD], vinv[kMaxD];
  double sf2, kappa, Y_std, min_std;             // kappa = sf2 + sn2, the diagonal entry sbo_model_append gives a new row
};

struct BatchState {                              // device: what the kernels of one call hand each other, and the result
  int stop, bad;                                 // min_std ended the batch / a conditioning step had s <= 0 (or no finite variance was left)
  double s;                                      // of the running conditioning step
  sbo_batch_result res;
};

// scaled coordinates b = (x - X_mean) / X_std * ell^-1/2 of a raw point and their sum of squares, axis order (GP_Safe.py:115-116)
template <int D>
__device__ __forceinline__ double bat_scale(const BatchArgs& A, const double* __restrict__ raw, bool on, double* b) {
  double bsq = 0.0;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    b[a] = (on && a < A.d) ? ((raw[a] - A.X_mean[a]) / A.X_std[a]) * A.vinv[a] : 0.0;
    bsq += b[a] * b[a];
  }
  return bsq;
}
// sf2 exp(-1/2 dist) with the expanded distance (-2 a.b + |a|^2) + |b|^2 of the reference (GP_Safe.py:119), as sbo_model_append forms it
template <int D>
__device__ __forceinline__ double bat_k(double sf2, const double* a, double asq, const double* b, double bsq) {
  double dot = 0.0;
#pragma unroll
  for (int t = 0; t < D; ++t) dot += a[t] * b[t];
  return sf2 * exp(-0.5 * ((-2.0 * dot + asq) + bsq));
}

// ---- the observations in scaled coordinates: As [ld][D] (rows >= n: filled as points are conditioned on), sq [ld] -----------------
template <int D>
__global__ __launch_bounds__(256) void k_batch_prep(const BatchArgs A, const double* __restrict__ Xn /* [n][d] */, double* __restrict__ As,
                                                    double* __restrict__ sq) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  double s = 0.0;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const double v = a < A.d ? Xn[(size_t)i * A.d + a] * A.vinv[a] : 0.0;
    As[(size_t)i * D + a] = v;
    s += v * v;
  }
  sq[i] = s;
}

// ---- v_0 = sf2 - ||M k_x||^2 -------------------------------------------------------------------------------------------------------
// A workgroup owns P pool points; thread (p, r) = (tid mod P, tid / P).  K(X, tile) is formed once into LDS as sK[j][p]; the rows of
// t = M k_x are taken in blocks of (1024 / P) kBatV0Rows rows from the bottom up, a thread owning kBatV0Rows consecutive rows of its
// point -- row i needs k[0 .. i] only, so a finished block's t overwrites the k entries nobody reads any more --, every row sum in
// column order; at the end one thread per point adds the squares in row order.  Nothing above the diagonal of M is read.
template <int D>
__global__ __launch_bounds__(kBatV0Threads) void k_batch_v0(const BatchArgs A, int P, const double* __restrict__ As, const double* __restrict__ sq,
                                                            const double* __restrict__ M, const double* __restrict__ pool, long long m,
                                                            double* __restrict__ v) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* sK = reinterpret_cast<double*>(smem);             // [n][P]
  const int n = A.n, ld = A.ld, tid = threadIdx.x, p = tid % P, r = tid / P, R = kBatV0Threads / P;
  const long long i = (long long)blockIdx.x * P + p;
  const bool on = i < m;
  double b[D];
  const double bsq = bat_scale<D>(A, pool + (size_t)(on ? i : 0) * A.d, on, b);
  for (int j = r; j < n; j += R) {
    double a[D];
#pragma unroll
    for (int t = 0; t < D; ++t) a[t] = As[(size_t)j * D + t];
    sK[j * P + p] = on ? bat_k<D>(A.sf2, a, sq[j], b, bsq) : 0.0;
  }
  __syncthreads();
  const int RB = R * kBatV0Rows;
  for (int blk = (n + RB - 1) / RB - 1; blk >= 0; --blk) {
    const int i0 = blk * RB + r * kBatV0Rows, cnt = min(kBatV0Rows, n - i0);      // this thread's rows i0 .. i0 + cnt - 1 (cnt <= 0: none)
    double t[kBatV0Rows];
#pragma unroll
    for (int u = 0; u < kBatV0Rows; ++u) t[u] = 0.0;
    if (cnt > 0) {
      const double* row[kBatV0Rows];
#pragma unroll
      for (int u = 0; u < kBatV0Rows; ++u) row[u] = M + (size_t)min(i0 + u, n - 1) * ld;    // (a missing row reads the last one; its sum is dropped)
#pragma unroll 4
      for (int j = 0; j <= i0; ++j) {
        const double kj = sK[j * P + p];
#pragma unroll
        for (int u = 0; u < kBatV0Rows; ++u) t[u] = fma(row[u][j], kj, t[u]);
      }
#pragma unroll
      for (int u = 1; u < kBatV0Rows; ++u)
        if (u < cnt)
          for (int j = i0 + 1; j <= i0 + u; ++j) t[u] = fma(row[u][j], sK[j * P + p], t[u]);
    }
    __syncthreads();                                    // (every k entry of this block of rows has been read)
#pragma unroll
    for (int u = 0; u < kBatV0Rows; ++u)
      if (u < cnt) sK[(i0 + u) * P + p] = t[u];
  }
  __syncthreads();
  if (tid < P && on) {                                  // (p == tid)
    double s = 0.0;
    for (int j = 0; j < n; ++j) {
      const double t = sK[j * P + tid];
      s += t * t;
    }
    v[i] = A.sf2 - s;
  }
}

// ---- one conditioning step, the part that does not depend on the pool --------------------------------------------------------------
// z = src[src_index] (a pending point) or, with src_index < 0, the pool point picked last.  One workgroup: k_z over the na augmented
// observations, t = M_aug k_z (a wave per row, lanes along the row, butterfly), u = M_aug^T t (a thread per column, rows in order),
// s = kappa - k_z . u.  s <= 0 sets `bad` and writes nothing; otherwise row na of the scratch factor becomes (-u / sqrt(s), 1 / sqrt(s))
// and z joins the observation arrays as row na -- the resident factor is never written.
template <int D>
__global__ __launch_bounds__(1024) void k_batch_u(const BatchArgs A, int na, double* __restrict__ As, double* __restrict__ sq, double* __restrict__ M,
                                                  const double* __restrict__ src, long long src_index, const double* __restrict__ pool,
                                                  double* __restrict__ u, BatchState* __restrict__ st) {
  __shared__ double kz[kBatMaxAug], tz[kBatMaxAug];
  __shared__ double red[16];
  __shared__ double s_sh;
  if (st->stop || st->bad) return;                      // (the same for the whole workgroup)
  const int ld = A.ld, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* raw = src_index >= 0 ? src + (size_t)src_index * A.d : pool + (size_t)st->res.index[st->res.n_selected - 1] * A.d;
  double b[D];
  const double bsq = bat_scale<D>(A, raw, true, b);
  for (int j = tid; j < na; j += 1024) {
    double a[D];
#pragma unroll
    for (int t = 0; t < D; ++t) a[t] = As[(size_t)j * D + t];
    kz[j] = bat_k<D>(A.sf2, a, sq[j], b, bsq);
  }
  __syncthreads();
  for (int i = wave; i < na; i += 16) {
    double s = 0.0;
    for (int j = lane; j <= i; j += 64) s = fma(M[(size_t)i * ld + j], kz[j], s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) tz[i] = s;
  }
  __syncthreads();
  double ku = 0.0;
  for (int j = tid; j < na; j += 1024) {
    double s = 0.0;
    for (int i = j; i < na; ++i) s = fma(M[(size_t)i * ld + j], tz[i], s);
    u[j] = s;
    ku += kz[j] * s;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ku += __shfl_xor(ku, off);
  if (lane == 0) red[wave] = ku;
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int w = 0; w < 16; ++w) sum += red[w];
    const double s = A.kappa - sum;
    s_sh = s;
    st->s = s;
    if (!(s > 0.0)) st->bad = 1;
  }
  __syncthreads();
  const double s = s_sh;
  if (!(s > 0.0)) return;
  const double rs = 1.0 / sqrt(s);
  for (int j = tid; j < na; j += 1024) M[(size_t)na * ld + j] = -u[j] * rs;
  if (tid == 0) {
    M[(size_t)na * ld + na] = rs;
    sq[na] = bsq;
#pragma unroll
    for (int t = 0; t < D; ++t) As[(size_t)na * D + t] = b[t];
  }
}

// ---- one conditioning step over the pool (na >= 0), and the (max v, lowest index) partials of the next pick ---------------------------
// A lane owns a pool point: c = k(x, z) - sum_{i < na} k(x, X_aug_i) u_i with the augmented observations i = 0 .. na - 1 in order (the
// rows and u come from LDS in chunks, a broadcast per word), z being row na; v <- v - c^2 / s.  na < 0: no update, the partials of
// the stored v only (the first pick of a call without pending points).
template <int D>
__global__ __launch_bounds__(kBatThreads) void k_batch_pass(const BatchArgs A, int na, const double* __restrict__ As, const double* __restrict__ sq,
                                                            const double* __restrict__ u, const BatchState* __restrict__ st,
                                                            const double* __restrict__ pool, long long m, double* __restrict__ v,
                                                            double* __restrict__ partv, long long* __restrict__ parti) {
  __shared__ double sA[kBatChunk * D], sS[kBatChunk], sU[kBatChunk];
  __shared__ double sv[kBatThreads / 64];
  __shared__ long long sk[kBatThreads / 64];
  if (st->stop || st->bad) return;                      // (the same for the whole grid)
  const int tid = threadIdx.x;
  const bool update = na >= 0;
  const double s = st->s;
  double z[D], zsq = 0.0;
#pragma unroll
  for (int t = 0; t < D; ++t) z[t] = update ? As[(size_t)na * D + t] : 0.0;
  if (update) zsq = sq[na];
  double bv = 0.0;
  long long bi = kArgNone;                              // (value, index): arg_take's order, ties to the lowest index
  for (long long base = (long long)blockIdx.x * kBatThreads; base < m; base += (long long)gridDim.x * kBatThreads) {
    const long long i = base + tid;
    const bool on = i < m;
    double vn = on ? v[i] : 0.0;
    if (update) {
      double b[D];
      const double bsq = bat_scale<D>(A, pool + (size_t)(on ? i : 0) * A.d, on, b);
      double acc = 0.0;
      for (int j0 = 0; j0 < na; j0 += kBatChunk) {
        const int cnt = min(kBatChunk, na - j0);
        __syncthreads();                                // (the chunk before this one has been read)
        for (int t = tid; t < cnt * D; t += kBatThreads) sA[t] = As[(size_t)j0 * D + t];
        for (int t = tid; t < cnt; t += kBatThreads) {
          sS[t] = sq[j0 + t];
          sU[t] = u[j0 + t];
        }
        __syncthreads();
        if (on)
          for (int j = 0; j < cnt; ++j) acc += bat_k<D>(A.sf2, sA + j * D, sS[j], b, bsq) * sU[j];
      }
      if (on) {
        const double c = bat_k<D>(A.sf2, z, zsq, b, bsq) - acc;
        vn = vn - c * c / s;
        v[i] = vn;
      }
    }
    arg_take(bv, bi, vn, (on && vn == vn) ? i : kArgNone);   // (a NaN is never taken)
  }
  arg_block_best(bv, bi, sv, sk);
  if (tid == 0) {
    partv[blockIdx.x] = bv;
    parti[blockIdx.x] = bi;
  }
}

// ---- pick j: the partials in workgroup order, the min_std stop, the result entry ------------------------------------------------------
__global__ __launch_bounds__(kBatThreads) void k_batch_finish(const BatchArgs A, int j, int nb, const double* __restrict__ partv,
                                                              const long long* __restrict__ parti, BatchState* __restrict__ st) {
  __shared__ double sv[kBatThreads / 64];
  __shared__ long long sk[kBatThreads / 64];
  if (st->stop || st->bad) return;
  double bv = 0.0;
  long long bi = kArgNone;                              // (value, index): arg_take's order, ties to the lowest index
  for (int k = threadIdx.x; k < nb; k += kBatThreads) arg_take(bv, bi, partv[k], parti[k]);
  arg_block_best(bv, bi, sv, sk);
  if (threadIdx.x == 0) {
    if (bi == kArgNone) {
      st->bad = 1;
      return;
    }
    const double sd = sqrt(fmax(0.0, bv)) * A.Y_std;
    if (sd < A.min_std) {
      st->stop = 1;
      return;
    }
    st->res.index[j] = bi;
    st->res.std[j] = sd;
    st->res.n_selected = j + 1;
  }
}

// ---- var_out = max(0, v) Y_std^2, in place -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_batch_var(double ys2, long long m, double* __restrict__ v) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x)
    v[i] = fmax(0.0, v[i]) * ys2;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct BatBufs {
  double *Xn, *As, *sq, *M, *pool, *pend, *v, *u, *partv;
  long long* parti;
  BatchState* st;
};

template <int D>
static int batch_enqueue(sbo_ctx* c, const BatchArgs& A, const BatBufs& B, long long m, int k, int n_pending, bool want_var) {
  hipStream_t st = c->stream;
  const int n = A.n;
  hipLaunchKernelGGL((k_batch_prep<D>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A, (const double*)B.Xn, B.As, B.sq);
  SBO_HIP(hipGetLastError());
  const int P = n <= 512 ? 32 : n <= 1024 ? 16 : 8;
  const size_t lds = sizeof(double) * (size_t)n * P;
  if (lds > kBatV0Lds) return fail(SBO_E_UNSUPPORTED, "sbo_batch_select: the model is too large");      // (n <= SBO_MAX_N: never)
  SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_batch_v0<D>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBatV0Lds));
  hipLaunchKernelGGL((k_batch_v0<D>), dim3((unsigned)((m + P - 1) / P)), dim3(kBatV0Threads), lds, st, A, P, (const double*)B.As,
                     (const double*)B.sq, (const double*)B.M, (const double*)B.pool, m, B.v);
  SBO_HIP(hipGetLastError());
  const int nb = (int)std::min<long long>((m + kBatThreads - 1) / kBatThreads, 8192);
  auto pass = [&](int na) {
    hipLaunchKernelGGL((k_batch_pass<D>), dim3((unsigned)nb), dim3(kBatThreads), 0, st, A, na, (const double*)B.As, (const double*)B.sq,
                       (const double*)B.u, (const BatchState*)B.st, (const double*)B.pool, m, B.v, B.partv, B.parti);
    return hipGetLastError();
  };
  auto condition = [&](int na, long long src_index) {
    hipLaunchKernelGGL((k_batch_u<D>), dim3(1), dim3(1024), 0, st, A, na, B.As, B.sq, B.M, (const double*)B.pend, src_index,
                       (const double*)B.pool, B.u, B.st);
    hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : pass(na);
  };
  int na = n;
  for (int p = 0; p < n_pending; ++p, ++na) SBO_HIP(condition(na, p));
  if (n_pending == 0) SBO_HIP(pass(-1));
  for (int j = 0; j < k; ++j) {
    hipLaunchKernelGGL(k_batch_finish, dim3(1), dim3(kBatThreads), 0, st, A, j, nb, (const double*)B.partv, (const long long*)B.parti, B.st);
    SBO_HIP(hipGetLastError());
    if (j + 1 < k || want_var) {                        // (nobody reads the variance behind the last pick otherwise)
      SBO_HIP(condition(na, -1));
      ++na;
    }
  }
  if (want_var) {
    hipLaunchKernelGGL(k_batch_var, dim3((unsigned)std::min<long long>((m + 255) / 256, 8192)), dim3(256), 0, st, A.Y_std * A.Y_std, m, B.v);
    SBO_HIP(hipGetLastError());
  }
  return SBO_OK;
}

static void batch_clear(sbo_batch_result* r) {
  std::memset(r, 0, sizeof(*r));
  for (int j = 0; j < SBO_MAX_BATCH; ++j) r->index[j] = -1;
}

}  // namespace sbo

using namespace sbo;

extern "C" int sbo_batch_select(sbo_ctx* c, const sbo_batch_opts* opts, int64_t m, const double* pool, const double* pending,
                                double* var_out, sbo_batch_result* result) {
  if (result) batch_clear(result);
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (!opts || !pool || !result) return fail(SBO_E_INVALID, "NULL argument");
  if (m < 1 || m > (1LL << 28)) return fail(SBO_E_INVALID, "m out of range");
  if (opts->k < 1 || opts->n_pending < 0 || opts->k > SBO_MAX_BATCH || opts->n_pending > SBO_MAX_BATCH ||
      opts->k + opts->n_pending > SBO_MAX_BATCH)
    return fail(SBO_E_INVALID, "k >= 1, n_pending >= 0 and k + n_pending <= SBO_MAX_BATCH are required");
  if (opts->n_pending > 0 && !pending) return fail(SBO_E_INVALID, "pending is NULL");
  if (!std::isfinite(opts->min_std) || opts->min_std < 0.0) return fail(SBO_E_INVALID, "min_std must be finite and >= 0");
  int rc;
  if ((rc = model_reader_check(c, "sbo_batch_select", false))) return rc;        // (d and q, which the checks below need)
  const ModelConst& mc = c->mc;
  const int n = mc.n, d = mc.d, o = opts->output, k = opts->k, np = opts->n_pending;
  if (o < 0 || o >= mc.q) return fail(SBO_E_INVALID, "output out of range [0, q)");
  for (size_t t = 0; t < (size_t)m * d; ++t)
    if (!std::isfinite(pool[t])) return fail(SBO_E_INVALID, "pool holds a non-finite coordinate");
  for (size_t t = 0; t < (size_t)np * d; ++t)
    if (!std::isfinite(pending[t])) return fail(SBO_E_INVALID, "pending holds a non-finite coordinate");
  if ((rc = model_reader_begin(c, "sbo_batch_select", false))) return rc;        // (the scratch factor starts as a copy of the resident one)
  BatchArgs A{};
  A.n = n;
  A.d = d;
  A.ld = n + np + k;
  for (int a = 0; a < d; ++a) {
    A.X_mean[a] = mc.X_mean[a];
    A.X_std[a] = mc.X_std[a];
    A.vinv[a] = mc.vinv[o][a];
  }
  A.sf2 = mc.sf2[o];
  A.kappa = mc.sf2[o] + mc.sn2[o];
  A.Y_std = mc.Y_std[o];
  A.min_std = opts->min_std;
  // scratch: X_norm [n][d] | scaled observations [ld][dpad] and their squares [ld] | the factor [ld][ld] | pool [m][d] | pending |
  // v [m] | u [ld] | the partials | the state block
  const int D = mc.dpad;
  const size_t ld = (size_t)A.ld, nbmax = 8192;
  BatBufs B;
  auto layout = [&](Carve cv) {
    cv.take(B.Xn, (size_t)n * d);
    cv.take(B.As, ld * D);
    cv.take(B.sq, ld);
    cv.take(B.M, ld * ld);
    cv.take(B.pool, (size_t)m * d);
    cv.take(B.pend, (size_t)std::max(np, 1) * d);
    cv.take(B.v, (size_t)m);
    cv.take(B.u, ld);
    cv.take(B.partv, nbmax);
    cv.take(B.parti, nbmax);
    cv.take(B.st, 1);
    return cv.off;
  };
  if ((rc = carve(c->batchbuf, layout, 256))) return rc;
  hipStream_t st = c->stream;
  BatchState init{};
  batch_clear(&init.res);
  SBO_HIP(hipMemcpyAsync(B.st, &init, sizeof(init), hipMemcpyHostToDevice, st));
  SBO_HIP(hipMemcpyAsync(B.Xn, c->h_Xnorm.data(), sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice, st));
  SBO_HIP(hipMemcpyAsync(B.pool, pool, sizeof(double) * (size_t)m * d, hipMemcpyHostToDevice, st));
  if (np) SBO_HIP(hipMemcpyAsync(B.pend, pending, sizeof(double) * (size_t)np * d, hipMemcpyHostToDevice, st));
  SBO_HIP(hipMemcpy2DAsync(B.M, sizeof(double) * ld, c->factor.F() + (size_t)o * c->factor.ld() * c->factor.ld(), sizeof(double) * c->factor.ld(),
                           sizeof(double) * n, n, hipMemcpyDeviceToDevice, st));
  rc = with_dpad(D, [&](auto DD) { return batch_enqueue<DD()>(c, A, B, m, k, np, var_out != nullptr); });
  if (rc) {
    (void)hipStreamSynchronize(st);                     // (nothing of the call may still read the caller's arrays)
    return rc;
  }
  BatchState out;
  SBO_HIP(hipMemcpyAsync(&out, B.st, sizeof(out), hipMemcpyDeviceToHost, st));
  if (var_out) SBO_HIP(hipMemcpyAsync(var_out, B.v, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, st));
  SBO_HIP(stream_wait(c, st));
  if (out.bad) return fail(SBO_E_INVALID, "a conditioning step has s <= 0 (a repeated point without noise?)");
  *result = out.res;
  return SBO_OK;
}
