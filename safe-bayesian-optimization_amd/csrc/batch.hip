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
// The kernel expression, the observations' scaled coordinates, the whitening tile of k_batch_v0 and the two mat-vecs of k_batch_u are
// whiten.hpp's, shared with expander.hip and paths.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include "whiten.hpp"

namespace sbo {

constexpr int kBatThreads = 256;                 // k_batch_pass / k_batch_finish
constexpr int kBatChunk = 512;                   // augmented observations of one LDS chunk of k_batch_pass (40 KiB at dpad = 8)
constexpr size_t kBatV0Lds = 128 * 1024;         // k_batch_v0: whiten_tile's image [n][P], P = whiten_tier(n): full at n = 512, 1024 and SBO_MAX_N
constexpr int kBatMaxAug = SBO_MAX_N + SBO_MAX_BATCH;

struct BatchArgs {                               // by value (kernarg segment)
  int n, ld;                                     // observations of the model, leading dimension n + n_pending + k of the scratch factor
  OutParams op;                                  // the selected output
  double kappa, Y_std, min_std;                  // kappa = sf2 + sn2, the diagonal entry sbo_model_append gives a new row
};

struct BatchState {                              // device: what the kernels of one call hand each other, and the result
  int stop, bad;                                 // min_std ended the batch / a conditioning step had s <= 0 (or no finite variance was left)
  double s;                                      // of the running conditioning step
  sbo_batch_result res;
};

// ---- v_0 = sf2 - ||M k_x||^2 -------------------------------------------------------------------------------------------------------
// A workgroup owns P pool points (whiten_tile, whiten.hpp); at the end one thread per point adds the squares in row order.
template <int D>
__global__ __launch_bounds__(kWhitenThreads) void k_batch_v0(const BatchArgs A, int P, const double* __restrict__ As, const double* __restrict__ sq,
                                                             const double* __restrict__ M, const double* __restrict__ pool, long long m,
                                                             double* __restrict__ v) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* sK = reinterpret_cast<double*>(smem);             // [n][P]
  const int n = A.n, tid = threadIdx.x;
  const long long i = (long long)blockIdx.x * P + tid % P;
  const bool on = i < m;
  double b[D];
  const double bsq = rbf_scale<D>(A.op, pool + (size_t)(on ? i : 0) * A.op.d, on, b);
  whiten_tile<D>(sK, P, P, n, A.op.sf2, As, sq, M, A.ld, b, bsq, on);
  if (tid < P && on) {                                  // (tid % P == tid)
    double s = 0.0;
    for (int j = 0; j < n; ++j) {
      const double t = sK[j * P + tid];
      s += t * t;
    }
    v[i] = A.op.sf2 - s;
  }
}

// ---- one conditioning step, the part that does not depend on the pool --------------------------------------------------------------
// z = src[src_index] (a pending point) or, with src_index < 0, the pool point picked last.  One workgroup: k_z over the na augmented
// observations, t = M_aug k_z (factor_lower_mv), u = M_aug^T t (factor_upper_mv), s = kappa - k_z . u.  s <= 0 sets `bad` and writes
// nothing; otherwise row na of the scratch factor becomes (-u / sqrt(s), 1 / sqrt(s)) and z joins the observation arrays as row na --
// the resident factor is never written.
template <int D>
__global__ __launch_bounds__(kFactorMvThreads) void k_batch_u(const BatchArgs A, int na, double* __restrict__ As, double* __restrict__ sq,
                                                              double* __restrict__ M, const double* __restrict__ src, long long src_index,
                                                              const double* __restrict__ pool, double* __restrict__ u,
                                                              BatchState* __restrict__ st) {
  __shared__ double kz[kBatMaxAug], tz[kBatMaxAug];
  __shared__ double red[16];
  __shared__ double s_sh;
  if (st->stop || st->bad) return;                      // (the same for the whole workgroup)
  const int ld = A.ld, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* raw = src_index >= 0 ? src + (size_t)src_index * A.op.d : pool + (size_t)st->res.index[st->res.n_selected - 1] * A.op.d;
  double b[D];
  const double bsq = rbf_scale<D>(A.op, raw, true, b);
  for (int j = tid; j < na; j += kFactorMvThreads) {
    double a[D];
#pragma unroll
    for (int t = 0; t < D; ++t) a[t] = As[(size_t)j * D + t];
    kz[j] = rbf_k<D>(A.op.sf2, a, sq[j], b, bsq);
  }
  __syncthreads();
  factor_lower_mv(M, ld, na, kz, tz, na);
  __syncthreads();
  double ku = 0.0;
  factor_upper_mv(M, ld, na, tz, [&](int j, double s) {
    u[j] = s;
    ku += kz[j] * s;
  });
  ku = wave_sum(ku);
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
  for (int j = tid; j < na; j += kFactorMvThreads) M[(size_t)na * ld + j] = -u[j] * rs;
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
      const double bsq = rbf_scale<D>(A.op, pool + (size_t)(on ? i : 0) * A.op.d, on, b);
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
          for (int j = 0; j < cnt; ++j) acc += rbf_k<D>(A.op.sf2, sA + j * D, sS[j], b, bsq) * sU[j];
      }
      if (on) {
        const double c = rbf_k<D>(A.op.sf2, z, zsq, b, bsq) - acc;
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
  SBO_HIP(obs_prep<D>(st, n, &A.op, 1, B.Xn, B.As, B.sq));      // (rows 0 .. n - 1 of As [ld][D], sq [ld]; k_batch_u fills the rest)
  const int P = whiten_tier(n);
  const size_t lds = sizeof(double) * (size_t)n * P;
  if (lds > kBatV0Lds) return fail(SBO_E_UNSUPPORTED, "sbo_batch_select: the model is too large");      // (n <= SBO_MAX_N: never)
  SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_batch_v0<D>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBatV0Lds));
  hipLaunchKernelGGL((k_batch_v0<D>), dim3((unsigned)((m + P - 1) / P)), dim3(kWhitenThreads), lds, st, A, P, (const double*)B.As,
                     (const double*)B.sq, (const double*)B.M, (const double*)B.pool, m, B.v);
  SBO_HIP(hipGetLastError());
  const int nb = (int)std::min<long long>((m + kBatThreads - 1) / kBatThreads, 8192);
  auto pass = [&](int na) {
    hipLaunchKernelGGL((k_batch_pass<D>), dim3((unsigned)nb), dim3(kBatThreads), 0, st, A, na, (const double*)B.As, (const double*)B.sq,
                       (const double*)B.u, (const BatchState*)B.st, (const double*)B.pool, m, B.v, B.partv, B.parti);
    return hipGetLastError();
  };
  auto condition = [&](int na, long long src_index) {
    hipLaunchKernelGGL((k_batch_u<D>), dim3(1), dim3(kFactorMvThreads), 0, st, A, na, B.As, B.sq, B.M, (const double*)B.pend, src_index,
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
  if (!all_finite(pool, (size_t)m * d)) return fail(SBO_E_INVALID, "pool holds a non-finite coordinate");
  if (!all_finite(pending, (size_t)np * d)) return fail(SBO_E_INVALID, "pending holds a non-finite coordinate");
  if ((rc = model_reader_begin(c, "sbo_batch_select", false))) return rc;        // (the scratch factor starts as a copy of the resident one)
  BatchArgs A{};
  A.n = n;
  A.ld = n + np + k;
  A.op = out_params(mc, o);
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
