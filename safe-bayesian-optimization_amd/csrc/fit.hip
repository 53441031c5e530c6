// fit.hip -- SURVEY.md section 8(f) rank 1: the hyper-parameter objective of the model fit, batched on the device.
//
// negative_loglikelihood (models/GP_Safe.py:169-192) for P hyper-parameter vectors at once -- what a population-based
// optimiser (the reference uses SciPy differential evolution, models/GP_Safe.py:224) evaluates every generation:
//     W = exp(2 h[:d]), sf2 = exp(2 h[d]), sn2 = exp(2 h[d+1])
//     K = sf2 exp(-1/2 D_W(X, X)) + (sn2 + 1e-8) I ;  K = (K + K^T)/2 ;  K = L L^T
//     NLL = y^T K^-1 y + log|K| = ||L^-1 y||^2 + 2 sum log L_ii          (no 1/2, no constant: :190)
// One workgroup per population member.  The factor is built as K = U^T U with U upper triangular stored row-major so
// that every inner loop walks contiguous memory; the right-hand side y rides along as an extra column, so the forward
// solve costs no extra synchronisation.  Matrices live in an HBM workspace (L2-resident at the reference's sizes).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>
#include "device_common.hpp"
#include "pbfgs.hpp"

namespace sbo {

// NLL of one hyper-parameter vector h[d + 2], evaluated by the whole workgroup (result valid in thread 0).
// U: this member's n x n workspace; smem: [n d + 2 n] doubles.
__device__ double nll_member(int n, int d, const double* __restrict__ X, const double* __restrict__ y, const double* h,
                             double* __restrict__ U, double* smem_d) {
  double* Xa = smem_d;                               // [n][d]  X * W^-1/2
  double* sq = Xa + (size_t)n * d;                   // [n]
  double* z = sq + n;                                // [n]     running right-hand side / solution
  __shared__ double sh_piv;
  __shared__ int sh_bad;
  const int tid = threadIdx.x;
  const double sf2 = exp(2.0 * h[d]);
  const double jit = exp(2.0 * h[d + 1]) + 1e-8;                        // GP_Safe.py:184
  __syncthreads();                                                      // (the buffers may still be read by a previous call)
  for (int idx = tid; idx < n * d; idx += blockDim.x) {
    const int a = idx % d;
    Xa[idx] = X[idx] * pow(exp(2.0 * h[a]), -0.5);                      // GP_Safe.py:112-115
  }
  if (tid == 0) sh_bad = 0;
  __syncthreads();
  for (int i = tid; i < n; i += blockDim.x) {
    double s = 0.0;
    for (int a = 0; a < d; ++a) s += Xa[i * d + a] * Xa[i * d + a];
    sq[i] = s;
    z[i] = y[i];
  }
  __syncthreads();
  // upper triangle of the symmetrised covariance
  for (long long idx = tid; idx < (long long)n * n; idx += blockDim.x) {
    const int i = (int)(idx / n), k = (int)(idx % n);
    if (k < i) continue;
    double dot = 0.0;
    for (int a = 0; a < d; ++a) dot += Xa[i * d + a] * Xa[k * d + a];
    const double d1 = (-2.0 * dot + sq[i]) + sq[k];                    // dist[i, k] as GP_Safe.py:119 evaluates it
    const double d2 = (-2.0 * dot + sq[k]) + sq[i];                    // dist[k, i]
    double v = (sf2 * exp(-0.5 * d1) + sf2 * exp(-0.5 * d2)) * 0.5;    // (K + K^T) / 2, GP_Safe.py:185
    if (i == k) v = sf2 * exp(-0.5 * d1) + jit;
    U[(size_t)i * n + k] = v;
  }
  __syncthreads();
  double logdet = 0.0, zz = 0.0;
  const int lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  for (int j = 0; j < n; ++j) {
    if (tid == 0) {
      const double piv = U[(size_t)j * n + j];
      if (!(piv > 0.0)) sh_bad = 1;
      sh_piv = piv > 0.0 ? sqrt(piv) : 1.0;
    }
    __syncthreads();
    const double ljj = sh_piv;
    double* uj = U + (size_t)j * n;
    for (int i = j + 1 + tid; i < n; i += blockDim.x) uj[i] /= ljj;     // row j of U
    if (tid == 0) {
      uj[j] = ljj;
      z[j] = z[j] / ljj;
      logdet += log(ljj);
      zz += z[j] * z[j];
    }
    __syncthreads();
    const double zj = z[j];
    for (int i = j + 1 + tid; i < n; i += blockDim.x) z[i] -= uj[i] * zj;   // forward substitution rides along
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
    }
    __syncthreads();
  }
  return sh_bad ? INFINITY : zz + 2.0 * logdet;                         // GP_Safe.py:187-190 (thread 0's value)
}

__global__ __launch_bounds__(1024) void k_nll_batch(int n, int d, const double* __restrict__ X, const double* __restrict__ y,
                                                    const double* __restrict__ hyper, double* __restrict__ work,
                                                    double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int p = blockIdx.x;
  const double v = nll_member(n, d, X, y, hyper + (size_t)p * (d + 2), work + (size_t)p * n * n, reinterpret_cast<double*>(smem));
  if (threadIdx.x == 0) out[p] = v;
}

// The same for q outputs at once (sbo_fit_de_batch): grid (P, q), member p of output o on hyper[o][p], column o of yT and its own
// n x n slice of the workspace.
__global__ __launch_bounds__(1024) void k_nll_batch_q(int n, int d, int P, const double* __restrict__ X, const double* __restrict__ yT,
                                                      const double* __restrict__ hyper, double* __restrict__ work,
                                                      double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const size_t m = (size_t)blockIdx.y * P + blockIdx.x;
  const double v = nll_member(n, d, X, yT + (size_t)blockIdx.y * n, hyper + m * (d + 2), work + m * n * n, reinterpret_cast<double*>(smem));
  if (threadIdx.x == 0) out[m] = v;
}

// ---- differential evolution on the device --------------------------------------------------------------------------
// One generation of SciPy's default strategy as the reference calls it (models/GP_Safe.py:224: best1bin, dithered
// mutation, recombination 0.7) with deferred updating: workgroup i builds the trial vector of member i from the current
// population, evaluates its NLL and keeps the better of (parent, trial) in the next population.
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {     // splitmix64 finaliser
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ double u01(unsigned long long seed, unsigned gen, unsigned member, unsigned draw) {
  const unsigned long long k = mix64(seed ^ mix64(((unsigned long long)gen << 32) | member) ^ mix64(0xda3e39cb94b95bdbull + draw));
  return (double)(k >> 11) * (1.0 / 9007199254740992.0);
}

// Member i of one population: trial vector (thread 0, into `trial`), its NLL on the workspace U, selection into the next generation.
__device__ __forceinline__ void de_member(int n, int d, const double* __restrict__ X, const double* __restrict__ y, int P, int i,
                                          const double* __restrict__ pop, const double* __restrict__ energy, double* __restrict__ pop_next,
                                          double* __restrict__ energy_next, const double* __restrict__ lo, const double* __restrict__ hi,
                                          double F, double CR, unsigned long long seed, unsigned gen, double* __restrict__ U,
                                          double* smem_d, double* trial) {
  const int D = d + 2;
  if (threadIdx.x == 0) {
    int best = 0;                                    // best of the current generation (lowest index on ties)
    for (int p = 1; p < P; ++p)
      if (energy[p] < energy[best]) best = p;
    // two distinct members other than i (scipy _select_samples: a random permutation without the candidate)
    int r0 = (int)(u01(seed, gen, i, 0) * (P - 1));
    int r1 = (int)(u01(seed, gen, i, 1) * (P - 2));
    if (r0 >= i) ++r0;
    int lo_ = r0 < i ? r0 : i, hi_ = r0 < i ? i : r0;
    if (r1 >= lo_) ++r1;
    if (r1 >= hi_) ++r1;
    const int fill = (int)(u01(seed, gen, i, 2) * D);
    for (int a = 0; a < D; ++a) {
      double v = pop[(size_t)i * D + a];
      if (a == fill || u01(seed, gen, i, 8 + a) < CR) {
        v = pop[(size_t)best * D + a] + F * (pop[(size_t)r0 * D + a] - pop[(size_t)r1 * D + a]);
        if (v < lo[a] || v > hi[a]) v = lo[a] + u01(seed, gen, i, 64 + a) * (hi[a] - lo[a]);   // scipy re-draws out-of-bounds entries
      }
      trial[a] = v;
    }
  }
  __syncthreads();
  const double e = nll_member(n, d, X, y, trial, U, smem_d);
  if (threadIdx.x == 0) {
    const bool take = e <= energy[i];                // scipy: "if energy <= self.population_energies[candidate]"
    for (int a = 0; a < D; ++a) pop_next[(size_t)i * D + a] = take ? trial[a] : pop[(size_t)i * D + a];
    energy_next[i] = take ? e : energy[i];
  }
}

__global__ __launch_bounds__(1024) void k_de_step(int n, int d, const double* __restrict__ X, const double* __restrict__ y, int P,
                                                  const double* __restrict__ pop, const double* __restrict__ energy,
                                                  double* __restrict__ pop_next, double* __restrict__ energy_next,
                                                  const double* __restrict__ lo, const double* __restrict__ hi, double F, double CR,
                                                  unsigned long long seed, unsigned gen, double* __restrict__ work) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double trial[SBO_MAX_D + 2];
  const int i = blockIdx.x;
  de_member(n, d, X, y, P, i, pop, energy, pop_next, energy_next, lo, hi, F, CR, seed, gen, work + (size_t)i * n * n,
            reinterpret_cast<double*>(smem), trial);
}

// One generation of q searches side by side (sbo_fit_de_batch): grid (P, q), workgroup (i, o) is member i of output o's population
// [o][P][d + 2], with that output's seed and dithered F.  An output whose search has stopped (active[o] == 0) is left as it is: its
// workgroups return at once and its population stays in the buffer its last generation wrote.
struct DeTable {
  double F[SBO_MAX_Q];
  unsigned long long seed[SBO_MAX_Q];
  int active[SBO_MAX_Q];
};

__global__ __launch_bounds__(1024) void k_de_step_q(int n, int d, const double* __restrict__ X, const double* __restrict__ yT, int P,
                                                    const double* __restrict__ pop, const double* __restrict__ energy,
                                                    double* __restrict__ pop_next, double* __restrict__ energy_next,
                                                    const double* __restrict__ lo, const double* __restrict__ hi, DeTable tab, double CR,
                                                    unsigned gen, double* __restrict__ work) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double trial[SBO_MAX_D + 2];
  const int i = blockIdx.x, o = blockIdx.y, D = d + 2;
  if (!tab.active[o]) return;
  const size_t po = (size_t)o * P;
  de_member(n, d, X, yT + (size_t)o * n, P, i, pop + po * D, energy + po, pop_next + po * D, energy_next + po, lo, hi, tab.F[o], CR,
            tab.seed[o], gen, work + (po + i) * n * n, reinterpret_cast<double*>(smem), trial);
}

// The best member of every output's final population (lowest energy, lowest index on ties), read from the buffer that output
// stopped in (bit o of `parity`): best_x[q][d + 2], best_e[q].
__global__ void k_de_best(int q, int P, int D, const double* __restrict__ pop0, const double* __restrict__ pop1,
                          const double* __restrict__ en0, const double* __restrict__ en1, unsigned parity, double* __restrict__ best_x,
                          double* __restrict__ best_e) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= q) return;
  const double* pop = ((parity >> o) & 1u ? pop1 : pop0) + (size_t)o * P * D;
  const double* en = ((parity >> o) & 1u ? en1 : en0) + (size_t)o * P;
  int best = 0;
  for (int p = 1; p < P; ++p)
    if (en[p] < en[best]) best = p;
  for (int a = 0; a < D; ++a) best_x[(size_t)o * D + a] = pop[(size_t)best * D + a];
  best_e[o] = en[best];
}

// What the model is built from: the polished point of output o where its NLL is strictly lower than the DE's best, the DE's best
// otherwise (always, without a polish: loc_f == nullptr).
__global__ void k_fit_pick(int q, int D, const double* __restrict__ de_x, const double* __restrict__ de_e, const double* __restrict__ loc_x,
                           const double* __restrict__ loc_f, double* __restrict__ x_out, double* __restrict__ f_out,
                           int* __restrict__ polished) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= q) return;
  const bool take = loc_f && loc_f[o] < de_e[o];
  for (int a = 0; a < D; ++a) x_out[(size_t)o * D + a] = take ? loc_x[(size_t)o * D + a] : de_x[(size_t)o * D + a];
  f_out[o] = take ? loc_f[o] : de_e[o];
  polished[o] = take ? 1 : 0;
}

}  // namespace sbo

using namespace sbo;

static unsigned long long mix64_host(unsigned long long x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

extern "C" int sbo_nll_batch(sbo_ctx* c, int n, int d, const double* X_norm, const double* y, int P, const double* hyper,
                             double* out) {
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (n < 1 || n > SBO_MAX_N || d < 1 || d > SBO_MAX_D || P < 1) return fail(SBO_E_INVALID, "n, d or P out of range");
  if (!X_norm || !y || !hyper || !out) return fail(SBO_E_INVALID, "NULL argument");
  SBO_HIP(hipSetDevice(c->device));
  const size_t lds = sizeof(double) * ((size_t)n * d + 2 * (size_t)n);
  if (lds > 150 * 1024) return fail(SBO_E_UNSUPPORTED, "n * d too large for the fit kernel's LDS staging");
  int rc;
  double *dX, *dy, *dh, *dout;
  auto layout = [&](Carve cv) {
    cv.take(dX, (size_t)n * d); cv.take(dy, n);
    cv.take(dh, (size_t)P * (d + 2)); cv.take(dout, P);
    return cv.off;
  };
  if ((rc = carve(c->fitbuf, layout))) return rc;
  if ((rc = ensure(c->fitwork, sizeof(double) * (size_t)P * n * n))) return rc;
  SBO_HIP(hipMemcpyAsync(dX, X_norm, sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dy, y, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dh, hyper, sizeof(double) * (size_t)P * (d + 2), hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_nll_batch), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // 1024 threads per member for the larger matrices (more rows of the trailing update in flight); small ones keep 256
  hipLaunchKernelGGL(k_nll_batch, dim3(P), dim3(n >= 96 ? 1024 : 256), lds, c->stream, n, d, (const double*)dX, (const double*)dy,
                     (const double*)dh, (double*)c->fitwork.p, dout);
  SBO_HIP(hipGetLastError());
  SBO_HIP(hipMemcpyAsync(out, dout, sizeof(double) * P, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipStreamSynchronize(c->stream));
  return SBO_OK;
}

// Differential evolution of the NLL over the box [lo, hi]^(d+2) entirely on the device:
// init_pop[P, d + 2] is the caller's initial population (SciPy draws a Latin hypercube), `seed` keys the counter-based
// generator of the trial vectors, F is dithered per generation in [0.5, 1) as SciPy's default mutation=(0.5, 1) does.
// Stops after maxiter generations or when std(energies) <= atol + tol |mean(energies)| (SciPy's criterion, checked
// every 8 generations).  Returns the best member, its NLL and the generations run.
extern "C" int sbo_fit_de(sbo_ctx* c, int n, int d, const double* X_norm, const double* y, int P, const double* lo, const double* hi,
                          const double* init_pop, uint64_t seed, int maxiter, double tol, double atol, double* best_x,
                          double* best_energy, int* generations) {
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (n < 1 || n > SBO_MAX_N || d < 1 || d > SBO_MAX_D || P < 4 || maxiter < 0) return fail(SBO_E_INVALID, "n, d, P or maxiter out of range");
  if (!X_norm || !y || !lo || !hi || !init_pop || !best_x || !best_energy) return fail(SBO_E_INVALID, "NULL argument");
  SBO_HIP(hipSetDevice(c->device));
  const int D = d + 2;
  const size_t lds = sizeof(double) * ((size_t)n * d + 2 * (size_t)n);
  if (lds > 150 * 1024) return fail(SBO_E_UNSUPPORTED, "n * d too large for the fit kernel's LDS staging");
  int rc;
  double *dX, *dy, *dpop[2], *den[2], *dlo, *dhi;
  auto layout = [&](Carve cv) {
    cv.take(dX, (size_t)n * d); cv.take(dy, n);
    cv.take(dpop[0], (size_t)P * D); cv.take(dpop[1], (size_t)P * D);
    cv.take(den[0], P); cv.take(den[1], P);
    cv.take(dlo, D); cv.take(dhi, D);
    return cv.off;
  };
  if ((rc = carve(c->fitbuf, layout))) return rc;
  if ((rc = ensure(c->fitwork, sizeof(double) * (size_t)P * n * n))) return rc;
  SBO_HIP(hipMemcpyAsync(dX, X_norm, sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dy, y, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dpop[0], init_pop, sizeof(double) * (size_t)P * D, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dlo, lo, sizeof(double) * D, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dhi, hi, sizeof(double) * D, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_nll_batch), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_de_step), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int threads = n >= 96 ? 1024 : 256;
  hipLaunchKernelGGL(k_nll_batch, dim3(P), dim3(threads), lds, c->stream, n, d, (const double*)dX, (const double*)dy,
                     (const double*)dpop[0], (double*)c->fitwork.p, den[0]);
  std::vector<double> he(P);
  int cur = 0, gen = 0;
  unsigned long long fstate = mix64_host(seed);
  for (; gen < maxiter; ++gen) {
    fstate = mix64_host(fstate);
    const double F = 0.5 + 0.5 * ((double)(fstate >> 11) * (1.0 / 9007199254740992.0));
    hipLaunchKernelGGL(k_de_step, dim3(P), dim3(threads), lds, c->stream, n, d, (const double*)dX, (const double*)dy, P,
                       (const double*)dpop[cur], (const double*)den[cur], dpop[cur ^ 1], den[cur ^ 1], (const double*)dlo,
                       (const double*)dhi, F, 0.7, (unsigned long long)seed, (unsigned)gen, (double*)c->fitwork.p);
    cur ^= 1;
    if ((gen & 7) == 7 || gen + 1 == maxiter) {
      SBO_HIP(hipMemcpyAsync(he.data(), den[cur], sizeof(double) * P, hipMemcpyDeviceToHost, c->stream));
      SBO_HIP(hipStreamSynchronize(c->stream));
      double mean = 0, var = 0;
      bool finite = true;
      for (double e : he) { mean += e; finite = finite && std::isfinite(e); }
      mean /= P;
      for (double e : he) var += (e - mean) * (e - mean);
      if (finite && std::sqrt(var / P) <= atol + tol * std::fabs(mean)) { ++gen; break; }
    }
  }
  SBO_HIP(hipGetLastError());
  std::vector<double> hp((size_t)P * D);
  SBO_HIP(hipMemcpyAsync(he.data(), den[cur], sizeof(double) * P, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipMemcpyAsync(hp.data(), dpop[cur], sizeof(double) * (size_t)P * D, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipStreamSynchronize(c->stream));
  int best = 0;
  for (int p = 1; p < P; ++p)
    if (he[p] < he[best]) best = p;
  for (int a = 0; a < D; ++a) best_x[a] = hp[(size_t)best * D + a];
  *best_energy = he[best];
  if (generations) *generations = gen;
  return SBO_OK;
}

// ---- analytic gradient of the NLL and the multistart local fit (models/GP_Classic.py:168-240) -------------------------------
// GP_Classic minimises the same objective as GP_Safe with SciPy SLSQP from Sobol starts and jac = grad(NLL).  With
// alpha = K^-1 y, Q = K^-1 - alpha alpha^T and Kf the noise-free part of K (W_a = exp(2 h_a), sn2 = exp(2 h_{d+1})):
//     dNLL/dh_a     = sum_ik Q_ik Kf_ik (x_ia - x_ka)^2 / W_a      (a < d)
//     dNLL/dh_d     = 2 sum_ik Q_ik Kf_ik
//     dNLL/dh_{d+1} = 2 sn2 tr Q
// nll_member leaves K = U^T U (U upper, row-major) and z = U^-T y.  The strictly lower triangle of the same buffer then takes
// V = U^-T (row j of V at U[j n + i], i < j; the diagonal 1 / U_jj lives in LDS), so K^-1 = V^T V is formed entry by entry as the
// contraction consumes it: K^-1_ik = sum_{j >= max(i, k)} V_ji V_jk.  Every sum runs in a fixed order; the workgroup reduction
// is a butterfly per wave and then the waves in index order, so repeated calls give the same bits.
namespace sbo {

constexpr int kFitD = SBO_MAX_D + 2;

// LDS of the gradient kernels: nll_member's [n d + 2 n] followed by col[n] and dinv[n]
inline size_t nll_grad_lds(int n, int d) { return sizeof(double) * ((size_t)n * d + 4 * (size_t)n); }

// NLL (bit for bit nll_member's) and its gradient grad[d + 2] (LDS, valid in every thread on return) of one h[d + 2].
__device__ double nll_grad_member(int n, int d, const double* __restrict__ X, const double* __restrict__ y, const double* h,
                                  double* __restrict__ U, double* smem_d, double* grad) {
  __shared__ double sh_f;
  __shared__ double sh_part[16][kFitD];               // per-wave partial sums (at most 1024 threads)
  const double f = nll_member(n, d, X, y, h, U, smem_d);
  const int tid = threadIdx.x, D = d + 2;
  const int lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  if (tid == 0) sh_f = f;
  __syncthreads();
  const double nll = sh_f;
  if (!(nll < INFINITY)) {                            // a pivot <= 0: no factor, no gradient
    if (tid == 0)
      for (int a = 0; a < D; ++a) grad[a] = NAN;
    __syncthreads();
    return nll;
  }
  double* Xa = smem_d;                                // nll_member's X W^-1/2, still in place
  double* alpha = Xa + (size_t)n * d;                 // (nll_member's sq: no longer needed)
  const double* z = alpha + n;
  double* col = alpha + 2 * n;
  double* dinv = col + n;
  for (int i = tid; i < n; i += blockDim.x) dinv[i] = 1.0 / U[(size_t)i * n + i];
  __syncthreads();
  // V = U^-T row by row: V_ji = -(1 / U_jj) sum_{m = i}^{j-1} U_mj V_mi
  for (int j = 1; j < n; ++j) {
    for (int m = tid; m < j; m += blockDim.x) col[m] = U[(size_t)m * n + j];
    __syncthreads();
    for (int i = tid; i < j; i += blockDim.x) {
      double s = 0.0;
      for (int m = j - 1; m > i; --m) s += col[m] * U[(size_t)m * n + i];      // (a common m per step: coalesced over i)
      s += col[i] * dinv[i];
      U[(size_t)j * n + i] = -dinv[j] * s;
    }
    __syncthreads();
  }
  // alpha = K^-1 y = V^T z
  for (int i = tid; i < n; i += blockDim.x) {
    double s = 0.0;
    for (int j = n - 1; j > i; --j) s += U[(size_t)j * n + i] * z[j];
    alpha[i] = s + dinv[i] * z[i];
  }
  __syncthreads();
  const double sf2 = exp(2.0 * h[d]);
  const double sn2 = exp(2.0 * h[d + 1]);
  double acc[SBO_MAX_D], acc_f = 0.0, acc_tr = 0.0;    // (length-scale terms, signal term, trace of Q)
#pragma unroll
  for (int a = 0; a < SBO_MAX_D; ++a) acc[a] = 0.0;
  // pairs i <= k of the symmetric sum (off-diagonal pairs count twice); lanes take consecutive k of one row i
  for (long long idx = tid; idx < (long long)n * n; idx += blockDim.x) {
    const int i = (int)(idx / n), k = (int)(idx % n);
    if (k < i) continue;
    double kinv = 0.0;
    for (int j = n - 1; j > k; --j) kinv += U[(size_t)j * n + i] * U[(size_t)j * n + k];
    kinv += (k > i ? U[(size_t)k * n + i] : dinv[k]) * dinv[k];
    const double qik = kinv - alpha[i] * alpha[k];
    double r2[SBO_MAX_D];
    double dist = 0.0;
#pragma unroll
    for (int a = 0; a < SBO_MAX_D; ++a) {
      if (a < d) {
        const double r = Xa[i * d + a] - Xa[k * d + a];
        r2[a] = r * r;
        dist += r2[a];
      }
    }
    const double w = (k == i ? 1.0 : 2.0) * (qik * (sf2 * exp(-0.5 * dist)));
#pragma unroll
    for (int a = 0; a < SBO_MAX_D; ++a)
      if (a < d) acc[a] += w * r2[a];
    acc_f += w;
    if (k == i) acc_tr += qik;
  }
#pragma unroll
  for (int a = 0; a < SBO_MAX_D + 2; ++a) {
    double v = a < SBO_MAX_D ? acc[a] : a == SBO_MAX_D ? acc_f : acc_tr;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int slot = a < SBO_MAX_D ? a : a - SBO_MAX_D + d;
    if (lane == 0 && (a < d || a >= SBO_MAX_D)) sh_part[wave][slot] = v;
  }
  __syncthreads();
  if (tid == 0) {
    for (int a = 0; a < D; ++a) {
      double s = 0.0;
      for (int w = 0; w < nw; ++w) s += sh_part[w][a];
      grad[a] = a < d ? s : a == d ? 2.0 * s : 2.0 * sn2 * s;
    }
  }
  __syncthreads();
  return nll;
}

__global__ __launch_bounds__(1024) void k_nll_grad_batch(int n, int d, const double* __restrict__ X, const double* __restrict__ y,
                                                         const double* __restrict__ hyper, double* __restrict__ work,
                                                         double* __restrict__ nll_out, double* __restrict__ grad_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double g[kFitD];
  const int p = blockIdx.x, D = d + 2;
  const double v = nll_grad_member(n, d, X, y, hyper + (size_t)p * D, work + (size_t)p * n * n, reinterpret_cast<double*>(smem), g);
  if (threadIdx.x == 0) {
    nll_out[p] = v;
    for (int a = 0; a < D; ++a) grad_out[(size_t)p * D + a] = g[a];
  }
}

// ---- projected BFGS on the box, one workgroup per (output, start) ------------------------------------------------------------
// Thread 0 runs the (d + 2)-dimensional algebra on LDS state -- the shared core of pbfgs.hpp in the unit metric --; the whole
// workgroup evaluates NLL + gradient at thread 0's trial point.  See DESIGN.md section 10 for the contract.
struct FitState {
  PbfgsState<kFitD> s;
  double lo[kFitD], hi[kFitD];
  double f;
  int phase, iter, nev, status;
};
enum { FIT_PH_START = 0, FIT_PH_SEARCH = 1 };

__device__ const double kFitUnit[kFitD] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0};

// the box of the hyper-parameters in the unit metric; a steepest-descent step moves at most one unit of log scale
__device__ __forceinline__ PbfgsBox fit_box(const FitState& S) { return {S.lo, S.hi, kFitUnit, kFitUnit, 1.0}; }

// Start a new iteration at the accepted point: true with the first trial of the line search in `trial`, false when done.
__device__ bool fit_new_iteration(FitState& S, int D, double* trial, int maxiter, double gtol) {
  const PbfgsBox bx = fit_box(S);
  if (pbfgs_pgnorm(S.s, bx, D) <= gtol) { S.status = SBO_FIT_GTOL; return false; }
  if (S.iter >= maxiter) { S.status = SBO_FIT_MAXITER; return false; }
  pbfgs_direction(S.s, bx, D, trial);
  S.phase = FIT_PH_SEARCH;
  return true;
}

// Consume the evaluation (ft, tg) of `trial`; true when `trial` holds the next point to evaluate.
__device__ __noinline__ bool fit_advance(FitState& S, int D, double ft, const double* tg, double* trial, int maxiter, double ftol, double gtol) {
  ++S.nev;
  bool ok = ft < INFINITY;            // (a trial without a factor, or with a non-finite gradient, is refused)
  for (int a = 0; a < D; ++a) ok = ok && isfinite(tg[a]);
  if (S.phase == FIT_PH_START) {
    for (int a = 0; a < D; ++a) { S.s.x[a] = trial[a]; S.s.g[a] = tg[a]; }
    S.f = ft;
    if (!ok) { S.status = SBO_FIT_NOT_PD; return false; }
    return fit_new_iteration(S, D, trial, maxiter, gtol);
  }
  const PbfgsBox bx = fit_box(S);
  bool moved;
  if (pbfgs_armijo(S.s, D, trial, ok, ft, S.f, moved)) {
    pbfgs_update(S.s, bx, D, trial, tg);
    const double fprev = S.f;
    S.f = ft;
    ++S.iter;
    if (fabs(fprev - S.f) < ftol) { S.status = SBO_FIT_FTOL; return false; }
    return fit_new_iteration(S, D, trial, maxiter, gtol);
  }
  if (pbfgs_backtrack(S.s, bx, D, moved, trial)) return true;
  if (S.s.h_identity) { S.status = SBO_FIT_LINESEARCH; return false; }
  pbfgs_reset_h(S.s, bx, D);                                         // the quasi-Newton direction failed: one steepest-descent try
  ++S.iter;
  return fit_new_iteration(S, D, trial, maxiter, gtol);
}

// starts: [P][d + 2] shared by the outputs (starts_per_output == 0) or [q][P][d + 2] (starts_per_output == P).
__global__ __launch_bounds__(1024) void k_fit_local(int n, int d, int P, const double* __restrict__ X, const double* __restrict__ yT,
                                                    const double* __restrict__ starts, int starts_per_output, const double* __restrict__ lo,
                                                    const double* __restrict__ hi, int maxiter, double ftol, double gtol,
                                                    double* __restrict__ work, double* __restrict__ h_out, double* __restrict__ f_out,
                                                    double* __restrict__ pg_out, int* __restrict__ it_out, int* __restrict__ ev_out,
                                                    int* __restrict__ st_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ FitState S;
  __shared__ double trial[kFitD], tg[kFitD];
  __shared__ int go;
  const int m = blockIdx.x, o = m / P, s = m % P, D = d + 2;
  if (threadIdx.x == 0) {
    for (int a = 0; a < D; ++a) {
      S.lo[a] = lo[a];
      S.hi[a] = hi[a];
      trial[a] = clip_to(starts[((size_t)o * starts_per_output + s) * D + a], lo[a], hi[a]);   // SLSQP clips x0 into the bounds
    }
    pbfgs_reset_h(S.s, fit_box(S), D);
    S.phase = FIT_PH_START;
    S.iter = S.nev = 0;
    S.status = -1;
    go = 1;
  }
  __syncthreads();
  double* U = work + (size_t)m * n * n;
  const double* y = yT + (size_t)o * n;
  while (go) {
    const double ft = nll_grad_member(n, d, X, y, trial, U, reinterpret_cast<double*>(smem), tg);
    if (threadIdx.x == 0) go = fit_advance(S, D, ft, tg, trial, maxiter, ftol, gtol);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    for (int a = 0; a < D; ++a) h_out[(size_t)m * D + a] = S.s.x[a];
    f_out[m] = S.f;
    pg_out[m] = S.status == SBO_FIT_NOT_PD ? NAN : pbfgs_pgnorm(S.s, fit_box(S), D);
    it_out[m] = S.iter;
    ev_out[m] = S.nev;
    st_out[m] = S.status;
  }
}

}  // namespace sbo

extern "C" int sbo_nll_grad_batch(sbo_ctx* c, int n, int d, const double* X_norm, const double* y, int P, const double* hyper,
                                  double* nll_out, double* grad_out) {
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (n < 1 || n > SBO_MAX_N || d < 1 || d > SBO_MAX_D || P < 1) return fail(SBO_E_INVALID, "n, d or P out of range");
  if (!X_norm || !y || !hyper || !nll_out || !grad_out) return fail(SBO_E_INVALID, "NULL argument");
  SBO_HIP(hipSetDevice(c->device));
  const int D = d + 2;
  const size_t lds = nll_grad_lds(n, d);
  if (lds > 150 * 1024) return fail(SBO_E_UNSUPPORTED, "n * d too large for the fit kernel's LDS staging");
  int rc;
  double *dX, *dy, *dh, *dg, *dout;
  auto layout = [&](Carve cv) {
    cv.take(dX, (size_t)n * d); cv.take(dy, n);
    cv.take(dh, (size_t)P * D); cv.take(dg, (size_t)P * D); cv.take(dout, P);
    return cv.off;
  };
  if ((rc = carve(c->fitbuf, layout))) return rc;
  if ((rc = ensure(c->fitwork, sizeof(double) * (size_t)P * n * n))) return rc;
  SBO_HIP(hipMemcpyAsync(dX, X_norm, sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dy, y, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dh, hyper, sizeof(double) * (size_t)P * D, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_nll_grad_batch), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_nll_grad_batch, dim3(P), dim3(n >= 96 ? 1024 : 256), lds, c->stream, n, d, (const double*)dX, (const double*)dy,
                     (const double*)dh, (double*)c->fitwork.p, dout, dg);
  SBO_HIP(hipGetLastError());
  SBO_HIP(hipMemcpyAsync(nll_out, dout, sizeof(double) * P, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipMemcpyAsync(grad_out, dg, sizeof(double) * (size_t)P * D, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipStreamSynchronize(c->stream));
  return SBO_OK;
}

extern "C" int sbo_fit_local(sbo_ctx* c, int n, int d, int q, const double* X_norm, const double* Y_norm, int P, const double* starts,
                             const double* lo, const double* hi, int maxiter, double ftol, double gtol, double* best_x, double* best_nll,
                             double* x_out, double* nll_out, int* iters_out, int* evals_out, double* pgnorm_out, int* status_out) {
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (n < 1 || n > SBO_MAX_N || d < 1 || d > SBO_MAX_D || q < 1 || q > SBO_MAX_Q || P < 1 || maxiter < 0)
    return fail(SBO_E_INVALID, "n, d, q, P or maxiter out of range");
  if (!X_norm || !Y_norm || !starts || !lo || !hi || !best_x || !best_nll) return fail(SBO_E_INVALID, "NULL argument");
  if (!(ftol >= 0.0) || !(gtol >= 0.0)) return fail(SBO_E_INVALID, "ftol and gtol must be >= 0");
  const int D = d + 2;
  for (int a = 0; a < D; ++a)
    if (!(lo[a] <= hi[a])) return fail(SBO_E_INVALID, "bounds need lo <= hi");
  SBO_HIP(hipSetDevice(c->device));
  const size_t lds = nll_grad_lds(n, d);
  if (lds > 150 * 1024) return fail(SBO_E_UNSUPPORTED, "n * d too large for the fit kernel's LDS staging");
  const size_t M = (size_t)q * P;
  int rc;
  double *dX, *dy, *dst, *dlo, *dhi, *dh, *df, *dpg;
  int *dit, *dev, *dstat;                              // (read back as one block of 3 M)
  auto layout = [&](Carve cv) {
    cv.take(dX, (size_t)n * d); cv.take(dy, (size_t)q * n);
    cv.take(dst, (size_t)P * D); cv.take(dlo, D); cv.take(dhi, D);
    cv.take(dh, M * D); cv.take(df, M); cv.take(dpg, M);
    cv.take(dit, M); cv.take(dev, M); cv.take(dstat, M);
    return cv.off;
  };
  if ((rc = carve(c->fitbuf, layout))) return rc;
  if ((rc = ensure(c->fitwork, sizeof(double) * M * n * n))) return rc;
  std::vector<double> yT((size_t)q * n);               // one contiguous column per output
  for (int i = 0; i < n; ++i)
    for (int o = 0; o < q; ++o) yT[(size_t)o * n + i] = Y_norm[(size_t)i * q + o];
  SBO_HIP(hipMemcpyAsync(dX, X_norm, sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dy, yT.data(), sizeof(double) * (size_t)q * n, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dst, starts, sizeof(double) * (size_t)P * D, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dlo, lo, sizeof(double) * D, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dhi, hi, sizeof(double) * D, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_fit_local), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_fit_local, dim3((unsigned)M), dim3(n >= 96 ? 1024 : 256), lds, c->stream, n, d, P, (const double*)dX,
                     (const double*)dy, (const double*)dst, 0, (const double*)dlo, (const double*)dhi, maxiter, ftol, gtol,
                     (double*)c->fitwork.p, dh, df, dpg, dit, dev, dstat);
  SBO_HIP(hipGetLastError());
  std::vector<double> hh(M * D), hf(M), hpg(M);
  std::vector<int> hit(3 * M);
  SBO_HIP(hipMemcpyAsync(hh.data(), dh, sizeof(double) * M * D, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipMemcpyAsync(hf.data(), df, sizeof(double) * M, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipMemcpyAsync(hpg.data(), dpg, sizeof(double) * M, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipMemcpyAsync(hit.data(), dit, sizeof(int) * 3 * M, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipStreamSynchronize(c->stream));
  for (int o = 0; o < q; ++o) {
    int best = 0;                                      // jnp.argmin: the first of equal values
    for (int s = 1; s < P; ++s)
      if (hf[(size_t)o * P + s] < hf[(size_t)o * P + best]) best = s;
    for (int a = 0; a < D; ++a) best_x[(size_t)o * D + a] = hh[((size_t)o * P + best) * D + a];
    best_nll[o] = hf[(size_t)o * P + best];
  }
  if (x_out) std::copy(hh.begin(), hh.end(), x_out);
  if (nll_out) std::copy(hf.begin(), hf.end(), nll_out);
  if (pgnorm_out) std::copy(hpg.begin(), hpg.end(), pgnorm_out);
  if (iters_out) std::copy(hit.begin(), hit.begin() + M, iters_out);
  if (evals_out) std::copy(hit.begin() + M, hit.begin() + 2 * M, evals_out);
  if (status_out) std::copy(hit.begin() + 2 * M, hit.end(), status_out);
  return SBO_OK;
}

// ---- all outputs side by side: batched DE, per-output polish --------------------------------------------
// The device side of sbo_fit_de_batch and sbo_model_fit.  The DE of output o is sbo_fit_de's for column o with seeds[o], launch for
// launch: the same nll_member on the same workgroup size, the same draws, the same F sequence and the same convergence test on
// the same cadence, so the result is the same bits.  One read-back of the q P energies per check is the only host wait of the
// search.  The polish (polish != 0) is one k_fit_local launch with one start per output, the DE's best as k_de_best left it in
// device memory; k_fit_pick keeps it where it is strictly lower.  One more read-back returns everything.
namespace sbo {

int fit_batch(sbo_ctx* c, int n, int d, int q, const double* X_norm, const double* Y_norm, int P, const double* lo, const double* hi,
              const double* init_pop, const uint64_t* seeds, int maxiter, double tol, double atol, int polish, int polish_maxiter,
              double ftol, double gtol, FitBatchResult& out) {
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  SBO_HIP(hipSetDevice(c->device));
  const int D = d + 2;
  const size_t lds = sizeof(double) * ((size_t)n * d + 2 * (size_t)n);
  const size_t lds_g = nll_grad_lds(n, d);
  if ((polish ? lds_g : lds) > 150 * 1024) return fail(SBO_E_UNSUPPORTED, "n * d too large for the fit kernel's LDS staging");
  const size_t M = (size_t)q * P;
  int rc;
  // X | yT | pop[2] | energy[2] | lo | hi | final x, nll, DE best x, nll (read back as one block) | polish x, f, pgnorm |
  // polish iters, evals, status, polished (ints)
  double *dX, *dy, *dpop[2], *den[2], *dlo, *dhi, *dfin_x, *dfin_f, *dde_x, *dde_f, *dloc_x, *dloc_f, *dloc_pg;
  int *dit, *dev, *dstat, *dpolished;                  // (read back as one block of 4 q)
  auto layout = [&](Carve cv) {
    cv.take(dX, (size_t)n * d); cv.take(dy, (size_t)q * n);
    cv.take(dpop[0], M * D); cv.take(dpop[1], M * D);
    cv.take(den[0], M); cv.take(den[1], M);
    cv.take(dlo, D); cv.take(dhi, D);
    cv.take(dfin_x, (size_t)q * D); cv.take(dfin_f, q); cv.take(dde_x, (size_t)q * D); cv.take(dde_f, q);
    cv.take(dloc_x, (size_t)q * D); cv.take(dloc_f, q); cv.take(dloc_pg, q);
    cv.take(dit, q); cv.take(dev, q); cv.take(dstat, q); cv.take(dpolished, q);
    return cv.off;
  };
  if ((rc = carve(c->fitbuf, layout))) return rc;
  const size_t res_elems = (size_t)(dloc_x - dfin_x);  // final x, nll, DE best x, nll
  if ((rc = ensure(c->fitwork, sizeof(double) * M * n * n))) return rc;
  std::vector<double> yT((size_t)q * n);               // one contiguous column per output
  for (int i = 0; i < n; ++i)
    for (int o = 0; o < q; ++o) yT[(size_t)o * n + i] = Y_norm[(size_t)i * q + o];
  SBO_HIP(hipMemcpyAsync(dX, X_norm, sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dy, yT.data(), sizeof(double) * (size_t)q * n, hipMemcpyHostToDevice, c->stream));
  for (int o = 0; o < q; ++o)                          // every output starts from the caller's population
    SBO_HIP(hipMemcpyAsync(dpop[0] + (size_t)o * P * D, init_pop, sizeof(double) * (size_t)P * D, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dlo, lo, sizeof(double) * D, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemcpyAsync(dhi, hi, sizeof(double) * D, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_nll_batch_q), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_de_step_q), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int threads = n >= 96 ? 1024 : 256;
  const dim3 grid(P, q);
  hipLaunchKernelGGL(k_nll_batch_q, grid, dim3(threads), lds, c->stream, n, d, P, (const double*)dX, (const double*)dy,
                     (const double*)dpop[0], (double*)c->fitwork.p, den[0]);
  std::vector<double> he(M);
  DeTable tab;
  unsigned long long fstate[SBO_MAX_Q];
  int n_active = 0;
  unsigned parity = 0;                                 // bit o: the buffer output o's final population is in
  out.host_syncs = 0;
  for (int o = 0; o < SBO_MAX_Q; ++o) {
    tab.F[o] = 0.0;
    tab.seed[o] = o < q ? seeds[o] : 0;
    tab.active[o] = o < q && maxiter > 0;
    fstate[o] = mix64_host(tab.seed[o]);
    if (o < q) out.generations[o] = maxiter > 0 ? maxiter : 0;
    n_active += tab.active[o];
  }
  int cur = 0;
  for (int gen = 0; gen < maxiter && n_active; ++gen) {
    for (int o = 0; o < q; ++o) {
      if (!tab.active[o]) continue;
      fstate[o] = mix64_host(fstate[o]);
      tab.F[o] = 0.5 + 0.5 * ((double)(fstate[o] >> 11) * (1.0 / 9007199254740992.0));
    }
    hipLaunchKernelGGL(k_de_step_q, grid, dim3(threads), lds, c->stream, n, d, (const double*)dX, (const double*)dy, P,
                       (const double*)dpop[cur], (const double*)den[cur], dpop[cur ^ 1], den[cur ^ 1], (const double*)dlo,
                       (const double*)dhi, tab, 0.7, (unsigned)gen, (double*)c->fitwork.p);
    cur ^= 1;
    for (int o = 0; o < q; ++o)
      if (tab.active[o]) parity = (parity & ~(1u << o)) | ((unsigned)cur << o);
    if ((gen & 7) == 7 || gen + 1 == maxiter) {
      SBO_HIP(hipMemcpyAsync(he.data(), den[cur], sizeof(double) * M, hipMemcpyDeviceToHost, c->stream));
      SBO_HIP(hipStreamSynchronize(c->stream));
      ++out.host_syncs;
      for (int o = 0; o < q; ++o) {
        if (!tab.active[o]) continue;
        const double* e = he.data() + (size_t)o * P;
        double mean = 0, var = 0;
        bool finite = true;
        for (int p = 0; p < P; ++p) { mean += e[p]; finite = finite && std::isfinite(e[p]); }
        mean /= P;
        for (int p = 0; p < P; ++p) var += (e[p] - mean) * (e[p] - mean);
        if (finite && std::sqrt(var / P) <= atol + tol * std::fabs(mean)) {
          tab.active[o] = 0;
          --n_active;
          out.generations[o] = gen + 1;
        }
      }
    }
  }
  SBO_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_de_best, dim3(1), dim3(64), 0, c->stream, q, P, D, (const double*)dpop[0], (const double*)dpop[1],
                     (const double*)den[0], (const double*)den[1], parity, dde_x, dde_f);
  const auto t1 = clk::now();                          // (the search's last check has drained the stream)
  if (polish) {
    SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_fit_local), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_g));
    hipLaunchKernelGGL(k_fit_local, dim3(q), dim3(threads), lds_g, c->stream, n, d, 1, (const double*)dX, (const double*)dy,
                       (const double*)dde_x, 1, (const double*)dlo, (const double*)dhi, polish_maxiter, ftol, gtol,
                       (double*)c->fitwork.p, dloc_x, dloc_f, dloc_pg, dit, dev, dstat);
  }
  hipLaunchKernelGGL(k_fit_pick, dim3(1), dim3(64), 0, c->stream, q, D, (const double*)dde_x, (const double*)dde_f,
                     (const double*)dloc_x, polish ? (const double*)dloc_f : (const double*)nullptr, dfin_x, dfin_f, dpolished);
  SBO_HIP(hipGetLastError());
  std::vector<double> hres(res_elems);
  std::vector<int> hint(4 * (size_t)q);
  SBO_HIP(hipMemcpyAsync(hres.data(), dfin_x, sizeof(double) * res_elems, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipMemcpyAsync(hint.data(), dit, sizeof(int) * 4 * (size_t)q, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipStreamSynchronize(c->stream));
  ++out.host_syncs;
  const double* hfin_f = hres.data() + (size_t)q * D;
  const double* hde_x = hfin_f + q;
  const double* hde_f = hde_x + (size_t)q * D;
  for (int o = 0; o < q; ++o) {
    for (int a = 0; a < D; ++a) {
      out.x[o][a] = hres[(size_t)o * D + a];
      out.de_x[o][a] = hde_x[(size_t)o * D + a];
    }
    out.nll[o] = hfin_f[o];
    out.de_nll[o] = hde_f[o];
    out.polish_evals[o] = polish ? hint[(size_t)q + o] : 0;
    out.polish_status[o] = polish ? hint[2 * (size_t)q + o] : -1;
    out.polished[o] = hint[3 * (size_t)q + o];
  }
  const auto t2 = clk::now();
  out.de_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
  out.polish_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
  return SBO_OK;
}

}  // namespace sbo

extern "C" int sbo_fit_de_batch(sbo_ctx* c, int n, int d, int q, const double* X_norm, const double* Y_norm, int P, const double* lo,
                                const double* hi, const double* init_pop, const uint64_t* seeds, int maxiter, double tol, double atol,
                                double* best_x, double* best_energy, int* generations) {
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (n < 1 || n > SBO_MAX_N || d < 1 || d > SBO_MAX_D || q < 1 || q > SBO_MAX_Q || P < 4 || maxiter < 0)
    return fail(SBO_E_INVALID, "n, d, q, P or maxiter out of range");
  if (!X_norm || !Y_norm || !lo || !hi || !init_pop || !seeds || !best_x || !best_energy) return fail(SBO_E_INVALID, "NULL argument");
  FitBatchResult r;
  const int rc = fit_batch(c, n, d, q, X_norm, Y_norm, P, lo, hi, init_pop, seeds, maxiter, tol, atol, 0, 0, 0.0, 0.0, r);
  if (rc) return rc;
  for (int o = 0; o < q; ++o) {
    for (int a = 0; a < d + 2; ++a) best_x[(size_t)o * (d + 2) + a] = r.de_x[o][a];
    best_energy[o] = r.de_nll[o];
    if (generations) generations[o] = r.generations[o];
  }
  return SBO_OK;
}
