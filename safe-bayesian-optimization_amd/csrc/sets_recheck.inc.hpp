// sets_recheck.inc.hpp: fp32 sweeps whose decisions equal the fp64 result -- part of the sets.hip translation unit (included
// inside namespace sbo; not a standalone header).
//
// SURVEY.md section 7, hard part 2: `lcb >= 0` flips for candidates whose bound lies inside the rounding band of the fp32
// posterior.  How wide that band is depends on the model (1e-6 normalised at cond(K) ~ 1e3, beyond 1e-3 at the noise floor of the
// reference's fit), so it is MEASURED per (model, candidate set) by the fp64 twin at probe candidates (rc_bands below: never under
// 1e-4 normalised, 16 x the largest deviation seen; sbo_profile.fp32_band_dm / fp32_band_dv), and every decision is first taken with
// INTERVALS: a candidate's bounds are known to +- (dm, dv), u* to [u_lo, u_hi], the largest variance over M from below.  Candidates
// whose intervals cannot decide
//   (iv) the sign of a constraint's lcb                          (S, U)
//   (i)  whether they attain u* = min_S ucb_0                    (u*)
//   (ii) lcb_0 <= u*                                             (M)
//   (iii) whether they hold the largest var_0 over M             (Minimizer's arg-max)
// are listed, their posterior is re-evaluated in fp64 by the model's fp64 twin (generic K1 kernel on the compacted list),
// and the whole set phase then runs in fp64 arithmetic on the widened fp32 posterior with the listed entries replaced.
// S, U, u*, M and the minimiser are then those of an fp64 sweep.  The expander sets need two more things: the Lipschitz
// constant in fp64 (k_rc_grad64: the mean gradient is O(n d) per candidate, no contraction) and verdict kernels that
// carry the band of an unrefined ucb (RcExp in sets_expander.inc.hpp): a verdict the band cannot settle defers the
// candidate, and so does an unrefined member of G_c that could hold its largest variance.  Deferred candidates are
// re-evaluated and the set phase runs again, until nothing is deferred (each candidate is refined at most once).
//
// r04: the same machinery serves the GUARD BAND of an approximating fp64 posterior (K1b / K1t, device_common.hpp: GuardBand): a
// sweep whose fast pass counted decisions inside the band (SweepScalars::n_guard) comes here with TP = double -- the intervals
// are +- (dm, dv) of the plan's band, the listed candidates are re-evaluated by the exact kernel (guard_exact_list) and their
// values replace the approximate ones IN PLACE, the Lipschitz keys are recomputed exactly, and the set phase runs again.
#pragma once

__device__ __forceinline__ void rc_interval(double m, double v, double b, double dm, double dv, double& lcb_lo, double& lcb_hi, double& ucb_lo,
                                            double& ucb_hi) {
  const double md = (double)m, vd = (double)v;
  const double s_hi = b * sqrt(vd + dv), s_lo = b * sqrt(fmax(0.0, vd - dv));
  lcb_lo = (md - dm) - s_hi;
  lcb_hi = (md + dm) - s_lo;
  ucb_lo = (md - dm) + s_lo;
  ucb_hi = (md + dm) + s_hi;
}

// possibly / surely safe from the constraints' intervals; `undecided`: some constraint's lcb interval contains zero
template <typename TP>
__device__ __forceinline__ void rc_safety(const TP* __restrict__ mean, const TP* __restrict__ var, long long n, long long g, int q,
                                          double b, const RcBand& bd, bool& possibly, bool& surely, bool& undecided) {
  possibly = surely = true;
  undecided = false;
  for (int c = 1; c < q; ++c) {
    double ll, lh, ul, uh;
    rc_interval((double)mean[(size_t)c * n + g], (double)var[(size_t)c * n + g], b, bd.dm[c], bd.dv[c], ll, lh, ul, uh);
    possibly = possibly && lh >= 0.0;
    surely = surely && ll >= 0.0;
    undecided = undecided || (ll <= 0.0 && lh >= 0.0);
  }
}

// pass 1: u_lo = min over possibly-safe of ucb0_lo, u_hi = min over surely-safe of ucb0_hi
template <typename TP>
__global__ __launch_bounds__(256) void k_rc_ustar(const TP* __restrict__ mean, const TP* __restrict__ var, long long n, int q, double b,
                                                  const RcBand bd, RcScal* sc) {
  unsigned long long klo = ~0ull, khi = ~0ull;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x) {
    bool ps, ss, un;
    rc_safety(mean, var, n, g, q, b, bd, ps, ss, un);
    if (!ps) continue;
    double ll, lh, ul, uh;
    rc_interval((double)mean[g], (double)var[g], b, bd.dm[0], bd.dv[0], ll, lh, ul, uh);
    const unsigned long long a = ord_key(ul), h = ord_key(uh);
    klo = a < klo ? a : klo;
    if (ss) khi = h < khi ? h : khi;
  }
  klo = block_ext_u64<false>(klo);
  khi = block_ext_u64<false>(khi);
  if (threadIdx.x == 0) {
    atomicMin(&sc->ulo_key, klo);
    atomicMin(&sc->uhi_key, khi);
  }
}
// pass 2: vmax_lo = max over surely-in-M (surely safe, lcb0_hi <= u_lo) of max(0, var0 - dv)
template <typename TP>
__global__ __launch_bounds__(256) void k_rc_vmax(const TP* __restrict__ mean, const TP* __restrict__ var, long long n, int q, double b,
                                                 const RcBand bd, RcScal* sc) {
  const double u_lo = ord_val(sc->ulo_key);
  unsigned long long kv = 0ull;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x) {
    bool ps, ss, un;
    rc_safety(mean, var, n, g, q, b, bd, ps, ss, un);
    if (!ss) continue;
    double ll, lh, ul, uh;
    rc_interval((double)mean[g], (double)var[g], b, bd.dm[0], bd.dv[0], ll, lh, ul, uh);
    if (lh <= u_lo) {
      const unsigned long long k = ord_key(fmax(0.0, (double)var[g] - bd.dv[0]));
      kv = k > kv ? k : kv;
    }
  }
  kv = block_ext_u64<true>(kv);
  if (threadIdx.x == 0) atomicMax(&sc->vmax_key, kv);
}
// pass 3: the list of candidates the intervals cannot decide
template <typename TP>
__global__ __launch_bounds__(256) void k_rc_flag(const TP* __restrict__ mean, const TP* __restrict__ var, long long n, int q, double b,
                                                 const RcBand bd, RcScal* sc, long long* __restrict__ list, int all_possibly_safe) {
  __shared__ int wcount[4];
  __shared__ long long base;
  const bool have_hi = sc->uhi_key != ~0ull;
  const double u_lo = sc->ulo_key != ~0ull ? ord_val(sc->ulo_key) : -kInfD;
  const double u_hi = have_hi ? ord_val(sc->uhi_key) : kInfD;
  const double vmax_lo = sc->vmax_key ? ord_val(sc->vmax_key) : -1.0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long span = (long long)gridDim.x * blockDim.x;
  for (long long g0 = (long long)blockIdx.x * blockDim.x; g0 < n; g0 += span) {
    const long long g = g0 + threadIdx.x;
    bool flag = false;
    if (g < n) {
      bool ps, ss, un;
      rc_safety(mean, var, n, g, q, b, bd, ps, ss, un);
      flag = un || (all_possibly_safe && ps && q > 1);
      if (ps && all_possibly_safe != 2) {
        double ll, lh, ul, uh;
        rc_interval((double)mean[g], (double)var[g], b, bd.dm[0], bd.dv[0], ll, lh, ul, uh);
        const bool maybe_m = ll <= u_hi;
        flag = flag || ul <= u_hi;                                     // may attain u*
        flag = flag || (maybe_m && lh >= u_lo);                        // lcb_0 <= u* undecided
        flag = flag || (maybe_m && (double)var[g] + bd.dv[0] >= vmax_lo);   // may hold the largest variance over M
      }
    }
    const unsigned long long m = __ballot(flag);
    if (lane == 0) wcount[wave] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
      const int tot = wcount[0] + wcount[1] + wcount[2] + wcount[3];
      base = tot ? (long long)atomicAdd((unsigned long long*)&sc->count, (unsigned long long)tot) : 0;
    }
    __syncthreads();
    if (flag) {
      long long off = base;
      for (int w = 0; w < wave; ++w) off += wcount[w];
      off += __popcll(m & ((1ull << lane) - 1ull));
      list[off] = g;
    }
    __syncthreads();
  }
}

template <int D>
__global__ __launch_bounds__(256) void k_rc_gather(const CandSpec cs, const long long* __restrict__ list, long long nf, double* __restrict__ pts) {
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < nf; k += (long long)gridDim.x * blockDim.x) {
    double x[D];
    cand_coords<D>(cs, list[k], x);
    for (int a = 0; a < cs.d; ++a) pts[k * cs.d + a] = x[a];
  }
}
__global__ __launch_bounds__(256) void k_rc_widen(const float* __restrict__ m32, const float* __restrict__ v32, long long total,
                                                  double* __restrict__ m64, double* __restrict__ v64) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    m64[i] = (double)m32[i];
    v64[i] = (double)v32[i];
  }
}
__global__ __launch_bounds__(256) void k_rc_scatter(const long long* __restrict__ list, long long nf, int q, long long n,
                                                    const double* __restrict__ ms, const double* __restrict__ vs, double* __restrict__ m64,
                                                    double* __restrict__ v64, uint8_t* __restrict__ refined) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nf * q; i += (long long)gridDim.x * blockDim.x) {
    const long long k = i % nf;
    const int o = (int)(i / nf);
    const long long g = list[k];
    m64[(size_t)o * n + g] = ms[(size_t)o * nf + k];
    v64[(size_t)o * n + g] = vs[(size_t)o * nf + k];
    if (o == 0) refined[g] = 1;
  }
}

// Lipschitz keys in fp64: max over the candidates of |d MEAN_i / d x_a| for every output (the analytic gradient of
// models/SafeOpt.py:68-71 on the twin's double arrays; one thread per candidate)
template <int D>
__global__ __launch_bounds__(256) void k_rc_grad64(const ModelConst mc, const CandSpec cs, const double* __restrict__ As,
                                                   const double* __restrict__ sqA, const double* __restrict__ alpha,
                                                   const double* __restrict__ Xn, unsigned long long* __restrict__ Lmax) {
  double gm[kMaxQ];
#pragma unroll
  for (int o = 0; o < kMaxQ; ++o) gm[o] = 0.0;
  const int n = mc.n, npad = mc.npad;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < cs.n_local; g += (long long)gridDim.x * blockDim.x) {
    double x[D], xn[D];
    cand_coords<D>(cs, g, x);
#pragma unroll
    for (int a = 0; a < D; ++a) xn[a] = a < mc.d ? (x[a] - mc.X_mean[a]) / mc.X_std[a] : 0.0;
    for (int o = 0; o < mc.q; ++o) {
      double bq[D], sqb = 0.0;
#pragma unroll
      for (int a = 0; a < D; ++a) {
        bq[a] = a < mc.d ? xn[a] * mc.vinv[o][a] : 0.0;
        sqb += bq[a] * bq[a];
      }
      const double* Ao = As + (size_t)o * npad * D;
      const double* so = sqA + (size_t)o * npad;
      const double* al = alpha + (size_t)o * npad;
      double s0 = 0.0, sa[D];
#pragma unroll
      for (int a = 0; a < D; ++a) sa[a] = 0.0;
      for (int j = 0; j < n; ++j) {
        double dot = 0.0;
#pragma unroll
        for (int a = 0; a < D; ++a) dot += Ao[(size_t)j * D + a] * bq[a];
        const double w = al[j] * (mc.sf2[o] * exp(-0.5 * ((-2.0 * dot + so[j]) + sqb)));
        s0 += w;
#pragma unroll
        for (int a = 0; a < D; ++a) sa[a] += w * Xn[(size_t)j * D + a];
      }
      double gn = 0.0;
#pragma unroll
      for (int a = 0; a < D; ++a) {
        if (a < mc.d) {
          double ga = mc.Y_std[o] * (sa[a] - xn[a] * s0) * mc.inv_ell[o][a] * mc.X_rstd[a];
          ga = ga < 0 ? -ga : ga;
          gn = ga > gn ? ga : gn;
        }
      }
      gm[o] = gn > gm[o] ? gn : gm[o];
    }
  }
  for (int o = 0; o < mc.q; ++o) {
    const unsigned long long k = block_ext_u64<true>((unsigned long long)__double_as_longlong(gm[o]));   // (values >= 0: bit order)
    if (threadIdx.x == 0) atomicMax(&Lmax[o], k);
    __syncthreads();
  }
}

// guard of Expander's arg-max: gkeys[c] = max over G_c of the lower end of var_0, then every unrefined member of G_c whose
// upper end reaches it is deferred
__global__ __launch_bounds__(256) void k_rc_gmax(const uint8_t* __restrict__ G, const double* __restrict__ var0, const uint8_t* __restrict__ refined,
                                                 long long n, double dv0, unsigned long long* __restrict__ gkeys) {
  const int c = blockIdx.y;
  const uint8_t* Gc = G + (size_t)c * n;
  unsigned long long k = 0ull;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x)
    if (Gc[g]) {
      const unsigned long long kk = ord_key(refined[g] ? var0[g] : fmax(0.0, var0[g] - dv0));
      k = kk > k ? kk : k;
    }
  k = block_ext_u64<true>(k);
  if (threadIdx.x == 0 && k) atomicMax(&gkeys[c], k);
}
__global__ __launch_bounds__(256) void k_rc_gdefer(const uint8_t* __restrict__ G, const double* __restrict__ var0, const uint8_t* __restrict__ refined,
                                                   long long n, double dv0, const unsigned long long* __restrict__ gkeys,
                                                   long long* __restrict__ list, unsigned long long* __restrict__ count) {
  const int c = blockIdx.y;
  const uint8_t* Gc = G + (size_t)c * n;
  if (!gkeys[c]) return;
  const double vlo = ord_val(gkeys[c]);
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x)
    if (Gc[g] && !refined[g] && var0[g] + dv0 >= vlo) list[atomicAdd(count, 1ull)] = g;
}

// re-evaluate list[0..nf) exactly and put the values in place (`scatter`; without it an fp32 model's twin keeps them).  fp32 models: the fp64 twin's generic kernel, into the widened
// copy recheck.mean / recheck.var; guard band of an approximating fp64 posterior (`guard`): the exact evaluator of the same model
// (guard.hip: guard_exact_list), into the posterior buffers themselves.
static int rc_refine(sbo_ctx* c, const long long* list, long long nf, bool guard = false, bool scatter = true) {
  sbo_ctx* s = guard ? c : c->recheck.shadow;
  const long long n = c->cs.n_local;
  const int q = c->mc.q, d = c->cs.d;
  int rc;
  if (nf <= 0) return SBO_OK;
  DevBuf& pbuf = guard ? c->gb.pts : s->pts;
  if ((rc = ensure(pbuf, sizeof(double) * (size_t)nf * d))) return rc;
  const unsigned nbf = (unsigned)std::max<long long>(1, std::min<long long>((nf + 255) / 256, 4096));
  with_dpad(c->mc.dpad, [&](auto D) {
    hipLaunchKernelGGL(k_rc_gather<D()>, dim3(nbf), dim3(256), 0, c->stream, c->cs, list, nf, (double*)pbuf.p);
  });
  if (guard) {
    if ((rc = ensure(c->gb.vals, sizeof(double) * 2 * (size_t)nf * q))) return rc;
    double* em = (double*)c->gb.vals.p;
    double* ev = em + (size_t)nf * q;
    if ((rc = guard_exact_list(c, (const double*)pbuf.p, nf, em, ev))) return rc;
    // (the standing audit takes its sample of what the posterior kernel stored before the exact values replace it)
    if (c->audit.pending) SBO_HIP(hipStreamWaitEvent(c->stream, c->audit.ev[0], 0));
    post_values_patched(c);                 // (exact values replace the plan's at the listed candidates: internal.hpp, BilinearPlan::vals_ready)
    hipLaunchKernelGGL(k_rc_scatter, dim3(nbf), dim3(256), 0, c->stream, list, nf, q, n, (const double*)em, (const double*)ev,
                       (double*)c->mean.p, (double*)c->var.p, (uint8_t*)c->recheck.refined.p);
    SBO_HIP(hipGetLastError());
    return SBO_OK;
  }
  memset(&s->cs, 0, sizeof(s->cs));
  s->cs.kind = 0;
  s->cs.d = d;
  s->cs.pts_dtype = SBO_F64;
  s->cs.pts = s->pts.p;
  s->cs.n_local = nf;
  s->cs.first = 0;
  s->dist.grid_total = nf;
  s->has_cand = true;
  s->opt.posterior_path = 0;
  if ((rc = ensure(s->mean, sizeof(double) * (size_t)nf * q))) return rc;
  if ((rc = ensure(s->var, sizeof(double) * (size_t)nf * q))) return rc;
  PostOutcome none;
  if ((rc = launch_posterior(s, PostRequest{}, none))) return rc;
  if (!scatter) return SBO_OK;             // (rc_probe: the twin's values stay in its own buffers, [q][nf])
  hipLaunchKernelGGL(k_rc_scatter, dim3(nbf), dim3(256), 0, c->stream, list, nf, q, n, (const double*)s->mean.p, (const double*)s->var.p,
                     (double*)c->recheck.mean.p, (double*)c->recheck.var.p, (uint8_t*)c->recheck.refined.p);
  SBO_HIP(hipGetLastError());
  return SBO_OK;
}

// Lipschitz keys in fp64 from the double arrays of `s` (the twin of an fp32 model, or the fp64 model itself) over the
// candidates of `c`
static int rc_lipschitz64(sbo_ctx* c, const sbo_ctx* s) {
  SBO_HIP(hipMemsetAsync(c->Lmax, 0, sizeof(unsigned long long) * kMaxQ, c->stream));
  const unsigned nbg = (unsigned)grid_blocks(c, c->cs.n_local, 8);
  with_dpad(c->mc.dpad, [&](auto D) {
    hipLaunchKernelGGL(k_rc_grad64<D()>, dim3(nbg), dim3(256), 0, c->stream, s->mc, c->cs, (const double*)s->As.p, (const double*)s->sqA.p,
                       (const double*)s->alpha.p, (const double*)s->Xn.p, c->Lmax);
  });
  SBO_HIP(hipGetLastError());
  return SBO_OK;
}

// ---- the band of an fp32 posterior: measured, not assumed ------------------------------------------------------------------------
// How far the fp32 kernels are from the fp64 values depends on the model: 1e-6 (normalised) at cond(K) ~ 1e3, beyond 1e-3 at the noise
// floor of the reference's fit (log sigma_n = -5, cond(K) 1e6 .. 1e8; profiles/fp32_band_checks.md).  So, in the idiom of guard.hip, the
// first fp32 sweep of a (model, candidate set) has the fp64 twin evaluate kRcProbes candidates through the compacted-list path of
// rc_refine and the band becomes max(1e-4 normalised, 16 x the largest deviation) per output, for mean and variance separately; it is
// kept until the model, the candidates or the posterior kernel change (plans_invalidate).  Ranks > 1 merge intervals through the
// collectives, so they all take the largest band of any rank.  The standing audit (sbo_profile.guard_audit_*) samples later sweeps of
// the same pair at other candidates and counts an output whose deviation there exceeds the band in force.
constexpr int kRcProbes = 256;
constexpr double kRcBandFloor = 1e-4, kRcBandFactor = 16.0;

// keys[o] / keys[kMaxQ + o]: largest |fp32 - twin| of output o's mean / variance over the probes (one block; non-negative doubles
// order as their bit patterns; a NaN counts as infinite: everything is rechecked then)
__global__ __launch_bounds__(256) void k_rc_probe_dev(const float* __restrict__ m32, const float* __restrict__ v32, long long n,
                                                      const long long* __restrict__ list, int P, int q, const double* __restrict__ m64,
                                                      const double* __restrict__ v64, unsigned long long* __restrict__ keys) {
  const int k = threadIdx.x;
  for (int o = 0; o < q; ++o) {
    double dm = 0.0, dv = 0.0;
    if (k < P) {
      const long long g = list[k];
      dm = fabs((double)m32[(size_t)o * n + g] - m64[(size_t)o * P + k]);
      dv = fabs((double)v32[(size_t)o * n + g] - v64[(size_t)o * P + k]);
      if (!(dm == dm)) dm = kInfD;
      if (!(dv == dv)) dv = kInfD;
    }
    const unsigned long long km = block_ext_u64<true>((unsigned long long)__double_as_longlong(dm));
    const unsigned long long kv = block_ext_u64<true>((unsigned long long)__double_as_longlong(dv));
    if (threadIdx.x == 0) {
      keys[o] = km;
      keys[kMaxQ + o] = kv;
    }
    __syncthreads();
  }
}

// the resident fp32 posterior against the fp64 twin at min(n, kRcProbes) candidates: largest deviation per output (un-normalised), and
// how many candidates were compared.  `round` picks the probe set: a golden-ratio sequence over the index range (no stride a grid axis
// could alias with), round 0 with the first and the last candidate in it.
static int rc_probe(sbo_ctx* c, long long round, double* dev_m, double* dev_v, int* probes) {
  const long long n = c->cs.n_local;
  const int q = c->mc.q;
  const int P = (int)std::min<long long>(n, kRcProbes);
  int rc;
  for (int o = 0; o < kMaxQ; ++o) dev_m[o] = dev_v[o] = 0.0;
  *probes = P;
  if ((rc = ensure(c->recheck.probe, sizeof(unsigned long long) * 2 * kMaxQ + sizeof(long long) * kRcProbes))) return rc;
  if (P <= 0) return SBO_OK;
  unsigned long long* keys = (unsigned long long*)c->recheck.probe.p;
  long long* list = (long long*)(keys + 2 * kMaxQ);
  long long h[kRcProbes];
  for (int k = 0; k < P; ++k) {
    const double t = (double)(round * P + k + 1) * 0.6180339887498949;
    h[k] = std::min<long long>(n - 1, (long long)((t - std::floor(t)) * (double)n));
  }
  if (round == 0) {
    h[0] = 0;
    h[P - 1] = n - 1;
  }
  SBO_HIP(hipMemcpyAsync(list, h, sizeof(long long) * P, hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipStreamSynchronize(c->stream));                      // (`h` is on this frame)
  if ((rc = rc_refine(c, list, P, false, false))) return rc;
  hipLaunchKernelGGL(k_rc_probe_dev, dim3(1), dim3(256), 0, c->stream, (const float*)c->mean.p, (const float*)c->var.p, n, (const long long*)list, P, q,
                     (const double*)c->recheck.shadow->mean.p, (const double*)c->recheck.shadow->var.p, keys);
  SBO_HIP(hipGetLastError());
  double hk[2 * kMaxQ];
  SBO_HIP(hipMemcpyAsync(hk, keys, sizeof(hk), hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipStreamSynchronize(c->stream));
  for (int o = 0; o < q; ++o) {
    dev_m[o] = hk[o];
    dev_v[o] = hk[kMaxQ + o];
  }
  return SBO_OK;
}

// the bands of the intervals (and of SetView::rc_band): of an fp32 model the measured band above, else the plan's guard band read back
// from the device
static int rc_bands(sbo_ctx* c, bool guard, RcBand& bd) {
  memset(&bd, 0, sizeof(bd));
  const int q = c->mc.q;
  int rc;
  if (guard) {
    GuardBand hb;
    SBO_HIP(hipMemcpyAsync(&hb, c->gb.buf.p, sizeof(hb), hipMemcpyDeviceToHost, c->stream));
    SBO_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < q; ++i) {
      if (!(hb.dm[i] >= 0.0) || !(hb.dv[i] >= 0.0)) return fail(SBO_E_HIP, "internal: guard band is not finite");
      bd.dm[i] = hb.dm[i];
      bd.dv[i] = hb.dv[i];
    }
    return SBO_OK;
  }
  double dev_m[kMaxQ], dev_v[kMaxQ];
  int probes = 0;
  if (!c->recheck.band_valid) {
    if ((rc = rc_probe(c, 0, dev_m, dev_v, &probes))) return rc;
    double hk[2 * kMaxQ] = {};
    for (int i = 0; i < q; ++i) {
      const double ys = std::max(1.0, c->mc.Y_std[i]);
      hk[i] = std::max(kRcBandFloor * ys, kRcBandFactor * dev_m[i]);
      hk[kMaxQ + i] = std::max(kRcBandFloor * ys * ys, kRcBandFactor * dev_v[i]);
    }
    if (multi_rank(c)) {                  // (one band for all ranks: the largest)
      unsigned long long* keys = (unsigned long long*)c->recheck.probe.p;
      SBO_HIP(hipMemcpyAsync(keys, hk, sizeof(hk), hipMemcpyHostToDevice, c->stream));
      SBO_HIP(hipStreamSynchronize(c->stream));
      if ((rc = comm_allreduce_max_u64(c, keys, 2 * kMaxQ))) return rc;
      SBO_HIP(hipMemcpyAsync(hk, keys, sizeof(hk), hipMemcpyDeviceToHost, c->stream));
      SBO_HIP(hipStreamSynchronize(c->stream));
    }
    for (int i = 0; i < q; ++i) {
      c->recheck.band_dm[i] = hk[i];
      c->recheck.band_dv[i] = hk[kMaxQ + i];
    }
    c->recheck.band_valid = true;
    c->recheck.probe_round = 0;
  } else if (c->opt.guard_audit > 0 && c->audit.tick++ % std::max(1, c->opt.guard_audit_every) == 0) {
    // the standing audit: another probe set against the band in force
    if ((rc = rc_probe(c, ++c->recheck.probe_round, dev_m, dev_v, &probes))) return rc;
    for (int i = 0; i < q && probes > 0; ++i) {
      const double wm = dev_m[i] / (c->recheck.band_dm[i] * c->opt.audit_scale), wv = dev_v[i] / (c->recheck.band_dv[i] * c->opt.audit_scale);
      c->audit.samples += 2 * probes;
      c->audit.violations += (wm > 1.0 ? 1 : 0) + (wv > 1.0 ? 1 : 0);
      c->audit.worst = std::max(c->audit.worst, std::max(wm, wv));
    }
  }
  for (int i = 0; i < q; ++i) {
    bd.dm[i] = c->recheck.band_dm[i];
    bd.dv[i] = c->recheck.band_dv[i];
  }
  return SBO_OK;
}

// what a recheck re-evaluated: the guard's count and passes go into the result, an fp32 sweep's count and the band it ran with into
// sbo_profile (the set phase inside the recheck rewrites the profile: called behind it)
template <class R>
static void rc_report(sbo_ctx* c, bool guard, R* res, long long total, int passes, const RcBand& bd) {
  if (guard) { res->guard_rechecks = total; res->guard_passes = passes; return; }
  c->prof.fp64_rechecks = total;
  for (int i = 0; i < c->mc.q; ++i) {
    c->prof.fp32_band_dm[i] = bd.dm[i];
    c->prof.fp32_band_dv[i] = bd.dv[i];
  }
}

// The front of every recheck: posterior, bands, (fp32) the widened copy, the first refinement list re-evaluated, fp64 Lipschitz keys;
// leaves the head and the list of Recheck::list ready for further rounds.  What the SafeOpt and the GoOSE / trust-region rechecks do differently:
//   reuse      no K1 launch, the resident posterior serves; the callers' rules differ, each is stated where it is evaluated
//   list_cap   entries of Recheck::list behind its head: what the caller's later rounds can append at most
//   flag_mode  k_rc_flag's all_possibly_safe -- 0: the undecided and the contenders of u*, M, the minimiser; 1: every possibly-safe candidate
//              too; 2: the undecided and the possibly safe alone --, < 0: no flag pass.  The interval passes k_rc_ustar / k_rc_vmax (with
//              their collectives) run in front of modes 0 and 1, which decide u*, M and the minimiser from them; no other mode reads them
//   marks      ev_join[0] in front of the posterior and ev_join[1] behind it (the SafeOpt recheck's profile)
template <typename TP>
static int rc_front(sbo_ctx* c, const sbo_sweep_opts* o, bool reuse, size_t list_cap, int flag_mode, bool marks, RcBand& bd, long long* total) {
  constexpr bool kGuard = std::is_same<TP, double>::value;
  const long long n = c->cs.n_local, n1 = std::max<long long>(n, 1);
  const int q = c->mc.q;
  int rc;
  if (marks) SBO_HIP(hipEventRecord(c->ev_join[0], c->stream));
  if (!reuse && (rc = posterior_enqueue(c, PostRequest{}, nullptr))) return rc;
  if (marks) SBO_HIP(hipEventRecord(c->ev_join[1], c->stream));
  if ((rc = rc_bands(c, kGuard, bd))) return rc;
  if ((rc = ensure(c->recheck.list, sizeof(RcHead) + sizeof(long long) * list_cap))) return rc;
  if (!kGuard) {
    if ((rc = ensure(c->recheck.mean, sizeof(double) * (size_t)q * n1))) return rc;
    if ((rc = ensure(c->recheck.var, sizeof(double) * (size_t)q * n1))) return rc;
  }
  if ((rc = ensure(c->recheck.refined, (size_t)n1))) return rc;
  RcHead* head = (RcHead*)c->recheck.list.p;
  RcScal* sc = &head->sc;
  long long* list = (long long*)(head + 1);
  SBO_HIP(hipMemsetAsync(head, 0, sizeof(RcHead), c->stream));
  const RcScal init{~0ull, ~0ull, 0ull, 0};
  SBO_HIP(hipMemcpyAsync(sc, &init, sizeof(init), hipMemcpyHostToDevice, c->stream));
  SBO_HIP(hipMemsetAsync(c->recheck.refined.p, 0, (size_t)n1, c->stream));
  const TP *m32 = (const TP*)c->mean.p, *v32 = (const TP*)c->var.p;
  const unsigned nbk = (unsigned)reduce_blocks(c);
  if (flag_mode == 0 || flag_mode == 1) {
    hipLaunchKernelGGL(k_rc_ustar<TP>, dim3(nbk), dim3(256), 0, c->stream, m32, v32, n, q, o->b, bd, sc);
    // (ranks > 1: the interval of u* and the variance guard are global quantities -- three keys through the collectives)
    if ((rc = comm_allreduce_min_u64(c, &sc->ulo_key, 2))) return rc;
    hipLaunchKernelGGL(k_rc_vmax<TP>, dim3(nbk), dim3(256), 0, c->stream, m32, v32, n, q, o->b, bd, sc);
    if ((rc = comm_allreduce_max_u64(c, &sc->vmax_key, 1))) return rc;
  }
  if (flag_mode >= 0) hipLaunchKernelGGL(k_rc_flag<TP>, dim3(nbk), dim3(256), 0, c->stream, m32, v32, n, q, o->b, bd, sc, list, flag_mode);
  if (!kGuard)
    hipLaunchKernelGGL(k_rc_widen, dim3(nbk), dim3(256), 0, c->stream, (const float*)c->mean.p, (const float*)c->var.p, (long long)q * n,
                       (double*)c->recheck.mean.p, (double*)c->recheck.var.p);
  SBO_HIP(hipGetLastError());
  SBO_HIP(hipMemcpyAsync(&c->h_back->rc, head, offsetof(RcHead, gkeys), hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipStreamSynchronize(c->stream));
  *total = c->h_back->rc.sc.count;
  if ((rc = rc_refine(c, list, *total, kGuard))) return rc;
  // Lipschitz keys in fp64 (the fp32 posterior kernel left fp32-accurate ones, an approximating one its own band)
  if (q > 1 && (rc = rc_lipschitz64(c, kGuard ? c : c->recheck.shadow))) return rc;
  return SBO_OK;
}

// The counter of a later round (RcHead::deferred) read back: *mine.  Ranks > 1: every rank goes round the same number of times --
// the collectives of a set phase are inside it --, so "nothing left" is a global statement: *all is the largest count over the ranks.
static int rc_count_all(sbo_ctx* c, long long* mine, long long* all) {
  RcHead* head = (RcHead*)c->recheck.list.p;
  RcHead& back = c->h_back->rc;
  SBO_HIP(hipMemcpyAsync(&back, head, offsetof(RcHead, gkeys), hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipStreamSynchronize(c->stream));
  *mine = *all = (long long)back.deferred;
  if (!multi_rank(c)) return SBO_OK;
  SBO_HIP(hipMemcpyAsync(&head->all_ranks, &back.deferred, sizeof(back.deferred), hipMemcpyHostToDevice, c->stream));
  if (int rc = comm_allreduce_max_u64(c, &head->all_ranks, 1)) return rc;
  SBO_HIP(hipMemcpyAsync(&back.all_ranks_back, &head->all_ranks, sizeof(back.all_ranks_back), hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipStreamSynchronize(c->stream));
  *all = (long long)back.all_ranks_back;
  return SBO_OK;
}

// TP = float: an fp32 model (posterior in fp32, the fp64 twin re-evaluates); TP = double: the guard band of an approximating fp64
// posterior (the posterior is resident and valid; its listed entries are replaced in place by exact values)
template <typename TP>
static int sweep_safeopt_recheck(sbo_ctx* c, const sbo_sweep_opts* o, sbo_safeopt_result* res) {
  constexpr bool kGuard = std::is_same<TP, double>::value;
  const long long n = c->cs.n_local;
  const int q = c->mc.q;
  int rc;
  if (!kGuard && n == 0 && !multi_rank(c)) return sweep_safeopt_t<float>(c, o, SetView(c), res);
  // Reuse -- guard: the fast pass of this call left the posterior resident, unless it was a lean sweep, which leaves part of it
  // unwritten and so not valid: K1 once more, in full.  fp32: the caller vouches for the resident posterior, and it must hold every
  // Lipschitz key this sweep reports: one a lean launch left out (post_l0_missing: L_0) serves a lean sweep alone, which reports L_0 = 0.
  const bool reuse = (kGuard && c->posterior_valid) || (o->posterior_ready && c->posterior_valid && (o->lean || !c->post_l0_missing));
  // (one pass can list a candidate once per constraint in the verdict kernels and once more per constraint in k_rc_gdefer;
  // the first list -- k_rc_flag -- holds every candidate at most once)
  const size_t list_cap = (size_t)std::max<long long>(n, 1) * (size_t)(2 * std::max(1, q - 1) + 1);
  RcBand bd;
  long long total = 0;
  // (flag mode 1: candidate sets without a grid to transform decide their expanders by exhaustive pair evaluation on the ucb of every
  // safe candidate, so there all possibly-safe candidates are re-evaluated)
  if ((rc = rc_front<TP>(c, o, reuse, list_cap, whole_planes(c) ? 0 : 1, true, bd, &total))) return rc;
  SBO_HIP(hipEventRecord(c->ev_join[2], c->stream));
  RcHead* head = (RcHead*)c->recheck.list.p;
  long long* list = (long long*)(head + 1);
  const unsigned nbk = (unsigned)reduce_blocks(c);
  // the set phase in fp64 arithmetic on the refined posterior (fp32: the widened copy -- the fp32 arrays stay what
  // sbo_posterior_get returns; guard: the band stays in force for unrefined entries, L is exact now); repeated while verdicts are deferred
  SetView view(kGuard ? c->mean : c->recheck.mean, kGuard ? c->var : c->recheck.var, kGuard ? SetBand::values : SetBand::plan);
  if (q > 1) {
    view.refined = (const uint8_t*)c->recheck.refined.p;
    view.rc_band = &bd;
    view.rc_list = list;
    view.rc_count = &head->deferred;
  }
  int passes = 0;
  for (;; ++passes) {
    SBO_HIP(hipMemsetAsync(&head->deferred, 0, offsetof(RcHead, pad) - offsetof(RcHead, deferred), c->stream));   // the deferral counter .. the G keys
    rc = sweep_safeopt_t<double>(c, o, view, res);
    if (rc != SBO_OK || q == 1) break;
    // Expander's arg-max over every G_c must not hinge on an unrefined variance
    const uint8_t* G = (const uint8_t*)c->maskG.p;
    const double* var0 = (const double*)view.var->p;
    hipLaunchKernelGGL(k_rc_gmax, dim3(nbk, (unsigned)(q - 1)), dim3(256), 0, c->stream, G, var0, (const uint8_t*)c->recheck.refined.p, n, bd.dv[0],
                       head->gkeys);
    if ((rc = comm_allreduce_max_u64(c, head->gkeys, q - 1))) return rc;        // (the expanders' arg-max is over all ranks)
    hipLaunchKernelGGL(k_rc_gdefer, dim3(nbk, (unsigned)(q - 1)), dim3(256), 0, c->stream, G, var0, (const uint8_t*)c->recheck.refined.p, n,
                       bd.dv[0], (const unsigned long long*)head->gkeys, list, &head->deferred);
    SBO_HIP(hipGetLastError());
    long long nd, nd_all;
    if ((rc = rc_count_all(c, &nd, &nd_all))) return rc;
    if (nd_all == 0) break;
    if ((size_t)nd > list_cap) return fail(SBO_E_HIP, "internal: refinement list overflow");
    // (every candidate is refined at most once, so the passes end; six without an end would be a defect, not a slow case)
    if (passes >= 6) return fail(SBO_E_UNSUPPORTED, "recheck: verdicts still deferred after 7 passes of the set phase");
    if ((rc = rc_refine(c, list, nd, kGuard))) return rc;
    total += nd;
  }
  float t01 = 0, t12 = 0, t04 = 0;
  (void)hipEventElapsedTime(&t01, c->ev_join[0], c->ev_join[1]);
  (void)hipEventElapsedTime(&t12, c->ev_join[1], c->ev_join[2]);
  (void)hipEventElapsedTime(&t04, c->ev_join[0], c->ev[4]);
  rc_report(c, kGuard, res, total, passes + 1, bd);
  if (kGuard) c->prof.guard_ms = t04;
  if (!kGuard) {
    c->prof.posterior_ms = t01;
    c->prof.recheck_ms = t12;
    c->prof.total_ms = t04;
    c->prof.posterior_launches = reuse ? 0 : 1;
    const double nn = c->mc.n, dd = c->mc.d;
    c->prof.posterior_flops = reuse ? 0.0 : q * (nn * nn + (2 * dd + 10) * nn) * (double)n;
  }
  return rc;
}

// ---- GoOSE and trust-region sweeps of fp32 models (r03) -------------------------------------------------------------------------
// Coarser than the SafeOpt scheme above, and sufficient: with constraints, EVERY possibly-safe candidate is re-evaluated in
// fp64 (the sources of the optimistic sets are the expanders, whose radii ucb_c / L must be exact, and arg-min lcb_0 over S_t
// wants every safe candidate's bound) together with the candidates whose S / U membership the fp32 bounds cannot decide; the
// set phase then runs in fp64 arithmetic on exact values wherever a value enters a decision -- except the target, arg-min
// lcb_0 over the optimistic sets O_c (unsafe candidates, not re-evaluated): its contenders are found from the intervals
// afterwards, re-evaluated, and the set phase runs once more if there were any.  Without constraints (q = 1) only the
// contenders of the one arg-min (over all candidates, or over the trust region's ball) are re-evaluated.
// min over the (unrefined: widened) members of `mask` of the upper end of lcb_0 -> key;  refined entries count exactly
__global__ __launch_bounds__(256) void k_rc_lmin(const double* __restrict__ m0, const double* __restrict__ v0, const uint8_t* __restrict__ refined,
                                                 const uint8_t* __restrict__ mask /* nullptr: all */, int nmask, long long n, double b, double dm,
                                                 double dv, unsigned long long* key) {
  unsigned long long k = ~0ull;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x) {
    bool in = mask == nullptr;
    for (int t = 0; t < nmask && !in; ++t) in = mask[(size_t)t * n + g] != 0;
    if (!in) continue;
    const double md = m0[g], vd = v0[g];
    const double hi = refined[g] ? md - b * sqrt(vd) : (md + dm) - b * sqrt(fmax(0.0, vd - dv));
    const unsigned long long kk = ord_key(hi);
    k = kk < k ? kk : k;
  }
  k = block_ext_u64<false>(k);
  if (threadIdx.x == 0) atomicMin(key, k);
}
// ... and the unrefined members whose lower end reaches it: they may hold the minimum
__global__ __launch_bounds__(256) void k_rc_lflag(const double* __restrict__ m0, const double* __restrict__ v0, const uint8_t* __restrict__ refined,
                                                  const uint8_t* __restrict__ mask, int nmask, long long n, double b, double dm, double dv,
                                                  const unsigned long long* key, long long* __restrict__ list, unsigned long long* count) {
  if (*key == ~0ull) return;
  const double best_hi = ord_val(*key);
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x) {
    if (refined[g]) continue;
    bool in = mask == nullptr;
    for (int t = 0; t < nmask && !in; ++t) in = mask[(size_t)t * n + g] != 0;
    if (!in) continue;
    const double lo = (m0[g] - dm) - b * sqrt(v0[g] + dv);
    if (lo <= best_hi) list[atomicAdd(count, 1ull)] = g;
  }
}
// trust region without constraints: the ball as a byte mask (geometry: exact)
template <int D>
__global__ void k_rc_ball(const CandSpec cs, long long n, const double* __restrict__ x0, double r, uint8_t* __restrict__ out) {
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x) {
    double x[D];
    cand_coords<D>(cs, g, x);
    double ss = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a)
      if (a < cs.d) { const double df = x[a] - x0[a]; ss = (a == 0) ? df * df : ss + df * df; }
    out[g] = sqrt(ss) <= r;
  }
}

// what the GoOSE / trust-region rechecks hand their set phase: the widened copy of an fp32 posterior, or (guard) the fp64 posterior
// itself, refined in place; every value that enters a decision is exact by then: no band
static SetView rc_exact_view(const sbo_ctx* c, bool guard) {
  return SetView(guard ? c->mean : c->recheck.mean, guard ? c->var : c->recheck.var, SetBand::none);
}

// The front as the GoOSE / trust-region rechecks run it.  q > 1: every possibly-safe or undecided candidate goes on the first list, no
// intervals (the contenders of the arg-mins come afterwards, rc_argmin_contenders: once more at most n entries); q = 1: nothing to flag.
// Reuse -- guard: the fast pass of this call left the posterior resident, and these sweeps have no lean form that could have left part of
// it unwritten.  fp32: the caller vouches for it; post_l0_missing does not matter: no decision of these sweeps reads the objective's key.
template <typename TP>
static int rc_front_all(sbo_ctx* c, const sbo_sweep_opts* o, RcBand& bd, long long* total) {
  const bool reuse = std::is_same<TP, double>::value || (o->posterior_ready && c->posterior_valid);
  return rc_front<TP>(c, o, reuse, (size_t)std::max<long long>(c->cs.n_local, 1) * 2, c->mc.q > 1 ? 2 : -1, false, bd, total);
}

// contenders of arg-min lcb_0 over `mask` (nmask stacked byte masks, nullptr: every candidate): re-evaluated exactly; returns
// how many there were (0: the arg-min already rests on exact values)
static int rc_argmin_contenders(sbo_ctx* c, const sbo_sweep_opts* o, const RcBand& bd, const uint8_t* mask, int nmask, long long* found,
                                bool guard) {
  const long long n = c->cs.n_local;
  int rc;
  RcHead* head = (RcHead*)c->recheck.list.p;
  unsigned long long* key = &head->lmin_key;
  long long* list = (long long*)(head + 1);
  const unsigned long long init[2] = {0ull, ~0ull};                    // deferred, lmin_key
  SBO_HIP(hipMemcpyAsync(&head->deferred, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
  const unsigned nbk = (unsigned)reduce_blocks(c);
  const double* m0 = guard ? (const double*)c->mean.p : (const double*)c->recheck.mean.p;
  const double* v0 = guard ? (const double*)c->var.p : (const double*)c->recheck.var.p;
  hipLaunchKernelGGL(k_rc_lmin, dim3(nbk), dim3(256), 0, c->stream, m0, v0, (const uint8_t*)c->recheck.refined.p, mask, nmask, n, o->b, bd.dm[0], bd.dv[0], key);
  if ((rc = comm_allreduce_min_u64(c, key, 1))) return rc;             // (ranks > 1: the arg-min is over all ranks)
  hipLaunchKernelGGL(k_rc_lflag, dim3(nbk), dim3(256), 0, c->stream, m0, v0, (const uint8_t*)c->recheck.refined.p, mask, nmask, n, o->b, bd.dm[0], bd.dv[0],
                     (const unsigned long long*)key, list, &head->deferred);
  SBO_HIP(hipGetLastError());
  long long mine;
  if ((rc = rc_count_all(c, &mine, found))) return rc;
  if ((rc = rc_refine(c, list, mine, guard))) return rc;
  return SBO_OK;
}

template <typename TP>
static int sweep_goose_recheck(sbo_ctx* c, const sbo_sweep_opts* o, sbo_goose_result* res) {
  constexpr bool kGuard = std::is_same<TP, double>::value;
  const long long n = c->cs.n_local;
  const int q = c->mc.q;
  if (n == 0) return kGuard ? sweep_goose_t<double>(c, o, SetView(c), res) : sweep_goose_t<float>(c, o, SetView(c), res);
  int rc;
  SBO_HIP(hipEventRecord(c->ev_join[0], c->stream));
  const bool reuse = kGuard || (o->posterior_ready && c->posterior_valid);
  RcBand bd;
  long long total = 0, more = 0;
  if ((rc = rc_front_all<TP>(c, o, bd, &total))) return rc;
  SBO_HIP(hipEventRecord(c->ev_join[1], c->stream));
  const SetView view = rc_exact_view(c, kGuard);
  sbo_sweep_opts o2 = *o;
  o2.want_masks = 1;
  int passes = 0;
  if (q == 1) {
    // arg-min lcb_0 over every candidate: its contenders, then one fp64 set phase
    if ((rc = rc_argmin_contenders(c, o, bd, nullptr, 0, &more, kGuard))) return rc;
    total += more;
    rc = sweep_goose_t<double>(c, &o2, view, res);
    passes = 1;
  } else {
    for (int pass = 0; pass < 3; ++pass) {
      rc = sweep_goose_t<double>(c, &o2, view, res);
      ++passes;
      if (rc != SBO_OK) break;
      // the target: arg-min lcb_0 over the union of the optimistic sets (members are unsafe candidates, so far unrefined values)
      if ((rc = rc_argmin_contenders(c, o, bd, (const uint8_t*)c->maskO.p, q - 1, &more, kGuard))) return rc;
      total += more;
      if (more == 0) break;
    }
  }
  float t01 = 0;
  (void)hipEventElapsedTime(&t01, c->ev_join[0], c->ev_join[1]);
  rc_report(c, kGuard, res, total, passes, bd);
  (kGuard ? c->prof.guard_ms : c->prof.recheck_ms) = t01;
  if (!kGuard) c->prof.posterior_launches = reuse ? 0 : 1;
  return rc;
}

template <typename TP>
static int sweep_tr_recheck(sbo_ctx* c, const sbo_sweep_opts* o, const double* x0, double r, sbo_tr_result* res) {
  constexpr bool kGuard = std::is_same<TP, double>::value;
  const long long n = c->cs.n_local;
  const int q = c->mc.q;
  if (n == 0) return kGuard ? sweep_tr_t<double>(c, o, SetView(c), x0, r, res) : sweep_tr_t<float>(c, o, SetView(c), x0, r, res);
  int rc;
  RcBand bd;
  long long total = 0, more = 0;
  if ((rc = rc_front_all<TP>(c, o, bd, &total))) return rc;
  if (q == 1) {
    // arg-min lcb_0 over the ball: the ball as a mask (exact geometry), then the contenders inside it
    if ((rc = ensure(c->maskM, (size_t)n))) return rc;
    double* dev_x0 = scal_block(c)->point;
    SBO_HIP(hipMemcpyAsync(dev_x0, x0, sizeof(double) * c->cs.d, hipMemcpyHostToDevice, c->stream));
    with_dpad(c->mc.dpad, [&](auto D) {
      hipLaunchKernelGGL((k_rc_ball<D()>), dim3((unsigned)reduce_blocks(c)), dim3(256), 0, c->stream, c->cs, n, (const double*)dev_x0, r, (uint8_t*)c->maskM.p);
    });
    if ((rc = rc_argmin_contenders(c, o, bd, (const uint8_t*)c->maskM.p, 1, &more, kGuard))) return rc;
    total += more;
  }
  rc = sweep_tr_t<double>(c, o, rc_exact_view(c, kGuard), x0, r, res);
  rc_report(c, kGuard, res, total, 1, bd);
  return rc;
}
