// bilinear_interp.inc.hpp: K1i, the first sweep of a model by interpolation from Chebyshev nodes -- its kernels and interp_setup.
// Part of the bilinear.hip translation unit (included inside namespace sbo; not a standalone header).

// ---- K1i: the first sweep of a model by interpolation from Chebyshev nodes (r04) -----------------------------------------------
// The reference refits its models after every sample (models/GP_Safe.py:283-304) and sweeps each of them ONCE
// (test/test_SafeOpt.py:144-179), so what an iteration pays for K1b is its plan: axis bases by pivoted Gram-Schmidt (0.16 ms the
// host has to wait for -- their ranks size everything after them), the core's contraction over rank^2 columns, guard probes:
// ~0.45 ms of a 1.07 ms iteration on config H.  K1b's own evaluation stage does not care where its Chebyshev coefficients come
// from.  So, for the first sweep of a model with a caller's invK:
//   1. the posterior's two scalar fields per output -- quad = k*^T invK k* and s1 = k*^T alpha -- EXACTLY (the reference formula,
//      models/GP_Safe.py:341-343, with the matrix as given) at the Dn x Dn tensor grid of Chebyshev nodes of the first kind on the
//      grid's box: K*^T as B fragments from two n x Dn tables of axis factors (the kernel is separable), C = invK K*^T on the matrix
//      cores (k_bgemm on the packed images of invK), then column dots quad_c = Z_c . C_c, s1_c = Z_c . alpha;
//   2. a 2-D discrete cosine transform of each field -> its Chebyshev coefficients, and those of the two gradient sums of the mean
//      by the derivative recurrence (d_{m-1} = d_{m+1} + 2 m c_m);
//   3. the coefficients through k_cheb_trunc / k_cheb_t4f / k_bstage1 / k_bpost as K1b's core goes: four coefficient sets per output.
// Nothing of this needs a number from the device on the host: the plan is enqueued by sbo_model_set behind the upload and the
// first sweep follows in stream order; the bases and K1b's own plan are built when the same model is swept a second time.
// Accuracy: Dn from the length scales as K1t chooses it (32 / 48 / 64); measured on the BASELINE models 1e-13 (mean) and 1e-12
// (variance: the rounding of the reference formula itself) -- and measured again for every plan at the guard band's probe points
// (values and gradient), so the sweep's decisions stay those of the exact kernel whatever the interpolation error is.
constexpr int kIMaxDn = 64;
constexpr double kGbAliasFactor = 4.0;   // aliasing estimate of an interpolant's band, in units of the last four degrees' coefficient sum
constexpr double kGbInf = 1.0e300;          // a probe that is not finite: everything is "inside the band" (guard.hip)
struct InterpDims {
  int Dn, q, n, npad, dpad;
  double mid[2], half[2];                  // node interval of each axis, normalised coordinates
};
// Everything of a plan that changes with the MODEL (hyper-parameters, normalisation, the box in normalised coordinates) reaches the
// plan's kernels through this block in device memory, read by pointer -- launch arguments then depend on the grid and on n only
// (interp_setup stages the block through pinned memory and copies it ahead of the plan's launches).
struct InterpParams {
  ModelConst mc;
  InterpDims id;
  BlDims dm;
  double dxi0, dxi1;                       // half a sampling cell of the gradient gate in xi units
};
// E[(2 o + axis)][p][j] = (axis == 0 ? sf2 : 1) exp(-1/2 (As_j,axis - xn_p vinv)^2)   (k_bl_zf multiplies the two axes)
__global__ __launch_bounds__(256) void k_i_etab(const InterpParams* __restrict__ P, const double* __restrict__ As, double* __restrict__ E) {
  const ModelConst& mc = P->mc;
  const InterpDims& id = P->id;
  const int job = blockIdx.y, o = job >> 1, axis = job & 1;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < id.Dn * id.n; e += gridDim.x * blockDim.x) {
    const int p = e / id.n, j = e % id.n;
    const double xn = id.mid[axis] + id.half[axis] * cospi(((double)p + 0.5) / (double)id.Dn);
    const double dlt = As[((size_t)o * id.npad + j) * id.dpad + axis] - xn * mc.vinv[o][axis];
    E[((size_t)job * kBlMaxR + p) * id.n + j] = (axis == 0 ? mc.sf2[o] : 1.0) * exp(-0.5 * dlt * dlt);
  }
}
// node values from the fragments of Z = K*^T and C = invK Z ([ncsR][KBn * 4][64], k = observation): V[o][0][c] = sum_j Z_jc C_jc,
// V[o][1][c] = sum_j Z_jc alpha_j.  A wave per strip of 16 columns.
__global__ __launch_bounds__(64) void k_i_nodevals(int KBn, int n, const double* __restrict__ Zfall, const double* __restrict__ Cfall, size_t nZf,
                                                   const double* __restrict__ alpha, int ald, int ncols, double* __restrict__ V) {
  const int o = blockIdx.y, cs = blockIdx.x, l = threadIdx.x;
  const double* Zf = Zfall + (size_t)o * nZf + (size_t)cs * KBn * 256;
  const double* Cf = Cfall + (size_t)o * nZf + (size_t)cs * KBn * 256;
  double aq[4] = {0.0, 0.0, 0.0, 0.0}, am[4] = {0.0, 0.0, 0.0, 0.0};
  for (int ks = 0; ks < KBn * 4; ks += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = ks + u, j = (k >> 2) * 16 + MM<double>::jslot(k & 3, l >> 4);
      const double z = Zf[(size_t)k * 64 + l];
      aq[u] = fma(z, Cf[(size_t)k * 64 + l], aq[u]);
      am[u] = fma(z, j < n ? alpha[(size_t)o * ald + j] : 0.0, am[u]);
    }
  }
  double sq = (aq[0] + aq[1]) + (aq[2] + aq[3]), sm = (am[0] + am[1]) + (am[2] + am[3]);
  sq += __shfl_xor(sq, 16); sm += __shfl_xor(sm, 16);
  sq += __shfl_xor(sq, 32); sm += __shfl_xor(sm, 32);
  const int c = cs * 16 + l;
  if (l < 16 && c < ncols) {
    V[((size_t)o * 2 + 0) * ncols + c] = sq;
    V[((size_t)o * 2 + 1) * ncols + c] = sm;
  }
}
// Chebyshev coefficients of the node fields, ChatT[4 o + f][b][a] (b: degree along axis 1, a: along axis 0; the layout k_cheb_trunc /
// k_cheb_t4f read): f = 0 quad, 1 s1, 2 / 3 the gradient sums g_a = (d s1 / d xn_a) / inv_ell_a of the two axes (k_bpost scales by
// Y_std inv_ell X_rstd).  One workgroup per output; node c = p Dn + s (p: axis 0).  T[m][k] = w_m cos(m pi (k + 1/2) / Dn) / Dn.
__global__ __launch_bounds__(1024) void k_i_dct(const InterpParams* __restrict__ P_, const double* __restrict__ V, double* __restrict__ ChatT_all) {
  const ModelConst& mc = P_->mc;
  const InterpDims& id = P_->id;
  extern __shared__ double sh[];                 // T [Dn][Dn + 1] | field [Dn][Dn + 1] | tmp [Dn][Dn + 1]  (rows padded: column walks)
  const int Dn = id.Dn, o = blockIdx.x >> 1, f = blockIdx.x & 1, tid = threadIdx.x, N2 = Dn * Dn, P = Dn + 1;
  double *T = sh, *F = sh + Dn * P, *W = sh + 2 * Dn * P;
  for (int e = tid; e < N2; e += blockDim.x) {
    const int m = e / Dn, k = e % Dn;
    T[m * P + k] = (m == 0 ? 1.0 : 2.0) / (double)Dn * cospi((double)m * ((double)k + 0.5) / (double)Dn);
    F[m * P + k] = V[((size_t)o * 2 + f) * N2 + e];                                         // F[p][s]
  }
  __syncthreads();
  for (int e = tid; e < N2; e += blockDim.x) {                                                // W[a][s] = sum_p T[a][p] F[p][s]
    const int a = e / Dn, s_ = e % Dn;
    double a0 = 0.0, a1 = 0.0;
    for (int p = 0; p + 1 < Dn; p += 2) {
      a0 = fma(T[a * P + p], F[p * P + s_], a0);
      a1 = fma(T[a * P + p + 1], F[(p + 1) * P + s_], a1);
    }
    W[a * P + s_] = a0 + a1;
  }
  __syncthreads();
  double* out = ChatT_all + (size_t)(4 * o + f) * N2;
  for (int e = tid; e < N2; e += blockDim.x) {                                                // C[a][b] = sum_s W[a][s] T[b][s]
    const int b = e / Dn, a = e % Dn;
    double a0 = 0.0, a1 = 0.0;
    for (int s_ = 0; s_ + 1 < Dn; s_ += 2) {
      a0 = fma(W[a * P + s_], T[b * P + s_], a0);
      a1 = fma(W[a * P + s_ + 1], T[b * P + s_ + 1], a1);
    }
    out[e] = a0 + a1;                                                                         // ChatT[b][a]
    F[b * P + a] = a0 + a1;
  }
  if (f == 0) return;                            // (uniform: the workgroup of the mean sum goes on to its derivatives)
  __syncthreads();
  // derivative series of s1: along axis 0 (index a) for g_0, along axis 1 (index b) for g_1; d xi / d xn = 1 / half
  double* g0 = ChatT_all + (size_t)(4 * o + 2) * N2;
  double* g1 = ChatT_all + (size_t)(4 * o + 3) * N2;
  const double sc0 = 1.0 / (id.half[0] * mc.inv_ell[o][0]), sc1 = 1.0 / (id.half[1] * mc.inv_ell[o][1]);
  for (int r = tid; r < 2 * Dn; r += blockDim.x) {
    const int line = r % Dn;
    const bool along0 = r < Dn;
    // coefficients c_m of this line: along axis 0 the line is a row b of F (stride 1), along axis 1 a column a (stride P)
    const int fb = along0 ? line * P : line, fs = along0 ? 1 : P;
    const int ob = along0 ? line * Dn : line, os = along0 ? 1 : Dn;
    double* dst = along0 ? g0 : g1;
    const double sc = along0 ? sc0 : sc1;
    double d2 = 0.0, d1 = 0.0;                  // d_{m+1}, d_m while walking m = Dn - 1 .. 1
    dst[ob + (Dn - 1) * os] = 0.0;
    for (int m = Dn - 1; m >= 1; --m) {
      const double dm1 = d2 + 2.0 * (double)m * F[fb + m * fs];            // d_{m-1}
      dst[ob + (m - 1) * os] = (m == 1 ? 0.5 * dm1 : dm1) * sc;
      d2 = d1;
      d1 = dm1;
    }
  }
}
// ---- K1i: where the gradient phases have to run (as k_bl_gradcoarse does it for K1b) -------------------------------------------
// The coarse kernel of K1b takes a rank-r0 bilinear form sum_p Vb[p][line] S0[p][x0]; a Chebyshev series is one with
// S0[a][x0] = T_a(xi0(x0)) and Vb[comp][a][line] = sum_b ChatT_comp[b][a] T_b(xi1(line)).
// K1i's tables of the grid positions in ONE launch (the plan is bound by the host's enqueue rate on the smaller grids: every launch
// less is ~7 us): normalised positions xn0 / xn1 (k_bl_axes), Chebyshev polynomials as B fragments of axis 0 / A images of axis 1
// (k_cheb_tab<1> / <0>) and the plain table of axis 0 for the gradient gate.  A thread per position.
__global__ __launch_bounds__(256) void k_i_tabs(const InterpParams* __restrict__ P_, const CandSpec cs, long long line0, double* __restrict__ xn0,
                                                double* __restrict__ xn1, double* __restrict__ P0f, double* __restrict__ P1A,
                                                double* __restrict__ S0all) {
  const ModelConst& mc = P_->mc;
  const BlDims& dm = P_->dm;
  const int KB = dm.KB0, Dn = dm.D0m;
  const long long n0 = (long long)dm.ncs0 * 16, n1 = (long long)dm.nrb * 16;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n0 + n1; t += (long long)gridDim.x * blockDim.x) {
    const int axis = t < n0 ? 0 : 1;
    const long long x = axis == 0 ? t : t - n0, count = axis == 0 ? dm.cnt0 : dm.nlines;
    double xi = 0.0;
    if (x < count) {
      const long long i = axis == 0 ? x : line0 + x, tot = cs.count[axis];
      const double xr = (i == tot - 1 && tot > 1) ? cs.hi[axis] : __dadd_rn(cs.lo[axis], __dmul_rn((double)i, cs.step[axis]));
      const double xn = (xr - mc.X_mean[axis]) / mc.X_std[axis];
      if (axis == 0) xn0[x] = xn; else xn1[x] = xn;
      xi = (2.0 * xn - (dm.a[axis] + dm.b[axis])) / (dm.b[axis] - dm.a[axis]);
      xi = xi < 1.0 ? xi : 1.0;
      xi = xi > -1.0 ? xi : -1.0;
    }
    double t0 = 1.0, t1 = xi;
    for (int k = 0; k < KB * 16; ++k) {
      double v = k == 0 ? t0 : t1;
      if (k >= 2) { v = 2.0 * xi * t1 - t0; t0 = t1; t1 = v; }
      if (x >= count) v = 0.0;
      const int kb = k >> 4, j = k & 15, kk = j >> 2, slot = j & 3;
      if (axis == 0) {
        P0f[(((size_t)(x >> 4) * (KB * 4) + (size_t)(kb * 4 + kk)) << 6) + (size_t)(slot * 16 + (x & 15))] = v;
        if (x < count && k < Dn)
          for (int o = 0; o < dm.q / 4; ++o) S0all[((size_t)o * Dn + k) * dm.cnt0 + x] = v;
      } else {
        P1A[(((size_t)(x >> 4) * KB + kb) << 8) + (size_t)MM<double>::pack_pos((int)(x & 15), slot, kk)] = v;
      }
    }
  }
}
// Vb[o][comp + 1][a][line] for the two gradient sums (comp 0: zero -- the slot K1b's form multiplies by xn); blockIdx.y = o.
// A thread per (line, eight degrees a -- blockIdx.z): its T_b(xi1) in registers, the coefficients through LDS.
template <int DM>
__global__ __launch_bounds__(256) void k_i_rtab(const InterpParams* __restrict__ P_, const double* __restrict__ ChatT_all, const int* __restrict__ eff,
                                                const double* __restrict__ xn1, double* __restrict__ Vball) {
  const BlDims& dm = P_->dm;
  __shared__ double Cs[DM * DM];
  const int o = blockIdx.y, Dn = dm.D0m;
  const long long line = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  double tb[DM];
  {
    double xi = 0.0;
    if (line < dm.nlines) {
      xi = (2.0 * xn1[line] - (dm.a[1] + dm.b[1])) / (dm.b[1] - dm.a[1]);
      xi = xi < 1.0 ? xi : 1.0;
      xi = xi > -1.0 ? xi : -1.0;
    }
    tb[0] = 1.0;
    if (DM > 1) tb[1] = xi;
#pragma unroll
    for (int b = 2; b < DM; ++b) tb[b] = 2.0 * xi * tb[b - 1] - tb[b - 2];
  }
  double* Vb = Vball + (size_t)o * 3 * Dn * dm.nlines;
  for (int comp = 0; comp < 2; ++comp) {
    const double* Ch = ChatT_all + (size_t)(4 * o + 2 + comp) * Dn * Dn;
    const int B = eff[4 * (4 * o + 2 + comp) + 2] * 16;                    // degrees of axis 1 the kernels run
    __syncthreads();
    for (int e = threadIdx.x; e < Dn * Dn; e += blockDim.x) Cs[e] = Ch[e];
    __syncthreads();
    if (line < dm.nlines) {
      for (int a = blockIdx.z * 8; a < (int)blockIdx.z * 8 + 8 && a < Dn; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < DM; ++b)
          if (b < B) s = fma(Cs[b * Dn + a], tb[b], s);
        Vb[((size_t)(comp + 1) * Dn + a) * dm.nlines + line] = s;
        if (comp == 0) Vb[(size_t)a * dm.nlines + line] = 0.0;
      }
    }
  }
}
// bound on what a gradient sum moves by over half a sampling cell, from its coefficients: sum |C| a^2 dxi0 + sum |C| b^2 dxi1
__global__ __launch_bounds__(256) void k_i_gradslack(const InterpParams* __restrict__ P_, const double* __restrict__ ChatT_all,
                                                     double* __restrict__ slack /* [q][2] */) {
  const BlDims& dm = P_->dm;
  const double dxi0 = P_->dxi0, dxi1 = P_->dxi1;
  __shared__ double red[4][2];
  const int oc = blockIdx.x, o = oc >> 1, comp = oc & 1, Dn = dm.D0m, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* Ch = ChatT_all + (size_t)(4 * o + 2 + comp) * Dn * Dn;
  double sa = 0.0, sb = 0.0;
  for (int e = tid; e < Dn * Dn; e += blockDim.x) {
    const double v = fabs(Ch[e]), a = (double)(e % Dn), b = (double)(e / Dn);
    sa = fma(v, a * a, sa);
    sb = fma(v, b * b, sb);
  }
  sa = wave_sum(sa);
  sb = wave_sum(sb);
  if (lane == 0) { red[wave][0] = sa; red[wave][1] = sb; }
  __syncthreads();
  if (tid == 0) {
    sa = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    sb = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    slack[oc] = (sa * dxi0 + sb * dxi1) * (1.0 + 1e-9);
  }
}
// the plan's own values at the guard band's probe points: raw[f][p] = sum over the degrees the kernels run of ChatT T_a(xi0) T_b(xi1),
// a wave per (probe, coefficient set)
__global__ __launch_bounds__(256) void k_gb_probe_series(const CandSpec cs, const InterpParams* __restrict__ P_, const double* __restrict__ ChatT_all,
                                                         const int* __restrict__ eff, const double* __restrict__ xn0, const double* __restrict__ xn1,
                                                         double* __restrict__ raw) {
  const BlDims& dm = P_->dm;
  const int f = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D0 = dm.D0m;
  const int p = blockIdx.x * 4 + wave;
  if (p >= kGbProbes) return;
  const int A = eff[4 * f] * 4, B = eff[4 * f + 2] * 16;
  const double* Ch = ChatT_all + (size_t)f * D0 * dm.D1m;
  long long x0, x1;
  gb_probe_xy(cs, dm.nlines, p, x0, x1);
  auto xi_of = [&](double xn, int axis) {
    double xi = (2.0 * xn - (dm.a[axis] + dm.b[axis])) / (dm.b[axis] - dm.a[axis]);
    xi = xi < 1.0 ? xi : 1.0;
    return xi > -1.0 ? xi : -1.0;
  };
  const double xi0 = xi_of(xn0[x0], 0), xi1 = xi_of(xn1[x1], 1);
  double sum = 0.0;
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
    sum = fma(row, tb, sum);
  }
  sum = wave_sum(sum);
  if (lane == 0) raw[(size_t)f * kGbProbes + p] = sum;
}
// K1i's band from its probes (as guard.hip's k_gb_band, with the mean's truncation tail and a MEASURED band of the Lipschitz
// keys: the gradient sums are derivatives of an interpolant).  raw [4 q][P]; ref_g [q][2][P] the exact gradient components.
__global__ __launch_bounds__(256) void k_gb_band_i(const InterpParams* __restrict__ P_, const double* __restrict__ raw, const double* __restrict__ ref_m,
                                                   const double* __restrict__ ref_v, const double* __restrict__ ref_g,
                                                   const double* __restrict__ tail /* [4 q] tails | [4 q] frames */, const double* __restrict__ alpha,
                                                   int a_ld, GuardBand* gb, GuardBand* gb_mirror /* pinned host copy (sbo_profile_get) */) {
  const ModelConst& mc = P_->mc;
  __shared__ double sh[4][6];
  __shared__ double sha[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int o = 0; o < mc.q; ++o) {
    const double ys = mc.Y_std[o];
    double e[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};          // |dm|, |dv|, |m|, |v|, |dg|, |g|
    bool bad = false;
    for (int p = tid; p < kGbProbes; p += blockDim.x) {
      double var = mc.sf2[o] - raw[(size_t)(4 * o) * kGbProbes + p];
      var = (var > 0.0 ? var : 0.0) * (ys * ys);
      const double m = (mc.mp[o] + raw[(size_t)(4 * o + 1) * kGbProbes + p]) * ys + mc.Y_mean[o];
      const double rm = ref_m[(size_t)o * kGbProbes + p], rv = ref_v[(size_t)o * kGbProbes + p];
      const double dm_ = fabs(m - rm), dv_ = fabs(var - rv);
      bad = bad || !(dm_ < kGbInf) || !(dv_ < kGbInf);
      e[0] = fmax(e[0], dm_); e[1] = fmax(e[1], dv_); e[2] = fmax(e[2], fabs(rm)); e[3] = fmax(e[3], fabs(rv));
      for (int a = 0; a < 2; ++a) {
        const double g = ys * mc.inv_ell[o][a] * mc.X_rstd[a] * raw[(size_t)(4 * o + 2 + a) * kGbProbes + p];
        const double rg = ref_g[((size_t)o * 2 + a) * kGbProbes + p];
        bad = bad || !(fabs(g - rg) < kGbInf);
        e[4] = fmax(e[4], fabs(g - rg));
        e[5] = fmax(e[5], fabs(rg));
      }
    }
    // (a probe whose deviation is not finite: fmax drops a NaN, so the flag joins the reduction itself -- every thread holds at most
    // one of the 144 probes, and only lane 1's flag used to be published)
    if (bad) e[0] = kGbInf;
    double a1p = 0.0;                                         // ||alpha_o||_1 (the worst-case rounding of the mean's sum: the check below)
    for (int j = tid; j < mc.n; j += blockDim.x) a1p += fabs(alpha[(size_t)o * a_ld + j]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a1p += __shfl_xor(a1p, off);
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) e[k] = fmax(e[k], __shfl_xor(e[k], off));
    __syncthreads();
    if (lane == 0) {
      for (int k = 0; k < 6; ++k) sh[wave][k] = e[k];
      sha[wave] = a1p;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 4; ++w)
        for (int k = 0; k < 6; ++k) e[k] = fmax(e[k], sh[w][k]);
      e[0] = fmax(e[0], sh[0][0]);
      const double eps = 2.220446049250313e-16;
      const bool inf = !(e[0] < kGbInf);
      // analytic part (r05): the dropped coefficients of the series that is run (|T_a T_b| <= 1), and the interpolation error of the node
      // fields -- at most twice the sum of the TRUE coefficients beyond the node count, which is extrapolated from the last four degrees
      // held (kGbAliasFactor x their sum: twice a geometric continuation at a ratio <= 0.8 per degree; the posterior of an RBF kernel is
      // entire, its coefficients decay faster than any such ratio once they decay at all)
      const double* frame = tail + 4 * mc.q;
      const double an_m = (tail[4 * o + 1] + kGbAliasFactor * frame[4 * o + 1]) * ys;
      const double an_v = (tail[4 * o] + kGbAliasFactor * frame[4 * o]) * ys * ys;
      const double fl_m = 64.0 * eps * fmax(e[2], fabs(mc.Y_mean[o]) + ys), fl_v = 64.0 * eps * fmax(e[3], mc.sf2[o] * ys * ys);
      gb->an_m[o] = an_m; gb->an_v[o] = an_v; gb->pr_m[o] = e[0]; gb->pr_v[o] = e[1];
      // ... plus the measured rounding level of the plan's sums; the check: a probe deviation that truncation + the worst-case rounding
      // of the reference formula do not explain (GuardBand, device_common.hpp)
      const double a1 = (sha[0] + sha[1]) + (sha[2] + sha[3]);
      const bool distrust = e[0] > an_m + gb_round_mean(mc.n, mc.sf2[o], a1, ys) || e[1] > an_v + gb_round_var(mc.n, mc.sf2[o], mc.sn2[o], ys);
      gb->dm[o] = (inf || distrust) ? kGbInf : an_m + kGbSafety * e[0] + fl_m;
      gb->dv[o] = (inf || distrust) ? kGbInf : an_v + kGbSafety * e[1] + fl_v;
      gb->rl[o] = (e[5] > 0.0 && !inf) ? 16.0 * e[4] / e[5] + 1e-9 : 1e-3;
      if (gb_mirror) {
        gb_mirror->dm[o] = gb->dm[o]; gb_mirror->dv[o] = gb->dv[o]; gb_mirror->rl[o] = gb->rl[o];
        gb_mirror->an_m[o] = an_m; gb_mirror->an_v[o] = an_v; gb_mirror->pr_m[o] = e[0]; gb_mirror->pr_v[o] = e[1];
      }
    }
    __syncthreads();
  }
}

bool interp_applicable(const sbo_ctx* c) {
  if (c->opt.bilinear != 1 || c->is_shadow || !bilinear_applicable(c)) return false;
  // (the node values come from the reference formula on the caller's matrix: the packed images sbo_model_set made of it)
  // (a grid that arrived after the model: the images are packed on demand from the upload that still sits in the build workspace)
  return c->mc.factor == SBO_FACTOR_INVK && c->opt.chol_async && (c->invk_img_valid || c->invk_w_valid) && c->mc.npad % 16 == 0 &&
         c->dtype == SBO_F64;
}

// Enqueues the plan for the current (model, grid) on the context's streams; nothing waits for the device.
int interp_setup(sbo_ctx* c) {
  InterpPlan& ip = c->bi;
  ip.valid = true;
  ip.usable = false;
  ip.used = false;
  ip.serial = c->model_serial;
  ip.ops = GemmOps();
  c->bl.bt_ready = false;    // (this plan lays its tables into bl_P1A / bl_T4f / bl_cheb / bl_BtA: K1b's stage-1 images do not survive it)
  GemmOps& g = ip.ops;
  const ModelConst& mc = c->mc;
  const CandSpec& cs = c->cs;
  const int n = mc.n, q = mc.q;
  const long long cnt0 = cs.count[0], nlines = cs.n_local / cnt0, line0 = cs.first / cnt0;
  double ab[4];
  if (!basis_intervals(c, ab)) return SBO_OK;
  // nodes per axis from the shortest length scale (tensor.hip's rule for its first two axes), one count for both
  int Dn = 32;
  for (int a = 0; a < 2; ++a) {
    double tmax = 0.0;
    for (int o = 0; o < q; ++o) tmax = std::max(tmax, (ab[2 * a + 1] - ab[2 * a]) * std::sqrt(mc.inv_ell[o][a]));
    const double want = 7.6 * tmax;
    const int need = want <= 32 ? 32 : (want <= 48 ? 48 : (want <= 64 ? 64 : 1 << 20));
    Dn = std::max(Dn, need);
  }
  if (Dn > kIMaxDn || 2 * Dn > cnt0 || 2 * Dn > cs.count[1]) return SBO_OK;      // (not worth it / not resolvable: K1b's plan takes over)
  const int QP = 4 * q;
  if (QP > 4 * kMaxQ) return SBO_OK;
  int rc;
  if (!c->invk_img_valid && (rc = model_pack_invk(c))) return rc;
  BlDims dm;
  memset(&dm, 0, sizeof(dm));
  const int KB = Dn / 16, KBn = mc.npad / 16, ncols = Dn * Dn, ncsR = ncols / 16;
  const int ncs0 = (int)((cnt0 + 15) / 16), nrb = (int)((nlines + 15) / 16);
  dm.q = QP; dm.n = n; dm.KBn = KBn; dm.ncsR = ncsR;
  for (int o = 0; o < kMaxQ; ++o) { dm.r0[o] = Dn; dm.r1[o] = Dn; dm.rc0[o] = Dn; dm.rc1[o] = Dn; }
  dm.r0u = dm.r1u = Dn; dm.KB0 = dm.KB1 = KB; dm.D0m = dm.D1m = Dn; dm.ncs0 = ncs0; dm.nrb = nrb; dm.cnt0 = cnt0; dm.nlines = nlines;
  for (int a = 0; a < 2; ++a) { dm.a[a] = ab[2 * a]; dm.b[a] = ab[2 * a + 1]; }
  InterpDims id;
  id.Dn = Dn; id.q = q; id.n = n; id.npad = mc.npad; id.dpad = mc.dpad;
  for (int a = 0; a < 2; ++a) { id.mid[a] = 0.5 * (ab[2 * a] + ab[2 * a + 1]); id.half[a] = 0.5 * (ab[2 * a + 1] - ab[2 * a]); }
  // (k_bpost's operands: BtA and VA are the stage-1 images of the four coefficient sets of an output -- VA from the second on --,
  // P0f is the B table of every phase)
  g.sets = 4; g.imode = 1;
  g.KB0 = g.KB1 = g.KBm = g.KBm2 = KB; g.KS0 = g.KSm = KB * 4; g.ncs0 = ncs0; g.nrb = nrb;
  g.sT4f = (size_t)KB * KB * 256;
  g.sBt1 = (size_t)nrb * KB * 256;
  g.sBtA = g.sVA = 4 * g.sBt1;
  const size_t nP0f = (size_t)ncs0 * KB * 256, nP1A = (size_t)nrb * KB * 256, nZf = (size_t)ncsR * KBn * 256;
  if ((rc = ensure(c->bl_P0f, sizeof(double) * nP0f))) return rc;
  if ((rc = ensure(c->bl_P1A, sizeof(double) * nP1A))) return rc;
  if ((rc = ensure(c->bl_T4f, sizeof(double) * g.sT4f * QP))) return rc;
  if ((rc = ensure(c->bl_BtA, sizeof(double) * g.sBt1 * QP))) return rc;
  g.BtA = (double*)c->bl_BtA.p; g.VA = g.BtA + g.sBt1; g.P0f = g.SBf = (double*)c->bl_P0f.p;
  if ((rc = ensure(c->bl_small, sizeof(double) * ((size_t)cnt0 + (size_t)nlines)))) return rc;
  // bl_work: E tables [2 q][kBlMaxR][n] | Zf | Cf | CtA (3 x q x nZf) | node fields [q][2][Dn^2]
  const size_t nE = (size_t)2 * q * kBlMaxR * n;
  if ((rc = ensure(c->bl_work, sizeof(double) * (nE + 3 * (size_t)q * nZf + (size_t)q * 2 * ncols)))) return rc;
  // bl_cheb: ChatT [4 q][Dn^2] | eff (4 QP ints) + tails (QP doubles)
  if ((rc = ensure(c->bl_cheb, sizeof(double) * ((size_t)QP * ncols + 4 * (size_t)QP + 16)))) return rc;
  double* E = (double*)c->bl_work.p;
  double* Zf = E + nE;
  double* Cf = Zf + (size_t)q * nZf;
  double* CtA = Cf + (size_t)q * nZf;
  double* V = CtA + (size_t)q * nZf;
  double* Chat = (double*)c->bl_cheb.p;
  int* eff = (int*)(Chat + (size_t)QP * ncols);
  double* dxn0 = (double*)c->bl_small.p;
  double* dxn1 = dxn0 + cnt0;
  const unsigned uq = (unsigned)q;
  auto blocks = [&](size_t total, unsigned y) { return dim3((unsigned)std::min<size_t>((total + 255) / 256, 1u << 16), y); };
  hipStream_t xs = c->stream, ys = c->stream2 ? c->stream2 : c->stream, zs = (ys != xs && c->stream3) ? c->stream3 : ys;
  const bool band = c->opt.guard_band != 0;
  // buffers of the gate and of the probes
  const int ntx = (ncs0 + 7) / 8, nty = (nrb + 3) / 4;
  const size_t nt = (size_t)ntx * nty, head = (size_t)q * 2 * nt + 4 * (size_t)q;
  const size_t nS0 = (size_t)q * Dn * cnt0, nVb = (size_t)q * 3 * Dn * nlines;
  if ((rc = ensure(c->bl_grad, sizeof(double) * (head + nS0 + nVb)))) return rc;
  if ((rc = ensure(c->gb.pts, sizeof(double) * ((size_t)QP * kGbProbes + 2 * (size_t)kGbProbes + 2 * (size_t)q * kGbProbes)))) return rc;
  if ((rc = ensure(c->bi_params, sizeof(InterpParams)))) return rc;
  if (!c->h_bi_params.p && hipHostMalloc(&c->h_bi_params.p, sizeof(InterpParams), hipHostMallocDefault) != hipSuccess)
    return fail(SBO_E_NOMEM, "pinned staging of the plan's parameters");
  double* gt = (double*)c->bl_grad.p;
  double* slack = gt + (size_t)q * 2 * nt;
  unsigned long long* gkey = (unsigned long long*)(slack + 2 * q);
  double* S0i = (double*)(gkey + 2 * q);
  double* Vbi = S0i + nS0;
  double* raw = (double*)c->gb.pts.p;
  double* ppts = raw + (size_t)QP * kGbProbes;
  double* pgrad = ppts + 2 * (size_t)kGbProbes;
  // ---- what changes with the model: one block, read by the plan's kernels from device memory
  InterpParams hp;
  memset(&hp, 0, sizeof(hp));
  hp.mc = mc;
  hp.id = id;
  hp.dm = dm;
  hp.dxi0 = cs.count[0] > 1 ? 0.5 * kGradStep * std::fabs(cs.step[0] / mc.X_std[0]) / id.half[0] : 0.0;
  hp.dxi1 = cs.count[1] > 1 ? 0.5 * kGradStep * std::fabs(cs.step[1] / mc.X_std[1]) / id.half[1] : 0.0;
  const InterpParams* dP = (const InterpParams*)c->bi_params.p;
  const bool gate = std::isfinite(hp.dxi0) && std::isfinite(hp.dxi1);
  g.gtmax = gate ? gt : nullptr;
  g.gkey = gate ? gkey : nullptr;
  // (the previous plan's copy of the block has normally run long ago -- a sweep has synchronised since --, but two model changes in
  // a row must not let the first plan's copy read the second model's block)
  if (c->ev_bi_params.e) SBO_HIP(hipEventSynchronize(c->ev_bi_params.e));
  else SBO_HIP(hipEventCreateWithFlags(&c->ev_bi_params.e, hipEventDisableTiming));
  memcpy(c->h_bi_params.p, &hp, sizeof(hp));
  const bool defer = gate && c->opt.grad_defer && zs != xs && zs != ys;
  ip.grad_deferred = defer;
  // (no gate at all -- the deferred launch runs both gradient phases on every tile -- where the grid is small enough for the gate's
  // three launches to cost more than the phases they save: A/B r05, config B 0.419 -> 0.398 ms per iteration, config H 0.870 -> 0.920.
  // grad_defer = 2: always; 3: never)
  const bool nogate = defer && (c->opt.grad_defer == 2 || (c->opt.grad_defer == 1 && (long long)ntx * nty * q <= 4ll * c->n_cu));
  if (nogate) { g.gtmax = nullptr; g.gkey = nullptr; }
  SBO_HIP(hipMemcpyAsync(c->bi_params.p, c->h_bi_params.p, sizeof(InterpParams), hipMemcpyHostToDevice, xs));
  if (ys != xs) {
    SBO_HIP(hipEventRecord(c->ev[7], xs));               // (the model's arrays and the block are in place at this point of the main stream)
    SBO_HIP(hipStreamWaitEvent(ys, c->ev[7], 0));
    if (zs != ys) SBO_HIP(hipStreamWaitEvent(zs, c->ev[7], 0));
  }
  // (enqueue order: the plan is host-bound on the smaller grids -- Z's one long kernel first, then the head of X, then Y's one launch)
  double *gref_m = nullptr, *gref_v = nullptr;
  if (band) {
    // Z: the guard band's references at the probe points -- the reference formula (guard.hip) and the exact gradient
    if ((rc = guard_probe_reference(c, zs, &gref_m, &gref_v, &dP->mc))) return rc;
    if ((rc = guard_probe_gradients(c, zs, ppts, pgrad, &dP->mc))) return rc;
    if (zs != ys) SBO_HIP(hipEventRecord(c->ev_join[6], zs));
  }
  // X: node fields and their coefficients
  hipLaunchKernelGGL(k_i_etab, blocks((size_t)Dn * n, 2 * uq), dim3(256), 0, xs, dP, (const double*)c->As.p, E);
  hipLaunchKernelGGL(k_bl_zf, blocks(nZf, uq), dim3(256), 0, xs, dm, (const double*)E, nZf, Zf);
  // (A/B r05: nine column strips per wave -- exactly one wave per SIMD on config H instead of 2.25 -- took 120 us against 93: the
  // fragment loads of a lone wave are not hidden by anything)
  hipLaunchKernelGGL((k_bgemm<4, 0, 1>), dim3((unsigned)((ncsR + 3) / 4), (unsigned)((KBn + 3) / 4), uq), dim3(256), 0, xs,
                     (const double*)c->invk_img.p, (size_t)mc.npad * mc.npad, (const double*)Zf, nZf, KBn, KBn, ncsR, Cf, nZf, CtA, 0ll);
  hipLaunchKernelGGL(k_i_nodevals, dim3((unsigned)ncsR, uq), dim3(64), 0, xs, KBn, n, (const double*)Zf, (const double*)Cf, nZf,
                     c->factor.alpha(), c->factor.a_ld(), ncols, V);
  {
    const size_t lds = sizeof(double) * 3 * (size_t)Dn * (Dn + 1);
    SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_i_dct), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_i_dct, dim3(2 * uq), dim3(1024), lds, xs, dP, (const double*)V, Chat);
  }
  // (deferred tail, r05: the fork of the gate's and the band's side chains rides on this kernel as its stop event -- a record of its own
  // would be a bubble in the chain)
  if (defer) hipExtLaunchKernelGGL(k_cheb_trunc, dim3((unsigned)QP), dim3(1024), 0, xs, nullptr, c->ev_grad[0], 0, dm, (const double*)Chat, c->opt.cheb_tol, eff);
  else hipLaunchKernelGGL(k_cheb_trunc, dim3((unsigned)QP), dim3(1024), 0, xs, dm, (const double*)Chat, c->opt.cheb_tol, eff);
  hipLaunchKernelGGL(k_cheb_t4f, blocks(g.sT4f, (unsigned)QP), dim3(256), 0, xs, dm, (const double*)Chat, g.sT4f, (double*)c->bl_T4f.p);
  // ... and which tiles of k_bpost can hold the largest gradient component (the gate of K1b's gradient phases, fed from the series.
  // A/B r04: without the gate -- 80 us of plan kernels against 45 us of gradient phases on every tile -- the iteration times are the
  // same within the spread)
  // (deferred gate, r05: these kernels are 80 us of small launches whose result only the Lipschitz keys need.  They run on stream3 --
  // behind the guard reference there, beside the plan's tail and the posterior launches --, followed by a launch of the gradient
  // phases alone on the tiles they name (launch_posterior_gemm); the posterior launches carry none)
  hipStream_t gs = defer ? zs : xs;
  if (defer) SBO_HIP(hipStreamWaitEvent(gs, c->ev_grad[0], 0));
  if (!nogate) hipLaunchKernelGGL(k_i_gradslack, dim3(2 * uq), dim3(256), 0, gs, dP, (const double*)Chat, slack);
  // Y: the tables of the grid positions (one launch)
  hipLaunchKernelGGL(k_i_tabs, dim3((unsigned)std::min<long long>(((long long)(ncs0 + nrb) * 16 + 255) / 256, 4096)), dim3(256), 0, ys, dP, cs, line0,
                     dxn0, dxn1, (double*)c->bl_P0f.p, (double*)c->bl_P1A.p, S0i);
  if (ys != xs) SBO_HIP(hipEventRecord(c->ev_join[3], ys));
  if (ys != xs) SBO_HIP(hipStreamWaitEvent(xs, c->ev_join[3], 0));
  // (X again, with the tables of Y: the lines' sums of the gradient series and the sums at the cell centres of every tile)
  if (defer && ys != gs) SBO_HIP(hipStreamWaitEvent(gs, c->ev_join[3], 0));
  if (gate && !nogate) {
    switch (Dn) {
      case 32: hipLaunchKernelGGL((k_i_rtab<32>), dim3((unsigned)((nlines + 255) / 256), uq, (unsigned)(Dn / 8)), dim3(256), 0, gs, dP, (const double*)Chat, (const int*)eff, (const double*)dxn1, Vbi); break;
      case 48: hipLaunchKernelGGL((k_i_rtab<48>), dim3((unsigned)((nlines + 255) / 256), uq, (unsigned)(Dn / 8)), dim3(256), 0, gs, dP, (const double*)Chat, (const int*)eff, (const double*)dxn1, Vbi); break;
      default: hipLaunchKernelGGL((k_i_rtab<64>), dim3((unsigned)((nlines + 255) / 256), uq, (unsigned)(Dn / 8)), dim3(256), 0, gs, dP, (const double*)Chat, (const int*)eff, (const double*)dxn1, Vbi); break;
    }
    hipLaunchKernelGGL(k_bl_gradcoarse, dim3((unsigned)(ntx * nty), uq), dim3(128), 0, gs, dm, (const double*)S0i, (const double*)Vbi,
                       (const double*)dxn0, (const double*)dxn1, ntx, gt, gkey);
    hipLaunchKernelGGL(k_bl_gradmax, dim3(2 * uq), dim3(256), 0, gs, (const double*)gt, ntx * nty, gkey);
  }
  if (band) {
    // (deferred: the plan's own values at the probes and the band from them on Y -- idle since its tables -- beside the series' fragments
    // and stage 1; the posterior launch, whose classification reads the band, waits for ev_grad[3]: launch_posterior_gemm)
    hipStream_t bs = defer ? ys : xs;
    if (defer) SBO_HIP(hipStreamWaitEvent(bs, c->ev_grad[0], 0));
    if (zs != ys) SBO_HIP(hipStreamWaitEvent(bs, c->ev_join[6], 0));
    hipLaunchKernelGGL(k_gb_probe_series, dim3((unsigned)((kGbProbes + 3) / 4), (unsigned)QP), dim3(256), 0, bs, cs, dP, (const double*)Chat,
                       (const int*)eff, (const double*)dxn0, (const double*)dxn1, raw);
    hipLaunchKernelGGL(k_gb_band_i, dim3(1), dim3(256), 0, bs, dP, (const double*)raw, (const double*)gref_m, (const double*)gref_v,
                       (const double*)pgrad, reinterpret_cast<const double*>(eff + 4 * QP), c->factor.alpha(), c->factor.a_ld(), (GuardBand*)c->gb.buf.p,
                       (GuardBand*)c->h_back->guard_band);
    c->gb.mirrored = true;
    if (defer) SBO_HIP(hipEventRecord(c->ev_grad[3], bs));
  }
  SBO_HIP(hipGetLastError());
  SBO_HIP(hipEventRecord(c->ev_bi_params.e, xs));
  if (band) c->gb.host_valid = false;
  g.eff = eff;
  g.band_ready = band;
  ip.usable = true;
  return SBO_OK;
}
