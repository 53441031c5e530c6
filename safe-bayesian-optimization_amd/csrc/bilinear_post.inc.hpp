// bilinear_post.inc.hpp: stage 2 of the GEMM posterior (k_bpost, k_bgrad, k_lmax_reduce, the column path's tile kernels) and
// launch_posterior_gemm, which launches it on the operands of either plan -- part of the bilinear.hip translation unit (included
// inside namespace sbo; not a standalone header).

// Fused stage 2: variance, mean and gradient keys of a 128 x 128 tile of the grid (8 row blocks x 8 column strips) per
// workgroup.  Four GEMM phases share the accumulators; operands are staged through LDS one 16-deep k-block at a time
// (double-buffered), so every fragment is fetched from L2 once per workgroup instead of once per wave:
//   phase 0  quad = Bt    . P0          (KS0 k-steps)  ->  var  = max(0, sf2 - quad) Y_std^2
//   phase 1  s1   = V[0]  . S0          (KSm)          ->  mean = (mp + s1) Y_std + Y_mean
//   phase 2  g0   = [V[1]; V[0]] . [S0; -xn0 S0]  (2 KSm)   gradient sum of axis 0 (the candidate's own xn0 sits in B)
//   phase 3  g1   = V1x   . S0          (KSm)              gradient sum of axis 1 (xn1 of the line is folded into V1x)

// = kClassifyRow of sets.hip: u* key, |S|, |U|, decisions inside the guard band, min-variance keys over S, radius keys
constexpr int kFuseRow = 4 + 2 * kMaxQ;
constexpr int kFuseVmin = 4, kFuseRmax = 4 + kMaxQ;
struct PostCtx {
  double* lds;
  int tid, lane, wave, rb0, cs0, nrb, ncs;
  int st_rb, st_cs, st_off, a_lo, b_st, a_rd;
  unsigned int ucnt0;
  long long nlines;
  bool full;          // the workgroup's 128 x 128 tile lies inside the grid: epilogues skip their bounds tests
  bool imode;         // K1i: every phase is a plain GEMM on its own Chebyshev coefficients (the gradient phases start from zero)
  // fused classification (one-constraint sweeps): the mean epilogue of the constraint's output reads back the variances this
  // thread stored in the variance phase and writes the S / U bytes; null = off
  const double* var_rd;
  uint8_t *S, *U;
  double bconf, bb;   // confidence multiplier and its square
  int cS, cU;         // this thread's counts
  double rmax;        // max ucb over its safe candidates (-1: none; ucb >= lcb >= 0 on S)
  // guard band of this posterior (guard.hip): sign tests the band of the constraint's output could move are counted, and the
  // smallest variance over the thread's safe candidates is kept (gdm < 0: no band in force)
  LcbBand lband;
  bool gb_on;
  double vminS;
  int cB;
  // column-word classification (r05): role 1 = the constraint's tile packs its S / U bits (bw: S in the low, U in the high 16
  // bits, bit 4 t + (lane >> 4) of the wave's 16 rows, one word per strip); role 2 = the objective's tile reads the S bits of its
  // candidates back (bw: its own four bits per strip at 0, 4, 8, 12) and keeps u* / min var_0 over them
  int role;
  unsigned int bw[8];
  unsigned int* lds_bits;   // [4 waves][128 columns] pieces of role 1
  double umin;              // role 2: min ucb_0 over the thread's safe candidates (+inf: none)
  double xmin;              // role 1: min of a lower bound of ucb_1 over its safe candidates; role 2: of lcb_0 (the tile's range for the set phase)
  bool skip_store;          // lean sweep: an objective tile without a safe candidate, or a constraint tile its enclosure proves unsafe -- mean / var are not stored (role 0)
};

// One GEMM phase of k_bpost on the workgroup's 128 x 128 tile: A images / B fragments of `KB` k-blocks per row block /
// strip, `KS` k-steps run.  PH selects the epilogue: 0 variance, 1 mean, 2 / 3 gradient component of axis 0 / 1.
// The accumulators belong to the caller: phase 2 does not start from zero but from phase 1's sums scaled by -xn0 of the
// candidate's column, g0 = V1 . S0 - xn0 (V0 . S0) -- six k-steps instead of twelve for the stacked [V1; V0] operand.
// S / U bits of one candidate from its stored mean / var: the arithmetic of k_classify (models/SafeOpt.py:37-43, 57-59, 73-77)
// (the sign of lcb without the square root -- lcb_sign, device_common.hpp -- and the exact ucb, for the radius key, only when
// its cheap upper bound beats this thread's running maximum: the IEEE f64 square root is a dozen dependent instructions on the
// datapath the matrix cores use, which is what made this epilogue cost the kernel as much as the separate pass saved)
__device__ __forceinline__ void post_classify_mv(PostCtx& cx, size_t g, double m, double v) {
  const LcbSign sg = cx.gb_on ? lcb_sign_gb(m, v, cx.bconf, cx.bb, cx.lband, cx.cB) : lcb_sign(m, v, cx.bconf, cx.bb);
  cx.S[g] = sg.ge;
  cx.U[g] = sg.le;
  cx.cS += sg.ge;
  cx.cU += sg.le;
  if (sg.ge) {
    cx.vminS = v < cx.vminS ? v : cx.vminS;
    if (!(ucb_upper(m, v, cx.bconf) <= cx.rmax)) {
      const double ucb = add_rn(m, mul_rn(cx.bconf, sqrt_rn(v)));
      if (ucb > cx.rmax) cx.rmax = ucb;
    }
  }
}
__device__ __forceinline__ void post_classify(PostCtx& cx, size_t g, double m) { post_classify_mv(cx, g, m, cx.var_rd[g]); }
// the same decisions as bits of the strip's word (role 1): no byte stores
// The classification of one tile row (eight strips) of the constraint, branch-lean: the kernel is bound by instruction issue on
// the datapath the matrix cores share, and three quarters of a grid's tiles hold no safe candidate at all.  The sign of
// lcb = m - b sqrt(v) as lcb_sign decides it (device_common.hpp) -- from m^2 against b^2 v wherever that is safe, as plain predicates
// without branches; what they leave open (a bound within a few ulp of zero, NaN, out-of-range products: rare) takes the IEEE
// square root behind ONE wave-uniform test per row.  |S| and |U| are the populations of the bit words at the end (no counters
// here); everything that concerns safe candidates only -- the smallest variance, the tile's range of ucb_1 -- runs behind a second
// uniform test, so a tile without a safe candidate never enters it.  Decisions identical to post_classify_mv.
__device__ __forceinline__ void post_classify_row(PostCtx& cx, unsigned int pos, const double (&mv)[8], const double (&vr)[8]) {
  constexpr double c = 1.0 + 0x1p-48, tiny = 1e-250, huge = 1e300;
  unsigned int gem = 0u, lem = 0u, und = 0u;
  const bool bok = cx.bconf >= 0.0;
#pragma unroll
  for (int s2 = 0; s2 < 8; ++s2) {
    const double m = mv[s2], v = vr[s2];
    const double P = m * m, Q = cx.bb * v;
    if (cx.gb_on) {
      const double gap = P > Q ? P - Q : Q - P, am = m < 0 ? -m : m;
      cx.cB += !(gap > fma(am, cx.lband.c1, cx.lband.c0));               // (NaN operands count as near)
    }
    const bool ok = bok && v >= 0.0, rng = P < huge && Q < huge;
    const bool neg = ok && m < 0.0;
    const bool ge = ok && !neg && rng && P > tiny && P >= Q * c;
    const bool le = neg || (ok && rng && !ge && Q > tiny && P * c <= Q && m >= 0.0);
    gem |= ge ? (1u << s2) : 0u;
    lem |= le ? (1u << s2) : 0u;
    und |= (!ge && !le) ? (1u << s2) : 0u;
  }
  if (__ballot(und != 0u) != 0ull) {
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2) {
      if ((und >> s2) & 1u) {
        const double sd = mul_rn(cx.bconf, sqrt_rn(vr[s2]));
        gem |= (mv[s2] >= sd) ? (1u << s2) : 0u;
        lem |= (mv[s2] <= sd) ? (1u << s2) : 0u;
      }
    }
  }
#pragma unroll
  for (int s2 = 0; s2 < 8; ++s2) cx.bw[s2] |= (((gem >> s2) & 1u) | (((lem >> s2) & 1u) << 16)) << pos;
  if (__ballot(gem != 0u) != 0ull) {
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2) {
      if ((gem >> s2) & 1u) {
        const double m = mv[s2], v = vr[s2];
        cx.vminS = v < cx.vminS ? v : cx.vminS;
        // bounds of ucb_1 from one single-precision square root (ucb_upper / ucb_lower, device_common.hpp: the hardware's 1-ulp root
        // is well inside their 2^-20 slack): the exact bound only when it could raise the radius key; the lower bound feeds the
        // tile's range
        const float sf = __builtin_amdgcn_sqrtf((float)v);
        const double s_up = (double)sf * (1.0 + 0x1p-20) + 1e-18;
        double s_lo = (double)sf * (1.0 - 0x1p-20) - 1e-18;
        s_lo = s_lo > 0.0 ? s_lo : 0.0;
        const bool fin = sf < 3.0e38f;
        const double xu = m + cx.bconf * s_up, xl = m + cx.bconf * (fin ? s_lo : 0.0);
        const double up = fin ? xu + (xu < 0 ? -xu : xu) * 0x1p-50 : 1e300, lo = xl - (xl < 0 ? -xl : xl) * 0x1p-50;
        cx.xmin = lo < cx.xmin ? lo : cx.xmin;
        if (!(up <= cx.rmax)) {
          const double ucb = add_rn(m, mul_rn(cx.bconf, sqrt_rn(v)));
          if (ucb > cx.rmax) cx.rmax = ucb;
        }
      }
    }
  }
}
// r06: does post_classify_row leave EVERY (m, v) of the box [mlo, mhi] x [vlo, vhi] with ge = 0, le = 1, outside the undecided branch
// and -- with a band in force -- outside the band test (no contribution to cB)?  Then a tile whose cells all pass adds nothing but
// |U| and the Lipschitz key, and need not be evaluated.  The predicate repeats the epilogue's arithmetic at the box's corners:
// m * m, bb * v and their products with c are monotone in the operand under rounding to nearest, so the corner bounds every point.
// The band test's differences are tested with a relative margin of 2^-40 of the operands on top (the build does not contract,
// Makefile: the margin only keeps the argument independent of that).  NaN anywhere: not decided.
__device__ __forceinline__ bool encl_unsafe(double mlo, double mhi, double vlo, double vhi, double bconf, double bb, bool gb_on, const LcbBand& lb) {
  constexpr double c = 1.0 + 0x1p-48, tiny = 1e-250, huge = 1e300, mg = 0x1p-40;
  if (!(bconf >= 0.0 && vlo >= 0.0 && vlo <= vhi && mlo <= mhi)) return false;          // (NaN: false)
  const double Ql = bb * vlo, Qh = bb * vhi;
  // classification: m < 0 is le outright; 0 <= m <= mhi needs rng, Q > tiny and P c <= Q (then ge is false: P <= P c <= Q < Q c)
  if (!(mhi < 0.0)) {
    const double Ph = mhi * mhi;
    if (!(Ph < huge && Qh < huge && Ql > tiny && Ph * c <= Ql)) return false;
  }
  if (!gb_on) return true;
  // band: |P - Q| > |m| c1 + c0 for every point -- Q above every P by the margin, or (all m < 0) every P above Q
  const double amax = fmax(fabs(mlo), fabs(mhi)), amin = (mlo <= 0.0 && mhi >= 0.0) ? 0.0 : fmin(fabs(mlo), fabs(mhi));
  const double Pmax = amax * amax, Pmin = amin * amin;
  const double rhs = fma(amax, lb.c1, lb.c0);
  if (!(amax < 1e150 && Qh < huge && rhs < huge)) return false;
  const bool qdom = (Ql - Pmax) - mg * (Ql + Pmax) > rhs * (1.0 + mg);
  const bool pdom = mhi < 0.0 && (Pmin - Qh) - mg * (Pmin + Qh) > rhs * (1.0 + mg);
  return qdom || pdom;
}
// The mirror of encl_unsafe: does post_classify_row leave EVERY (m, v) of the box with ge = 1, le = 0, outside the undecided branch and
// -- with a band in force -- outside the band test?  Then every candidate of a tile whose cells all pass is in S and none in U, at this
// sweep's b and band, whatever the tile's values are inside their enclosures.  The predicate is the epilogue's arithmetic at the corner
// (m_lo, v_hi): m > 0 throughout, so m * m is increasing in m and bb * v in v under rounding to nearest, and so are their products
// with c.  For a point of the box P = m * m lies in [Pl, Ph] and Q = bb * v in [0, Qh]: `ok` holds (bconf >= 0, v >= v_lo >= 0), `neg`
// does not (m >= m_lo > 0), `rng` holds (P <= Ph < huge, Q <= Qh < huge), P >= Pl > tiny, and P >= Pl >= Qh * c >= Q * c: ge = 1.  le is
// then false (neg is, and its other branch asks for !ge), so the point is not undecided either.  The band test counts a point unless
// |P - Q| > fma(|m|, c1, c0): here P - Q >= Pl - Qh and the right side is at most its value at m_hi, tested with the same relative
// margin of 2^-40 on the operands as encl_unsafe.  NaN anywhere: not decided.
__device__ __forceinline__ bool encl_safe(double mlo, double mhi, double vlo, double vhi, double bconf, double bb, bool gb_on, const LcbBand& lb) {
  constexpr double c = 1.0 + 0x1p-48, tiny = 1e-250, huge = 1e300, mg = 0x1p-40;
  if (!(bconf >= 0.0 && vlo >= 0.0 && vlo <= vhi && mlo <= mhi && mlo > 0.0)) return false;          // (NaN: false)
  const double Pl = mlo * mlo, Ph = mhi * mhi, Qh = bb * vhi;
  if (!(Ph < huge && Qh < huge && Pl > tiny && Pl >= Qh * c)) return false;
  if (!gb_on) return true;
  const double rhs = fma(mhi, lb.c1, lb.c0);
  if (!(mhi < 1e150 && rhs < huge)) return false;
  return (Pl - Qh) - mg * (Pl + Qh) > rhs * (1.0 + mg);
}
// What a proved-safe tile hands the set phase in place of its candidates' own values, from one cell's enclosure (min / max over the
// tile's 128 cells by the caller).  vlo: the cell's smallest stored variance -- S is the whole tile and the enclosure holds the minimum
// of the stored values, so the variance key is EXACT.  up / lo: bounds of ucb_1 = fl(m + fl(b fl(sqrt v))) over the cell, by the
// arithmetic post_classify_row bounds a candidate's with (one single-precision root, 2^-20 slack, widened by 2^-50): every step of
// ucb_1 is monotone in m and v, so its values on the cell lie between those at (m_lo, v_lo) and (m_hi, v_hi).
// The radius key is therefore an UPPER BOUND of max ucb_1 over the tile, not the maximum itself.  Its readers on the column path, each of
// which takes it as a cap or an interval end and nothing else:
//   * k_col_decide, capC = rmax / L (+ slack): distances beyond it are "beyond every radius"; a larger cap examines more entries and
//     declares fewer cells beyond, never a cell within a true radius beyond;
//   * k_col_decide, the whole-unit tests on [tumin, tumax] (fields 0 and kFuseRmax + 1 of the tile's partial row): a wider interval
//     settles fewer units wholesale, the rest take the per-candidate path on their own values and reach the same verdicts;
//   * the late exhaustive recheck (launch_exact_d -> edt_scan_body and the goose / expander kernels' rmax / L): the same cap;
//   * the host: halo_learn / halo_for (sets.hip), multi-rank only -- the column path runs on one rank --, again rmax / L as a halo width.
// Nobody compares it for equality, reports it, or takes an arg-max from it.
// CELLS (option k1_cells, k_bhead): a tile the boundary of S crosses takes the same three values from each of its cells that is proved
// safe and its candidates' own values from the cells it evaluates, merged by min / max.  vlo stays exact (the minimum over proved cells
// of their smallest stored variance and over the evaluated safe candidates' own: S of the tile is exactly their union).  up / lo are
// then an upper bound of max ucb_1 and a lower bound of min ucb_1 over the tile's safe candidates, tighter than a whole proved tile's
// (a part of the terms is exact); the readers above take them in the same three ways, per tile, and nothing reads them per cell.
struct EnclKeys { double vlo, up, lo; };
__device__ __forceinline__ EnclKeys encl_keys(double mlo, double mhi, double vlo, double vhi, double bconf) {
  const float sfh = __builtin_amdgcn_sqrtf((float)vhi), sfl = __builtin_amdgcn_sqrtf((float)vlo);
  const double s_up = (double)sfh * (1.0 + 0x1p-20) + 1e-18;
  double s_lo = (double)sfl * (1.0 - 0x1p-20) - 1e-18;
  s_lo = s_lo > 0.0 ? s_lo : 0.0;
  const double xu = mhi + bconf * s_up, xl = mlo + bconf * (sfl < 3.0e38f ? s_lo : 0.0);
  EnclKeys k;
  k.vlo = vlo;
  k.up = sfh < 3.0e38f ? xu + (xu < 0 ? -xu : xu) * 0x1p-50 : 1e300;
  k.lo = xl - (xl < 0 ? -xl : xl) * 0x1p-50;
  return k;
}
// role 2: a safe candidate of the objective -- u* = min over S of ucb_0 (models/SafeOpt.py:47-51), the exact bound only when the
// cheap lower bound could beat the thread's running minimum (as k_classify's objective pass), and the smallest var_0 over S
__device__ __forceinline__ void post_objective(PostCtx& cx, bool set, double m, double v) {
  if (set) {
    cx.vminS = v < cx.vminS ? v : cx.vminS;
    const float sf = __builtin_amdgcn_sqrtf((float)v);
    const double s_up = (double)sf * (1.0 + 0x1p-20) + 1e-18;
    double s_lo = (double)sf * (1.0 - 0x1p-20) - 1e-18;
    s_lo = s_lo > 0.0 ? s_lo : 0.0;
    const bool fin = sf < 3.0e38f;
    const double xl = m + cx.bconf * (fin ? s_lo : 0.0), yl = m - cx.bconf * s_up;
    const double ulo = xl - (xl < 0 ? -xl : xl) * 0x1p-50;                      // ucb_0 >= ulo
    const double llo = fin ? yl - (yl < 0 ? -yl : yl) * 0x1p-50 : -1e300;       // lcb_0 >= llo: the tile's range for the minimiser
    cx.xmin = llo < cx.xmin ? llo : cx.xmin;
    if (ulo < cx.umin) {
      const double ucb = add_rn(m, mul_rn(cx.bconf, sqrt_rn(v)));
      cx.umin = ucb < cx.umin ? ucb : cx.umin;
    }
  }
}

// End of a posterior kernel: the waves' Lipschitz maxima (already reduced over the lanes) and, with the fused classification,
// their counts and radius maxima, merged through LDS into ONE value / row per workgroup.  `sh`: NW x 4 doubles of LDS nobody
// reads any more (barrier first).
template <int NW>
__device__ __forceinline__ void post_partials(double* sh, int lane, int wave, double gmax, bool fuse, int cS_, int cU_, double rmax_,
                                              int cB_, double vmin_, double* __restrict__ lrow, unsigned long long* __restrict__ crow /* this
                                              workgroup's row of the field-major partials */, int pcap,
                                              bool objrow = false /* the row of an objective tile (column path): rmax_ carries -min ucb_0 over
                                              its safe candidates (so that the maximum below is the minimum), vmin_ their smallest var_0 */,
                                              unsigned long long* __restrict__ slots = nullptr /* column path: the scalars also join slot
                                              `slot` of every field by atomics (internal.hpp: ColSlotField) */, int slot = 0, int o = 0,
                                              int tile_row = -1, int tile_col = 0,
                                              double xmin_ = 1e300 /* column path: the tile's smallest lower bound of ucb_1 (constraint rows,
                                              field 0) / of lcb_0 (objective rows, field 1) over its safe candidates */,
                                              bool multi = false /* several constraints: this row is constraint o's (its plane's populations are
                                              not |S| / |U|; its variance / radius keys are taken over ITS safe candidates, a superset of S) */) {
  int cS = cS_, cU = cU_, cB = cB_;
  double rm = rmax_, vm = vmin_, xm = xmin_;
  if (fuse || objrow) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      cS += __shfl_xor(cS, off);
      cU += __shfl_xor(cU, off);
      cB += __shfl_xor(cB, off);
      const double other = __shfl_xor(rm, off);
      rm = other > rm ? other : rm;
      const double ov = __shfl_xor(vm, off);
      vm = ov < vm ? ov : vm;
      const double ox = __shfl_xor(xm, off);
      xm = ox < xm ? ox : xm;
    }
  }
  __syncthreads();
  if (lane == 0) {
    sh[wave * 6 + 0] = gmax;
    sh[wave * 6 + 1] = rm;
    reinterpret_cast<int*>(sh + wave * 6 + 2)[0] = cS;
    reinterpret_cast<int*>(sh + wave * 6 + 2)[1] = cU;
    reinterpret_cast<int*>(sh + wave * 6 + 3)[0] = cB;
    sh[wave * 6 + 4] = vm;
    sh[wave * 6 + 5] = xm;
  }
  __syncthreads();
  if (wave == 0) {
    double g = sh[0], r = sh[1], vmn = sh[4], xmn = sh[5];
    long long s_ = 0, u_ = 0, b_ = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      g = sh[w * 6] > g ? sh[w * 6] : g;
      r = sh[w * 6 + 1] > r ? sh[w * 6 + 1] : r;
      vmn = sh[w * 6 + 4] < vmn ? sh[w * 6 + 4] : vmn;
      xmn = sh[w * 6 + 5] < xmn ? sh[w * 6 + 5] : xmn;
      s_ += reinterpret_cast<const int*>(sh + w * 6 + 2)[0];
      u_ += reinterpret_cast<const int*>(sh + w * 6 + 2)[1];
      b_ += reinterpret_cast<const int*>(sh + w * 6 + 3)[0];
    }
    if (lane == 0) *lrow = g;
    if (slots) {
      // (no return values: the wave does not wait for them)
      if (lane == 0) atomicMax(&slots[(size_t)(o == 0 ? kSlotL0 : kSlotL1) * kColSlots + slot], (unsigned long long)__double_as_longlong(g));
      if (objrow) {
        if (lane == 1 && r > -1e300) atomicMin(&slots[(size_t)kSlotUmin * kColSlots + slot], ord_key(-r));
        if (lane == 2 && vmn < 1e300) atomicMin(&slots[(size_t)kSlotVmin0 * kColSlots + slot], ord_key(vmn));
      } else {
        if (lane == 1 && s_ != 0) atomicAdd(&slots[(size_t)kSlotS * kColSlots + slot], (unsigned long long)s_);
        if (lane == 2 && u_ != 0) atomicAdd(&slots[(size_t)kSlotU * kColSlots + slot], (unsigned long long)u_);
        if (lane == 3 && b_ != 0) atomicAdd(&slots[(size_t)kSlotB * kColSlots + slot], (unsigned long long)b_);
        if (lane == 4 && vmn < 1e300) atomicMin(&slots[(size_t)kSlotVmin1 * kColSlots + slot], ord_key(vmn));
        if (lane == 5 && r >= 0.0) atomicMax(&slots[(size_t)kSlotRmax1 * kColSlots + slot], ord_key(r));
        if (lane == 6 && s_ != 0 && tile_row >= 0) atomicOr(&slots[(size_t)kSlotRowMask * kColSlots + tile_row], 1ull << tile_col);
      }
    }
    if (objrow && lane < kFuseRow) {
      // [u* key, 0, 0, 0, min-variance key of output 0, none.., no radius keys]
      unsigned long long v = 0ull;
      if (lane == 0) v = r > -1e300 ? ord_key(-r) : ~0ull;
      else if (lane == 1) v = xmn < 1e300 ? ord_key(xmn) : ~0ull;                 // (the tile's range of lcb_0 over S: sets_colpath's minimiser)
      else if (lane >= kFuseVmin && lane < kFuseRmax) v = (lane == kFuseVmin && vmn < 1e300) ? ord_key(vmn) : ~0ull;
      crow[(size_t)lane * pcap] = v;
    } else
    if (fuse && lane < kFuseRow) {
      // partial row of the classification, merged by k_classify_final: [u* key (none here), |S|, |U|, decisions inside the guard
      // band, min-variance keys over S (output 1 only), radius keys (constraint 1 only)]
      unsigned long long v = 0ull;
      if (lane == 0) v = (slots && xmn < 1e300) ? ord_key(xmn) : ~0ull;           // (column path: the tile's lower end of ucb_1 over S)
      else if (lane == 1) v = multi ? 0ull : (unsigned long long)s_;
      else if (lane == 2) v = multi ? 0ull : (unsigned long long)u_;
      else if (lane == 3) v = (unsigned long long)b_;
      else if (lane >= kFuseVmin && lane < kFuseRmax) v = (lane == kFuseVmin + (o >= 1 ? o : 1) && vmn < 1e300) ? ord_key(vmn) : ~0ull;
      else if (lane == kFuseRmax + (o >= 1 ? o : 1)) v = r >= 0.0 ? ord_key(r) : 0ull;       // radius key of this constraint
      crow[(size_t)lane * pcap] = v;
    }
  }
}

// Epilogue of phase PH for the RB x 8 accumulator tiles of a wave (row blocks cx.rb0 + RB cx.wave + i, strips cx.cs0 + s2)
template <int PH, int RB, int ROLE>
__device__ __forceinline__ void post_epilogue(PostCtx& cx, double* __restrict__ outp, double c0, double c1, double c2, double& gmax_io,
                                              d4_t (&acc)[RB][8]) {
  // gradient phases: max |c0 v| = fl(|c0| max |v|) -- rounding is monotone --, so the tile keeps max |v| (one v_max_f64 with
  // |.| modifiers per element on the datapath the matrix cores share) and scales once
  double gmax = 0.0;
  struct Fold {
    double& io; const double& raw; double c0; bool on;
    __device__ ~Fold() {
      if (on) {
        double ga = c0 * raw;
        ga = ga < 0 ? -ga : ga;
        io = ga > io ? ga : io;
      }
    }
  } fold{gmax_io, gmax, c0, PH >= 2};
  // epilogue: accumulator element t of lane l is row 4 t + (l >> 4), column l & 15 of its 16 x 16 tile
  const unsigned int col_in = cx.lane & 15, row_in = cx.lane >> 4;
  if (PH == 1 && RB == 1 && ROLE != 0 && cx.role != 0) {
    // Column path (r05; its tiles are all interior).  Role 1, the constraint: the classification with its S / U decisions packed as
    // bits of the strip's word.  Role 2, the objective: u* and the range of lcb_0 over the tile's safe candidates (bits read back
    // from the constraint's launch).  Both need the variances this thread stored in the variance phase: the eight of row t + 1 are
    // requested BEFORE row t's means are stored (the stores may alias anything as far as the compiler knows, so it would not move
    // the loads across them itself) -- three of the four round trips to L2 run under the arithmetic of the row before.
    auto row_g0 = [&](int t) {
      const unsigned int line = (unsigned int)(cx.rb0 + cx.wave) * 16u + 4u * t + row_in;
      return (size_t)line * cx.ucnt0 + (unsigned int)cx.cs0 * 16u + col_in;
    };
    // (the objective's tiles: 2 us per launch on config H; the constraint's epilogue holds too much in registers for it -- with the
    // prefetch its allocation spilt 22 vector registers and the launch took 138 us against 132)
    constexpr bool kPrefetch = ROLE == 2;
    double vn[8];
    if (kPrefetch) {
      const size_t g0 = row_g0(0);
#pragma unroll
      for (int s2 = 0; s2 < 8; ++s2) vn[s2] = cx.var_rd[g0 + s2 * 16];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const size_t g0 = row_g0(t), g1 = row_g0(t + 1 < 4 ? t + 1 : t);
      double* const rowp = outp + g0;
      if (ROLE == 1) {
        double vr[8], mv[8];
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) vr[s2] = cx.var_rd[g0 + s2 * 16];
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) {
          mv[s2] = (c0 + acc[0][s2][t]) * c1 + c2;
          rowp[s2 * 16] = mv[s2];
        }
        post_classify_row(cx, 4u * t + row_in, mv, vr);
      } else {
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) {
          const double v = vn[s2];
          if (t + 1 < 4) vn[s2] = cx.var_rd[g1 + s2 * 16];       // (the next row's variance: a row of arithmetic ahead of its use)
          const double m = (c0 + acc[0][s2][t]) * c1 + c2;
          rowp[s2 * 16] = m;
          post_objective(cx, ((cx.bw[s2] >> (4 * t)) & 1u) != 0u, m, v);
        }
      }
    }
    if (ROLE == 1) {
      // |S| / |U| of this thread: the populations of its words (S low half, U high half)
#pragma unroll
      for (int s2 = 0; s2 < 8; ++s2) { cx.cS += __popc(cx.bw[s2] & 0xffffu); cx.cU += __popc(cx.bw[s2] >> 16); }
      // the wave's 16 rows of every column: the four lanes that hold a column OR their bits together, lanes 0..15 put the piece
      // (S low half, U high half) where the end of the kernel assembles the 64-bit words of the tile
#pragma unroll
      for (int s2 = 0; s2 < 8; ++s2) {
        unsigned int w = cx.bw[s2];
        w |= (unsigned int)__shfl_xor((int)w, 16);
        w |= (unsigned int)__shfl_xor((int)w, 32);
        if (cx.lane < 16) cx.lds_bits[cx.wave * 128 + s2 * 16 + cx.lane] = w;
      }
    }
    return;
  }
  if (cx.full) {
    // interior tile: no bounds tests, one pointer per row, the eight strips at immediate offsets.  The matrix cores
    // share the f64 VALU datapath, so every instruction saved here is matrix time.
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const unsigned int line = (unsigned int)(cx.rb0 + RB * cx.wave + i) * 16u + 4u * t + row_in;
        const size_t g0 = (size_t)line * cx.ucnt0 + (unsigned int)cx.cs0 * 16u + col_in;
        double* const rowp = outp + g0;
        if (PH == 1 && ROLE == 0 && cx.S) {
          // fused classification: the eight variances of this row first (all loads in flight; the byte stores below may
          // alias anything as far as the compiler knows), then bounds, S / U bytes and the partial sums
          double vr[8], mv[8];
#pragma unroll
          for (int s2 = 0; s2 < 8; ++s2) vr[s2] = cx.var_rd[g0 + s2 * 16];
#pragma unroll
          for (int s2 = 0; s2 < 8; ++s2) {
            mv[s2] = (c0 + acc[i][s2][t]) * c1 + c2;
            rowp[s2 * 16] = mv[s2];
          }
#pragma unroll
          for (int s2 = 0; s2 < 8; ++s2) post_classify_mv(cx, g0 + s2 * 16, mv[s2], vr[s2]);
          continue;
        }
        if (PH <= 1 && RB == 1 && ROLE != 0 && cx.skip_store) continue;     // (lean sweep: nobody reads this tile's mean / var)
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) {
          const double v = acc[i][s2][t];
          if (PH == 0) {
            double var = c0 - v;
            var = var > 0.0 ? var : 0.0;
            rowp[s2 * 16] = var * c1;
          } else if (PH == 1) {
            rowp[s2 * 16] = (c0 + v) * c1 + c2;
          } else {
            gmax = fmax(gmax, fabs(v));
          }
        }
      }
    return;
  }
#pragma unroll
  for (int i = 0; i < RB; ++i) {
    const int rb = cx.rb0 + RB * cx.wave + i;
    if (rb >= cx.nrb) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const unsigned int line = (unsigned int)rb * 16u + 4u * t + row_in;
      if ((long long)line >= cx.nlines) continue;
      double* const rowp = outp + (size_t)line * cx.ucnt0;
#pragma unroll
      for (int s2 = 0; s2 < 8; ++s2) {
        const unsigned int x0 = (unsigned int)(cx.cs0 + s2) * 16u + col_in;
        if (cx.cs0 + s2 >= cx.ncs || x0 >= cx.ucnt0) continue;
        const double v = acc[i][s2][t];
        if (PH == 0) {
          double var = c0 - v;                                              // models/GP_Safe.py:343, clipped at 0
          var = var > 0.0 ? var : 0.0;
          rowp[x0] = var * c1;                                              // :347
        } else if (PH == 1) {
          const double m = (c0 + v) * c1 + c2;                              // :342, :346
          rowp[x0] = m;
          if (ROLE == 0 && cx.S) post_classify(cx, (size_t)line * cx.ucnt0 + x0, m);
        } else {
          // component of the gradient of the un-normalised mean (analytic jax.grad(self.mean), SafeOpt.py:68-71)
          gmax = fmax(gmax, fabs(v));
        }
      }
    }
  }
}

template <int PH, int RB, int ROLE>
__device__ __forceinline__ void post_phase(PostCtx& cx, const double* __restrict__ A, const double* __restrict__ B, int KB,
                                           int KS, double* __restrict__ outp, double c0, double c1, double c2, double& gmax,
                                           d4_t (&acc)[RB][8], const double* __restrict__ xn0, d4_t (&pre)[4],
                                           const double* __restrict__ An, const double* __restrict__ Bn, int KBn) {
  const double* Ap = A + (size_t)cx.st_rb * KB * 256 + cx.st_off;
  const double* Bp = B + (size_t)cx.st_cs * KB * 256 + cx.st_off;
  const int nkb = (KS + 3) >> 2;
  double* const lds = cx.lds;
  auto stage = [&](double* buf, const d4_t& r0, const d4_t& r1, const d4_t& q0, const d4_t& q1) {
    if (RB == 2 || cx.a_lo >= 0) {
      *reinterpret_cast<d4_t*>(buf + cx.a_lo) = d4_t{r0[0], r0[1], r1[0], r1[1]};
      *reinterpret_cast<d4_t*>(buf + cx.a_lo + 32) = d4_t{r0[2], r0[3], r1[2], r1[3]};
    }
    *reinterpret_cast<d4_t*>(buf + cx.b_st) = q0;
    *reinterpret_cast<d4_t*>(buf + cx.b_st + 4) = q1;
  };
  if (PH == 2 && !cx.imode) {
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2) {
      const unsigned int x = (unsigned int)(cx.cs0 + s2) * 16u + (cx.lane & 15);
      const double f = x < cx.ucnt0 ? -xn0[x] : 0.0;
#pragma unroll
      for (int i = 0; i < RB; ++i) acc[i][s2] = d4_t{acc[i][s2][0] * f, acc[i][s2][1] * f, acc[i][s2][2] * f, acc[i][s2][3] * f};
    }
  } else {
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
      for (int s2 = 0; s2 < 8; ++s2) acc[i][s2] = d4_t{0.0, 0.0, 0.0, 0.0};
  }
  const bool stage_a = RB == 2 || cx.a_lo >= 0;
  // the first k-block's 64 + 64 bytes of this thread: requested by the previous phase before its epilogue (`pre`), so that
  // their latency runs under that epilogue instead of in front of this loop; phase 0 asks here
  // (128 x 128 tiles only: the 64 x 128 form runs three workgroups per CU on 168 registers and would spill the four)
  d4_t &ra0 = pre[0], &ra1 = pre[1], &rb0v = pre[2], &rb1v = pre[3];
  if (PH == 0 || RB == 1) {
    ra0 = ra1 = d4_t{0.0, 0.0, 0.0, 0.0};
    if (stage_a) { ra0 = *reinterpret_cast<const d4_t*>(Ap); ra1 = *reinterpret_cast<const d4_t*>(Ap + 4); }
    rb0v = *reinterpret_cast<const d4_t*>(Bp);
    rb1v = *reinterpret_cast<const d4_t*>(Bp + 4);
  }
  __syncthreads();                             // the previous phase has finished reading the buffers
  stage(lds, ra0, ra1, rb0v, rb1v);
  __syncthreads();
#pragma unroll 1
  for (int kb = 0; kb < nkb; ++kb) {
    const int cur = kb & 1;
    if (kb + 1 < nkb) {
      if (stage_a) {
        ra0 = *reinterpret_cast<const d4_t*>(Ap + (size_t)(kb + 1) * 256);
        ra1 = *reinterpret_cast<const d4_t*>(Ap + (size_t)(kb + 1) * 256 + 4);
      }
      rb0v = *reinterpret_cast<const d4_t*>(Bp + (size_t)(kb + 1) * 256);
      rb1v = *reinterpret_cast<const d4_t*>(Bp + (size_t)(kb + 1) * 256 + 4);
    }
    constexpr int BUF = RB == 2 ? 4096 : 3072, BOFF = RB == 2 ? 2048 : 1024;   // doubles per buffer: 4 RB A images, 8 B strips
    const double* LA = lds + cur * BUF + (RB * cx.wave) * 256 + cx.a_rd;
    const double* LB = lds + cur * BUF + BOFF + cx.lane;
    const int kkn = KS - kb * 4 < 4 ? KS - kb * 4 : 4;
    // operands of k-step kk + 1 are requested before the products of kk are issued (two register sets, no copies): the LDS
    // latency of a k-step's ten reads otherwise sits in front of its 64 matrix instructions
    d4_t fa[2][RB];
    double fb[2][8];
    auto ld = [&](int kk, d4_t (&a)[RB], double (&b)[8]) {
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const d2_t l = *reinterpret_cast<const d2_t*>(LA + i * 256 + kk * 64), h = *reinterpret_cast<const d2_t*>(LA + i * 256 + kk * 64 + 32);
        a[i] = d4_t{l[0], l[1], h[0], h[1]};
      }
#pragma unroll
      for (int s2 = 0; s2 < 8; ++s2) b[s2] = LB[(s2 * 4 + kk) * 64];
    };
    auto mm = [&](const d4_t (&a)[RB], const double (&b)[8]) {
#pragma unroll
      for (int s2 = 0; s2 < 8; ++s2)
#pragma unroll
        for (int i = 0; i < RB; ++i) acc[i][s2] = MM<double>::mfma(a[i], b[s2], acc[i][s2]);
    };
    if constexpr (RB == 2) {
      ld(0, fa[0], fb[0]);
      int kk = 0;
#pragma unroll 1
      for (; kk + 1 < kkn; kk += 2) {
        ld(kk + 1, fa[1], fb[1]);
        mm(fa[0], fb[0]);
        if (kk + 2 < kkn) ld(kk + 2, fa[0], fb[0]);
        mm(fa[1], fb[1]);
      }
      if (kk < kkn) mm(fa[0], fb[0]);
    } else {                               // (three workgroups per CU and 168 registers: no room for a second operand set)
#pragma unroll 1
      for (int kk = 0; kk < kkn; ++kk) {
        ld(kk, fa[0], fb[0]);
        mm(fa[0], fb[0]);
      }
    }
    if (kb + 1 < nkb) stage(lds + (cur ^ 1) * BUF, ra0, ra1, rb0v, rb1v);
    __syncthreads();
  }
  if (RB == 2 && An) {
    const double* Apn = An + (size_t)cx.st_rb * KBn * 256 + cx.st_off;
    const double* Bpn = Bn + (size_t)cx.st_cs * KBn * 256 + cx.st_off;
    if (stage_a) { ra0 = *reinterpret_cast<const d4_t*>(Apn); ra1 = *reinterpret_cast<const d4_t*>(Apn + 4); }
    rb0v = *reinterpret_cast<const d4_t*>(Bpn);
    rb1v = *reinterpret_cast<const d4_t*>(Bpn + 4);
  }
  post_epilogue<PH, RB, ROLE>(cx, outp, c0, c1, c2, gmax, acc);
}

#ifdef SBO_PHASE_CLOCKS
// Diagnostic build only (make phaseclk -> libsafebo_phaseclk.so, tools/dev_phase_clocks.py): the constant 100 MHz counter at the
// phase boundaries of every k_bpost workgroup, a row per workgroup (same-address atomics from 4096 workgroups would themselves
// take 0.1 ms); [4] = gradient phases the workgroup ran.  The host sums the rows.
constexpr int kPhaseClkRows = 1 << 14;
__device__ unsigned long long g_phase_clk[kPhaseClkRows][8];
// r07: and a row per workgroup of the column path's two launches (the last sweep's: overwritten by every launch), in dispatch order
// (linear block index): [0] entry, [1] start of the partial rows (post_partials, the words and their Usum / slot atomics), [2] exit --
// all wall_clock64 --, [3] tile | kind << 24 (0 evaluated, 1 skipped: partial rows only, 2 skipped but its gradient phases run,
// 3 past the tile list: exited at once) | 1 << 31 (row written), [4] HW_REG_HW_ID, [5] HW_REG_XCC_ID.  tools/dev_wg_timeline.py.
constexpr int kWgTraceRows = 1 << 13;
__device__ unsigned long long g_wg_trace[2][kWgTraceRows][8];
__device__ __forceinline__ void wg_trace_row(int o, unsigned long long t0, unsigned long long t1, unsigned long long t2, unsigned int tile, unsigned int kind) {
  unsigned int hw, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  unsigned long long* r = g_wg_trace[o & 1][(blockIdx.y * gridDim.x + blockIdx.x) & (kWgTraceRows - 1)];
  r[0] = t0; r[1] = t1; r[2] = t2;
  r[3] = (unsigned long long)(tile & 0xffffffu) | ((unsigned long long)kind << 24) | (1ull << 31);
  r[4] = hw; r[5] = xcc;
}
#define SBO_CLK(i)                                                                                \
  do {                                                                                           \
    __syncthreads();                                                                             \
    if (threadIdx.x == 0) {                                                                      \
      const unsigned long long now_ = wall_clock64();                                            \
      g_phase_clk[clk_row_ & (kPhaseClkRows - 1)][i] += now_ - clk_;                             \
      clk_ = now_;                                                                               \
    }                                                                                            \
  } while (0)
#else
#define SBO_CLK(i) do { } while (0)
#endif

// r06: the enclosures of the constraint's posterior per 8 x 8 cell of every 64 x 128 column-path tile, taken from what the constraint's
// launch stored -- once per plan, behind its first launch that evaluated every tile.  k_bpost is deterministic for a plan (the same
// operands, the same k-order of the matrix instructions; b and the band enter only the classification), so [min, max] of the stored
// values encloses exactly what any later launch of the plan computes: no bound on derivatives, no rounding allowance.  Layout
// [tile][cell = 16 r + c][m_lo, m_hi, v_lo, v_hi]; a cell holding NaN or inf gets NaN (encl_unsafe: never decided).
// THE INVARIANT THIS RESTS ON: phases 0 / 1 of the constraint's launch compute the same bits on every launch of a plan.  Anything that
// changes their operands, k-steps or k-order between sweeps of one plan (a per-sweep truncation, another tile shape, a different
// accumulation order) must clear BilinearPlan::encl_ready.  The standing audit checks it where it samples an evaluated tile: the stored
// values must lie inside the recorded enclosure bit for bit (guard.hip: k_audit_compare).
// SECOND INVARIANT (k1_skip_safe): a tile proved safe is not evaluated, and the set phase reads its STORED mean / var -- so the
// constraint's regions of sbo_ctx::mean / var must hold the plan's bits on every tile, not only be enclosed by what was recorded.  Who
// may write them, and who drops the flags: BilinearPlan::encl_ready / vals_ready (internal.hpp).  The audit checks a sample on such a
// tile both ways.
__global__ __launch_bounds__(128) void k_bl_enclose(const double* __restrict__ mean, const double* __restrict__ var, long long cnt0,
                                                    double* __restrict__ encl, const double* __restrict__ lrow1 /* the recording launch's
                                                    rows of output 1 in the Lipschitz partials */, double* __restrict__ lrec /* nullptr, or
                                                    where the plan keeps them (BilinearPlan::lrows_ready) */) {
  const int cell = threadIdx.x, cr = cell >> 4, cc = cell & 15;
  const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (cell == 0 && lrec) lrec[tile] = lrow1[tile];
  const size_t base = ((size_t)blockIdx.y * 64 + (size_t)cr * 8) * (size_t)cnt0 + (size_t)blockIdx.x * 128 + (size_t)cc * 8;
  double mlo = 1e308, mhi = -1e308, vlo = 1e308, vhi = -1e308;
  bool fin = true;
  for (int r = 0; r < 8; ++r) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const double m = mean[base + (size_t)r * cnt0 + k], v = var[base + (size_t)r * cnt0 + k];
      fin = fin && fabs(m) <= 1e308 && fabs(v) <= 1e308;                  // (NaN: false)
      mlo = fmin(mlo, m); mhi = fmax(mhi, m); vlo = fmin(vlo, v); vhi = fmax(vhi, v);
    }
  }
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double4 e = fin ? double4{mlo, mhi, vlo, vhi} : double4{nan, nan, nan, nan};
  reinterpret_cast<double4*>(encl)[tile * 128 + cell] = e;
}

// r07: the tile lists of a lean-2 column-path sweep (option k1_sched).  One workgroup per tile left 1451 of config H's 2048 constraint
// workgroups and 1533 of its objective ones doing nothing but their partial rows, interleaved with the evaluated tiles: the evaluated
// ones ran as two partial rounds of workgroups.  Instead the constraint's launch and the objective's run over lists of the tiles that
// need a workgroup -- a 1-D grid, workgroup i takes entry i and exits at once past the list -- so the evaluated tiles are dispatched
// first and fit the CUs in one round.  What a left-out tile produced is written here, bit for bit what its workgroup wrote.
//
// The constraint's tiles, one wave each, kSchedWaves to a workgroup (before the constraint's launch): the skip decision of k_bpost (encl_unsafe on every cell of
// the tile, at this sweep's b and band) and the gradient gate's decision for output 1.  Class 0 = skipped, no gradient phase: no
// workgroup; written here is what its workgroup wrote -- S = 0 and U = all ones words, its bit of Usum in its 128 columns, its
// Lipschitz row, its partial row of the classification (|U| = 8192, no keys) and its scalars in the slot block (|U|, the Lipschitz
// key, the skip count).  1 = evaluated with gradient phases, 2 = skipped but runs gradient phases, 3 = evaluated: these go into the
// list.  The skip byte of every tile for the audit (guard.hip).
// Option k1_skip_safe adds the mirror image: a tile whose every cell encl_safe proves SAFE at this b and band.  Class 4 = proved safe, no
// gradient phase: no workgroup; written here is what its workgroup wrote -- S = all ones and U = 0 words, no bit of Usum, its bit of
// the tile row's mask, its Lipschitz row, its partial row (|S| = 8192, the keys of encl_keys) and its scalars (|S|, the variance,
// radius and Lipschitz keys, the count of such tiles).  Class 5 = proved safe but runs gradient phases: listed at the front like
// class 2, bit 30 of its entry set.  The tile's mean / var stay what the plan's recording launch stored, and the set phase READS them
// (k_col_decide, on the units it cannot settle wholesale): BilinearPlan::encl_ready says who may write those regions.
//
// The list has two ends: classes 1 and 2 -- the tiles with gradient phases, the longest -- fill the front upwards, class 3 fills the
// back downwards, each end behind a counter bumped by one atomic per listed tile; bit 31 of an entry marks class 2.  One pair of
// counters took config H's 738 returning atomics on two addresses: the kernel ran 13.8 us against the 7.1 us it takes without a
// list (profiles/sched_head_H_timeline.txt, variant A; B and C for the figures below).  So the list is kTlistShards lists of that form (PostExtra::tlist): of every kTlistShards consecutive tiles each goes to
// another shard -- rotated by three from one such block to the next, so that a band of unsafe tile columns does not leave the same
// shards short: shards of unequal length put workgroups that exit at once between the launch's real ones, which cost k_bpost<1, 1>
// 6 us when whole classifier workgroups shared a shard --, a shard has room for its share of the tiles (cap), and workgroup i of the
// launch takes entry i / kTlistShards of shard i mod kTlistShards -- front entries upwards, then the back entries from the last one
// down (k_bpost) --, so the long tiles are still dispatched first.  The order inside an end is whatever the atomics give, and no result depends on it: a tile's words, partial row,
// Lipschitz row and slot (tile mod kColSlots) depend on the tile alone, and every merge into the slot block and into Usum is an
// integer add, an OR, or a min / max of ordered keys.
// The counters are zero when this kernel starts: k_bl_sched_list2, which follows the constraint's launch in every sweep that runs
// this kernel, resets them once the list is dead (sbo_ctx::bl_sched, a ResetBuf).  Usum is zero as well (col_words_prepare, k_col_decide), as
// the launch over the whole tile grid needs it; the listed tiles OR their bits in behind.
// The slot block: one atomic per scalar and tile -- config H's 3900 on the twelve cache lines of three fields -- took 4 of the kernel's
// 10.5 us; the kSchedWaves tiles of a workgroup are merged in LDS first and join one slot (sums and a maximum: the slot does not
// change them).  The 128 ORs per tile into Usum cost nothing measurable (they spread over 4096 words).
constexpr int kSchedWaves = 8;
__global__ __launch_bounds__(64 * kSchedWaves) void k_bl_sched_tiles1(const ModelConst mc, const double* __restrict__ encl, int ntiles, int tgx, int tgy,
                                                         unsigned int cnt0, double bconf, const GuardBand* __restrict__ gb,
                                                         const double* __restrict__ gtmax, const unsigned long long* __restrict__ gkey, int q,
                                                         uint8_t* __restrict__ skip, unsigned int* __restrict__ list, int cap, unsigned long long* __restrict__ Sw,
                                                         unsigned long long* __restrict__ Uw, unsigned long long* __restrict__ Usum,
                                                         unsigned long long* __restrict__ slots, double* __restrict__ Lpart,
                                                         unsigned long long* __restrict__ cpart, int pcap, int skip_safe /* option k1_skip_safe */,
                                                         const double* __restrict__ lrec /* option k1_resident: nullptr, or the plan's rows of
                                                         output 1 (BilinearPlan::lrows_ready) -- a tile's Lipschitz row comes from there and no
                                                         tile is listed for its gradient phases: class 2 becomes 0, 5 becomes 4, 1 becomes 3 */,
                                                         int count_res /* the listed tiles are classified from memory (k_bres<1>): counted */) {
  __shared__ unsigned long long sh_key[kSchedWaves];     // per wave: the Lipschitz key of a class-0 / class-4 tile (0: none)
  __shared__ unsigned int sh_cnt[kSchedWaves];            // ... bit 0: a class-0 tile, bit 1: a tile proved unsafe (class 0 or 2), bit 2: a class-4 tile, bit 3: a tile proved safe (class 4 or 5), bit 4: a listed tile k_bres<1> classifies
  __shared__ unsigned long long sh_vmin[kSchedWaves], sh_rmax[kSchedWaves];   // ... a class-4 tile's variance / radius key (~0 / 0: none)
  const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6), tile = (int)blockIdx.x * kSchedWaves + wave;
  unsigned long long my_key = 0ull, my_vmin = ~0ull, my_rmax = 0ull;
  unsigned int my_cnt = 0u;
  if (tile < ntiles) {                                    // (a whole wave or none of it)
    const double bb = bconf * bconf;
    const bool gb_on = gb != nullptr;
    const LcbBand lb = gb_on ? lcb_band(bb, gb->dm[1], gb->dv[1]) : LcbBand{0.0, 0.0};
    bool ok = true, oks = skip_safe != 0;
    double kv = 1e300, ku = -1.0, kl = 1e300;             // (the tile's keys, should it be proved safe: encl_keys)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const double4 e = reinterpret_cast<const double4*>(encl)[(size_t)tile * 128 + h * 64 + lane];
      ok = ok && encl_unsafe(e.x, e.y, e.z, e.w, bconf, bb, gb_on, lb);
      oks = oks && encl_safe(e.x, e.y, e.z, e.w, bconf, bb, gb_on, lb);
      if (oks) {
        const EnclKeys ek = encl_keys(e.x, e.y, e.z, e.w, bconf);
        kv = ek.vlo < kv ? ek.vlo : kv;
        ku = ek.up > ku ? ek.up : ku;
        kl = ek.lo < kl ? ek.lo : kl;
      }
    }
    const bool dec = __ballot(!ok) == 0ull;
    const bool sdec = !dec && __ballot(!oks) == 0ull;       // (proved safe: classes 4 / 5)
    // (k_bpost's gate, output 1, and the largest coarse sample it folds in)
    bool run2 = true, run3 = true;
    double gfold = 0.0;
    if (gtmax) {
      const size_t nt = (size_t)ntiles;
      const double* slack = gtmax + (size_t)q * 2 * nt;
      const double ystd = mc.Y_std[1];
      const double cg0 = ystd * mc.inv_ell[1][0] * mc.X_rstd[0], cg1 = ystd * mc.inv_ell[1][1] * mc.X_rstd[1];
      const double t0 = gtmax[(size_t)2 * nt + tile], t1 = gtmax[(size_t)3 * nt + tile];
      const double G0 = __longlong_as_double((long long)gkey[2]), G1 = __longlong_as_double((long long)gkey[3]);
      run2 = !(t0 + slack[2] < G0 * (1.0 - 1e-12));
      run3 = !(t1 + slack[3] < G1 * (1.0 - 1e-12));
      gfold = fmax(fabs(cg0 * t0), fabs(cg1 * t1));
    }
    const bool grad = !lrec && (run2 || run3);             // (k1_resident: the row below holds what the gradient phases found)
    // (4 = proved safe, no gradient phase: no workgroup, written below; 5 = proved safe but runs gradient phases: listed like class 2)
    const unsigned int k = dec ? (grad ? 2u : 0u) : (sdec ? (grad ? 5u : 4u) : (grad ? 1u : 3u));
    if (lane == 0) skip[tile] = dec ? kSkipUnsafe : (sdec ? kSkipSafe : 0);
    my_cnt = k == 0u ? 3u : (k == 2u ? 2u : (k == 4u ? 12u : (k == 5u ? 8u : ((k == 3u && count_res) ? 16u : 0u))));
    if (k != 0u && k != 4u) {
      if (lane == 0) {
        // (p < cap whenever the counters started from zero; the test keeps a store inside the shard whatever they held)
        const unsigned int sh = ((unsigned int)tile + 3u * ((unsigned int)tile >> kTlistShift)) & (kTlistShards - 1);
        const unsigned int p = atomicAdd(&list[sh * kTlistHead + (k == 3u ? 1 : 0)], 1u);
        if (p < (unsigned int)cap)
          list[kTlistShards * kTlistHead + sh * cap + (k == 3u ? (unsigned int)(cap - 1) - p : p)] =
              (unsigned int)tile | (k == 2u ? kTlistUnsafe : (k == 5u ? kTlistSafe : 0u));
      }
    } else if (k == 4u) {
      // what the tile's workgroup wrote (k_bpost, csafe): every S bit, no U bit -- so no bit of Usum --, its Lipschitz row, its partial
      // row (|S| = 8192, the lower end of ucb_1, the variance and radius keys of encl_keys) and, below, its scalars in the slot block
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(kv, off), ou = __shfl_xor(ku, off), ol = __shfl_xor(kl, off);
        kv = ov < kv ? ov : kv;
        ku = ou > ku ? ou : ku;
        kl = ol < kl ? ol : kl;
      }
      const int bx = tile % tgx, by = tile / tgx;
      const size_t w0 = (size_t)by * cnt0 + (size_t)bx * 128;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        Sw[w0 + h * 64 + lane] = ~0ull;
        Uw[w0 + h * 64 + lane] = 0ull;
      }
      const double lrow = lrec ? lrec[tile] : fmax(0.0, gfold);
      my_key = (unsigned long long)__double_as_longlong(lrow);
      my_vmin = kv < 1e300 ? ord_key(kv) : ~0ull;
      my_rmax = ku >= 0.0 ? ord_key(ku) : 0ull;
      if (lane == 0) {
        Lpart[((size_t)tgy + by) * tgx + bx] = lrow;
        atomicOr(&slots[(size_t)kSlotRowMask * kColSlots + by], 1ull << bx);      // (no return value)
      }
      if (lane < kFuseRow) {                                // (post_partials' row, fuse && slots)
        unsigned long long v = 0ull;
        if (lane == 0) v = kl < 1e300 ? ord_key(kl) : ~0ull;
        else if (lane == 1) v = 64ull * 128ull;
        else if (lane >= kFuseVmin && lane < kFuseRmax) v = lane == kFuseVmin + 1 ? my_vmin : ~0ull;
        else if (lane == kFuseRmax + 1) v = my_rmax;
        cpart[(size_t)lane * pcap + tile] = v;
      }
    } else {
      const int bx = tile % tgx, by = tile / tgx;
      const size_t w0 = (size_t)by * cnt0 + (size_t)bx * 128;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        Sw[w0 + h * 64 + lane] = 0ull;
        Uw[w0 + h * 64 + lane] = ~0ull;
        atomicOr(&Usum[(size_t)bx * 128 + h * 64 + lane], 1ull << by);      // (no return value: the wave does not wait for it)
      }
      const double lrow = lrec ? lrec[tile] : fmax(0.0, gfold);
      my_key = (unsigned long long)__double_as_longlong(lrow);               // (the key in post_partials' encoding)
      if (lane == 0) Lpart[((size_t)tgy + by) * tgx + bx] = lrow;
      // (post_partials' row of a tile with every candidate in U: no safe candidate, no decision in the band, no keys)
      if (lane < kFuseRow) {
        unsigned long long v = 0ull;
        if (lane == 0) v = ~0ull;
        else if (lane == 2) v = 64ull * 128ull;
        else if (lane >= kFuseVmin && lane < kFuseRmax) v = ~0ull;
        cpart[(size_t)lane * pcap + tile] = v;
      }
    }
  }
  if (lane == 0) { sh_key[wave] = my_key; sh_cnt[wave] = my_cnt; sh_vmin[wave] = my_vmin; sh_rmax[wave] = my_rmax; }
  __syncthreads();
  if (threadIdx.x < 8) {
    unsigned long long key = 0ull, n0 = 0ull, nskip = 0ull, n4 = 0ull, nsafe = 0ull, nres = 0ull, vmin = ~0ull, rmax = 0ull;
#pragma unroll
    for (int w = 0; w < kSchedWaves; ++w) {
      key = sh_key[w] > key ? sh_key[w] : key;
      n0 += sh_cnt[w] & 1u;
      nskip += (sh_cnt[w] >> 1) & 1u;
      n4 += (sh_cnt[w] >> 2) & 1u;
      nsafe += (sh_cnt[w] >> 3) & 1u;
      nres += (sh_cnt[w] >> 4) & 1u;
      vmin = sh_vmin[w] < vmin ? sh_vmin[w] : vmin;
      rmax = sh_rmax[w] > rmax ? sh_rmax[w] : rmax;
    }
    const int slot = (int)(blockIdx.x & (kColSlots - 1));
    if (threadIdx.x == 0 && n0) atomicAdd(&slots[(size_t)kSlotU * kColSlots + slot], 64ull * 128ull * n0);
    if (threadIdx.x == 1 && (n0 || n4)) atomicMax(&slots[(size_t)kSlotL1 * kColSlots + slot], key);
    if (threadIdx.x == 2 && nskip) atomicAdd(&slots[(size_t)kSlotSkip * kColSlots + slot], nskip);
    if (threadIdx.x == 3 && n4) atomicAdd(&slots[(size_t)kSlotS * kColSlots + slot], 64ull * 128ull * n4);
    if (threadIdx.x == 4 && nsafe) atomicAdd(&slots[(size_t)kSlotSkipSafe * kColSlots + slot], nsafe);
    if (threadIdx.x == 5 && vmin != ~0ull) atomicMin(&slots[(size_t)kSlotVmin1 * kColSlots + slot], vmin);
    if (threadIdx.x == 6 && rmax != 0ull) atomicMax(&slots[(size_t)kSlotRmax1 * kColSlots + slot], rmax);
    if (threadIdx.x == 7 && nres) atomicAdd(&slots[(size_t)kSlotResC * kColSlots + slot], nres);
  }
}

// Positions in a list of the tiles a 1024-thread workgroup holds in one round (tile = 1024 round + thread), three classes: a ballot per
// class gives the rank inside the wave, every thread sums the 16 waves' counts from LDS.  Returns the thread's position in the list for
// its class k (0..2; -1: none) -- base[k] + the tiles of class k before it in this round -- and adds the round's totals to base[].
__device__ __forceinline__ unsigned int sched_rank3(int k, unsigned int (&base)[3], unsigned int* __restrict__ sh /* [3][16] */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned int rank = 0u;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const unsigned long long m = __ballot(k == j);
    if (k == j) rank = (unsigned int)__popcll(m & below);
    if (lane == 0) sh[j * 16 + wave] = (unsigned int)__popcll(m);
  }
  __syncthreads();
  unsigned int pos = 0u, tot[3] = {0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 3; ++j)
    for (int w = 0; w < 16; ++w) {
      const unsigned int c = sh[j * 16 + w];
      if (k == j && w < wave) pos += c;
      tot[j] += c;
    }
  __syncthreads();
  const unsigned int r = k >= 0 ? base[k] + pos + rank : 0u;
#pragma unroll
  for (int j = 0; j < 3; ++j) base[j] += tot[j];
  return r;
}

// The objective's list (one workgroup, behind the constraint's launch): the tiles that hold a safe candidate (field 1 of the
// constraint's partial rows), in tile order.  The others' objective rows as their workgroups wrote them in a lean-2 sweep (no safe
// candidate, no gradient phase): no u* key, no range of lcb_0, no variance key, Lipschitz row 0.  One shard; without `omap` one end: [1] = 0.
// With it (option k1_resident) the tiles whose residency byte stands fill the back, and their count joins slot 0 of kSlotResO.
// It also resets the counters of the constraint's list (`head1`), which is dead by now -- the constraint's launch, its only reader,
// has finished on this stream --, for the next sweep's k_bl_sched_tiles1.
__global__ __launch_bounds__(1024) void k_bl_sched_list2(unsigned long long* __restrict__ cpart, int pcap, int ntiles, unsigned int* __restrict__ list,
                                                         double* __restrict__ Lpart0, unsigned int* __restrict__ head1,
                                                         const uint8_t* __restrict__ omap /* option k1_resident: nullptr, or the plan's residency
                                                         bytes -- the list is split by them, the tiles whose byte stands fill the back downwards
                                                         (k_bres<2> reads their stored mean / var), the others the front (k_bpost<1, 2>) */,
                                                         unsigned long long* __restrict__ slots) {
  __shared__ unsigned int sh[3 * 16];
  const int t = threadIdx.x;
  const unsigned long long* nS = cpart + (size_t)1 * pcap;
  unsigned long long* orow = cpart + ntiles;
  unsigned int base[3] = {0u, 0u, 0u};
  for (int r = 0; r * 1024 < ntiles; ++r) {
    const int i = r * 1024 + t;
    const bool in = i < ntiles, has = in && nS[i] != 0ull, res = has && omap && omap[i] != 0;
    const unsigned int p = sched_rank3(has ? (res ? 1 : 0) : -1, base, sh);
    if (has) {
      list[kTlistHead + (res ? (unsigned int)(ntiles - 1) - p : p)] = (unsigned int)i;
    } else if (in) {
      Lpart0[i] = 0.0;
#pragma unroll
      for (int lane = 0; lane < kFuseRow; ++lane)
        orow[(size_t)lane * pcap + i] = (lane <= 1 || (lane >= kFuseVmin && lane < kFuseRmax)) ? ~0ull : 0ull;
    }
  }
  if (t == 0) {
    list[0] = base[0];
    list[1] = base[1];
    if (base[1]) atomicAdd(&slots[(size_t)kSlotResO * kColSlots], (unsigned long long)base[1]);
  }
  if (t < kTlistShards) head1[t * kTlistHead] = head1[t * kTlistHead + 1] = 0u;
}

// RB: row blocks per wave.  2 = the 128 x 128 tile above; 1 = a 64 x 128 tile for grids whose 128 x 128 tiles would leave
// CUs without a workgroup (1024 x 1024 x 3 outputs: 192 tiles on 256 CUs) -- half the reuse of a B fragment, twice the
// workgroups.
template <int RB, int ROLE = 0 /* column path: 1 = the constraint's launch (S / U column words), 2 = the objective's (u* over S) */>
__global__ __launch_bounds__(256, (RB == 2 ? 2 : 3)) void k_bpost(const ModelConst mc, const CandSpec cs, const double* __restrict__ BtA, size_t sBtA,
                                                  const double* __restrict__ P0f, size_t sP0f, const double* __restrict__ VA,
                                                  size_t sVA, const double* __restrict__ SBf, size_t sSBf, int KB0, int KS0, int KBm,
                                                  int KSm, int KBm2, int nrb, int ncs, long long nlines, double* __restrict__ mean_out,
                                                  double* __restrict__ var_out, double* __restrict__ Lpart,
                                                  const double* __restrict__ xn0, uint8_t* __restrict__ Sfuse, uint8_t* __restrict__ Ufuse,
                                                  double bconf, unsigned long long* __restrict__ cpart /* [kFuseRow][pcap]: a row per workgroup of output 1 */,
                                                  int pcap,
                                                  const GuardBand* __restrict__ gb /* nullptr: no guard band */,
                                                  const int* __restrict__ eff /* nullptr, or the Chebyshev core's k-steps of the variance phase at [4 o] */,
                                                  const double* __restrict__ gtmax /* nullptr (every tile runs the gradient phases), or the plan's
                                                  largest gradient samples per tile [q][2][tiles], followed by the slacks [q][2] */,
                                                  const unsigned long long* __restrict__ gkey /* the grid's largest samples [q][2] */,
                                                  int imode /* K1i (interpolation from Chebyshev nodes): BtA / VA hold the stage-1 images of four
                                                  coefficient sets per output (quadratic form, mean sum, two gradient sums), SBf the Chebyshev table
                                                  P0f; the k-steps of every phase come from eff[4 (4 o + phase)] */,
                                                  const PostExtra px /* column path: one launch per output (o0), the S / U column words */) {
  extern __shared__ double lds[];               // [2][A: 8 x 256 | B: 8 x 256] (+ 2 KB of bit pieces behind them, column path)
  const int o = px.o0 + (int)blockIdx.z;
  // r07: a launch over a tile list (PostExtra::tlist) takes its tile from entry blockIdx.x of a 1-D grid; every index below that names
  // the tile -- row block, strip, the words, the partial rows, the gate's table -- comes from (bx, by) and the tile grid (tgx, tgy)
  const bool listed = ROLE != 0 && px.tlist != nullptr;
  unsigned int ent = 0u;
  if (listed) {
    // (shard i mod 2^tshift, entry i >> tshift of it: the front entries upwards, then the back entries from the last one down --
    // k_bl_sched_tiles1)
    const unsigned int sh = blockIdx.x & ((1u << px.tshift) - 1u), at = blockIdx.x >> px.tshift;
    const unsigned int nfront = px.tlist[sh * kTlistHead], nback = px.front_only ? 0u : px.tlist[sh * kTlistHead + 1];
    if (at >= nfront + nback) {
#ifdef SBO_PHASE_CLOCKS
      // (front_only: the rows of this dispatch index belong to k_bres<2>, which ran first)
      if (threadIdx.x == 0 && !px.front_only) { const unsigned long long t_ = wall_clock64(); wg_trace_row(o, t_, t_, t_, 0xffffffu, 3u); }
#endif
      return;                                   // (past the list: the tile was written by the list's kernels)
    }
    ent = px.tlist[(kTlistHead << px.tshift) + sh * (unsigned int)px.tcap + (at < nfront ? at : (unsigned int)px.tcap - 1u - (at - nfront))];
  }
  const unsigned int tgx = listed ? (unsigned int)px.tgx : gridDim.x, tgy = listed ? (unsigned int)px.tgy : gridDim.y;
  const unsigned int bx = listed ? (ent & 0xffffffu) % tgx : blockIdx.x, by = listed ? (ent & 0xffffffu) / tgx : blockIdx.y;
  PostCtx cx;
  cx.lds = lds;
  cx.tid = threadIdx.x; cx.lane = cx.tid & 63; cx.wave = cx.tid >> 6;
  cx.rb0 = by * (4 * RB); cx.cs0 = bx * 8; cx.nrb = nrb; cx.ncs = ncs;
  cx.ucnt0 = (unsigned int)cs.count[0];
  cx.nlines = nlines;
  cx.full = (long long)(cx.rb0 + 4 * RB) * 16 <= nlines && (long long)(cx.cs0 + 8) * 16 <= cs.count[0];
  cx.imode = imode != 0;
  // staging role of this thread: 64 bytes of one A image and 64 bytes of one B strip per k-block.
  // LDS image of an A block: per k-step the 16 lane-chunks are split into their first and second 16 bytes
  // ([16 x 16 B][16 x 16 B]) so that both ds_read_b128 of a fragment load touch 256 contiguous bytes (no bank conflicts)
  const int st_i = cx.tid >> 5, st_j = cx.tid & 31;
  cx.st_off = st_j * 8;
  cx.st_rb = cx.rb0 + st_i < nrb ? cx.rb0 + st_i : nrb - 1;
  cx.st_cs = cx.cs0 + st_i < ncs ? cx.cs0 + st_i : ncs - 1;
  cx.a_lo = st_i < 4 * RB ? st_i * 256 + (st_j >> 3) * 64 + (st_j & 7) * 4 : -1;   // (RB = 1: four images, half the threads stage one)
  cx.b_st = (RB == 2 ? 2048 : 1024) + st_i * 256 + cx.st_off;
  cx.a_rd = (((cx.lane >> 4) << 2) + (cx.lane & 3)) * 2;
  // per-output operands; VA holds [V0 | V1;V0 | V1x] as three image sets, SBf holds [S0 | S0;-xn0 S0] as two fragment sets
  const double* VAo = VA + (size_t)o * sVA;
  const double* SBo = SBf + (size_t)o * sSBf;
  const double sf2 = mc.sf2[o], ystd = mc.Y_std[o];
  double* const vo = var_out + (size_t)o * cs.n_local;
  double* const mo = mean_out + (size_t)o * cs.n_local;
  // (one constraint: the masks themselves; several, r05: constraint o writes byte plane o - 1, AND-ed by k_classify_and)
  const bool fuse = Sfuse != nullptr && o >= 1;
  const bool fmulti = px.fstride != 0;
  cx.var_rd = vo;
  cx.S = fuse ? Sfuse + (size_t)(o - 1) * (size_t)px.fstride : nullptr;
  cx.U = fuse ? Ufuse + (size_t)(o - 1) * (size_t)px.fstride : Ufuse;
  cx.bconf = bconf;
  cx.bb = bconf * bconf;
  cx.cS = cx.cU = cx.cB = 0;
  cx.rmax = -1.0;
  // column path: a tile is 64 rows (one segment of the column words) x 128 columns
  const bool cbits = RB == 1 && ROLE == 1 && px.cb.Sw != nullptr && o == 1, obits = RB == 1 && ROLE == 2 && px.cb.Sw != nullptr && o == 0;
  const size_t ctile = (size_t)by * tgx + bx, ntile = (size_t)tgx * tgy;
  // (objective: how many safe candidates the constraint's launch counted in this tile -- field 1 of its partial row)
  const unsigned long long tile_nS = obits ? cpart[(size_t)1 * pcap + ctile] : 0ull;
  cx.role = cbits ? 1 : ((obits && tile_nS != 0ull) ? 2 : 0);
  cx.skip_store = obits && tile_nS == 0ull && px.lean != 0;
  cx.lds_bits = reinterpret_cast<unsigned int*>(lds + 2 * (RB == 2 ? 4096 : 3072));
  cx.umin = 1e300;
  cx.xmin = 1e300;
#pragma unroll
  for (int s2 = 0; s2 < 8; ++s2) cx.bw[s2] = 0u;
  cx.gb_on = (fuse || cbits) && gb != nullptr;
  cx.lband = cx.gb_on ? lcb_band(cx.bb, gb->dm[o >= 1 ? o : 1], gb->dv[o >= 1 ? o : 1]) : LcbBand{0.0, 0.0};
  cx.vminS = 1e300;
  double gmax = 0.0;
  // (Tried: odd outputs running the three short phases first and the variance phase last, so that the two workgroups of a
  // CU do not reach their phase changes together -- no gain on config B, 2.5 % slower on H; one order for all.)
  d4_t acc[RB][8];
  d4_t pre[4];
  const double* const A2 = VAo + (size_t)nrb * KBm * 256;
  const double* const B2 = imode ? SBo : SBo + (size_t)ncs * KBm * 256;
  const double* const A3 = VAo + (size_t)nrb * (KBm + KBm2) * 256;
  const int es = imode ? 4 : 1;
  const int KS1 = imode ? eff[4 * (4 * o + 1)] : KSm, KS2 = imode ? eff[4 * (4 * o + 2)] : KSm, KS3 = imode ? eff[4 * (4 * o + 3)] : KSm;
#ifdef SBO_PHASE_CLOCKS
  unsigned long long clk_ = wall_clock64();
  const unsigned long long clk_in_ = clk_;
  unsigned long long clk_part_ = clk_;
  const unsigned int clk_row_ = ((unsigned int)o * tgy + by) * tgx + bx;
#endif
  // The gradient phases (their maxima are the Lipschitz keys, models/SafeOpt.py:68-83) run on the tiles that can hold the grid's
  // maximum: the tile's largest coarse sample + the plan's bound on what lies between the samples reaches the grid's largest
  // sample (k_bl_gradbound / k_bl_gradcoarse above).  Every tile folds its own samples in (true grid values).  NaN: run.
  const double cg0 = ystd * mc.inv_ell[o][0] * mc.X_rstd[0], cg1 = ystd * mc.inv_ell[o][1] * mc.X_rstd[1];
  bool run2 = true, run3 = true;
  double gfold = 0.0;                       // (uniform: scalar registers -- folded in behind the phases)
  if (gtmax) {
    const size_t nt = ntile, tile = ctile;
    const double* slack = gtmax + (size_t)px.q * 2 * nt;
    const double t0 = gtmax[((size_t)o * 2 + 0) * nt + tile], t1 = gtmax[((size_t)o * 2 + 1) * nt + tile];
    const double G0 = __longlong_as_double((long long)gkey[2 * o + 0]), G1 = __longlong_as_double((long long)gkey[2 * o + 1]);
    run2 = !(t0 + slack[2 * o + 0] < G0 * (1.0 - 1e-12));
    run3 = !(t1 + slack[2 * o + 1] < G1 * (1.0 - 1e-12));
    const double f0 = fabs(cg0 * t0), f1 = fabs(cg1 * t1);
    gfold = fmax(f0, f1);
  }
  if (px.nograd) { run2 = run3 = false; gfold = 0.0; }          // (the keys come from a launch of the gradient phases alone: k_bgrad)
  if (ROLE == 2 && px.lean) { run2 = run3 = false; gfold = 0.0; }   // (a lean sweep: nobody reads the objective's key, include/safebo.h)
  // lean sweeps, level 2: the objective's posterior of a tile without a safe candidate is not even evaluated -- u*, M and the
  // arg-max reductions read it on S only (models/SafeOpt.py:47-66); the tile still runs the gradient phases the gate asks for
  // (L_0 is a maximum over the whole grid), and with K1b's operands the mean phase those continue from
  // r06, the same for the constraint: a tile whose every 8 x 8 cell the plan's enclosure proves unsafe at this b (encl_unsafe: ge = 0,
  // le = 1, no undecided branch, outside the band test) is not evaluated either -- its words, counts and keys are those of a tile in
  // which every candidate is in U, written here; its gradient phases run as the gate says.  Nothing of this sweep reads its mean /
  // var: the set phase reads the constraint's posterior on tiles with a safe candidate only (G within S), and the audit checks a
  // sample that lands here against the enclosure instead (guard.hip).
  // (r07, a listed launch: the list's kernel took the decision, wrote the skip byte and counted the tile; its entry carries it)
  // k1_skip_safe, the mirror image: a tile whose every cell the enclosure proves SAFE at this b and band (encl_safe) is not evaluated
  // either -- every S bit, no U bit, |S| = 8192, the keys of encl_keys (the variance key exact, the ends of ucb_1 as bounds), its
  // gradient phases as the gate says.  Unlike an unsafe tile's, its mean / var ARE read by this sweep (k_col_decide, on the units it
  // cannot settle wholesale): they are what the plan's recording launch stored, which is what this launch would store again
  // (BilinearPlan::encl_ready: nobody else writes those regions while the flag stands).
  bool cskip = false, csafe = false;
  if (ROLE == 1 && cbits && px.lean >= 2 && px.encl != nullptr) {
    if (listed) {
      cskip = (ent & kTlistUnsafe) != 0u;
      csafe = (ent & kTlistSafe) != 0u;
    } else {
      bool dec = true, sdec = px.skip_safe != 0;
      if (cx.tid < 128) {
        const double4 e = reinterpret_cast<const double4*>(px.encl)[ctile * 128 + cx.tid];
        dec = encl_unsafe(e.x, e.y, e.z, e.w, cx.bconf, cx.bb, cx.gb_on, cx.lband);
        sdec = sdec && encl_safe(e.x, e.y, e.z, e.w, cx.bconf, cx.bb, cx.gb_on, cx.lband);
      }
      cskip = __syncthreads_and(dec ? 1 : 0) != 0;
      csafe = __syncthreads_and(sdec ? 1 : 0) != 0 && !cskip;
      if (cx.tid == 0) px.skip[ctile] = cskip ? kSkipUnsafe : (csafe ? kSkipSafe : 0);
      if (cskip && cx.tid == 0) atomicAdd(&px.cb.slots[(size_t)kSlotSkip * kColSlots + (ctile & (kColSlots - 1))], 1ull);
      if (csafe && cx.tid == 0) atomicAdd(&px.cb.slots[(size_t)kSlotSkipSafe * kColSlots + (ctile & (kColSlots - 1))], 1ull);
    }
    if (cskip) {
      cx.role = 0;
      cx.skip_store = true;
      cx.cU = 64 * 128 / 256;               // (every candidate in U, spread over the threads: the partials sum to 8192)
      for (int i = cx.tid; i < 4 * 128; i += 256) cx.lds_bits[i] = 0xffff0000u;      // (S pieces 0, U pieces all ones)
    }
    if (csafe) {
      cx.role = 0;
      cx.skip_store = true;
      cx.cS = 64 * 128 / 256;               // (every candidate in S)
      for (int i = cx.tid; i < 4 * 128; i += 256) cx.lds_bits[i] = 0x0000ffffu;      // (S pieces all ones, U pieces 0)
      if (cx.tid < 128) {                   // (a cell per thread; post_partials takes the minima / the maximum over the workgroup)
        const double4 e = reinterpret_cast<const double4*>(px.encl)[ctile * 128 + cx.tid];
        const EnclKeys ek = encl_keys(e.x, e.y, e.z, e.w, cx.bconf);
        cx.vminS = ek.vlo;
        cx.rmax = ek.up;
        cx.xmin = ek.lo;
      }
    }
  }
  const bool skip_tile = (ROLE == 2 && obits && tile_nS == 0ull && px.lean >= 2) || cskip || csafe;
  // (k1_resident: this workgroup stores the objective's mean / var of its tile -- the plan's bits: a later sweep may read them, k_bres<2>)
  if (ROLE == 2 && obits && px.omap != nullptr && !cx.skip_store && cx.tid == 0) px.omap[ctile] = 1;
  if (!skip_tile)
    post_phase<0, RB, ROLE>(cx, BtA + (size_t)o * sBtA, P0f + (size_t)o * sP0f, KB0, eff ? eff[4 * o * es] : KS0, vo, sf2, ystd * ystd, 0.0, gmax, acc, xn0, pre,
                            VAo, SBo, KBm);
  SBO_CLK(0);
  if (ROLE == 2 && cx.role == 2) {
    // the thread's own S bits: rows 16 wave + 4 t + (lane >> 4) of the segment, column (cs0 + s2) 16 + (lane & 15)
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2) {
      const unsigned long long w = px.cb.Sw[(size_t)by * cx.ucnt0 + (unsigned int)(cx.cs0 + s2) * 16u + (cx.lane & 15)];
      cx.bw[s2] = (unsigned int)(w >> (16 * cx.wave + (cx.lane >> 4))) & 0x1111u;
    }
  }
  // (the mean phase requests the first operands of whichever phase follows it)
  if (!skip_tile || (run2 && !imode))
    post_phase<1, RB, ROLE>(cx, VAo, SBo, KBm, KS1, mo, mc.mp[o], ystd, mc.Y_mean[o], gmax, acc, xn0, pre, run2 ? A2 : A3, run2 ? B2 : SBo,
                            run2 ? KBm2 : KBm);
  SBO_CLK(1);
  // phase 2 continues on phase 1's sums: only the V1 half (the first KSm k-steps) of the stacked operands is run
  if (run2) post_phase<2, RB, ROLE>(cx, A2, B2, KBm2, KS2, nullptr, cg0, 0.0, 0.0, gmax, acc, xn0, pre, A3, SBo, KBm);
  if (run3) post_phase<3, RB, ROLE>(cx, A3, SBo, KBm, KS3, nullptr, cg1, 0.0, 0.0, gmax, acc, xn0, pre, nullptr, nullptr, 0);
  gmax = fmax(gmax, gfold);
  SBO_CLK(2);
#ifdef SBO_PHASE_CLOCKS
  clk_part_ = clk_;
#endif
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double other = __shfl_xor(gmax, off);
    gmax = other > gmax ? other : gmax;
  }
  // one plain store per WORKGROUP, merged by k_lmax_reduce / the classification's final merge: every workgroup of this launch
  // is resident at once and ends at the same time, so atomics on the q keys would queue up in L2 as the kernel's tail -- and
  // a row per wave made that merge (one workgroup, 16384 rows of 88 bytes on config H) the longest job of the launch it shares
  // (column path: the constraint's rows first, the objective's rows behind them)
  post_partials<4>(cx.lds, cx.lane, cx.wave, gmax, fuse || cbits, cx.cS, cx.cU, obits ? -cx.umin : cx.rmax, cx.cB, cx.vminS,
                   Lpart + ((size_t)o * tgy + by) * tgx + bx,
                   cpart + (obits ? ntile : (fmulti && o >= 1 ? (size_t)(o - 1) * ntile : (size_t)0)) + ctile, pcap, obits,
                   (cbits || obits) ? px.cb.slots : nullptr, (int)(ctile & (kColSlots - 1)), o, cbits ? (int)by : -1, (int)bx, cx.xmin, fmulti);
  if (cbits && cx.tid < 128) {
    // the tile's words: column tid, the four waves' 16-row pieces (written before the barriers of post_partials)
    unsigned long long sw = 0ull, uw = 0ull;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const unsigned int pc = cx.lds_bits[w * 128 + cx.tid];
      sw |= (unsigned long long)(pc & 0xffffu) << (16 * w);
      uw |= (unsigned long long)(pc >> 16) << (16 * w);
    }
    const size_t col = (size_t)cx.cs0 * 16u + cx.tid;
    px.cb.Sw[(size_t)by * cx.ucnt0 + col] = sw;
    px.cb.Uw[(size_t)by * cx.ucnt0 + col] = uw;
    if (uw != 0ull) atomicOr(&px.cb.Usum[col], 1ull << by);
  }
  SBO_CLK(3);
#ifdef SBO_PHASE_CLOCKS
  if (threadIdx.x == 0) {
    g_phase_clk[clk_row_ & (kPhaseClkRows - 1)][4] += (unsigned long long)((run2 ? 1 : 0) + (run3 ? 1 : 0));
    g_phase_clk[clk_row_ & (kPhaseClkRows - 1)][5] += 1ull;
    if (ROLE != 0)
      wg_trace_row(o, clk_in_, clk_part_, clk_, (unsigned int)ctile, skip_tile ? ((!(cskip || csafe) || !(run2 || run3)) ? 1u : 2u) : 0u);
  }
#endif
}
#ifdef SBO_PHASE_CLOCKS
extern "C" int sbo_debug_phase_clocks(unsigned long long* out /* [16]: sums over the rows below `split` | from `split` on */, int reset, int split) {
  std::vector<unsigned long long> h((size_t)kPhaseClkRows * 8);
  if (hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_phase_clk), sizeof(unsigned long long) * h.size()) != hipSuccess) return 1;
  for (int k = 0; k < 16; ++k) out[k] = 0;
  for (size_t r = 0; r < (size_t)kPhaseClkRows; ++r)
    for (int k = 0; k < 8; ++k) out[(r < (size_t)split ? 0 : 8) + k] += h[r * 8 + k];
  if (reset) {
    std::fill(h.begin(), h.end(), 0ull);
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase_clk), h.data(), sizeof(unsigned long long) * h.size()) != hipSuccess) return 1;
  }
  return 0;
}
// r07: the per-workgroup rows of the column path's two launches (g_wg_trace: [o][dispatch index][8]); reset: zero them afterwards
extern "C" int sbo_debug_wg_trace(unsigned long long* out /* [2][rows][8] */, int rows, int reset) {
  if (rows != kWgTraceRows) return 2;
  const size_t bytes = sizeof(unsigned long long) * 2 * kWgTraceRows * 8;
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wg_trace), bytes) != hipSuccess) return 1;
  if (reset) {
    std::vector<unsigned long long> z(bytes / sizeof(unsigned long long), 0ull);
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_wg_trace), z.data(), bytes) != hipSuccess) return 1;
  }
  return 0;
}
#endif

// Option k1_resident: the listed tiles of a lean-2 column-path launch classified from the mean / var an earlier launch of the plan
// stored -- k_bpost's epilogue without its GEMM phases.  ROLE 1, the constraint (BilinearPlan::vals_ready stands: its regions hold the
// plan's bits on every tile, which are the bits phases 0 / 1 would compute again -- invariant 1 at k_bl_enclose): post_classify_row on
// the stored values, words, Usum, partial row and slots as k_bpost writes them; the tile's Lipschitz row is the plan's (`lrec`,
// BilinearPlan::lrows_ready).  ROLE 2, the objective (the back entries of its list: tiles whose residency byte stands): post_objective
// over the S bits of the constraint's words, u*, the range of lcb_0 and the variance key into the objective's partial row and slots; its
// Lipschitz row is 0 as in every lean launch.  Nothing is stored to mean / var.
// The thread <-> candidate mapping is the accumulators' (row 16 wave + 4 t + (lane >> 4), column 16 s2 + (lane & 15)), so the bit
// pieces and the partials are assembled by the same code; every merge is an integer add, an OR, or a min / max of ordered keys, and
// b and the band enter here exactly as they enter the epilogue: the results are k_bpost's bit for bit.  All 64 values of a thread are
// requested before the first is used: there are no accumulators to hold.
// With option k1_cells (the default) the constraint's head is k_bhead, below; k_bres<1> stays for k1_cells 0, the A/B and identity
// switch.  k_bres<2> is the objective's light launch either way.
template <int ROLE>
__global__ __launch_bounds__(256) void k_bres(const CandSpec cs, const double* __restrict__ mean, const double* __restrict__ var,
                                              double* __restrict__ Lpart, double bconf, unsigned long long* __restrict__ cpart, int pcap,
                                              const GuardBand* __restrict__ gb, const double* __restrict__ lrec, const PostExtra px) {
  __shared__ double sh[4 * 6];
  __shared__ unsigned int bits[4 * 128];
  const int o = px.o0;
  // (the entry of workgroup i: k_bpost's rule; the objective's light launch takes the back entries alone)
  const unsigned int shd = blockIdx.x & ((1u << px.tshift) - 1u), at = blockIdx.x >> px.tshift;
  const unsigned int nfront = ROLE == 2 ? 0u : px.tlist[shd * kTlistHead], nback = px.tlist[shd * kTlistHead + 1];
#ifdef SBO_PHASE_CLOCKS
  const unsigned long long clk_in_ = wall_clock64();      // (g_wg_trace: kind 4 = classified from memory, [1] = the loads have arrived)
  unsigned long long clk_ld_ = clk_in_;
#endif
  if (at >= nfront + nback) {
#ifdef SBO_PHASE_CLOCKS
    if (threadIdx.x == 0) wg_trace_row(o, clk_in_, clk_in_, clk_in_, 0xffffffu, 3u);
#endif
    return;
  }
  const unsigned int ent = px.tlist[(kTlistHead << px.tshift) + shd * (unsigned int)px.tcap + (at < nfront ? at : (unsigned int)px.tcap - 1u - (at - nfront))];
  const unsigned int tgx = (unsigned int)px.tgx, tgy = (unsigned int)px.tgy;
  const unsigned int bx = (ent & 0xffffffu) % tgx, by = (ent & 0xffffffu) / tgx;
  const size_t ctile = (size_t)by * tgx + bx, ntile = (size_t)tgx * tgy;
  PostCtx cx;
  cx.lds = sh;
  cx.tid = threadIdx.x; cx.lane = cx.tid & 63; cx.wave = cx.tid >> 6;
  cx.rb0 = by * 4; cx.cs0 = bx * 8;
  cx.ucnt0 = (unsigned int)cs.count[0];
  cx.var_rd = nullptr; cx.S = nullptr; cx.U = nullptr;
  cx.bconf = bconf;
  cx.bb = bconf * bconf;
  cx.cS = cx.cU = cx.cB = 0;
  cx.rmax = -1.0;
  cx.role = ROLE;
  cx.lds_bits = bits;
  cx.umin = 1e300;
  cx.xmin = 1e300;
  cx.vminS = 1e300;
  cx.skip_store = true;
#pragma unroll
  for (int s2 = 0; s2 < 8; ++s2) cx.bw[s2] = 0u;
  cx.gb_on = ROLE == 1 && gb != nullptr;
  cx.lband = cx.gb_on ? lcb_band(cx.bb, gb->dm[1], gb->dv[1]) : LcbBand{0.0, 0.0};
  const unsigned int col_in = cx.lane & 15, row_in = cx.lane >> 4;
  const double* const mo = mean + (size_t)o * cs.n_local;
  const double* const vo = var + (size_t)o * cs.n_local;
  double mv[4][8], vr[4][8];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const unsigned int line = (unsigned int)(cx.rb0 + cx.wave) * 16u + 4u * t + row_in;
    const size_t g0 = (size_t)line * cx.ucnt0 + (unsigned int)cx.cs0 * 16u + col_in;
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2) {
      mv[t][s2] = mo[g0 + s2 * 16];
      vr[t][s2] = vo[g0 + s2 * 16];
    }
  }
  if (ROLE == 2) {
    // the thread's own S bits: rows 16 wave + 4 t + (lane >> 4) of the segment, column (cs0 + s2) 16 + (lane & 15)
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2) {
      const unsigned long long w = px.cb.Sw[(size_t)by * cx.ucnt0 + (unsigned int)(cx.cs0 + s2) * 16u + col_in];
      cx.bw[s2] = (unsigned int)(w >> (16 * cx.wave + (int)row_in)) & 0x1111u;
    }
  }
#ifdef SBO_PHASE_CLOCKS
  {
    double sum_ = 0.0;                                    // (a use of every value: the clock below is read behind the loads)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int s2 = 0; s2 < 8; ++s2) sum_ += mv[t][s2] + vr[t][s2];
    if (__syncthreads_or(sum_ == 0x1p-1070 ? 1 : 0) == 0) clk_ld_ = wall_clock64();
  }
#endif
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (ROLE == 1) {
      post_classify_row(cx, 4u * t + row_in, mv[t], vr[t]);
    } else {
#pragma unroll
      for (int s2 = 0; s2 < 8; ++s2) post_objective(cx, ((cx.bw[s2] >> (4 * t)) & 1u) != 0u, mv[t][s2], vr[t][s2]);
    }
  }
  if (ROLE == 1) {
    // (|S| / |U| and the wave's 16-row pieces of every column: as the epilogue of k_bpost<1, 1>)
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2) { cx.cS += __popc(cx.bw[s2] & 0xffffu); cx.cU += __popc(cx.bw[s2] >> 16); }
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2) {
      unsigned int w = cx.bw[s2];
      w |= (unsigned int)__shfl_xor((int)w, 16);
      w |= (unsigned int)__shfl_xor((int)w, 32);
      if (cx.lane < 16) bits[cx.wave * 128 + s2 * 16 + cx.lane] = w;
    }
  }
  const double gmax = ROLE == 1 ? lrec[ctile] : 0.0;
  post_partials<4>(sh, cx.lane, cx.wave, gmax, ROLE == 1, cx.cS, cx.cU, ROLE == 2 ? -cx.umin : cx.rmax, cx.cB, cx.vminS,
                   Lpart + ((size_t)o * tgy + by) * tgx + bx, cpart + (ROLE == 2 ? ntile : (size_t)0) + ctile, pcap, ROLE == 2, px.cb.slots,
                   (int)(ctile & (kColSlots - 1)), o, ROLE == 1 ? (int)by : -1, (int)bx, cx.xmin, false);
  if (ROLE == 1 && cx.tid < 128) {
    unsigned long long sw = 0ull, uw = 0ull;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const unsigned int pc = bits[w * 128 + cx.tid];
      sw |= (unsigned long long)(pc & 0xffffu) << (16 * w);
      uw |= (unsigned long long)(pc >> 16) << (16 * w);
    }
    const size_t col = (size_t)cx.cs0 * 16u + cx.tid;
    px.cb.Sw[(size_t)by * cx.ucnt0 + col] = sw;
    px.cb.Uw[(size_t)by * cx.ucnt0 + col] = uw;
    if (uw != 0ull) atomicOr(&px.cb.Usum[col], 1ull << by);
  }
#ifdef SBO_PHASE_CLOCKS
  __syncthreads();
  if (threadIdx.x == 0) wg_trace_row(o, clk_in_, clk_ld_, wall_clock64(), (unsigned int)ctile, 4u);
#endif
}

// post_classify_row for ONE candidate (k_bhead: a lane holds one candidate of an 8 x 8 cell): the same sign test, the same fallback
// through the IEEE root for what the predicates leave open, the same band test, and for a safe candidate the same variance, range and
// radius arithmetic -- statement for statement the row form's, which stays as it is (k_bpost's and k_bres' code objects do not move).
// The radius filter compares against the LANE's running maximum instead of a thread's over 32 candidates: it only ever skips a
// candidate whose upper bound cannot raise the maximum, so the maximum over any set of candidates is the same whatever the order.
struct CandAcc { double vminS, xmin, rmax; };           // (1e300, 1e300, -1: none)
__device__ __forceinline__ void post_classify_cand(double m, double v, double bconf, double bb, bool gb_on, const LcbBand& lband, bool& ge_out,
                                                   bool& le_out, bool& near_out, CandAcc& a) {
  constexpr double c = 1.0 + 0x1p-48, tiny = 1e-250, huge = 1e300;
  const bool bok = bconf >= 0.0;
  const double P = m * m, Q = bb * v;
  near_out = false;
  if (gb_on) {
    const double gap = P > Q ? P - Q : Q - P, am = m < 0 ? -m : m;
    near_out = !(gap > fma(am, lband.c1, lband.c0));                     // (NaN operands count as near)
  }
  const bool ok = bok && v >= 0.0, rng = P < huge && Q < huge;
  const bool neg = ok && m < 0.0;
  bool ge = ok && !neg && rng && P > tiny && P >= Q * c;
  bool le = neg || (ok && rng && !ge && Q > tiny && P * c <= Q && m >= 0.0);
  if (!ge && !le) {
    const double sd = mul_rn(bconf, sqrt_rn(v));
    ge = m >= sd;
    le = m <= sd;
  }
  if (ge) {
    a.vminS = v < a.vminS ? v : a.vminS;
    const float sf = __builtin_amdgcn_sqrtf((float)v);
    const double s_up = (double)sf * (1.0 + 0x1p-20) + 1e-18;
    double s_lo = (double)sf * (1.0 - 0x1p-20) - 1e-18;
    s_lo = s_lo > 0.0 ? s_lo : 0.0;
    const bool fin = sf < 3.0e38f;
    const double xu = m + bconf * s_up, xl = m + bconf * (fin ? s_lo : 0.0);
    const double up = fin ? xu + (xu < 0 ? -xu : xu) * 0x1p-50 : 1e300, lo = xl - (xl < 0 ? -xl : xl) * 0x1p-50;
    a.xmin = lo < a.xmin ? lo : a.xmin;
    if (!(up <= a.rmax)) {
      const double ucb = add_rn(m, mul_rn(bconf, sqrt_rn(v)));
      if (ucb > a.rmax) a.rmax = ucb;
    }
  }
  ge_out = ge;
  le_out = le;
}

// Option k1_cells: the head of a lean-2 column-path sweep on a resident plan (res_c: the plan's Lipschitz rows and the constraint's
// stored values stand) in ONE launch -- k_bl_sched_tiles1's tile decision and, for the tiles it would have listed, k_bres<1>'s
// classification, cell by cell.  encl_unsafe / encl_safe are statements about a CELL (8 x 8 candidates); the boundary of S is a curve, so
// of the 128 cells of a tile it crosses most are proved one way or the other by the enclosure the deciding wave holds anyway.  A cell
// proved unsafe is its 64 U bits and 64 to |U|; a cell proved safe (k1_skip_safe) its 64 S bits, 64 to |S|, its smallest stored variance
// (exact) and the ends of encl_keys (bounds: see EnclKeys); nothing of either is counted in the band -- exactly what the predicates
// prove post_classify_row does with every candidate of the box.  Only the other cells -- undecided, NaN enclosures, b < 0 -- load
// their 64 stored mean / var pairs and classify them (post_classify_cand).  This rests on invariant 2 at k_bl_enclose harder than
// anything before: the stored values must be the plan's bits, inside the recorded enclosures bit for bit (the audit checks both).
// Shape: a resident-sized grid of kHeadWaves-wave workgroups; in a round wave w DECIDES tile (kHeadWaves round + w) gridDim + block --
// a stride of gridDim tiles apart, so the tiles of a workgroup are not neighbours on the grid (the boundary runs through neighbours:
// what the shard rotation of the tile list was for).  Classes 0 and 4 are written by that wave as k_bl_sched_tiles1 writes them.  For
// any other tile it builds the column words of the proved cells from four ballots, puts them in LDS and queues the undecided (tile,
// cell) pairs; behind a barrier EVERY wave drains the queue, kHeadBatch cells to a batch, all loads of a batch requested before the
// first is used, a lane per candidate (row lane & 7, column lane >> 3 of the cell: a ballot IS the cell's eight column bytes).  A
// cell owns one byte of each of its eight column words, so the bytes are plain LDS stores; counts and keys join the tile's record in
// LDS by integer adds and min / max of ordered keys whenever a wave moves on to another tile.  A tile with all 128 cells undecided
// costs its workgroup 32 batches over four waves -- what k_bres<1> costs --, not four times that.  Behind a second barrier the
// deciding wave writes the tile's words, Usum bits, Lipschitz row, partial row and row-mask bit; the slot scalars of all the
// workgroup's tiles are merged in LDS and join ONE slot (sums, minima, maxima: the slot does not change them; what un-merged atomics
// cost: k_bl_sched_tiles1).  No list, no fence, no ticket; no result depends on the order of anything.
constexpr int kHeadWaves = 4, kHeadBatch = 4;
struct HeadRec { unsigned int cS, cU, cB, ncell; unsigned long long vmin, rmax, xmin; };
__global__ __launch_bounds__(64 * kHeadWaves) void k_bhead(const double* __restrict__ encl, int ntiles, int tgx, int tgy, unsigned int cnt0, double bconf,
                                                           const GuardBand* __restrict__ gb, const double* __restrict__ mean1,
                                                           const double* __restrict__ var1 /* output 1's stored values */,
                                                           uint8_t* __restrict__ skip, unsigned long long* __restrict__ Sw,
                                                           unsigned long long* __restrict__ Uw, unsigned long long* __restrict__ Usum,
                                                           unsigned long long* __restrict__ slots, double* __restrict__ Lpart,
                                                           unsigned long long* __restrict__ cpart, int pcap, int skip_safe,
                                                           const double* __restrict__ lrec) {
  __shared__ unsigned long long sh_w[kHeadWaves][2][128];    // a mixed tile's S / U column words
  __shared__ unsigned short sh_q[kHeadWaves * 128];          // undecided cells: (wave that decided the tile) << 7 | cell
  __shared__ HeadRec sh_rec[kHeadWaves];
  __shared__ unsigned int sh_xy[kHeadWaves];                 // the tile's bx | by << 16
  __shared__ unsigned int sh_qn;
  __shared__ unsigned long long sh_acc[kHeadWaves][10];
  const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6);
  const unsigned long long below = (1ull << lane) - 1ull;
  const double bb = bconf * bconf;
  const bool gb_on = gb != nullptr;
  const LcbBand lb = gb_on ? lcb_band(bb, gb->dm[1], gb->dv[1]) : LcbBand{0.0, 0.0};
  // the wave's share of the slot scalars, over its tiles of every round (wave-uniform)
  unsigned long long a_key = 0ull, a_vmin = ~0ull, a_rmax = 0ull;
  unsigned int a_S = 0u, a_U = 0u, a_B = 0u, a_n0 = 0u, a_n4 = 0u, a_res = 0u, a_cells = 0u;      // (a wave's tiles: far below 2^32 candidates)
#ifdef SBO_PHASE_CLOCKS
  const unsigned long long clk_in_ = wall_clock64();        // (g_wg_trace: kind 5 = the head launch, [1] = the first round's decisions are made)
  unsigned long long clk_dec_ = clk_in_;
  unsigned int clk_tile_ = 0xffffffu;
#endif
  const int per_round = kHeadWaves * (int)gridDim.x;
  for (int t0 = 0; t0 < ntiles; t0 += per_round) {          // (uniform over the workgroup: the barriers below are met by all)
    const int tile = t0 + wave * (int)gridDim.x + (int)blockIdx.x;
    const bool have = tile < ntiles;                        // (a whole wave or none of it)
    if (threadIdx.x == 0) sh_qn = 0u;
    __syncthreads();
    bool mixed = false;
    int bx = 0, by = 0;
    double lrow = 0.0;
    if (have) {
      bx = tile % tgx;
      by = tile / tgx;
      lrow = lrec[tile];
      a_key = (unsigned long long)__double_as_longlong(lrow) > a_key ? (unsigned long long)__double_as_longlong(lrow) : a_key;
      bool us[2], sf[2];
      double kv = 1e300, ku = -1.0, kl = 1e300;             // (the keys of the cells proved safe: encl_keys)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const double4 e = reinterpret_cast<const double4*>(encl)[(size_t)tile * 128 + h * 64 + lane];
        us[h] = encl_unsafe(e.x, e.y, e.z, e.w, bconf, bb, gb_on, lb);
        sf[h] = skip_safe != 0 && !us[h] && encl_safe(e.x, e.y, e.z, e.w, bconf, bb, gb_on, lb);
        if (sf[h]) {
          const EnclKeys ek = encl_keys(e.x, e.y, e.z, e.w, bconf);
          kv = ek.vlo < kv ? ek.vlo : kv;
          ku = ek.up > ku ? ek.up : ku;
          kl = ek.lo < kl ? ek.lo : kl;
        }
      }
      const unsigned long long mU[2] = {__ballot(us[0]), __ballot(us[1])}, mS[2] = {__ballot(sf[0]), __ballot(sf[1])};
      const bool dec = (mU[0] & mU[1]) == ~0ull, sdec = (mS[0] & mS[1]) == ~0ull;
      const size_t w0 = (size_t)by * cnt0 + (size_t)bx * 128;
      if (lane == 0) {
        skip[tile] = dec ? kSkipUnsafe : (sdec ? kSkipSafe : 0);
        Lpart[((size_t)tgy + by) * tgx + bx] = lrow;
      }
      if (!dec) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double ov = __shfl_xor(kv, off), ou = __shfl_xor(ku, off), ol = __shfl_xor(kl, off);
          kv = ov < kv ? ov : kv;
          ku = ou > ku ? ou : ku;
          kl = ol < kl ? ol : kl;
        }
      }
      const unsigned long long kvmin = kv < 1e300 ? ord_key(kv) : ~0ull, krmax = ku >= 0.0 ? ord_key(ku) : 0ull, kxmin = kl < 1e300 ? ord_key(kl) : ~0ull;
      if (dec) {
        // (class 0, as k_bl_sched_tiles1 writes it: every U bit, its bit of Usum in its 128 columns, |U| = 8192, no keys)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          Sw[w0 + h * 64 + lane] = 0ull;
          Uw[w0 + h * 64 + lane] = ~0ull;
          atomicOr(&Usum[(size_t)bx * 128 + h * 64 + lane], 1ull << by);      // (no return value: the wave does not wait for it)
        }
        if (lane < kFuseRow) {
          unsigned long long v = 0ull;
          if (lane == 0) v = ~0ull;
          else if (lane == 2) v = 64ull * 128ull;
          else if (lane >= kFuseVmin && lane < kFuseRmax) v = ~0ull;
          cpart[(size_t)lane * pcap + tile] = v;
        }
        a_n0 += 1u;
      } else if (sdec) {
        // (class 4, as k_bl_sched_tiles1 writes it: every S bit, no U bit, its bit of the row mask, |S| = 8192, the keys of encl_keys)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          Sw[w0 + h * 64 + lane] = ~0ull;
          Uw[w0 + h * 64 + lane] = 0ull;
        }
        if (lane == 0) atomicOr(&slots[(size_t)kSlotRowMask * kColSlots + by], 1ull << bx);      // (no return value)
        if (lane < kFuseRow) {
          unsigned long long v = 0ull;
          if (lane == 0) v = kxmin;
          else if (lane == 1) v = 64ull * 128ull;
          else if (lane >= kFuseVmin && lane < kFuseRmax) v = lane == kFuseVmin + 1 ? kvmin : ~0ull;
          else if (lane == kFuseRmax + 1) v = krmax;
          cpart[(size_t)lane * pcap + tile] = v;
        }
        a_n4 += 1u;
        a_vmin = kvmin < a_vmin ? kvmin : a_vmin;
        a_rmax = krmax > a_rmax ? krmax : a_rmax;
      } else {
        mixed = true;
        // the proved cells' bytes of the column words (cell 16 cr + cc is lane 16 (cr & 3) + cc of ballot cr >> 2); an undecided cell's
        // byte is zero until the wave that classifies the cell stores it
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int cc = (h * 64 + lane) >> 3;
          unsigned long long sw = 0ull, uw = 0ull;
#pragma unroll
          for (int cr = 0; cr < 8; ++cr) {
            const int bit = 16 * (cr & 3) + cc;
            sw |= ((mS[cr >> 2] >> bit) & 1ull) ? 0xffull << (8 * cr) : 0ull;
            uw |= ((mU[cr >> 2] >> bit) & 1ull) ? 0xffull << (8 * cr) : 0ull;
          }
          sh_w[wave][0][h * 64 + lane] = sw;
          sh_w[wave][1][h * 64 + lane] = uw;
        }
        const unsigned long long mN[2] = {~(mU[0] | mS[0]), ~(mU[1] | mS[1])};
        const unsigned int n0 = (unsigned int)__popcll(mN[0]), n1 = (unsigned int)__popcll(mN[1]);
        unsigned int base = 0u;
        if (lane == 0) {
          base = atomicAdd(&sh_qn, n0 + n1);
          sh_rec[wave] = HeadRec{64u * (unsigned int)(__popcll(mS[0]) + __popcll(mS[1])), 64u * (unsigned int)(__popcll(mU[0]) + __popcll(mU[1])), 0u,
                                 n0 + n1, kvmin, krmax, kxmin};
          sh_xy[wave] = (unsigned int)bx | ((unsigned int)by << 16);
        }
        base = (unsigned int)__shfl((int)base, 0);
        if ((mN[0] >> lane) & 1ull) sh_q[base + (unsigned int)__popcll(mN[0] & below)] = (unsigned short)((wave << 7) | lane);
        if ((mN[1] >> lane) & 1ull) sh_q[base + n0 + (unsigned int)__popcll(mN[1] & below)] = (unsigned short)((wave << 7) | (64 + lane));
      }
    }
    __syncthreads();
#ifdef SBO_PHASE_CLOCKS
    if (t0 == 0) clk_dec_ = wall_clock64();
    if (mixed && clk_tile_ == 0xffffffu) clk_tile_ = (unsigned int)tile;
#endif
    {
      // every wave drains the queue: batch i goes to wave i mod kHeadWaves
      const unsigned int nq = sh_qn;
      const unsigned int r8 = (unsigned int)lane & 7u, c8 = (unsigned int)lane >> 3;
      CandAcc acc{1e300, 1e300, -1.0};
      unsigned int cS = 0u, cU = 0u, cB = 0u;
      int cur = -1;
      auto flush = [&]() {
        if (cur < 0) return;
        double vm = acc.vminS, xm = acc.xmin, rm = acc.rmax;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double ov = __shfl_xor(vm, off), ox = __shfl_xor(xm, off), orr = __shfl_xor(rm, off);
          vm = ov < vm ? ov : vm;
          xm = ox < xm ? ox : xm;
          rm = orr > rm ? orr : rm;
        }
        if (lane == 0) {
          HeadRec& r = sh_rec[cur];
          if (cS) atomicAdd(&r.cS, cS);
          if (cU) atomicAdd(&r.cU, cU);
          if (cB) atomicAdd(&r.cB, cB);
          if (vm < 1e300) atomicMin(&r.vmin, ord_key(vm));
          if (xm < 1e300) atomicMin(&r.xmin, ord_key(xm));
          if (rm >= 0.0) atomicMax(&r.rmax, ord_key(rm));
        }
        acc = CandAcc{1e300, 1e300, -1.0};
        cS = cU = cB = 0u;
      };
      for (unsigned int b0 = (unsigned int)wave * kHeadBatch; b0 < nq; b0 += kHeadWaves * kHeadBatch) {
        unsigned int ent[kHeadBatch];
        double m[kHeadBatch], v[kHeadBatch];
#pragma unroll
        for (int k = 0; k < kHeadBatch; ++k) {
          // (past the end of the queue: the batch's first entry again -- a load nobody uses, inside the grid)
          ent[k] = (unsigned int)__builtin_amdgcn_readfirstlane((int)sh_q[b0 + k < nq ? b0 + k : b0]);
          const unsigned int xy = (unsigned int)__builtin_amdgcn_readfirstlane((int)sh_xy[ent[k] >> 7]), cell = ent[k] & 127u;
          const size_t g = ((size_t)(xy >> 16) * 64 + (size_t)(cell >> 4) * 8 + r8) * cnt0 + (size_t)(xy & 0xffffu) * 128 + (size_t)(cell & 15u) * 8 + c8;
          m[k] = mean1[g];
          v[k] = var1[g];
        }
#pragma unroll
        for (int k = 0; k < kHeadBatch; ++k) {
          if (b0 + k < nq) {
            const int w = (int)(ent[k] >> 7);
            const unsigned int cell = ent[k] & 127u;
            if (w != cur) {
              flush();
              cur = w;
            }
            bool ge, le, nr;
            post_classify_cand(m[k], v[k], bconf, bb, gb_on, lb, ge, le, nr, acc);
            const unsigned long long gm = __ballot(ge), lm = __ballot(le);
            cS += (unsigned int)__popcll(gm);
            cU += (unsigned int)__popcll(lm);
            cB += (unsigned int)__popcll(__ballot(nr));
            // (byte c of a ballot: column c of the cell, rows 0..7 -- bits 8 (cell >> 4) .. + 7 of that column's word)
            if (lane < 16) {
              const unsigned long long bits = lane < 8 ? gm : lm;
              reinterpret_cast<unsigned char*>(&sh_w[w][lane >> 3][(cell & 15u) * 8 + (lane & 7)])[cell >> 4] = (unsigned char)(bits >> (8 * (lane & 7)));
            }
          }
        }
      }
      flush();
    }
    __syncthreads();
    if (mixed) {
      // the deciding wave writes what the tile's workgroup wrote (k_bres<1>: words, Usum, post_partials' row and scalars)
      const size_t w0 = (size_t)by * cnt0 + (size_t)bx * 128;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const unsigned long long sw = sh_w[wave][0][h * 64 + lane], uw = sh_w[wave][1][h * 64 + lane];
        Sw[w0 + h * 64 + lane] = sw;
        Uw[w0 + h * 64 + lane] = uw;
        if (uw != 0ull) atomicOr(&Usum[(size_t)bx * 128 + h * 64 + lane], 1ull << by);
      }
      const HeadRec r = sh_rec[wave];
      if (lane == 0 && r.cS != 0u) atomicOr(&slots[(size_t)kSlotRowMask * kColSlots + by], 1ull << bx);
      if (lane < kFuseRow) {
        unsigned long long v = 0ull;
        if (lane == 0) v = r.xmin;
        else if (lane == 1) v = r.cS;
        else if (lane == 2) v = r.cU;
        else if (lane == 3) v = r.cB;
        else if (lane >= kFuseVmin && lane < kFuseRmax) v = lane == kFuseVmin + 1 ? r.vmin : ~0ull;
        else if (lane == kFuseRmax + 1) v = r.rmax;
        cpart[(size_t)lane * pcap + tile] = v;
      }
      a_S += r.cS;
      a_U += r.cU;
      a_B += r.cB;
      a_res += 1u;
      a_cells += r.ncell;
      a_vmin = r.vmin < a_vmin ? r.vmin : a_vmin;
      a_rmax = r.rmax > a_rmax ? r.rmax : a_rmax;
    }
  }
  if (lane == 0) {
    unsigned long long* a = sh_acc[wave];
    a[0] = a_key; a[1] = (unsigned long long)a_S + 64ull * 128ull * a_n4; a[2] = (unsigned long long)a_U + 64ull * 128ull * a_n0; a[3] = a_B; a[4] = a_n0; a[5] = a_n4;
    a[6] = a_res; a[7] = a_cells;
    a[8] = a_vmin; a[9] = a_rmax;
  }
  __syncthreads();
  if (threadIdx.x < 10) {
    const int f = (int)threadIdx.x;
    unsigned long long x = sh_acc[0][f];
#pragma unroll
    for (int w = 1; w < kHeadWaves; ++w) {
      const unsigned long long y = sh_acc[w][f];
      x = f == 8 ? (y < x ? y : x) : ((f == 0 || f == 9) ? (y > x ? y : x) : x + y);
    }
    const int slot = (int)(blockIdx.x & (kColSlots - 1));
    const int field = f == 0 ? kSlotL1 : f == 1 ? kSlotS : f == 2 ? kSlotU : f == 3 ? kSlotB : f == 4 ? kSlotSkip : f == 5 ? kSlotSkipSafe :
                      f == 6 ? kSlotResC : f == 7 ? kSlotCells : f == 8 ? kSlotVmin1 : kSlotRmax1;
    unsigned long long* p = &slots[(size_t)field * kColSlots + slot];
    // (no return values: nobody waits for them)
    if (f == 8) { if (x != ~0ull) atomicMin(p, x); }
    else if (f == 0 || f == 9) { if (x != 0ull) atomicMax(p, x); }
    else if (x != 0ull) atomicAdd(p, x);
  }
#ifdef SBO_PHASE_CLOCKS
  if (threadIdx.x == 0) wg_trace_row(1, clk_in_, clk_dec_, wall_clock64(), clk_tile_, 5u);
#endif
}


// K1i's deferred gradient launch (r05): the two gradient series of every output on the tiles the gate names, nothing else -- on
// stream3 behind the gate's kernels, beside the posterior launches, which then carry no gradient phases (PostExtra::nograd).  A
// resident-sized grid walks the (output, tile) table: a tile the gate excludes costs two loads, and its row of the Lipschitz partials
// holds its largest coarse sample as before.  Rows [q][tiles] as k_bpost writes them; column path: the workgroup's maximum per output
// also joins the slot block.
__global__ __launch_bounds__(256, 3) void k_bgrad(const ModelConst mc, const CandSpec cs, const double* __restrict__ VA, size_t sVA,
                                                  const double* __restrict__ P0f, int KB, int nrb, int ncs, long long nlines, int gx, int gy,
                                                  const int* __restrict__ eff, const double* __restrict__ gtmax,
                                                  const unsigned long long* __restrict__ gkey, const double* __restrict__ xn0, int q,
                                                  double* __restrict__ Lpart, unsigned long long* __restrict__ slots,
                                                  int o_first /* 1: a lean sweep -- nobody reads the objective's key, its rows stay zero */) {
  extern __shared__ double lds[];
  PostCtx cx;
  cx.lds = lds;
  cx.tid = threadIdx.x; cx.lane = cx.tid & 63; cx.wave = cx.tid >> 6;
  cx.nrb = nrb; cx.ncs = ncs;
  cx.ucnt0 = (unsigned int)cs.count[0];
  cx.nlines = nlines;
  cx.imode = true;
  const int st_i = cx.tid >> 5, st_j = cx.tid & 31;
  cx.st_off = st_j * 8;
  cx.a_lo = st_i < 4 ? st_i * 256 + (st_j >> 3) * 64 + (st_j & 7) * 4 : -1;
  cx.b_st = 1024 + st_i * 256 + cx.st_off;
  cx.a_rd = (((cx.lane >> 4) << 2) + (cx.lane & 3)) * 2;
  cx.var_rd = nullptr; cx.S = nullptr; cx.U = nullptr;
  cx.bconf = 0.0; cx.bb = 0.0; cx.cS = cx.cU = cx.cB = 0; cx.rmax = -1.0;
  cx.lband = LcbBand{0.0, 0.0}; cx.gb_on = false; cx.vminS = 1e300;
  cx.role = 0; cx.lds_bits = nullptr; cx.umin = 1e300; cx.xmin = 1e300; cx.skip_store = false;
#pragma unroll
  for (int s2 = 0; s2 < 8; ++s2) cx.bw[s2] = 0u;
  const size_t nt = (size_t)gx * gy;
  const double* slack = gtmax ? gtmax + (size_t)q * 2 * nt : nullptr;       // (no gate: every tile runs both phases)
  d4_t acc[1][8];
  d4_t pre[4];
  for (size_t tile = blockIdx.x; o_first > 0 && tile < nt; tile += gridDim.x)
    if (cx.tid == 0) Lpart[tile] = 0.0;
  for (int o = o_first; o < q; ++o) {
    const double ystd = mc.Y_std[o];
    const double cg0 = ystd * mc.inv_ell[o][0] * mc.X_rstd[0], cg1 = ystd * mc.inv_ell[o][1] * mc.X_rstd[1];
    const double G0 = gtmax ? __longlong_as_double((long long)gkey[2 * o + 0]) : 0.0, G1 = gtmax ? __longlong_as_double((long long)gkey[2 * o + 1]) : 0.0;
    const double s0 = gtmax ? slack[2 * o + 0] : 0.0, s1 = gtmax ? slack[2 * o + 1] : 0.0;
    const int KS2 = eff[4 * (4 * o + 2)], KS3 = eff[4 * (4 * o + 3)];
    const double* VAo = VA + (size_t)o * sVA;
    const double* A2 = VAo + (size_t)nrb * KB * 256;
    const double* A3 = VAo + (size_t)nrb * (2 * KB) * 256;
    double wg_max = 0.0;
    for (size_t tile = blockIdx.x; tile < nt; tile += gridDim.x) {
      const double t0 = gtmax ? gtmax[((size_t)o * 2 + 0) * nt + tile] : 0.0, t1 = gtmax ? gtmax[((size_t)o * 2 + 1) * nt + tile] : 0.0;
      const bool run2 = !(t0 + s0 < G0 * (1.0 - 1e-12)), run3 = !(t1 + s1 < G1 * (1.0 - 1e-12));          // (NaN: run)
      double g = fmax(fabs(cg0 * t0), fabs(cg1 * t1));
      if (run2 || run3) {
        const int bx = (int)(tile % (size_t)gx), by = (int)(tile / (size_t)gx);
        cx.rb0 = by * 4; cx.cs0 = bx * 8;
        cx.full = (long long)(cx.rb0 + 4) * 16 <= nlines && (long long)(cx.cs0 + 8) * 16 <= cs.count[0];
        cx.st_rb = cx.rb0 + st_i < nrb ? cx.rb0 + st_i : nrb - 1;
        cx.st_cs = cx.cs0 + st_i < ncs ? cx.cs0 + st_i : ncs - 1;
        double gmax = 0.0;
        if (run2) post_phase<2, 1, 0>(cx, A2, P0f, KB, KS2, nullptr, cg0, 0.0, 0.0, gmax, acc, xn0, pre, nullptr, nullptr, 0);
        if (run3) post_phase<3, 1, 0>(cx, A3, P0f, KB, KS3, nullptr, cg1, 0.0, 0.0, gmax, acc, xn0, pre, nullptr, nullptr, 0);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double other = __shfl_xor(gmax, off);
          gmax = other > gmax ? other : gmax;
        }
        __syncthreads();
        if (cx.lane == 0) lds[cx.wave] = gmax;
        __syncthreads();
        gmax = fmax(fmax(lds[0], lds[1]), fmax(lds[2], lds[3]));
        __syncthreads();
        g = fmax(g, gmax);
      }
      if (cx.tid == 0) Lpart[(size_t)o * nt + tile] = g;
      wg_max = fmax(wg_max, g);
    }
    if (slots && cx.tid == 0)
      atomicMax(&slots[(size_t)(o == 0 ? kSlotL0 : kSlotL1) * kColSlots + (blockIdx.x & (kColSlots - 1))], (unsigned long long)__double_as_longlong(wg_max));
  }
}

// Lipschitz keys of a K1b launch: Lmax[o] = max of the per-wave partials (values >= 0, so the bit pattern orders them)
__global__ __launch_bounds__(256) void k_lmax_reduce(const double* __restrict__ Lpart, int per_out, unsigned long long* __restrict__ Lmax) {
  __shared__ double sh[4];
  lmax_reduce_body((int)blockIdx.x, sh, Lpart, per_out, Lmax);
}

// Column path (r05): can this launch deliver the classification as column words?  One constraint, fp64 grid of whole 64 x 128
// tiles (every workgroup's tile inside the grid), at most 64 segments (Usum is one word per column); the sweep asked for it.
static bool col_words_ok(const sbo_ctx* c, const PostRequest& req, long long cnt0, long long nlines) {
  if (!req.col || !c->opt.col_path) return false;
  const bool shape = c->mc.q == 2 && c->cs.kind == 1 && c->cs.d == 2 && c->cs.first == 0 && cnt0 % 128 == 0 && nlines % 64 == 0 &&
                     nlines / 64 <= 64 && nlines >= 64 && cnt0 >= 128 && cnt0 <= 4096 && c->dist.world == 1 && !c->opt.comm_selftest;
  // (auto: from four tiles per CU and output on -- config H.  Below that the two launches per sweep cost more than the column
  // kernels save: config B, 512 tiles per output, 0.171 ms against 0.162 with the byte masks.  Option col_path = 2: whenever the shape fits.)
  const long long tiles = (cnt0 / 128) * (nlines / 64);
  return shape && (c->opt.col_path == 2 || tiles >= 4ll * c->n_cu);
}
static_assert(kFuseRmax + 1 == kColRowRmax1, "ColPartRows::tumax is the radius key of constraint 1");

// ---- launch_posterior_gemm: the GEMM posterior on the operands of a plan -- K1i's when `interp`, else K1b's: stage 1, the k_bpost launches
// and the Lipschitz tail.  Only K1i has the deferred gradient launch (k_bgrad on stream3); only K1b the column path's enclosures and tile
// lists (r06, r07).  A driver over the steps below, which hand each other a GemmLaunch; what is enqueued, with which arguments, on which
// stream and in which order does not depend on how the steps are cut.
struct GemmLaunch {
  sbo_ctx* c;
  bool interp;
  const PostRequest& req;
  PostOutcome& out;
  const GemmOps& g;
  int q;
  long long cnt0, nlines;
  bool defer;                 // K1i: the posterior launches write their -- empty -- Lipschitz rows behind the real ones, which the gradient launch fills
  bool run_stage1;
  unsigned gx = 0, gy = 0, rows_out = 0;      // the tile grid; partial rows per output: one per workgroup
  size_t lds = 0, ntiles = 0;
  bool fuse = false, colw = false;            // classification as S / U bytes | as column words (never both)
  PostExtra px;
  double* encl = nullptr;                     // column path, K1b: the plan's enclosures; this launch records them | a lean-2 launch uses them (px.encl)
  bool record_encl = false;
  // option k1_resident (BilinearPlan::lrows_ready / omap_dirty; sbo_ctx::bl_res)
  double* lrec = nullptr;                     // the plan's rows of output 1: recorded with the enclosures | read by k_bl_sched_tiles1 and k_bres<1> (res_rows)
  uint8_t* omap = nullptr;                    // the objective's residency bytes; nullptr: the option is off
  bool res_rows = false;                      // k_bl_sched_tiles1 takes the Lipschitz rows from lrec and lists no tile for its gradient phases
  bool res_c = false, res_o = false;          // the constraint's listed tiles go to k_bres<1> | the objective's list is split, its back goes to k_bres<2>
  unsigned int *sched_l1 = nullptr, *sched_l2 = nullptr;      // the tile lists of the constraint's launch (kTlistShards shards of sched_cap1) and the objective's
  int sched_cap1 = 0;
  const GuardBand* gb_fused = nullptr;        // the fused classification counts its sign tests inside the plan's guard band
  double* lrows = nullptr;
};

// stage 1: Bt = P1^T T4qq^T, written as the packed A operand of stage 2 (three strips per workgroup measured best on
// config B: 27.7 us against 28.8 with two and 31.3 with four; the per-wave k_bgemm<2, 0, 0> took 32.6)
static void gemm_stage1(const GemmLaunch& L) {
  constexpr int S1 = 3;
  sbo_ctx* c = L.c;
  const GemmOps& g = L.g;
  const dim3 grid((unsigned)((g.KB0 + S1 - 1) / S1), (unsigned)((g.nrb + 3) / 4), (unsigned)(g.sets * L.q));
  if (L.defer)
    hipExtLaunchKernelGGL((k_bstage1<S1>), grid, dim3(256), 0, c->stream, nullptr, c->ev_grad[1], 0, (const double*)c->bl_P1A.p, g.sP1A,
                          (const double*)c->bl_T4f.p, g.sT4f, g.KB1, g.nrb, g.KB0, g.BtA, g.sBt1, (const int*)g.eff);
  else
    hipLaunchKernelGGL((k_bstage1<S1>), grid, dim3(256), 0, c->stream, (const double*)c->bl_P1A.p, g.sP1A, (const double*)c->bl_T4f.p,
                       g.sT4f, g.KB1, g.nrb, g.KB0, g.BtA, g.sBt1, (const int*)g.eff);
}

// stage 2 (fused): variance, mean, Lipschitz keys.  64 x 128 tiles (k_bpost<1>, three workgroups per CU): with the Chebyshev
// core the variance phase is ~12 k-steps and no longer dominates, and the third workgroup per CU is worth more than the
// B-fragment reuse of a 128 x 128 tile (r03: config B 0.204 -> 0.189 ms per sweep, H 0.547 -> 0.543)
static int gemm_shape(GemmLaunch& L) {
  L.gx = (unsigned)((L.g.ncs0 + 7) / 8);
  L.gy = (unsigned)((L.g.nrb + 3) / 4);
  L.rows_out = L.gx * L.gy;
  L.ntiles = (size_t)L.gx * L.gy;
  L.lds = sizeof(double) * 2 * 3072 + 2048;
  return ensure(L.c->bl_lpart, sizeof(double) * (size_t)L.rows_out * L.q * (L.interp ? 2 : 1));
}

// What the launch classifies, and into what: S / U bytes (`fuse`), column words (`colw`) or nothing; the rows of cpart either form
// writes, and the stride of the byte planes of several constraints.
// A sweep may ask for the S / U bytes, |S|, |U| and the radius key straight from the mean epilogue of the constraint
// (one-constraint models; the masks are allocated by the sweep before it enqueues the posterior)
// (r03: with the sqrt-free sign tests the fused epilogue saves the separate pass 76 us on config H and costs the GEMM 36;
// on config B, two workgroups per CU, the two cancel -- "auto" asks for at least four workgroups per CU)
static int gemm_classify_plan(GemmLaunch& L) {
  sbo_ctx* c = L.c;
  const CandSpec& cs = c->cs;
  const int q = L.q;
  const bool fuse_wanted = L.req.fuse == 1 || (L.req.fuse == 2 && ((long long)L.gx * L.gy * q >= 4ll * c->n_cu || q > 2));   // (several constraints: the separate pass costs more than one constraint's)
  L.fuse = fuse_wanted && q >= 2 && c->maskS.p && c->maskU.p && c->maskS.bytes >= (size_t)cs.n_local && c->maskU.bytes >= (size_t)cs.n_local &&
           (q == 2 || (c->fuseS.bytes >= (size_t)cs.n_local * (q - 1) && c->fuseU.bytes >= (size_t)cs.n_local * (q - 1)));
  L.colw = L.fuse && col_words_ok(c, L.req, L.cnt0, L.nlines);
  memset(&L.px, 0, sizeof(L.px));
  L.px.q = q;
  if (!L.fuse) return SBO_OK;
  L.out.fuse_rows = (int)L.rows_out * (L.colw ? 2 : (q - 1));
  L.px.fstride = q > 2 ? (long long)cs.n_local : 0ll;
  // (room behind the rows for the partials of the objective pass, see sweep_common_front)
  if (int rc = ensure(c->cpart, sizeof(unsigned long long) * kFuseRow * ((size_t)L.out.fuse_rows + 4 * (size_t)c->n_cu + 64))) return rc;
  c->cpart_cap = (int)(c->cpart.bytes / (sizeof(unsigned long long) * kFuseRow));
  if (L.colw) L.out.col_rows = ColPartRows{(unsigned long long*)c->cpart.p, c->cpart_cap, (int)L.rows_out};
  return SBO_OK;
}

// The word buffers, Usum and the slot block of a column-path launch.  The slot block's fill is a host array on this stack: the one
// host wait of the path, on first use or after a sweep that failed.
static int col_words_prepare(sbo_ctx* c, long long cnt0, long long nlines, ColBits* cb) {
  const size_t words = (size_t)(nlines / 64) * (size_t)cnt0;
  int rc;
  if ((rc = ensure(c->col.S, 8 * words)) || (rc = ensure(c->col.U, 8 * words)) || (rc = ensure(c->col.M, 8 * words)) || (rc = ensure(c->col.G, 8 * words))) return rc;
  DevBuf& usum = c->col.Usum.buf;
  if ((rc = c->col.Usum.acquire(8 * (size_t)cnt0, [&]() -> int {
        SBO_HIP(hipMemsetAsync(usum.p, 0, usum.bytes, c->stream));
        return SBO_OK;
      })))
    return rc;
  const size_t sbytes = sizeof(unsigned long long) * kColSlotFields * kColSlots;
  if ((rc = c->col.slots.acquire(sbytes, [&]() -> int {
        unsigned long long init[kColSlotFields * kColSlots];
        for (int f = 0; f < kColSlotFields; ++f)
          for (int k = 0; k < kColSlots; ++k) init[f * kColSlots + k] = col_slot_is_min(f) ? ~0ull : 0ull;
        SBO_HIP(hipMemcpyAsync(c->col.slots.buf.p, init, sbytes, hipMemcpyHostToDevice, c->stream));
        SBO_HIP(hipStreamSynchronize(c->stream));           // (`init` is on this stack)
        return SBO_OK;
      })))
    return rc;
  cb->Sw = (unsigned long long*)c->col.S.p;
  cb->Uw = (unsigned long long*)c->col.U.p;
  cb->Usum = (unsigned long long*)usum.p;
  cb->slots = (unsigned long long*)c->col.slots.buf.p;
  return SBO_OK;
}

// r06: the constraint's enclosures per 8 x 8 cell (per plan) and a skip byte per tile (per sweep); a lean-2 sweep hands them to
// the constraint's launch once the plan's first launch has recorded them.  Leaves the audit its record of this launch (guard.hip).
static int col_enclosures(GemmLaunch& L) {
  sbo_ctx* c = L.c;
  const size_t ebytes = sizeof(double) * 4 * 128 * L.ntiles;
  const void* was = c->bl_encl.p;
  if (int rc = ensure(c->bl_encl, ebytes + L.ntiles)) return rc;
  if (c->bl_encl.p != was) c->bl.encl_ready = false;
  L.encl = (double*)c->bl_encl.p;
  L.record_encl = !c->bl.encl_ready;
  c->k1_audit.encl_tiles = L.ntiles;
  c->k1_audit.encl_check = !L.record_encl;
  if (!L.record_encl && L.req.col_lean >= 2) {
    L.px.encl = L.encl;
    L.px.skip = (uint8_t*)c->bl_encl.p + ebytes;
    L.px.skip_safe = (c->opt.k1_skip_safe && c->bl.vals_ready) ? 1 : 0;     // (a proved-safe tile's stored values are read: internal.hpp)
    c->k1_audit.skip_armed = true;
  }
  return SBO_OK;
}

// r07: lean 2 -- the objective's launch over the tiles with a safe candidate, and, once the enclosures decide skips, the
// constraint's over the tiles that need a workgroup (k_bl_sched_tiles1 and on).  [list 1: kTlistShards shards][list 2: one],
// PostExtra::tlist: the constraint's counters stay at the head of the buffer whatever the grid.
// The counters are zero from the last sweep's k_bl_sched_list2 -- a fill only for a new buffer, or after a sweep that failed or ran no
// lists, and only in front of a k_bl_sched_tiles1 (a launch with enclosures to decide by: nothing else reads them).  Every column-path
// launch takes the block in use; col_set_phase says when a sweep whose k_bl_sched_list2 reset the counters has come through.
static int col_tile_lists(GemmLaunch& L) {
  sbo_ctx* c = L.c;
  if (L.interp || !c->opt.k1_sched || L.req.col_lean < 2) {
    c->bl_sched.in_use();
    return SBO_OK;
  }
  // (of every kTlistShards consecutive tiles a shard gets one)
  L.sched_cap1 = (int)((L.ntiles + kTlistShards - 1) / kTlistShards);
  const size_t words1 = (size_t)kTlistShards * (kTlistHead + (size_t)L.sched_cap1);
  if (int rc = c->bl_sched.acquire(sizeof(unsigned int) * (words1 + kTlistHead + L.ntiles), [&]() -> int {
        if (L.px.encl) SBO_HIP(hipMemsetAsync(c->bl_sched.buf.p, 0, sizeof(unsigned int) * kTlistShards * kTlistHead, c->stream));
        return SBO_OK;
      }))
    return rc;
  L.sched_l1 = (unsigned int*)c->bl_sched.buf.p;
  L.sched_l2 = L.sched_l1 + words1;
  return SBO_OK;
}

// Option k1_resident: what this launch takes from memory, and the plan's record of it (sbo_ctx::bl_res: the rows of output 1, the
// objective's residency bytes).  The rows are recorded with the enclosures whatever the option says -- one store per tile and plan --, so
// that switching it on finds them.  It takes effect on the path that has lists: K1b, lean 2, k1_sched, enclosures recorded.  The bytes
// are kept only while the option is on: a launch without the map rewrites the plan's bits, so bytes that stand stay true, but the tiles
// it stores for the first time go unrecorded -- the map starts again when the option comes back.
static int col_resident(GemmLaunch& L) {
  sbo_ctx* c = L.c;
  const size_t rbytes = sizeof(double) * L.ntiles;
  const void* was = c->bl_res.p;
  if (int rc = ensure(c->bl_res, rbytes + L.ntiles)) return rc;
  if (c->bl_res.p != was) {
    c->bl.lrows_ready = false;
    c->bl.omap_dirty = true;
  }
  L.lrec = (double*)c->bl_res.p;
  if (!c->opt.k1_resident) {
    c->bl.omap_dirty = true;
    return SBO_OK;
  }
  const bool on = L.sched_l1 != nullptr && L.sched_l2 != nullptr && L.px.encl != nullptr;
  L.res_rows = on && c->bl.lrows_ready;
  L.res_c = L.res_rows && c->bl.vals_ready;
  L.res_o = on;
  L.omap = (uint8_t*)c->bl_res.p + rbytes;
  if (c->bl.omap_dirty) {
    SBO_HIP(hipMemsetAsync(L.omap, 0, L.ntiles, c->stream));
    c->bl.omap_dirty = false;
  }
  L.px.omap = L.omap;
  return SBO_OK;
}

// K1i's deferred gradient launch: the gradient phases alone, behind the gate on stream3 and behind stage 1 (its images): one launch for all outputs
static int gemm_grad_deferred(GemmLaunch& L) {
  sbo_ctx* c = L.c;
  const GemmOps& g = L.g;
  hipStream_t gs = c->stream3;
  SBO_HIP(hipStreamWaitEvent(gs, c->ev_grad[1], 0));
  SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_bgrad), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
  hipLaunchKernelGGL(k_bgrad, dim3((unsigned)std::min<long long>((long long)L.rows_out, 2ll * c->n_cu)), dim3(256), L.lds, gs, c->mc, c->cs, g.VA,
                     g.sVA, g.P0f, g.KB0, g.nrb, g.ncs0, L.nlines, (int)L.gx, (int)L.gy, (const int*)g.eff, g.gtmax, g.gkey,
                     (const double*)c->bl_small.p, L.q, L.lrows, L.colw ? L.px.cb.slots : (unsigned long long*)nullptr, (L.req.sweep_lean && L.q >= 2) ? 1 : 0);
  SBO_HIP(hipEventRecord(c->ev_grad[2], gs));
  c->grad_pending = true;
  L.px.nograd = 1;
  return SBO_OK;
}

// One k_bpost launch: all outputs (part 0 of 1), or on the column path the constraint's (part 0) and then the objective's (part 1), whose
// tiles read the constraint's words and its counts of safe candidates per tile.  In front of it the kernel that builds its tile list (r07:
// on this stream, right in front of the launch that reads the list), behind the constraint's the plan's enclosures where it records them.
// The K1 stop event rides on the last launch (hipExtLaunchKernel): a separate hipEventRecord behind it is a barrier packet
// the next kernel waits ~6 us for.  A sweep merges the Lipschitz partials in its own first small kernel (req.lmax_defer).
static void gemm_post_part(GemmLaunch& L, int part) {
  sbo_ctx* c = L.c;
  const GemmOps& g = L.g;
  const CandSpec& cs = c->cs;
  const bool colw = L.colw, fuse = L.fuse;
  const int q = L.q;
  const ColPartRows& rows = L.out.col_rows;
  PostExtra& px = L.px;
  px.o0 = colw ? 1 - part : 0;
  const bool last = !colw || part == 1;
  const decltype(&k_bpost<1, 0>) kposts[3] = {k_bpost<1, 0>, k_bpost<1, 1>, k_bpost<1, 2>};
  const auto kpost = kposts[colw ? 1 + part : 0];
  px.tlist = nullptr;
  // option k1_cells, a resident plan (res_c): the tile decisions and the listed tiles' classification in ONE launch, per cell, with
  // the fork event -- no list, no k_bres<1>.  Resident-sized: a tile per wave and round, so the deciding waves of a workgroup sit a
  // grid's width of tiles apart.
  const bool head_c = L.res_c && c->opt.k1_cells && L.sched_l1 && part == 0 && px.encl;
  if (head_c) {
    const unsigned nt = L.gx * L.gy;
    const unsigned hgrid = std::max(1u, std::min((nt + kHeadWaves - 1) / kHeadWaves, 4u * (unsigned)c->n_cu));
    hipExtLaunchKernelGGL(k_bhead, dim3(hgrid), dim3(64 * kHeadWaves), 0, c->stream, nullptr, c->col.ev[0], 0, (const double*)px.encl, (int)nt, (int)L.gx,
                          (int)L.gy, (unsigned int)L.cnt0, L.req.fuse_b, L.gb_fused, (const double*)c->mean.p + (size_t)cs.n_local,
                          (const double*)c->var.p + (size_t)cs.n_local, px.skip, px.cb.Sw, px.cb.Uw, px.cb.Usum, px.cb.slots, L.lrows, rows.base,
                          rows.cap, px.skip_safe, (const double*)L.lrec);
  }
  if (L.sched_l1 && part == 0 && px.encl && !head_c) {
    hipLaunchKernelGGL(k_bl_sched_tiles1, dim3((L.gx * L.gy + kSchedWaves - 1) / kSchedWaves), dim3(64 * kSchedWaves), 0, c->stream, c->mc, (const double*)px.encl, (int)(L.gx * L.gy), (int)L.gx,
                       (int)L.gy, (unsigned int)L.cnt0, L.req.fuse_b, L.gb_fused, g.gtmax, g.gkey, q, px.skip, L.sched_l1, L.sched_cap1, px.cb.Sw, px.cb.Uw,
                       px.cb.Usum, px.cb.slots, L.lrows, rows.base, rows.cap, px.skip_safe, L.res_rows ? (const double*)L.lrec : (const double*)nullptr,
                       L.res_c ? 1 : 0);
    px.tlist = L.sched_l1;
    px.tshift = kTlistShift;
    px.tcap = L.sched_cap1;
  }
  if (L.sched_l2 && part == 1) {
    hipLaunchKernelGGL(k_bl_sched_list2, dim3(1), dim3(1024), 0, c->stream, rows.base, rows.cap, (int)(L.gx * L.gy), L.sched_l2,
                       L.lrows, L.sched_l1, L.res_o ? (const uint8_t*)L.omap : (const uint8_t*)nullptr, px.cb.slots);
    px.tlist = L.sched_l2;
    px.tshift = 0;
    px.tcap = (int)(L.gx * L.gy);
    L.out.col_sched = true;
  }
  px.tgx = (int)L.gx;
  px.tgy = (int)L.gy;
  const dim3 grid = px.tlist ? dim3((unsigned)px.tcap << px.tshift) : dim3(L.gx, L.gy, (unsigned)(colw ? 1 : q));
  // option k1_resident.  The constraint's listed tiles from memory: k_bres<1> in place of k_bpost<1, 1>, with its fork event.  The
  // objective's: k_bres<2> over the back of its list first, then k_bpost<1, 2> over the front (empty when nothing changed since the
  // last sweep: its workgroups exit at once), which carries the stop event as before.
  px.front_only = 0;
  const bool light_c = L.res_c && part == 0 && px.tlist != nullptr, light_o = L.res_o && part == 1 && px.tlist != nullptr;
  if (light_c) {
    hipExtLaunchKernelGGL(k_bres<1>, grid, dim3(256), 0, c->stream, nullptr, c->col.ev[0], 0, cs, (const double*)c->mean.p, (const double*)c->var.p,
                          L.lrows, L.req.fuse_b, (unsigned long long*)c->cpart.p, c->cpart_cap, L.gb_fused, (const double*)L.lrec, px);
  }
  if (light_o) {
    hipLaunchKernelGGL(k_bres<2>, grid, dim3(256), 0, c->stream, cs, (const double*)c->mean.p, (const double*)c->var.p, L.lrows, L.req.fuse_b,
                       (unsigned long long*)c->cpart.p, c->cpart_cap, (const GuardBand*)nullptr, (const double*)nullptr, px);
    px.front_only = 1;
  }
  if (!light_c && !head_c) {
    hipExtLaunchKernelGGL(kpost, grid, dim3(256), L.lds, c->stream, nullptr,
                          (L.req.lmax_defer && last) ? c->ev[1] : ((colw && part == 0) ? c->col.ev[0] : nullptr), 0,
                          c->mc, cs, g.BtA, g.sBtA, g.P0f, g.sP0f, g.VA, g.sVA, g.SBf, g.sSBf, g.KB0, g.KS0, g.KBm, g.KSm, g.KBm2, g.nrb, g.ncs0,
                          L.nlines, (double*)c->mean.p, (double*)c->var.p, L.defer ? L.lrows + (size_t)L.rows_out * q : L.lrows,
                          (const double*)c->bl_small.p /* xn0 */, fuse ? (uint8_t*)(q > 2 ? c->fuseS.p : c->maskS.p) : (uint8_t*)nullptr,
                          fuse ? (uint8_t*)(q > 2 ? c->fuseU.p : c->maskU.p) : (uint8_t*)nullptr, L.req.fuse_b, (unsigned long long*)c->cpart.p,
                          c->cpart_cap, L.gb_fused, (const int*)g.eff, g.gtmax, g.gkey, g.imode, px);
  }
  if (colw && part == 0 && L.record_encl) {
    // (the plan's first constraint launch evaluated and stored every tile: its enclosures, ~270 MB read once per plan)
    hipLaunchKernelGGL(k_bl_enclose, dim3(L.gx, L.gy), dim3(128), 0, c->stream, (const double*)c->mean.p + (size_t)cs.n_local,
                       (const double*)c->var.p + (size_t)cs.n_local, L.cnt0, L.encl, (const double*)L.lrows + L.ntiles, L.lrec);
    c->bl.encl_ready = true;
    c->bl.lrows_ready = L.lrec != nullptr;
  }
  // (a constraint's launch without a skip list evaluated and stored every tile: the stored values are the plan's again)
  if (colw && part == 0 && !L.interp && c->bl.encl_ready && !px.encl) c->bl.vals_ready = true;
}

// sbo_profile's flop figure of the launch
static void gemm_flops(const GemmLaunch& L) {
  sbo_ctx* c = L.c;
  const GemmOps& g = L.g;
  const int q = L.q;
  const double tiles2 = (double)g.nrb * g.ncs0;
  if (L.interp) {
    // flops issued: stage 1 of four coefficient sets per output + four full phases of stage 2 (an upper bound: the counts the kernels
    // run to stay on the device -- a read-back per plan is a launch the host-bound plan does not need)
    c->last_k1_flops = (double)q * 2.0 * 1024.0 * 4.0 * (4.0 * (double)g.nrb * g.KB0 * g.KB0 + tiles2 * g.KB0 * 4);
    return;
  }
  const double s1 = L.run_stage1 ? 1.0 : 0.0;
  // flops issued on the matrix cores: stage 1 (when this launch ran it) + the four phases of stage 2 (KS0 + 3 KSm k-steps: the axis-0 gradient phase
  // runs on the mean phase's sums; 16 x 16 x 4 steps, 2 flops per multiply-add)
  c->last_k1_flops = (double)q * 2.0 * 1024.0 * (s1 * 4.0 * (double)g.nrb * g.KB0 * g.KB1 + tiles2 * (g.KS0 + 3 * g.KSm));
  // (a 64 x 128 tile is 32 of the 16 x 16 blocks tiles2 counts: what sets.hip takes off for a tile classified from memory)
  for (int o = 0; o < 2; ++o) c->last_k1_tile_flops[o] = 32.0 * 2.0 * 1024.0 * (g.KS0 + 3 * g.KSm);
  // Chebyshev core: the counts the kernels actually run to (k_cheb_trunc; copied to the pinned block when the plan was built --
  // they have arrived long before a sweep's result is read: a plan build is followed by the sweep's own synchronisation
  // before anyone asks for the profile).  Until then the upper bound above stands.
  const int* he = c->h_back->tile_eff;
  double f = 0.0;
  for (int o = 0; o < q; ++o) {
    const int ks = he[4 * o], kb0 = he[4 * o + 1], kb1 = he[4 * o + 2];
    if (ks < 1 || ks > g.KS0 || kb0 < 1 || kb0 > g.KB0 || kb1 < 1 || kb1 > g.KB1) return;
    // (the gradient phases run on the few tiles that can hold the maximum: not counted)
    f += 2.0 * 1024.0 * (s1 * 4.0 * (double)g.nrb * kb0 * kb1 + tiles2 * (ks + (g.gtmax ? 1 : 3) * g.KSm));
    if (o < 2) c->last_k1_tile_flops[o] = 32.0 * 2.0 * 1024.0 * (ks + (g.gtmax ? 1 : 3) * g.KSm);
  }
  c->last_k1_flops = f;
}

int launch_posterior_gemm(sbo_ctx* c, bool interp, const PostRequest& req, PostOutcome& out) {
  GemmLaunch L{c, interp, req, out, interp ? c->bi.ops : c->bl.ops, c->mc.q, c->cs.count[0], c->cs.n_local / c->cs.count[0]};
  const GemmOps& g = L.g;
  if (interp) c->bi.used = true;
  L.defer = interp && c->bi.grad_deferred && c->stream3 != nullptr;
  // K1b: stage 1 once per plan -- P1A, T4f and the counts are the plan's, so a resident model swept again would rebuild the same images
  // (BilinearPlan::bt_ready states who may write them).  K1i: every launch (its images belong to a model's single first sweep, and
  // they take the place of K1b's in bl_BtA).
  L.run_stage1 = interp || !c->bl.bt_ready;
  if (interp) c->bl.bt_ready = false;
  if (!interp && L.run_stage1) {
    gemm_stage1(L);
    c->bl.bt_ready = true;
  }
  int rc;
  if ((rc = gemm_shape(L)) || (rc = gemm_classify_plan(L))) return rc;
  if (L.colw) {
    if ((rc = col_words_prepare(c, L.cnt0, L.nlines, &L.px.cb))) return rc;
    L.px.lean = req.col_lean;
    out.col_active = true;
    out.col_forked = true;
    out.col_lean = req.col_lean;
    L.fuse = false;                    // (no byte masks: the words are the classification)
    if (!interp && (rc = col_enclosures(L))) return rc;
    if ((rc = col_tile_lists(L))) return rc;
    if (!interp && (rc = col_resident(L))) return rc;
  }
  // (K1b's byte-mask launch stores the plan's values through another epilogue: not relied on -- BilinearPlan::encl_ready)
  if (!interp && !L.colw) post_regions_written(c);
  // (K1i: stage 1 behind col_words_prepare -- the gradient launch, which follows it on another stream, merges into the slot block)
  if (interp) gemm_stage1(L);
  if (L.defer && g.band_ready) SBO_HIP(hipStreamWaitEvent(c->stream, c->ev_grad[3], 0));     // (the band: written on Y beside stage 1)
  L.gb_fused = (c->opt.guard_band && !c->is_shadow && g.band_ready && c->gb.buf.p) ? (const GuardBand*)c->gb.buf.p : nullptr;
  for (auto k : {k_bpost<1, 0>, k_bpost<1, 1>, k_bpost<1, 2>})
    SBO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
  L.lrows = (double*)c->bl_lpart.p;
  if (L.defer && (rc = gemm_grad_deferred(L))) return rc;
  // (column path: the constraint's launch first)
  for (int part = 0; part < (L.colw ? 2 : 1); ++part) gemm_post_part(L, part);
  // (whoever merges the Lipschitz rows on this stream -- the reduction below, a sweep's first small kernel -- waits for the gradient launch;
  // the column path reads the keys from the slot block on stream3 itself, in stream order behind that launch: sets_colpath.inc.hpp)
  if (L.defer && !L.colw) {
    SBO_HIP(hipStreamWaitEvent(c->stream, c->ev_grad[2], 0));
    c->grad_pending = false;
  }
  if (req.lmax_defer) {
    out.lmax_pending = true;
    out.lmax_per_out = (int)L.rows_out;
  } else {
    hipExtLaunchKernelGGL(k_lmax_reduce, dim3((unsigned)L.q), dim3(256), 0, c->stream, nullptr, c->ev[1], 0, (const double*)L.lrows,
                          (int)L.rows_out, c->Lmax);
  }
  out.stop_attached = true;
  c->gb.active = c->opt.guard_band && !c->is_shadow && g.band_ready;     // (the band came with the plan)
  gemm_flops(L);
  SBO_HIP(hipGetLastError());
  return SBO_OK;
}
