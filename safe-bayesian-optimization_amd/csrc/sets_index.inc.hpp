// sets_index.inc.hpp: spatial index of an explicit candidate list for the expander / coverage searches -- part of the sets.hip
// translation unit (included inside namespace sbo; not a standalone header).
//
// Built once per candidate list (lazily, at the first sweep that needs it): Morton keys of the points quantised over the list's
// bounding box, a device LSD radix sort of (key, index), the permutation and a copy of the coordinates in sorted order.  Caller
// order stays the order of mean / var / masks / reported indices; the sorted order is used inside the set phase only.
// Per sweep (U changes): a hierarchy of boxes of the U members -- leaves of kIdxLeaf sorted candidates, kIdxFan children per node
// above -- that the expander verdict walks with one wave per safe candidate.  A node is skipped when the lower bound of the
// reference's shifted distance to its box exceeds the candidate's radius ucb_c / L; a node whose box lies entirely inside the
// radius (upper bound) holds a witness for sure; leaves evaluate the reference pair expression itself (lipschitz_pair).  Both
// bounds carry the "+1e-8" of the reference and the rounding, so every verdict equals the exhaustive one (k_expander_exact).

constexpr int kIdxLeaf = 256;             // sorted candidates per leaf
constexpr int kIdxFan = 64;               // children per node above the leaves (one per lane of the walking wave)
constexpr int kIdxMaxLevels = 6;          // leaves < 2^23 (lists < 2^31): at most four levels of nodes
constexpr int kSortTile = 4096;           // items per workgroup and radix pass (256 lanes x 16 rounds)
constexpr int kIdxBoxHead = 2 * kMaxD;    // bounding-box block: ord keys of lo[kMaxD], then of -hi[kMaxD]

// what a walk needs: the sorted list, this sweep's node boxes and the sorted U mask
struct IdxTree {
  long long n;
  int d, nlev;                            // nodes on levels 0 (leaves) .. nlev - 1; the top level has at most kIdxFan nodes
  long long cnt[kIdxMaxLevels];
  long long off[kIdxMaxLevels];           // first node of each level (units of nodes of 2 D doubles)
  const unsigned* perm;                   // sorted position -> caller index
  const double* xs;                       // sorted coordinates [n][d], fp64
  const unsigned long long* box;          // bounding box of the list (ord keys)
  double* nodes;                          // [lo[D], hi[D]] per node; lo[0] > hi[0]: no U member below
  uint8_t* Us;                            // U in sorted order
  unsigned long long* stats;              // [0] leaf pairs evaluated, [1] nodes skipped (cumulative over the sweep's constraints)
};

// ---- build: bounding box, Morton keys, radix sort, sorted copy ----------------------------------------------------------
__global__ __launch_bounds__(256) void k_idx_box_init(unsigned long long* box) {
  if (threadIdx.x < kIdxBoxHead) box[threadIdx.x] = ~0ull;       // (min of ord keys of lo and of -hi)
}
template <int D>
__global__ __launch_bounds__(256) void k_idx_box(const CandSpec cs, unsigned long long* box) {
  double lo[D], hi[D];
#pragma unroll
  for (int a = 0; a < D; ++a) { lo[a] = 1e300; hi[a] = -1e300; }
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < cs.n_local; g += (long long)gridDim.x * blockDim.x) {
    double x[D];
    cand_coords<D>(cs, g, x);
#pragma unroll
    for (int a = 0; a < D; ++a) { lo[a] = fmin(lo[a], x[a]); hi[a] = fmax(hi[a], x[a]); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int a = 0; a < D; ++a) { lo[a] = fmin(lo[a], __shfl_xor(lo[a], o)); hi[a] = fmax(hi[a], __shfl_xor(hi[a], o)); }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < D; ++a) {
      if (a >= cs.d) continue;
      atomicMin(&box[a], ord_key(lo[a]));
      atomicMin(&box[kMaxD + a], ord_key(-hi[a]));
    }
  }
}
__device__ __forceinline__ void idx_box_of(const unsigned long long* box, int a, double& lo, double& hi) {
  lo = ord_val(box[a]);
  hi = -ord_val(box[kMaxD + a]);
}
__device__ __forceinline__ double idx_xscale(const unsigned long long* box, int d) {
  double s = 0.0;
  for (int a = 0; a < d; ++a) {
    double lo, hi;
    idx_box_of(box, a, lo, hi);
    s = fmax(s, fmax(fabs(lo), fabs(hi)));
  }
  return s;
}

__host__ __device__ __forceinline__ int idx_bits_per_axis(int d) { return d == 1 ? 21 : (64 / d < 21 ? 64 / d : 21); }

// Morton (Z-order) key of every point over the list's bounding box; values: the caller's index
template <int D>
__global__ __launch_bounds__(256) void k_idx_keys(const CandSpec cs, const unsigned long long* box, unsigned long long* keys,
                                                  unsigned* vals) {
  const int d = cs.d, bpa = idx_bits_per_axis(d);
  const double levels = (double)(1ull << bpa);
  double lo[D], inv[D];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    lo[a] = 0.0;
    inv[a] = 0.0;
    if (a < d) {
      double l, h;
      idx_box_of(box, a, l, h);
      lo[a] = l;
      inv[a] = h > l ? levels / (h - l) : 0.0;
    }
  }
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < cs.n_local; g += (long long)gridDim.x * blockDim.x) {
    double x[D];
    cand_coords<D>(cs, g, x);
    unsigned qa[D];
#pragma unroll
    for (int a = 0; a < D; ++a) {
      double t = (x[a] - lo[a]) * inv[a];
      t = t >= 0.0 ? t : 0.0;                               // (NaN too)
      t = t < levels - 1.0 ? t : levels - 1.0;
      qa[a] = (unsigned)t;
    }
    unsigned long long k = 0ull;
    for (int j = bpa - 1; j >= 0; --j) {
#pragma unroll
      for (int a = 0; a < D; ++a)
        if (a < d) k = (k << 1) | (unsigned long long)((qa[a] >> j) & 1u);
    }
    keys[g] = k;
    vals[g] = (unsigned)g;
  }
}

// LSD radix sort, 8 bits per pass: per-tile digit counts -> per-digit exclusive scan over the tiles -> stable scatter
__global__ __launch_bounds__(256) void k_idx_hist(const unsigned long long* __restrict__ keys, long long n, int shift,
                                                  unsigned* __restrict__ hist, int ntiles) {
  __shared__ unsigned cnt[256];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const long long t0 = (long long)blockIdx.x * kSortTile;
  for (int r = 0; r < kSortTile / 256; ++r) {
    const long long i = t0 + r * 256 + threadIdx.x;
    if (i < n) atomicAdd(&cnt[(unsigned)(keys[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(long long)threadIdx.x * ntiles + blockIdx.x] = cnt[threadIdx.x];
}
// one workgroup per digit: exclusive scan of its row over the tiles (in place), row total -> dtot[digit]
__global__ __launch_bounds__(256) void k_idx_scan_rows(unsigned* __restrict__ hist, int ntiles, unsigned* __restrict__ dtot) {
  __shared__ unsigned part[256];
  unsigned* row = hist + (long long)blockIdx.x * ntiles;
  unsigned carry = 0;
  for (int base = 0; base < ntiles; base += 256) {
    const int i = base + threadIdx.x;
    const unsigned v = i < ntiles ? row[i] : 0u;
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const unsigned w = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0u;
      __syncthreads();
      part[threadIdx.x] += w;
      __syncthreads();
    }
    if (i < ntiles) row[i] = carry + part[threadIdx.x] - v;
    carry += part[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) dtot[blockIdx.x] = carry;
}
__global__ __launch_bounds__(256) void k_idx_scatter(const unsigned long long* __restrict__ kin, const unsigned* __restrict__ vin,
                                                     unsigned long long* __restrict__ kout, unsigned* __restrict__ vout, long long n,
                                                     int shift, const unsigned* __restrict__ hist, const unsigned* __restrict__ dtot,
                                                     int ntiles) {
  __shared__ unsigned base[256];
  __shared__ unsigned wcnt[4][256];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  {   // digit bases: exclusive scan of the digit totals, plus this tile's offset inside each digit
    base[t] = dtot[t];
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const unsigned w = t >= o ? base[t - o] : 0u;
      __syncthreads();
      base[t] += w;
      __syncthreads();
    }
    const unsigned excl = base[t] - dtot[t];
    __syncthreads();
    base[t] = excl + hist[(long long)t * ntiles + blockIdx.x];
    for (int w = 0; w < 4; ++w) wcnt[w][t] = 0;
    __syncthreads();
  }
  const unsigned long long lt = (1ull << lane) - 1ull;
  const long long t0 = (long long)blockIdx.x * kSortTile;
  for (int r = 0; r < kSortTile / 256; ++r) {
    const long long i = t0 + r * 256 + t;
    const bool valid = i < n;
    unsigned long long k = 0ull;
    unsigned v = 0u, dg = 0u;
    if (valid) { k = kin[i]; v = vin[i]; dg = (unsigned)(k >> shift) & 255u; }
    // lanes of this wave with the same digit (ranks inside the wave keep the input order: the sort is stable)
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bt = 0; bt < 8; ++bt) {
      const bool bit = (dg >> bt) & 1u;
      const unsigned long long m = __ballot(valid && bit);
      peers &= bit ? m : ~m;
    }
    const unsigned rank = (unsigned)__popcll(peers & lt);
    if (valid && rank == 0) wcnt[wave][dg] = (unsigned)__popcll(peers);
    __syncthreads();
    if (valid) {
      unsigned pos = base[dg] + rank;
      for (int w = 0; w < wave; ++w) pos += wcnt[w][dg];
      kout[pos] = k;
      vout[pos] = v;
    }
    __syncthreads();
    base[t] += wcnt[0][t] + wcnt[1][t] + wcnt[2][t] + wcnt[3][t];
    wcnt[0][t] = wcnt[1][t] = wcnt[2][t] = wcnt[3][t] = 0;
    __syncthreads();
  }
}
// coordinates in sorted order, fp64, stride d (a CandSpec of kind 0 over them reads the same values cand_coords gives)
template <int D>
__global__ __launch_bounds__(256) void k_idx_sorted_coords(const CandSpec cs, const unsigned* __restrict__ perm, double* __restrict__ xs) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < cs.n_local; i += (long long)gridDim.x * blockDim.x) {
    double x[D];
    cand_coords<D>(cs, (long long)perm[i], x);
#pragma unroll
    for (int a = 0; a < D; ++a)
      if (a < cs.d) xs[i * cs.d + a] = x[a];
  }
}

// ---- per sweep: boxes of the U members ------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void k_idx_leaves(const IdxTree tr, const uint8_t* __restrict__ U) {
  __shared__ double red[4][2 * D];
  const long long i = (long long)blockIdx.x * kIdxLeaf + threadIdx.x;
  const bool isU = i < tr.n && U[tr.perm[i]];
  if (i < tr.n) tr.Us[i] = isU ? 1 : 0;
  double lo[D], hi[D];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const double x = (isU && a < tr.d) ? tr.xs[i * tr.d + a] : 0.0;
    lo[a] = isU ? x : 1e300;
    hi[a] = isU ? x : -1e300;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int a = 0; a < D; ++a) { lo[a] = fmin(lo[a], __shfl_xor(lo[a], o)); hi[a] = fmax(hi[a], __shfl_xor(hi[a], o)); }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < D; ++a) { red[wave][a] = lo[a]; red[wave][D + a] = hi[a]; }
  }
  __syncthreads();
  if (threadIdx.x < 2 * D) {
    const int a = threadIdx.x;
    const double v = a < D ? fmin(fmin(red[0][a], red[1][a]), fmin(red[2][a], red[3][a]))
                           : fmax(fmax(red[0][a], red[1][a]), fmax(red[2][a], red[3][a]));
    tr.nodes[(tr.off[0] + blockIdx.x) * 2 * D + a] = v;
  }
}
// one wave per parent node: the union of its children's boxes
template <int D>
__global__ __launch_bounds__(256) void k_idx_parents(const IdxTree tr, int lev) {
  const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= tr.cnt[lev]) return;
  const int lane = threadIdx.x & 63;
  const long long ch = p * kIdxFan + lane;
  const bool ok = ch < tr.cnt[lev - 1];
  const double* cn = tr.nodes + (tr.off[lev - 1] + ch) * 2 * D;
  double lo[D], hi[D];
#pragma unroll
  for (int a = 0; a < D; ++a) { lo[a] = ok ? cn[a] : 1e300; hi[a] = ok ? cn[D + a] : -1e300; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int a = 0; a < D; ++a) { lo[a] = fmin(lo[a], __shfl_xor(lo[a], o)); hi[a] = fmax(hi[a], __shfl_xor(hi[a], o)); }
  }
  if (lane < 2 * D) tr.nodes[(tr.off[lev] + p) * 2 * D + lane] = lane < D ? lo[lane] : hi[lane - D];
}

// ---- the expander verdict on the index --------------------------------------------------------------------------------------
// One wave per safe candidate, taken in sorted order (a workgroup's queries are neighbours in space).  Depth-first walk from the
// top level; a node's kIdxFan children are tested by the lanes at once.  gband (guard band of an approximating posterior, as in
// k_expander_exact): the walk decides with ucb - du (sure witness) and ucb + du (no witness); a candidate with a witness only under
// ucb + du goes to the exhaustive recheck (amb), which decides it and counts it, exactly as the exhaustive path does.
template <typename T, int D>
__global__ __launch_bounds__(256) void k_idx_expander(const IdxTree tr, const T* __restrict__ mean_c, const T* __restrict__ var_c, T b,
                                                      const uint8_t* __restrict__ S, const unsigned long long* Lkeys, int lidx,
                                                      SweepScalars* sc, uint8_t* __restrict__ G, long long* __restrict__ amb,
                                                      const RcExp rx) {
  __shared__ unsigned long long smask[4][kIdxMaxLevels];
  __shared__ long long sbase[4][kIdxMaxLevels];
  const double L = __longlong_as_double((long long)Lkeys[lidx]);
  const bool gband = rx.gb_c > 0 && !rx.list;
  const RcBandK bk = rc_band(rx, sc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, d = tr.d;
  const bool prune = L > 0 && L < INFINITY;                 // (L = 0 / inf / NaN: no radius -- every leaf is evaluated)
  const double xscale = idx_xscale(tr.box, d);
  const double e_ax = 1.01e-8 + 1e-14 * xscale + 1e-13;     // |x_g - x_h + 1e-8| vs |x_g - x_h|: the shift and the rounding
  const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
  const int top = tr.nlev - 1;
  unsigned long long pairs = 0, skipped = 0;
  for (long long i = (long long)blockIdx.x * (blockDim.x >> 6) + wave; i < tr.n; i += nwaves) {
    const long long g = (long long)tr.perm[i];
    if (!S[g]) continue;                                     // (G was cleared ahead of the launch)
    T lcbT, ucbT;
    lcb_ucb(mean_c[g], var_c[g], b, lcbT, ucbT);
    const double ucb = (double)ucbT;
    const double du = gband ? rc_du(rx, bk, g, 0.0, (double)b, ucb) : 0.0;
    const double ucb_lo = ucb - du, ucb_hi = ucb + du;
    if (prune && !(ucb_hi >= 0.0)) continue;                // ucb - L dist <= ucb < 0 for every h: no witness
    double xg[D];
#pragma unroll
    for (int a = 0; a < D; ++a) xg[a] = a < d ? tr.xs[i * d + a] : 0.0;
    const double rh = prune ? ucb_hi / L * (1.0 + 1e-9) : 0.0;
    const double r2 = rh * rh;
    bool f_lo = false, f_mid = false, f_hi = false;
    // children [base, base + cnt) of one node on level lev: lanes test their box; returns the children to visit
    auto expand = [&](int lev, long long base, long long cnt) -> unsigned long long {
      const bool valid = lane < cnt;
      bool visit = false, sure = false, nonempty = false;
      if (valid) {
        const double* nd = tr.nodes + (tr.off[lev] + base + lane) * 2 * D;
        double lo[D], hi[D];
#pragma unroll
        for (int a = 0; a < D; ++a) { lo[a] = nd[a]; hi[a] = nd[D + a]; }
        nonempty = lo[0] <= hi[0];
        if (nonempty) {
          if (!prune) {
            visit = true;
          } else {
            double lb2 = 0.0, ub2 = 0.0;
#pragma unroll
            for (int a = 0; a < D; ++a) {
              if (a < d) {
                const double gap = fmax(0.0, fmax(lo[a] - xg[a], xg[a] - hi[a]));
                const double gl = fmax(0.0, gap * (1.0 - 1e-12) - e_ax);
                const double gu = fmax(fabs(xg[a] - lo[a]), fabs(xg[a] - hi[a])) * (1.0 + 1e-12) + e_ax;
                lb2 += gl * gl;
                ub2 += gu * gu;
              }
            }
            lb2 *= 1.0 - 1e-12;
            // every U point of the box is within sqrt(ub2) (and the box holds one): a witness for sure under ucb - du
            sure = ucb_lo > 0.0 && L * sqrt(ub2) * (1.0 + 1e-9) < ucb_lo;
            visit = lb2 <= r2;
          }
        }
      }
      if (__ballot(sure)) { f_lo = f_mid = f_hi = true; return 0ull; }
      const unsigned long long vm = __ballot(visit);
      skipped += (unsigned long long)__popcll(__ballot(nonempty && !visit));
      return vm;
    };
    auto leaf = [&](long long k) {
      bool lo_ = false, mid = false, hi_ = false;
      unsigned long long nU = 0;
#pragma unroll
      for (int s = 0; s < kIdxLeaf / 64; ++s) {
        const long long j = k * kIdxLeaf + s * 64 + lane;
        const bool isU = j < tr.n && tr.Us[j];
        nU += (unsigned long long)__popcll(__ballot(isU));
        if (isU) {
          double xh[D];
#pragma unroll
          for (int a = 0; a < D; ++a) xh[a] = a < d ? tr.xs[j * d + a] : 0.0;
          if (lipschitz_pair<D>(xg, xh, d, ucb, L)) mid = true;
          if (gband) {
            if (lipschitz_pair<D>(xg, xh, d, ucb_hi, L)) hi_ = true;
            if (lipschitz_pair<D>(xg, xh, d, ucb_lo, L)) lo_ = true;
          }
        }
      }
      pairs += nU;
      if (__ballot(mid)) f_mid = true;
      if (gband) {
        if (__ballot(hi_)) f_hi = true;
        if (__ballot(lo_)) f_lo = true;
      } else if (f_mid) {
        f_lo = f_hi = true;
      }
    };
    // depth-first walk; stack slot s holds level top - s
    int sp = 0;
    {
      const unsigned long long m = expand(top, 0, tr.cnt[top]);
      smask[wave][0] = m;                                    // (wave-uniform values: every lane stores the same)
      sbase[wave][0] = 0;
      sp = 1;
    }
    while (sp > 0 && !f_lo && !(f_mid && !gband)) {
      const int s = sp - 1, lev = top - s;
      unsigned long long m = smask[wave][s];
      if (m == 0ull) { --sp; continue; }
      const int cidx = __ffsll((long long)m) - 1;
      m &= m - 1ull;
      const long long child = sbase[wave][s] + cidx;
      smask[wave][s] = m;
      if (lev == 0) {
        leaf(child);
      } else {
        const long long b0 = child * kIdxFan;
        const long long nc = tr.cnt[lev - 1] - b0 < kIdxFan ? tr.cnt[lev - 1] - b0 : kIdxFan;
        const unsigned long long cm = expand(lev - 1, b0, nc);
        smask[wave][sp] = cm;
        sbase[wave][sp] = b0;
        ++sp;
      }
    }
    if (lane == 0) {
      if (!gband) {
        if (f_mid) G[g] = 1;
      } else if (f_lo) {
        G[g] = 1;
      } else if (f_hi) {
        amb[atomicAdd((unsigned long long*)&sc->n_amb, 1ull)] = g;   // (in the band: k_expander_exact decides and counts it)
      }
    }
  }
  if (lane == 0) {
    if (pairs) atomicAdd(&tr.stats[0], pairs);
    if (skipped) atomicAdd(&tr.stats[1], skipped);
  }
}

// ---- GoOSE on the sorted order: gathers into / scatter out of it -------------------------------------------------------------
template <typename V>
__global__ __launch_bounds__(256) void k_idx_gather(const V* __restrict__ src, const unsigned* __restrict__ perm, long long n,
                                                    V* __restrict__ dst) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dst[i] = src[perm[i]];
}
__global__ __launch_bounds__(256) void k_idx_scatter_u8(const uint8_t* __restrict__ src, const unsigned* __restrict__ perm, long long n,
                                                        uint8_t* __restrict__ dst) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dst[perm[i]] = src[i];
}
