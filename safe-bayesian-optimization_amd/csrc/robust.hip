// robust.hip -- StableOpt's robust min-max on a joint (xc, d) tensor grid (models/StableOpt.py:139-164, on models/GP_Robust.py).
//
// The control axes are the fast ones, so disturbance plane p of the resident grid is one contiguous run of Nc candidates and the
// posterior's [q][n_local] arrays hold, for output o, plane after plane of the control sub-grid.  One thread per control point walks
// the planes in order (consecutive lanes read consecutive xc: coalesced) and keeps
//   f[xc]    = max_d  bound_0(xc, d)   (kind: mean / ucb / lcb of the objective)  and the first plane reaching it, arg_d[xc]
//   g_c[xc]  = min_d  lcb_c(xc, d)     for every constraint c >= 1
// Max and min are exact, so these are bit for bit what NumPy's max / min of the same posterior give.  When the control points alone
// cannot fill the GPU, the planes are split over blockIdx.y and a second kernel merges the splits in plane order (no atomics).
// The sweep then masks the controls with min_d lcb_c >= 0 for all c and takes the arg-min of f over them (sets.hip: robust_argmin,
// the k_arg_masked / k_arg_final machinery of the other sweeps: ties -> lowest index, the same guard-band accounting).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "device_common.hpp"
#include "internal.hpp"

namespace sbo {

int comm_allreduce_max_u64(sbo_ctx* c, unsigned long long* dev, int count);
int comm_allreduce_min_u64(sbo_ctx* c, unsigned long long* dev, int count);
int comm_allgather_bytes(sbo_ctx* c, const void* send, void* recv, size_t bytes_per_rank);
int guard_audit_enqueue(sbo_ctx* c, int first_output);
// sets.hip: the masked arg-min of f (band fb, gb_on) over mask[Nc] with k_arg_masked / k_arg_final; out4 (device) receives the winner's
// index (-1: none), the mask's population, the decisions its band leaves open and the winner's value (as bits)
int robust_argmin(sbo_ctx* c, const double* f, const double* fb, const uint8_t* mask, long long Nc, bool gb_on, long long* out4);

namespace {

constexpr int kRobBlock = 256;
constexpr int kRowFields = 8;   // winner's row: index, f (global), f (this rank), second f (this rank), arg_d (global plane), band of f, ...

struct RobArgs {
  const double* mean;   // [q][n_local]
  const double* var;
  long long nc, planes, plane0;   // control points, local disturbance planes, global index of the first one
  long long n_local;
  int q, kind;
  double b;
  const GuardBand* gb;
  long long pps;        // planes per split (blockIdx.y)
  // outputs of split s (s = 0 .. gridDim.y - 1): arrays of Nc at  base + s * stride
  double* f;            // max_d bound_0
  double* fsec;         // second largest value over d (ties included)
  long long* argd;      // first global plane of the maximum
  double* fb;           // band of f: max over d of the band of bound_0
  double* g;            // [q - 1][Nc] min_d lcb_c
  double* gbd;          // [q - 1][Nc] its band
  long long sstride;    // elements between splits (scalar arrays); the constraint arrays use sstride * (q - 1)
};

__device__ __forceinline__ double bound_of(double m, double v, double b, int kind) {
  if (kind == SBO_MEAN) return m;
  const double sd = mul_rn(b, sqrt_rn(v));    // models/StableOpt.py:64-95: mean +- b sqrt(var), as lcb_ucb in sets.hip
  return kind == SBO_UCB ? add_rn(m, sd) : sub_rn(m, sd);
}
__device__ __forceinline__ double band_of(double v, double b, int kind, double dm, double dv) {
  if (kind == SBO_MEAN || !(dv > 0.0)) return dm;
  return dm + b * gb_dsqrt(v, dv);
}

__global__ __launch_bounds__(kRobBlock) void k_robust_reduce(const RobArgs a) {
  const long long x = (long long)blockIdx.x * kRobBlock + threadIdx.x;
  if (x >= a.nc) return;
  const long long p0 = (long long)blockIdx.y * a.pps;
  const long long p1 = min(a.planes, p0 + a.pps);
  const int qc = a.q - 1;
  double dm[kMaxQ], dv[kMaxQ];
#pragma unroll
  for (int o = 0; o < kMaxQ; ++o) {
    dm[o] = (a.gb && o < a.q) ? a.gb->dm[o] : 0.0;
    dv[o] = (a.gb && o < a.q) ? a.gb->dv[o] : 0.0;
  }
  double fm = -INFINITY, fsec = -INFINITY, fband = 0.0;
  long long arg = -1;
  double gmin[kMaxQ - 1], gband[kMaxQ - 1];
#pragma unroll
  for (int c = 0; c < kMaxQ - 1; ++c) { gmin[c] = INFINITY; gband[c] = 0.0; }
  for (long long p = p0; p < p1; ++p) {
    const long long i = p * a.nc + x;
    const double m0 = a.mean[i], v0 = a.var[i];
    const double v = bound_of(m0, v0, a.b, a.kind);
    if (v > fm) {                                 // strict: the first plane of the maximum is kept
      fsec = fm;
      fm = v;
      arg = a.plane0 + p;
    } else if (v > fsec) {
      fsec = v;
    }
    fband = fmax(fband, band_of(v0, a.b, a.kind, dm[0], dv[0]));
#pragma unroll
    for (int c = 0; c < kMaxQ - 1; ++c) {
      if (c < qc) {
        const size_t off = (size_t)(c + 1) * a.n_local + i;
        const double vc = a.var[off];
        const double l = bound_of(a.mean[off], vc, a.b, SBO_LCB);
        gmin[c] = l < gmin[c] ? l : gmin[c];
        gband[c] = fmax(gband[c], band_of(vc, a.b, SBO_LCB, dm[c + 1], dv[c + 1]));
      }
    }
  }
  const long long s = blockIdx.y;
  const size_t o1 = (size_t)s * a.sstride + x;
  a.f[o1] = fm;
  a.fsec[o1] = fsec;
  a.argd[o1] = arg;
  a.fb[o1] = fband;
#pragma unroll
  for (int c = 0; c < kMaxQ - 1; ++c) {
    if (c < qc) {
      const size_t oc = (size_t)s * a.sstride * qc + (size_t)c * a.nc + x;
      a.g[oc] = gmin[c];
      a.gbd[oc] = gband[c];
    }
  }
}

// merge of the splits in plane order: strict comparisons keep the first plane of a maximum
__global__ __launch_bounds__(kRobBlock) void k_robust_combine(const RobArgs a, int splits, double* f, double* fsec, long long* argd, double* fb,
                                                              double* g, double* gbd) {
  const long long x = (long long)blockIdx.x * kRobBlock + threadIdx.x;
  if (x >= a.nc) return;
  const int qc = a.q - 1;
  double fm = a.f[x], fs = a.fsec[x], band = a.fb[x];
  long long arg = a.argd[x];
  for (int s = 1; s < splits; ++s) {
    const size_t o = (size_t)s * a.sstride + x;
    const double sm = a.f[o], ss = a.fsec[o];
    if (sm > fm) {
      fs = fmax(fm, ss);
      fm = sm;
      arg = a.argd[o];
    } else {
      fs = fmax(fs, sm);
    }
    band = fmax(band, a.fb[o]);
  }
  f[x] = fm;
  fsec[x] = fs;
  argd[x] = arg;
  fb[x] = band;
  for (int c = 0; c < qc; ++c) {
    double gm = a.g[(size_t)c * a.nc + x], gbm = a.gbd[(size_t)c * a.nc + x];
    for (int s = 1; s < splits; ++s) {
      const size_t o = (size_t)s * a.sstride * qc + (size_t)c * a.nc + x;
      const double v = a.g[o];
      gm = v < gm ? v : gm;
      gbm = fmax(gbm, a.gbd[o]);
    }
    g[(size_t)c * a.nc + x] = gm;
    gbd[(size_t)c * a.nc + x] = gbm;
  }
}

// ranks > 1: the local arrays as order-preserving keys (max: f | fb | gbd; min: g), and back after the all-reduces
__global__ __launch_bounds__(kRobBlock) void k_robust_keys(const double* f, const double* fb, const double* g, const double* gbd, long long nc,
                                                           int qc, unsigned long long* kmax, unsigned long long* kmin) {
  const long long x = (long long)blockIdx.x * kRobBlock + threadIdx.x;
  if (x >= nc) return;
  kmax[x] = ord_key(f[x]);
  kmax[nc + x] = ord_key(fb[x]);
  for (int c = 0; c < qc; ++c) {
    kmax[(2 + c) * nc + x] = ord_key(gbd[(size_t)c * nc + x]);
    kmin[(size_t)c * nc + x] = ord_key(g[(size_t)c * nc + x]);
  }
}
__global__ __launch_bounds__(kRobBlock) void k_robust_unkeys(const unsigned long long* kmax, const unsigned long long* kmin, long long nc, int qc,
                                                             double* f, double* fb, double* g, double* gbd) {
  const long long x = (long long)blockIdx.x * kRobBlock + threadIdx.x;
  if (x >= nc) return;
  f[x] = ord_val(kmax[x]);
  fb[x] = ord_val(kmax[nc + x]);
  for (int c = 0; c < qc; ++c) {
    gbd[(size_t)c * nc + x] = ord_val(kmax[(2 + c) * nc + x]);
    g[(size_t)c * nc + x] = ord_val(kmin[(size_t)c * nc + x]);
  }
}

// robust-safe mask: min_d lcb_c >= 0 for every constraint (models/StableOpt.py:146-150); open[0] += controls whose verdict the band
// leaves open (some c with g_c - band < 0 <= g_c + band)
__global__ __launch_bounds__(kRobBlock) void k_robust_safe(const double* g, const double* gbd, long long nc, int qc, uint8_t* mask,
                                                           unsigned long long* open) {
  const long long x = (long long)blockIdx.x * kRobBlock + threadIdx.x;
  bool safe = true, amb = false;
  if (x < nc) {
    for (int c = 0; c < qc; ++c) {
      const double v = g[(size_t)c * nc + x], e = gbd[(size_t)c * nc + x];
      safe = safe && v >= 0.0;
      amb = amb || (e > 0.0 && v - e < 0.0 && v + e >= 0.0);
    }
    mask[x] = safe ? 1 : 0;
  }
  const unsigned long long bal = __ballot(amb);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(open, (unsigned long long)__popcll(bal));
}

// winner's row: [0] index (as double), [1] f global, [2] f of this rank, [3] second value of this rank, [4] first plane of this rank's
// maximum (-1: none), [5] band of f; index < 0: no robust-safe control
__global__ void k_robust_row(const long long* idx, const double* fG, const double* floc, const double* fsec, const long long* argd,
                             const double* fb, double* row) {
  const long long w = *idx;
  row[0] = (double)w;
  row[1] = w >= 0 ? fG[w] : INFINITY;
  row[2] = w >= 0 ? floc[w] : -INFINITY;
  row[3] = w >= 0 ? fsec[w] : -INFINITY;
  row[4] = w >= 0 ? (double)argd[w] : -1.0;
  row[5] = w >= 0 ? fb[w] : 0.0;
  row[6] = row[7] = 0.0;
}

struct RobLayout {   // offsets into sbo_ctx::rob (doubles)
  long long nc;
  int qc;
  double *floc, *fsec, *fb, *g, *gbd, *fG, *fbG, *gG, *gbG, *row, *rows;
  long long* argd;
  unsigned long long *kmax, *kmin, *open;
};

int rob_layout(sbo_ctx* c, long long nc, RobLayout& L) {
  const int qc = c->mc.q - 1;
  const bool mr = multi_rank(c);
  const size_t nA = (size_t)nc;
  // local f | fsec | argd | fb | g | gbd;  ranks > 1: global f | fb | g | gbd and the key arrays (2 x (2 + qc) Nc);  the scalars; the rows
  int rc;
  if ((rc = carve(c->rob.vals, [&](Carve cv) {
        cv.take(L.floc, nA); cv.take(L.fsec, nA); cv.take(L.argd, nA); cv.take(L.fb, nA);
        cv.take(L.g, nA * qc); cv.take(L.gbd, nA * qc);
        if (mr) {
          cv.take(L.fG, nA); cv.take(L.fbG, nA);
          cv.take(L.gG, nA * qc); cv.take(L.gbG, nA * qc);
          cv.take(L.kmax, nA * (2 + qc)); cv.take(L.kmin, nA * (2 + qc));   // (kmin: qc x Nc used)
        }
        cv.take(L.open, 64); cv.take(L.row, kRowFields); cv.take(L.rows, (size_t)kRowFields * c->dist.world);
        return cv.off;
      })))
    return rc;
  if ((rc = ensure(c->rob.mask, nA + 8))) return rc;
  L.nc = nc;
  L.qc = qc;
  if (!mr) {
    L.fG = L.floc; L.fbG = L.fb; L.gG = L.g; L.gbG = L.gbd;
    L.kmax = L.kmin = nullptr;
  }
  return SBO_OK;
}

struct PhaseOut {
  long long index, count_safe, open, argd, worst_open;
  double value;
};

// reduction over the planes, masks, arg-min and the winner's worst disturbance on the resident posterior; `gb` its band (nullptr: exact)
int robust_phase(sbo_ctx* c, const sbo_sweep_opts* o, int kind, long long nc, const GuardBand* gb, PhaseOut& out) {
  const long long n = c->cs.n_local, planes = nc > 0 ? n / nc : 0;
  const int q = c->mc.q, qc = q - 1;
  RobLayout L;
  int rc;
  if ((rc = rob_layout(c, nc, L))) return rc;
  const unsigned bx = (unsigned)((nc + kRobBlock - 1) / kRobBlock);
  SBO_HIP(hipMemsetAsync(L.open, 0, 64, c->stream));
  if (planes > 0) {
    // the control points alone below ~4 workgroups per CU: the planes are split over blockIdx.y (at least 8 planes a split)
    const long long want = std::max<long long>(1, (4LL * c->n_cu + bx - 1) / bx);
    const long long splits = std::max<long long>(1, std::min<long long>(want, planes / 8));
    const long long pps = (planes + splits - 1) / splits;
    const int sp = (int)((planes + pps - 1) / pps);
    RobArgs a{};
    a.mean = (const double*)c->mean.p;
    a.var = (const double*)c->var.p;
    a.nc = nc;
    a.planes = planes;
    a.plane0 = c->cs.first / nc;
    a.n_local = n;
    a.q = q;
    a.kind = kind;
    a.b = o->b;
    a.gb = gb;
    a.pps = pps;
    a.sstride = nc;
    if (sp == 1) {
      a.f = L.floc; a.fsec = L.fsec; a.argd = L.argd; a.fb = L.fb; a.g = L.g; a.gbd = L.gbd;
      hipLaunchKernelGGL(k_robust_reduce, dim3(bx, 1), dim3(kRobBlock), 0, c->stream, a);
    } else {
      const size_t per = (size_t)sp * nc;                // (one array of a split's partials)
      if ((rc = carve(c->rob.part, [&](Carve cv) {
            cv.take(a.f, per); cv.take(a.fsec, per); cv.take(a.argd, per); cv.take(a.fb, per);
            cv.take(a.g, per * qc); cv.take(a.gbd, per * qc);
            return cv.off;
          })))
        return rc;
      hipLaunchKernelGGL(k_robust_reduce, dim3(bx, (unsigned)sp), dim3(kRobBlock), 0, c->stream, a);
      hipLaunchKernelGGL(k_robust_combine, dim3(bx), dim3(kRobBlock), 0, c->stream, a, sp, L.floc, L.fsec, L.argd, L.fb, L.g, L.gbd);
    }
  } else if (nc > 0) {   // (a rank without planes: the neutral elements of the all-reduces)
    std::vector<double> h((size_t)nc * (4 + 2 * (size_t)qc), 0.0);
    for (long long x = 0; x < nc; ++x) { h[x] = -INFINITY; h[nc + x] = -INFINITY; ((long long*)h.data())[2 * nc + x] = -1; }
    for (size_t i = (size_t)4 * nc; i < (size_t)(4 + qc) * nc; ++i) h[i] = INFINITY;
    SBO_HIP(hipMemcpyAsync(L.floc, h.data(), h.size() * 8, hipMemcpyHostToDevice, c->stream));
  }
  SBO_HIP(hipGetLastError());
  if (multi_rank(c) && nc > 0) {
    hipLaunchKernelGGL(k_robust_keys, dim3(bx), dim3(kRobBlock), 0, c->stream, L.floc, L.fb, L.g, L.gbd, nc, qc, L.kmax, L.kmin);
    SBO_HIP(hipGetLastError());
    if ((rc = comm_allreduce_max_u64(c, L.kmax, (int)(nc * (2 + qc))))) return rc;
    if (qc > 0 && (rc = comm_allreduce_min_u64(c, L.kmin, (int)(nc * qc)))) return rc;
    hipLaunchKernelGGL(k_robust_unkeys, dim3(bx), dim3(kRobBlock), 0, c->stream, L.kmax, L.kmin, nc, qc, L.fG, L.fbG, L.gG, L.gbG);
  }
  if (nc > 0) hipLaunchKernelGGL(k_robust_safe, dim3(bx), dim3(kRobBlock), 0, c->stream, L.gG, L.gbG, nc, qc, (uint8_t*)c->rob.mask.p, L.open);
  SBO_HIP(hipGetLastError());
  long long* a4 = (long long*)(L.open + 1);
  if ((rc = robust_argmin(c, L.fG, L.fbG, (const uint8_t*)c->rob.mask.p, nc, gb != nullptr, a4))) return rc;
  // the winner's worst disturbance: every rank's first plane of the maximum and runner-up value, merged on the host
  hipLaunchKernelGGL(k_robust_row, dim3(1), dim3(1), 0, c->stream, (const long long*)a4, L.fG, L.floc, L.fsec, L.argd, L.fbG, L.row);
  SBO_HIP(hipGetLastError());
  const int nrows = multi_rank(c) ? c->dist.world : 1;
  const double* rows = L.row;
  if (multi_rank(c)) {
    if ((rc = comm_allgather_bytes(c, L.row, L.rows, sizeof(double) * kRowFields))) return rc;
    rows = L.rows;
  }
  unsigned long long hb[8];
  std::vector<double> hr((size_t)nrows * kRowFields);
  SBO_HIP(hipMemcpyAsync(hb, L.open, sizeof(hb), hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipMemcpyAsync(hr.data(), rows, hr.size() * 8, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipStreamSynchronize(c->stream));
  ++c->host_syncs;
  out.open = (long long)hb[0];
  out.index = (long long)hb[1];
  out.count_safe = (long long)hb[2];
  out.open += (long long)hb[3];
  memcpy(&out.value, &hb[4], 8);
  out.argd = -1;
  out.worst_open = 0;
  if (out.index < 0) {
    out.value = INFINITY;
    return SBO_OK;
  }
  // rank of the maximum: largest local value, ties -> lowest plane (the ranks own ascending planes)
  int best = -1;
  for (int r = 0; r < nrows; ++r) {
    const double* w = &hr[(size_t)r * kRowFields];
    if (w[4] < 0) continue;
    if (best < 0 || w[2] > hr[(size_t)best * kRowFields + 2]) best = r;
  }
  if (best < 0) return SBO_OK;
  const double* wb = &hr[(size_t)best * kRowFields];
  double second = -INFINITY;
  for (int r = 0; r < nrows; ++r) {
    const double* w = &hr[(size_t)r * kRowFields];
    if (w[4] < 0) continue;
    second = std::max(second, w[3]);
    if (r != best) second = std::max(second, w[2]);
  }
  out.argd = (long long)wb[4];
  const double band = wb[5];
  out.worst_open = (band > 0.0 && !(wb[2] - second > 2.0 * band)) ? 1 : 0;
  return SBO_OK;
}

int sweep_robust(sbo_ctx* c, const sbo_sweep_opts* o, int nca, int kind, sbo_robust_result* res) {
  const CandSpec& cs = c->cs;
  long long nc = 1, nd = 1;
  for (int a = 0; a < cs.d; ++a) (a < nca ? nc : nd) *= cs.count[a];
  if (cs.first % nc != 0 || cs.n_local % nc != 0)
    return fail(SBO_E_INVALID, "this rank's candidates are not whole disturbance planes of the control sub-grid");
  if (!multi_rank(c) && (cs.first != 0 || cs.n_local != nc * nd))
    return fail(SBO_E_INVALID, "a one-rank robust sweep needs the whole grid resident");
  int rc;
  SBO_HIP(hipEventRecord(c->ev[0], c->stream));
  c->host_syncs = 0;
  const bool reuse = o->posterior_ready && c->posterior_valid;
  PostOutcome out;                          // (a plain request: no classification rides on this posterior, the lean options do not apply)
  if (!reuse && (rc = posterior_enqueue(c, PostRequest{}, &out))) return rc;
  SBO_HIP(k1_stop(c, out));
  if (!reuse && (rc = guard_audit_enqueue(c, out))) return rc;
  const GuardBand* gb = resident_band(c);      // (fp64 models only: sbo_sweep_robust)
  const int k1_first = c->last_k1;
  PhaseOut P{};
  if ((rc = robust_phase(c, o, kind, nc, gb, P))) return rc;
  const long long first_open = P.open + P.worst_open;
  // an approximating posterior whose band left a decision open (or option guard_band 2): the exact kernel on the whole grid, decide again.
  // The ranks decide together -- the re-evaluation contains collectives.
  unsigned long long want[2] = {(unsigned long long)(gb && (first_open > 0 || c->opt.guard_band == 2) ? 1 : 0), 0};
  if (multi_rank(c)) {
    RobLayout L;
    if ((rc = rob_layout(c, nc, L))) return rc;
    unsigned long long* dw = L.open + 6;
    SBO_HIP(hipMemcpyAsync(dw, want, 8, hipMemcpyHostToDevice, c->stream));
    if ((rc = comm_allreduce_max_u64(c, dw, 1))) return rc;
    SBO_HIP(hipMemcpyAsync(want, dw, 8, hipMemcpyDeviceToHost, c->stream));
    SBO_HIP(hipStreamSynchronize(c->stream));
  }
  long long rechecks = 0;
  int passes = 0;
  float t_guard = 0.f;
  if (want[0]) {
    hipEvent_t g0 = c->ev[5], g1 = c->ev[6];
    SBO_HIP(hipEventRecord(g0, c->stream));
    PostRequest exact;
    exact.exact = true;
    if ((rc = posterior_enqueue(c, exact, &out))) return rc;
    c->last_k1 = k1_first;                  // (sbo_profile.posterior_kernel names the sweep's own posterior, as after the other sweeps' rechecks)
    if ((rc = robust_phase(c, o, kind, nc, nullptr, P))) return rc;
    SBO_HIP(hipEventRecord(g1, c->stream));
    SBO_HIP(hipEventSynchronize(g1));
    SBO_HIP(hipEventElapsedTime(&t_guard, g0, g1));
    rechecks = cs.n_local;
    passes = 1;
  }
  SBO_HIP(hipEventRecord(c->ev[2], c->stream));
  SBO_HIP(hipEventSynchronize(c->ev[2]));
  float t01 = 0, t12 = 0, t02 = 0;
  SBO_HIP(hipEventElapsedTime(&t01, c->ev[0], c->ev[1]));
  SBO_HIP(hipEventElapsedTime(&t12, c->ev[1], c->ev[2]));
  SBO_HIP(hipEventElapsedTime(&t02, c->ev[0], c->ev[2]));
  const int host_syncs = c->host_syncs;
  memset(&c->prof, 0, sizeof(c->prof));
  c->prof.posterior_ms = t01;
  c->prof.argreduce_ms = t12 - t_guard;
  c->prof.set_phase_ms = t12;
  c->prof.guard_ms = t_guard;
  c->prof.total_ms = t02;
  c->prof.candidates = cs.n_local;
  c->prof.posterior_launches = (!reuse && cs.n_local > 0) ? 1 : 0;
    c->prof.host_syncs = host_syncs;
  const double nn = c->mc.n, dd = c->mc.d;
  c->prof.posterior_flops = reuse ? 0.0 : c->mc.q * (nn * nn + (2 * dd + 10) * nn) * (double)cs.n_local;
  memset(res, 0, sizeof(*res));
  res->index = P.index;
  res->value = P.value;
  res->worst_d_index = P.index >= 0 ? P.argd : -1;
  res->candidate_index = P.index >= 0 ? P.argd * nc + P.index : -1;
  res->count_control = nc;
  res->count_disturbance = nd;
  res->count_safe = P.count_safe;
  res->guard_band = first_open;
  res->guard_rechecks = rechecks;
  res->guard_passes = passes;
  if (P.index >= 0) {   // coordinates from the grid's axes (host restatement of cand_coords, as coords_of in sets.hip)
    long long fx = P.index, fd = P.argd;
    for (int a = 0; a < cs.d; ++a) {
      long long& fl = a < nca ? fx : fd;
      const long long cnt = cs.count[a], i = fl % cnt;
      fl /= cnt;
      const double x = (i == cnt - 1 && cnt > 1) ? cs.hi[a] : cs.lo[a] + (double)i * cs.step[a];
      if (a < nca) res->xc[a] = x;
      else res->worst_d[a - nca] = x;
    }
  }
  c->rob.nc = nc;
  c->rob.q = c->mc.q;
  c->rob.valid = true;
  return SBO_OK;
}

}  // namespace

}  // namespace sbo

using namespace sbo;

extern "C" {

int sbo_sweep_robust(sbo_ctx* c, const sbo_sweep_opts* opts, int n_control_axes, int kind, sbo_robust_result* result) {
  if (!c || !opts || !result) return fail(SBO_E_INVALID, "NULL argument");
  if (!c->has_model) return fail(SBO_E_NO_MODEL, "sbo_model_set has not been called");
  if (!c->has_cand) return fail(SBO_E_NO_CANDIDATES, "no candidates resident");
  if (c->cs.d != c->mc.d) return fail(SBO_E_INVALID, "ERROR W and X_norm dimension should be same");
  if (c->cs.kind != 1) return fail(SBO_E_INVALID, "the robust sweep needs a grid of candidates (sbo_candidates_grid / _sharded)");
  if (n_control_axes < 1 || n_control_axes > c->cs.d - 1) return fail(SBO_E_INVALID, "n_control_axes must lie in [1, d - 1]");
  if (kind != SBO_MEAN && kind != SBO_UCB && kind != SBO_LCB) return fail(SBO_E_INVALID, "kind must be SBO_MEAN, SBO_UCB or SBO_LCB");
  if (!(opts->b >= 0.0) || !std::isfinite(opts->b)) return fail(SBO_E_INVALID, "confidence multiplier b must be finite and >= 0");
  if (c->dtype != SBO_F64) return fail(SBO_E_UNSUPPORTED, "the robust sweep runs fp64 models only");
  SBO_HIP(hipSetDevice(c->device));
  c->gb.first = 0;
  c->rob.valid = false;
  const int rc = sweep_robust(c, opts, n_control_axes, kind, result);
  if (rc != SBO_OK) drain_streams(c);
  return rc;
}

int sbo_robust_get(sbo_ctx* c, double* f_out, double* g_out) {
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (!c->rob.valid) return fail(SBO_E_INVALID, "no robust sweep has run on the resident model and candidates");
  SBO_HIP(hipSetDevice(c->device));
  RobLayout L;
  const int rc = rob_layout(c, c->rob.nc, L);   // (the buffer is already that size: no reallocation)
  if (rc) return rc;
  const size_t nc = (size_t)c->rob.nc;
  if (f_out && nc) SBO_HIP(hipMemcpyAsync(f_out, L.fG, nc * 8, hipMemcpyDeviceToHost, c->stream));
  if (g_out && nc && c->rob.q > 1) SBO_HIP(hipMemcpyAsync(g_out, L.gG, nc * (c->rob.q - 1) * 8, hipMemcpyDeviceToHost, c->stream));
  SBO_HIP(hipStreamSynchronize(c->stream));
  return SBO_OK;
}

}  // extern "C"
