// api.hip -- C-ABI entry points of libsafebo.so: context, model upload, candidates, posterior, bounds.
// (sweeps live in sets.hip, collectives in comm.hip).  See include/safebo.h for the contract.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <chrono>
#include "internal.hpp"
#include "device_common.hpp"

namespace sbo {

static thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int hip_fail(hipError_t e, const char* what) {
  g_err = std::string("HIP: ") + hipGetErrorString(e) + " in " + what;
  return SBO_E_HIP;
}
int ensure(DevBuf& b, size_t bytes) {
  if (bytes == 0) bytes = 16;
  if (b.bytes >= bytes) return SBO_OK;
  b.reset();
  hipError_t e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) {
    g_err = std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? SBO_E_NOMEM : SBO_E_HIP;
  }
  b.bytes = bytes;
  return SBO_OK;
}
// The runtime's blocking wait parks the thread and wakes it through an interrupt (~15-25 us after the stream drained); a
// sweep is 0.3 ms, so the host polls for up to 5 ms first and only then sleeps.
hipError_t stream_wait(const sbo_ctx* c, hipStream_t st) {
  {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      const hipError_t e = hipStreamQuery(st);
      if (e != hipErrorNotReady) return e;
      if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) break;
    }
  }
  return hipStreamSynchronize(st);
}

// after a failed call: nothing of it may still be running on the side streams when the caller comes back (a later call
// synchronises the main stream only and would race with orphaned kernels on the shared scratch)
void drain_streams(sbo_ctx* c) {
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->stream2) (void)hipStreamSynchronize(c->stream2);
  if (c->stream3) (void)hipStreamSynchronize(c->stream3);
  if (c->stream4) (void)hipStreamSynchronize(c->stream4);
}

// The reverse Cholesky factor of a caller's invK may still be in the making (sbo_ctx::factor_pending): every consumer of
// Fpk / the fp64 factor (sbo_ctx::factor) waits here first.  The positive-definiteness verdict arrives with it.
int factor_sync(sbo_ctx* c) {
  if (c->factor_todo) {                   // (not even enqueued: a model change that failed half-way)
    const int rc = model_factor_enqueue(c);
    if (rc) return rc;
  }
  if (!c->factor_pending) return SBO_OK;
  SBO_HIP(hipEventSynchronize(c->ev_factor));
  c->factor_pending = false;
  for (int o = 0; o < c->mc.q; ++o)
    if (c->h_back->factor_bad[o]) {
      c->has_model = false;
      return fail(SBO_E_INVALID, "invK is not positive definite (its factor was needed by this call)");
    }
  return SBO_OK;
}

int model_reader_check(const sbo_ctx* c, const char* who, bool need_f64) {
  if (!c->has_model) return fail(SBO_E_NO_MODEL, "sbo_model_set has not been called");
  if (need_f64 && c->dtype != SBO_F64) return fail(SBO_E_UNSUPPORTED, std::string(who) + " needs an fp64 model");
  return SBO_OK;
}
int model_reader_begin(sbo_ctx* c, const char* who, bool need_f64) {
  if (const int rc = model_reader_check(c, who, need_f64)) return rc;
  SBO_HIP(hipSetDevice(c->device));
  return factor_sync(c);
}

void release(DevBuf& b) { b.reset(); }

int launch_soa_to_aos(sbo_ctx* c, const void* soa, void* aos);

}  // namespace sbo

using namespace sbo;

extern "C" {

int sbo_version(void) { return SBO_ABI_VERSION; }
const char* sbo_last_error(void) { return g_err.c_str(); }

int sbo_device_count(int* count) {
  if (!count) return fail(SBO_E_INVALID, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *count = 0; return hip_fail(e, "hipGetDeviceCount"); }
  *count = n;
  return SBO_OK;
}

int sbo_init(int device_id, sbo_ctx** out) {
  if (!out) return fail(SBO_E_INVALID, "out is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(SBO_E_HIP, "no HIP device available: libsafebo has no CPU fallback");
  if (device_id < 0 || device_id >= n) return fail(SBO_E_INVALID, "device_id out of range");
  SBO_HIP(hipSetDevice(device_id));
  std::unique_ptr<sbo_ctx> guard(new sbo_ctx());   // (a failure exit below deletes it: the holders destroy what has been created by then)
  sbo_ctx* c = guard.get();
  sbo_ctx::Owned& own = c->own;
  c->device = device_id;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) c->n_cu = prop.multiProcessorCount;
  {
    const int rc = col_decide_resident(&c->decide_wg_per_cu);
    if (rc) return rc;
  }
  e = hipStreamCreateWithFlags(&own.stream.s, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&own.stream2.s, hipStreamNonBlocking);
  if (e == hipSuccess) {
    // the chain stream of an overlapped sweep carries many short kernels next to one long GEMM launch: highest priority,
    // so that its workgroups are placed ahead of the GEMM's when both queues have work
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = greatest = 0;
    e = hipStreamCreateWithPriority(&own.stream3.s, hipStreamNonBlocking, greatest);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&own.stream_audit.s, hipStreamNonBlocking, least);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&own.stream4.s, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&own.ev_factor.e, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&own.ev_w.e, hipEventDisableTiming);
    for (auto& ev : own.ev_grad)
      if (e == hipSuccess) e = hipEventCreateWithFlags(&ev.e, hipEventDisableTiming);
    for (auto& ev : own.ev_col)
      if (e == hipSuccess) e = hipEventCreateWithFlags(&ev.e, hipEventDisableTiming);
    for (auto& ev : own.ev_audit)
      if (e == hipSuccess) e = hipEventCreateWithFlags(&ev.e, hipEventDisableTiming);
  }
  if (e != hipSuccess) return hip_fail(e, "hipStreamCreate");
  for (auto& ev : own.ev) {
    e = hipEventCreate(&ev.e);
    if (e != hipSuccess) return hip_fail(e, "hipEventCreate");
  }
  for (auto& ev : own.ev_join) {
    e = hipEventCreate(&ev.e);
    if (e != hipSuccess) return hip_fail(e, "hipEventCreate");
  }
  if (hipHostMalloc(&own.h_c1.p, sizeof(unsigned long long) * (1 + 2 * kMaxQ), hipHostMallocDefault) != hipSuccess) return fail(SBO_E_HIP, "hipHostMalloc");
  if (hipHostMalloc(&own.h_back.p, sizeof(PinnedBack), hipHostMallocDefault) != hipSuccess) return fail(SBO_E_HIP, "hipHostMalloc");
  // the handles the code uses (the twin gets copies of some: shadow_ensure)
  c->stream = own.stream.s, c->stream2 = own.stream2.s, c->stream3 = own.stream3.s, c->stream_audit = own.stream_audit.s, c->stream4 = own.stream4.s;
  c->ev_factor = own.ev_factor.e, c->ev_w = own.ev_w.e;
  for (int i = 0; i < 8; ++i) c->ev[i] = own.ev[i].e;
  for (int i = 0; i < SBO_MAX_Q; ++i) c->ev_join[i] = own.ev_join[i].e;
  for (int i = 0; i < 3; ++i) c->col.ev[i] = own.ev_col[i].e;
  for (int i = 0; i < 4; ++i) c->ev_grad[i] = own.ev_grad[i].e;
  for (int i = 0; i < 2; ++i) c->audit.ev[i] = own.ev_audit[i].e;
  c->dist.h_c1 = (unsigned long long*)own.h_c1.p;
  c->h_back = (PinnedBack*)own.h_back.p;
  // the sweep's scalar block with the Lipschitz keys in it (internal.hpp: ScalBlock)
  c->lane[0].stream = c->stream;
  c->lane[1].stream = c->stream2;
  int rc = ensure(c->lane[0].scal, sizeof(ScalBlock));
  if (rc) return rc;
  c->Lmax = scal_block(c)->lip_keys;
  *out = guard.release();
  return SBO_OK;
}

int sbo_comm_destroy_internal(sbo_ctx* ctx);

// fp64 twin of an fp32 model: a context of its own (model arrays, candidate list, posterior buffers) on the owner's streams.  It
// borrows the handles; its `own` stays empty, so deleting it frees its buffers and its h_stage and nothing of the owner's
static int shadow_ensure(sbo_ctx* c) {
  if (c->recheck.shadow) return SBO_OK;
  std::unique_ptr<sbo_ctx> guard(new sbo_ctx());
  sbo_ctx* s = guard.get();
  s->is_shadow = true;
  s->device = c->device;
  s->n_cu = c->n_cu;
  s->decide_wg_per_cu = c->decide_wg_per_cu;
  s->stream = c->stream;
  s->stream2 = c->stream2;
  s->stream3 = c->stream3;
  s->stream4 = c->stream4;
  s->ev_factor = c->ev_factor;
  s->ev_w = c->ev_w;
  s->opt.chol_async = 0;
  for (int i = 0; i < 8; ++i) s->ev[i] = c->ev[i];
  s->h_back = c->h_back;
  s->opt.fp64_recheck = 0;
  s->opt.bilinear = 0;
  s->lane[0].stream = c->stream;
  s->lane[1].stream = c->stream2;
  int rc = ensure(s->lane[0].scal, sizeof(ScalBlock));
  if (rc) return rc;
  s->Lmax = scal_block(s)->lip_keys;
  c->recheck.shadow = guard.release();
  return SBO_OK;
}

int sbo_shutdown(sbo_ctx* c) {
  if (!c) return SBO_OK;
  (void)hipSetDevice(c->device);
  guard_audit_harvest(c, true);
  drain_streams(c);
  sbo_comm_destroy_internal(c);
  delete c;   // the twin first (Recheck), then every buffer, pinned block, event and stream (internal.hpp: the holders)
  return SBO_OK;
}

int sbo_synchronize(sbo_ctx* c) {
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  SBO_HIP(hipStreamSynchronize(c->stream));
  // (everything the library may still have in flight for this context: a deferred factorisation, the bases of a model)
  if (c->stream2) SBO_HIP(hipStreamSynchronize(c->stream2));
  if (c->stream3) SBO_HIP(hipStreamSynchronize(c->stream3));
  if (c->stream4) SBO_HIP(hipStreamSynchronize(c->stream4));
  if (c->stream_audit) SBO_HIP(hipStreamSynchronize(c->stream_audit));
  return SBO_OK;
}

}  // extern "C"

// One row per option, one macro per way of taking the value: its bounds, what it makes stale (internal.hpp: option_changed), its hook
namespace {
enum OptTake {
  kTakeBool,     // value ? 1 : 0
  kTakeInt,      // as given
  kTakeClamp,    // as given; outside lo .. hi the default `fallback`
  kTakeScaled    // double: value x scale
};
using Options = sbo_ctx::Options;
struct OptRow {
  const char* name;
  int Options::* ifield;
  double Options::* dfield;
  OptTake take;
  const char* reject;       // not nullptr: a value outside lo .. hi fails with this message
  int64_t lo, hi;
  int fallback;
  double scale;
  OptEffect effect;
  int (*hook)(sbo_ctx*, int64_t);   // runs on an accepted value, before it is stored
};
int hook_halo(sbo_ctx* c, int64_t) { for (auto& g : c->dist.halo_guess) g = -1; return SBO_OK; }
int hook_tensor_guess(sbo_ctx* c, int64_t) { c->tn.bump = 0; return SBO_OK; }
int hook_audit(sbo_ctx* c, int64_t) { guard_audit_harvest(c, true); return SBO_OK; }
// (test hook: the audit compares against the band times value / 1e6 -- with a band a thousand times too narrow it MUST count
// violations, which is how the suite shows that it compares real values; setting it clears the counts)
int hook_audit_scale(sbo_ctx* c, int64_t) {
  guard_audit_harvest(c, true);
  c->audit.samples = c->audit.violations = c->audit.skipped = 0;
  c->audit.worst = 0.0;
  return SBO_OK;
}
int hook_audit_every(sbo_ctx* c, int64_t) { c->audit.tick = 0; return SBO_OK; }
int hook_selftest(sbo_ctx* c, int64_t value) {
  if (value && !c->dist.comm && !c->dist.relay_allreduce)
    return fail(SBO_E_INVALID, "comm_selftest needs a communicator: call sbo_comm_init(ctx, 1, 0, id) with a unique id first");
  return SBO_OK;
}
#define OPT_BOOL(name, effect, hook) {#name, &Options::name, nullptr, kTakeBool, nullptr, 0, 0, 0, 0.0, effect, hook}
#define OPT_RANGE(name, lo, hi, msg, effect, hook) {#name, &Options::name, nullptr, kTakeInt, msg, lo, hi, 0, 0.0, effect, hook}
#define OPT_CLAMP(name, lo, hi, fallback, effect, hook) {#name, &Options::name, nullptr, kTakeClamp, nullptr, lo, hi, fallback, 0.0, effect, hook}
#define OPT_RAW(name, effect, hook) {#name, &Options::name, nullptr, kTakeInt, nullptr, 0, 0, 0, 0.0, effect, hook}
#define OPT_SCALED(key, field, scale, lo, hi, msg, effect, hook) {key, nullptr, &Options::field, kTakeScaled, msg, lo, hi, 0, scale, effect, hook}
const OptRow kOptions[] = {
    OPT_BOOL(halo_spec, kOptNothing, hook_halo),
    OPT_BOOL(comm_events, kOptNothing, nullptr),
    OPT_SCALED("cheb_tol_e17", cheb_tol, 1e-17, 0, 0, nullptr, kOptPlans, nullptr),
    OPT_RANGE(tensor_guess_pct, 10, 400, "tensor_guess_pct must be within 10 .. 400", kOptTensor, hook_tensor_guess),
    OPT_BOOL(tensor_cheb, kOptTensor, nullptr),
    OPT_CLAMP(exact_lazy, 0, 2, 1, kOptNothing, nullptr),   // 2: the late-recheck path runs on every sweep (test)
    OPT_BOOL(chol_async, kOptNothing, nullptr),
    OPT_RANGE(bilinear, 0, 2, "bilinear must be 0 (off), 1 (on; a model's first sweep by node interpolation) or 2 (on, K1b's plan from the first sweep)", kOptPlans, nullptr),
    OPT_BOOL(phase_events, kOptNothing, nullptr),
    // 0: off; 8 / 16 / 32 / 64: lanes per listed candidate (anything else: the default, 16)
    OPT_RAW(scan_waves, kOptNothing, nullptr),
    OPT_BOOL(set_lanes, kOptNothing, nullptr),
    OPT_BOOL(result_mirror, kOptNothing, nullptr),
    OPT_BOOL(set_fuse, kOptNothing, nullptr),
    OPT_RANGE(col_path, 0, 2, "col_path must be 0 (never), 1 (auto) or 2 (whenever the grid's shape allows)", kOptNothing, nullptr),
    OPT_RANGE(guard_audit, 0, 1 << 20, "guard_audit: samples per sweep, 0 (off) .. 1048576", kOptNothing, hook_audit),
    OPT_SCALED("guard_audit_scale_ppm", audit_scale, 1e-6, 1, 1000000000, "guard_audit_scale_ppm: 1 .. 1e9", kOptNothing, hook_audit_scale),
    OPT_RANGE(guard_audit_every, 1, 1 << 20, "guard_audit_every: 1 .. 1048576 sweeps", kOptNothing, hook_audit_every),
    OPT_RANGE(grad_defer, 0, 3, "grad_defer must be 0 .. 3", kOptInterp, nullptr),
    OPT_BOOL(k1_sched, kOptNothing, nullptr),
    OPT_BOOL(k1_resident, kOptNothing, nullptr),        // (read per sweep: launch_posterior_gemm decides what it takes from memory)
    OPT_BOOL(k1_skip_safe, kOptNothing, nullptr),       // (read per sweep: the decision is taken at every sweep's b and band)
    OPT_BOOL(k1_cells, kOptNothing, nullptr),           // (read per sweep: gemm_post_part picks the head of a resident plan's lean-2 sweep)
    OPT_BOOL(col_overlap, kOptNothing, nullptr),
    OPT_RANGE(col_queue, 64, 128, "col_queue must be within 64 .. 128 (the default)", kOptNothing, nullptr),
    OPT_BOOL(scan_blocks, kOptNothing, nullptr),
    OPT_RANGE(fuse_classify, -1, 1, "fuse_classify must be -1 (auto), 0 or 1", kOptNothing, nullptr),
    OPT_BOOL(goose_pairs, kOptNothing, nullptr),
    OPT_RANGE(guard_band, 0, 2, "guard_band must be 0 (off), 1 (on) or 2 (re-evaluate on every sweep)", kOptPlansBand, nullptr),
    OPT_BOOL(fp64_recheck, kOptNothing, nullptr),       // (takes effect at the next sbo_model_set: the fp64 twin is built there)
    OPT_BOOL(comm_selftest, kOptNothing, hook_selftest),
    OPT_RANGE(refine_lds, 0, 1, "refine_lds must be 0 (stream M) or 1 (LDS when it fits)", kOptNothing, nullptr),
    OPT_RANGE(lipschitz_lds, 0, 1, "lipschitz_lds must be 0 (stream X_norm and alpha) or 1 (LDS when they fit)", kOptNothing, nullptr),
    OPT_RANGE(list_index, -1, 1, "list_index must be -1 (auto), 0 (never) or 1 (always)", kOptNothing, nullptr),
    OPT_RANGE(posterior_path, 0, 2, "posterior_path must be 0 (auto), 1 (generic) or 2 (generic, chunked)", kOptPosterior, nullptr),
};
#undef OPT_BOOL
#undef OPT_RANGE
#undef OPT_CLAMP
#undef OPT_RAW
#undef OPT_SCALED
}  // namespace

int sbo_set_option(sbo_ctx* c, const char* key, int64_t value) {
  if (!c || !key) return fail(SBO_E_INVALID, "ctx/key is NULL");
  for (const OptRow& r : kOptions) {
    if (strcmp(key, r.name)) continue;
    const bool inside = value >= r.lo && value <= r.hi;
    if (r.reject && !inside) return fail(SBO_E_INVALID, r.reject);
    if (r.hook) {
      const int rc = r.hook(c, value);
      if (rc) return rc;
    }
    switch (r.take) {
      case kTakeBool: c->opt.*r.ifield = value ? 1 : 0; break;
      case kTakeInt: c->opt.*r.ifield = (int)value; break;
      case kTakeClamp: c->opt.*r.ifield = inside ? (int)value : r.fallback; break;
      case kTakeScaled: c->opt.*r.dfield = (double)value * r.scale; break;
    }
    option_changed(c, r.effect);
    return SBO_OK;
  }
  return fail(SBO_E_INVALID, std::string("unknown option ") + key);
}

extern "C" {

static int model_set_impl(sbo_ctx* c, int dtype, const char* kernel, int n, int d, int q, const double* X_mean,
                          const double* X_std, const double* Y_mean, const double* Y_std, const double* X_norm,
                          const double* Y_norm, const double* hypopt, const double* const* invK, const double* mean_prior = nullptr) {
  // (a standing audit of the last sweep reads the outgoing model's matrix out of the build workspace this call reuses)
  if (c) guard_audit_harvest(c, true);
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (!kernel || strcmp(kernel, "RBF") != 0)      // models/GP_Safe.py:159-162
    return fail(SBO_E_INVALID, std::string("ERROR no kernel with name ") + (kernel ? kernel : "(null)"));
  if (dtype != SBO_F64 && dtype != SBO_F32) return fail(SBO_E_INVALID, "dtype must be SBO_F64 or SBO_F32");
  if (n < 1 || n > SBO_MAX_N) return fail(SBO_E_INVALID, "n out of range [1, SBO_MAX_N]");
  if (d < 1 || d > SBO_MAX_D) return fail(SBO_E_INVALID, "d out of range [1, SBO_MAX_D]");
  if (q < 1 || q > SBO_MAX_Q) return fail(SBO_E_INVALID, "q out of range [1, SBO_MAX_Q]");
  if (!X_mean || !X_std || !Y_mean || !Y_std || !X_norm || !Y_norm || !hypopt)
    return fail(SBO_E_INVALID, "NULL model array");
  SBO_HIP(hipSetDevice(c->device));
  c->has_model = false;
  model_changed(c);
  ModelConst& mc = c->mc;
  memset(&mc, 0, sizeof(mc));
  mc.n = n; mc.d = d; mc.q = q;
  mc.npad = (n + 15) / 16 * 16;
  mc.dpad = d <= 2 ? 2 : (d <= 4 ? 4 : 8);
  mc.factor = invK ? SBO_FACTOR_INVK : SBO_FACTOR_CHOL;
  for (int a = 0; a < kMaxD; ++a) { mc.X_mean[a] = a < d ? X_mean[a] : 0.0; mc.X_std[a] = a < d ? X_std[a] : 1.0; mc.X_rstd[a] = 1.0 / mc.X_std[a]; }
  c->h_Xnorm.assign(X_norm, X_norm + (size_t)n * d);
  c->h_Ynorm.assign(Y_norm, Y_norm + (size_t)n * q);
  const double f32eps = (double)std::numeric_limits<float>::epsilon();
  for (int o = 0; o < q; ++o) {
    mc.Y_mean[o] = Y_mean[o];
    mc.Y_std[o] = Y_std[o];
    mc.mp[o] = (o == 0) ? 0.0 : (-2.0 * Y_mean[o]) / Y_std[o];          // GP_Safe.py:331-332
    if (mean_prior) mc.mp[o] = mean_prior[o];                            // the caller's prior (GP_Robust.py:322-324: zero)
    mc.sf2[o] = std::exp(2.0 * hypopt[(size_t)d * q + o]);               // GP_Safe.py:338
    mc.sn2[o] = std::exp(2.0 * hypopt[(size_t)(d + 1) * q + o]) + f32eps;   // GP_Safe.py:229
    for (int a = 0; a < d; ++a) {
      const double ell = std::exp(2.0 * hypopt[(size_t)a * q + o]);
      mc.vinv[o][a] = std::pow(ell, -0.5);                               // GP_Safe.py:112
      mc.inv_ell[o][a] = 1.0 / ell;
    }
  }
  c->dtype = dtype;
  ++c->model_serial;
  // derived arrays (As, sqA, Xn, rhs), factorisation, alpha and the fragment images of the factor: on the device (model.hip)
  int rc = model_build(c, invK, X_norm, Y_norm);
  if (rc) return rc;
  // A grid is resident and qualifies for the GEMM posterior: its per-(model, grid) tables are enqueued now, so that they
  // run while the caller is on its way from this call to the sweep (the bases' ranks came back with the build's own
  // synchronisation; nothing here waits).  A grid change before the next sweep simply drops the plan.
  if (!c->is_shadow && interp_applicable(c)) {
    if ((rc = interp_setup(c))) return rc;
  } else if (!c->is_shadow && bilinear_applicable(c) && (rc = bilinear_setup(c))) return rc;
  if (dtype == SBO_F32 && c->opt.fp64_recheck && !c->is_shadow) {
    // the fp64 twin: same constants, double arrays and factor images (built from the same inputs)
    if ((rc = shadow_ensure(c))) return rc;
    sbo_ctx* s = c->recheck.shadow;
    s->mc = c->mc;
    s->dtype = SBO_F64;
    s->has_model = false;
    model_changed(s);
    s->h_Xnorm = c->h_Xnorm;
    s->h_Ynorm = c->h_Ynorm;
    ++s->model_serial;
    if ((rc = model_build(s, invK, X_norm, Y_norm))) return rc;
    s->has_model = true;
    c->recheck.serial = c->model_serial;
  }
  c->has_model = true;
  return SBO_OK;
}

int sbo_model_set(sbo_ctx* c, int dtype, const char* kernel, int n, int d, int q, const double* X_mean,
                  const double* X_std, const double* Y_mean, const double* Y_std, const double* X_norm,
                  const double* Y_norm, const double* hypopt, const double* invK) {
  const double* parts[SBO_MAX_Q];
  if (invK && q >= 1 && q <= SBO_MAX_Q && n >= 1)
    for (int o = 0; o < q; ++o) parts[o] = invK + (size_t)o * n * n;
  return model_set_impl(c, dtype, kernel, n, d, q, X_mean, X_std, Y_mean, Y_std, X_norm, Y_norm, hypopt, invK ? parts : nullptr);
}

int sbo_model_set_list(sbo_ctx* c, int dtype, const char* kernel, int n, int d, int q, const double* X_mean,
                       const double* X_std, const double* Y_mean, const double* Y_std, const double* X_norm,
                       const double* Y_norm, const double* hypopt, const double* const* invK_list) {
  if (invK_list && q >= 1 && q <= SBO_MAX_Q)
    for (int o = 0; o < q; ++o)
      if (!invK_list[o]) return fail(SBO_E_INVALID, "invK_list holds a NULL matrix");
  return model_set_impl(c, dtype, kernel, n, d, q, X_mean, X_std, Y_mean, Y_std, X_norm, Y_norm, hypopt, invK_list);
}

int sbo_model_set_prior(sbo_ctx* c, int dtype, const char* kernel, int n, int d, int q, const double* X_mean,
                        const double* X_std, const double* Y_mean, const double* Y_std, const double* X_norm,
                        const double* Y_norm, const double* hypopt, const double* const* invK_list, const double* mean_prior) {
  if (invK_list && q >= 1 && q <= SBO_MAX_Q)
    for (int o = 0; o < q; ++o)
      if (!invK_list[o]) return fail(SBO_E_INVALID, "invK_list holds a NULL matrix");
  if (mean_prior && q >= 1 && q <= SBO_MAX_Q)
    for (int o = 0; o < q; ++o)
      if (!std::isfinite(mean_prior[o])) return fail(SBO_E_INVALID, "mean_prior must be finite");
  return model_set_impl(c, dtype, kernel, n, d, q, X_mean, X_std, Y_mean, Y_std, X_norm, Y_norm, hypopt, invK_list, mean_prior);
}

// From (X_norm, Y_norm) to a resident model without the host in the middle: the DE of every output side by
// side, a polish from every output's best, then the build of sbo_model_set_prior(..., hypopt_out, NULL, mean_prior).  Everything that
// can fail before the build is checked before the resident model is touched.
int sbo_model_fit(sbo_ctx* c, int dtype, const char* kernel, int n, int d, int q, const double* X_mean, const double* X_std,
                  const double* Y_mean, const double* Y_std, const double* X_norm, const double* Y_norm, const double* mean_prior,
                  const sbo_fit_opts* opts, const double* init_pop, double* hypopt_out, sbo_fit_report* report) {
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (!kernel || strcmp(kernel, "RBF") != 0)      // models/GP_Safe.py:159-162
    return fail(SBO_E_INVALID, std::string("ERROR no kernel with name ") + (kernel ? kernel : "(null)"));
  if (dtype != SBO_F64 && dtype != SBO_F32) return fail(SBO_E_INVALID, "dtype must be SBO_F64 or SBO_F32");
  if (n < 1 || n > SBO_MAX_N) return fail(SBO_E_INVALID, "n out of range [1, SBO_MAX_N]");
  if (d < 1 || d > SBO_MAX_D) return fail(SBO_E_INVALID, "d out of range [1, SBO_MAX_D]");
  if (q < 1 || q > SBO_MAX_Q) return fail(SBO_E_INVALID, "q out of range [1, SBO_MAX_Q]");
  if (!X_mean || !X_std || !Y_mean || !Y_std || !X_norm || !Y_norm) return fail(SBO_E_INVALID, "NULL model array");
  if (!opts || !init_pop || !hypopt_out) return fail(SBO_E_INVALID, "NULL argument");
  if (opts->P < 4 || opts->maxiter < 0) return fail(SBO_E_INVALID, "P or maxiter out of range");
  const int D = d + 2;
  for (int a = 0; a < D; ++a)
    if (!(opts->lo[a] <= opts->hi[a])) return fail(SBO_E_INVALID, "bounds need lo <= hi");
  if (mean_prior)
    for (int o = 0; o < q; ++o)
      if (!std::isfinite(mean_prior[o])) return fail(SBO_E_INVALID, "mean_prior must be finite");
  uint64_t seeds[SBO_MAX_Q];
  for (int o = 0; o < q; ++o) seeds[o] = opts->seed + (uint64_t)o;
  const double f32eps = (double)std::numeric_limits<float>::epsilon();
  FitBatchResult r;
  int rc = fit_batch(c, n, d, q, X_norm, Y_norm, opts->P, opts->lo, opts->hi, init_pop, seeds, opts->maxiter, opts->tol, opts->atol,
                     opts->polish ? 1 : 0, opts->polish_maxiter > 0 ? opts->polish_maxiter : 10000,
                     opts->polish_ftol > 0.0 ? opts->polish_ftol : f32eps, opts->polish_gtol > 0.0 ? opts->polish_gtol : 1e-8, r);
  if (rc) return rc;
  for (int o = 0; o < q; ++o)
    if (!std::isfinite(r.nll[o])) return fail(SBO_E_INVALID, "the fit of output " + std::to_string(o) + " found no member with a finite likelihood");
  for (int o = 0; o < q; ++o)
    for (int a = 0; a < D; ++a) hypopt_out[(size_t)a * q + o] = r.x[o][a];
  const auto t1 = clk::now();
  rc = model_set_impl(c, dtype, kernel, n, d, q, X_mean, X_std, Y_mean, Y_std, X_norm, Y_norm, hypopt_out, nullptr, mean_prior);
  const auto t2 = clk::now();
  if (report) {
    memset(report, 0, sizeof(*report));
    for (int o = 0; o < q; ++o) {
      report->de_nll[o] = r.de_nll[o];
      report->nll[o] = r.nll[o];
      report->generations[o] = r.generations[o];
      report->polish_status[o] = r.polish_status[o];
      report->polish_evals[o] = r.polish_evals[o];
      report->polished[o] = r.polished[o];
    }
    report->de_ms = r.de_ms;
    report->polish_ms = r.polish_ms;
    report->build_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
    report->total_ms = std::chrono::duration<double, std::milli>(t2 - t0).count();
    report->host_syncs = r.host_syncs;
  }
  return rc;
}

// What sbo_model_append, sbo_model_append_batch and sbo_model_remove ask of the resident model once their arguments are checked:
// `rows` = +1 with block == false (one row, k_model_append), +k with block == true (the block kernels), -1 (row `index` leaves).
struct ModelUpdateRequest { int rows; bool block; int index; const double *x_norm_new /* [rows][d] */, *y_norm_new /* [rows][q] */; };

// The one sequence of a model update under frozen hyper-parameters and normalisation.  Every output's update is computed and checked
// before anything is written: a refused update leaves the model as it was.  The fp64 twin of this model makes the same public call and
// must accept before the owner commits (a twin left behind by an earlier model takes no part); until the owner is done it is not current.
static int model_update_run(sbo_ctx* c, const ModelUpdateRequest& r) {
  ModelConst& mc = c->mc;
  const int d = mc.d;
  SBO_HIP(hipSetDevice(c->device));
  int rc;
  if ((rc = factor_sync(c))) return rc;                    // (the update works on the resident factor)
  ModelUpdate u;
  if (r.rows < 0) u = model_update_staged(c, -1, r.index);
  else if ((rc = r.block ? model_append_block_stage(c, r.rows, r.x_norm_new, r.y_norm_new, u) : model_append_stage(c, r.x_norm_new, r.y_norm_new, u)))
    return rc;
  const bool twin = twin_current(c);
  if (twin) {
    sbo_ctx* s = c->recheck.shadow;
    rc = r.rows < 0 ? sbo_model_remove(s, r.index)
                    : (r.block ? sbo_model_append_batch(s, r.rows, r.x_norm_new, r.y_norm_new) : sbo_model_append(s, r.x_norm_new, r.y_norm_new));
    if (rc) return rc;
    c->recheck.serial = Recheck::kNoSerial;
  }
  if ((rc = model_update_commit(c, u))) return rc;
  // the derived arrays over the rows the model now holds (device), then one re-pack of the factor images
  if (r.rows < 0) c->h_Xnorm.erase(c->h_Xnorm.begin() + (size_t)r.index * d, c->h_Xnorm.begin() + (size_t)(r.index + 1) * d);
  else c->h_Xnorm.insert(c->h_Xnorm.end(), r.x_norm_new, r.x_norm_new + (size_t)r.rows * d);
  if (r.rows < 0) c->h_Ynorm.erase(c->h_Ynorm.begin() + (size_t)r.index * mc.q, c->h_Ynorm.begin() + (size_t)(r.index + 1) * mc.q);
  else c->h_Ynorm.insert(c->h_Ynorm.end(), r.y_norm_new, r.y_norm_new + (size_t)r.rows * mc.q);
  mc.n += r.rows;
  mc.npad = (mc.n + 15) / 16 * 16;
  if ((rc = model_prep(c, c->h_Xnorm.data()))) return rc;
  if ((rc = model_repack(c))) return rc;
  ++c->model_serial;
  if (twin) c->recheck.serial = c->model_serial;
  model_changed(c);
  return SBO_OK;
}

// one more observation under frozen hyper-parameters and normalisation, O(n^2) on the
// device instead of a refit (the reference always refits and renormalises, models/GP_Safe.py:283-304 -- this is an
// opt-in fast path, not its behaviour).
int sbo_model_append(sbo_ctx* c, const double* x_norm_new, const double* y_norm_new) {
  if (c) guard_audit_harvest(c, true);
  if (!c || !x_norm_new || !y_norm_new) return fail(SBO_E_INVALID, "NULL argument");
  if (!c->has_model || !c->factor.present()) return fail(SBO_E_NO_MODEL, "sbo_model_set has not been called");
  for (int a = 0; a < c->mc.d; ++a)
    if (!std::isfinite(x_norm_new[a])) return fail(SBO_E_INVALID, "x_norm_new must be finite");
  for (int o = 0; o < c->mc.q; ++o)
    if (!std::isfinite(y_norm_new[o])) return fail(SBO_E_INVALID, "y_norm_new must be finite");
  if (c->mc.n + 1 > SBO_MAX_N) return fail(SBO_E_UNSUPPORTED, "model is at its capacity: rebuild it with sbo_model_set");
  return model_update_run(c, {1, false, -1, x_norm_new, y_norm_new});
}

// k observations in one block update: one verdict wait, one re-pack, one invalidation for the k rows.
int sbo_model_append_batch(sbo_ctx* c, int k, const double* x_norm_new, const double* y_norm_new) {
  if (c) guard_audit_harvest(c, true);
  if (!c || !x_norm_new || !y_norm_new) return fail(SBO_E_INVALID, "NULL argument");
  if (k < 1 || k > SBO_MAX_APPEND) return fail(SBO_E_INVALID, "k out of range [1, SBO_MAX_APPEND]");
  if (!c->has_model || !c->factor.present()) return fail(SBO_E_NO_MODEL, "sbo_model_set has not been called");
  for (size_t i = 0; i < (size_t)k * c->mc.d; ++i)
    if (!std::isfinite(x_norm_new[i])) return fail(SBO_E_INVALID, "x_norm_new must be finite");
  for (size_t i = 0; i < (size_t)k * c->mc.q; ++i)
    if (!std::isfinite(y_norm_new[i])) return fail(SBO_E_INVALID, "y_norm_new must be finite");
  if (c->mc.n + k > SBO_MAX_N) return fail(SBO_E_UNSUPPORTED, "the block does not fit below SBO_MAX_N: rebuild the model with sbo_model_set");
  return model_update_run(c, {k, true, -1, x_norm_new, y_norm_new});
}

// Observation `index` leaves the resident model, O(n^2) on the device; the rows behind it move up by one.
int sbo_model_remove(sbo_ctx* c, int index) {
  if (c) guard_audit_harvest(c, true);
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (!c->has_model || !c->factor.present()) return fail(SBO_E_NO_MODEL, "sbo_model_set has not been called");
  if (index < 0 || index >= c->mc.n) return fail(SBO_E_INVALID, "index out of range [0, n)");
  if (c->mc.n == 1) return fail(SBO_E_INVALID, "a model holds at least one observation");
  return model_update_run(c, {-1, false, index, nullptr, nullptr});
}

// Leave-one-out diagnostics of the resident model: read-only, O(n^2) on the device, O(n q) bytes back.
int sbo_model_loo(sbo_ctx* c, double b, double* resid_out, double* var_out, sbo_model_loo_result* result) {
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (!std::isfinite(b) || b < 0.0) return fail(SBO_E_INVALID, "b must be finite and >= 0");
  if (const int rcb = model_reader_begin(c, "sbo_model_loo", false)) return rcb;     // (the sums run over the resident factor)
  const int n = c->mc.n, q = c->mc.q;
  const unsigned char* h = nullptr;
  const int rc = model_loo(c, b, resid_out || var_out, &h);
  if (rc) return rc;
  const size_t head = sizeof(LooSummary) * kMaxQ, nq = sizeof(double) * (size_t)n * q;
  if (resid_out) std::memcpy(resid_out, h + head, nq);
  if (var_out) std::memcpy(var_out, h + head + nq, nq);
  if (result) {
    std::memset(result, 0, sizeof(*result));
    result->n = n;
    result->q = q;
    const LooSummary* s = (const LooSummary*)h;
    for (int o = 0; o < q; ++o) {
      result->logdet[o] = s[o].logdet;
      result->lpd[o] = s[o].lpd;
      result->z_max[o] = s[o].z_max;
      result->z_argmax[o] = s[o].z_argmax;
      result->outside[o] = s[o].outside;
    }
  }
  return SBO_OK;
}

static int alloc_workspace(sbo_ctx* c) {
  const size_t es = c->dtype == SBO_F64 ? 8 : 4;
  const size_t n = (size_t)std::max<long long>(c->cs.n_local, 1);
  int rc;
  const void *had_m = c->mean.p, *had_v = c->var.p;
  if ((rc = ensure(c->mean, es * n * c->mc.q))) return rc;
  if ((rc = ensure(c->var, es * n * c->mc.q))) return rc;
  if (c->mean.p != had_m || c->var.p != had_v) post_regions_written(c);     // (new buffers hold nothing of the plan's)
  return SBO_OK;
}

int sbo_candidates_points(sbo_ctx* c, const void* points, int points_dtype, int64_t n_local, int d, int64_t first) {
  if (c) guard_audit_harvest(c, true);
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (n_local < 0 || (n_local > 0 && !points)) return fail(SBO_E_INVALID, "bad points / n_local");
  if (d < 1 || d > SBO_MAX_D) return fail(SBO_E_INVALID, "d out of range");
  if (points_dtype != SBO_F64 && points_dtype != SBO_F32) return fail(SBO_E_INVALID, "points_dtype");
  SBO_HIP(hipSetDevice(c->device));
  const size_t es = points_dtype == SBO_F64 ? 8 : 4;
  int rc = ensure(c->pts, es * (size_t)std::max<int64_t>(n_local, 1) * d);
  if (rc) return rc;
  if (n_local) {
    SBO_HIP(hipMemcpyAsync(c->pts.p, points, es * (size_t)n_local * d, hipMemcpyHostToDevice, c->stream));
    SBO_HIP(hipStreamSynchronize(c->stream));
  }
  memset(&c->cs, 0, sizeof(c->cs));
  c->cs.kind = 0; c->cs.d = d; c->cs.pts_dtype = points_dtype; c->cs.pts = c->pts.p;
  c->cs.n_local = n_local; c->cs.first = first;
  c->dist.grid_total = n_local;
  c->has_cand = true;
  candidates_changed(c, kCandPoints);
  return SBO_OK;
}

static int grid_set(sbo_ctx* c, int d, const double* lo, const double* hi, const int64_t* count, int64_t first, int64_t n_local, CandKind kind) {
  if (c) guard_audit_harvest(c, true);
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (d < 1 || d > SBO_MAX_D || !lo || !hi || !count) return fail(SBO_E_INVALID, "bad grid description");
  long double total = 1;
  for (int a = 0; a < d; ++a) {
    if (count[a] < 1) return fail(SBO_E_INVALID, "grid count must be >= 1");
    total *= (long double)count[a];
  }
  if (total > 9.0e18L) return fail(SBO_E_INVALID, "grid too large");
  if (first < 0 || n_local < 0 || (long double)first + (long double)n_local > total)
    return fail(SBO_E_INVALID, "shard range outside the grid");
  memset(&c->cs, 0, sizeof(c->cs));
  c->cs.kind = 1; c->cs.d = d; c->cs.n_local = n_local; c->cs.first = first;
  for (int a = 0; a < d; ++a) {
    c->cs.lo[a] = lo[a]; c->cs.hi[a] = hi[a]; c->cs.count[a] = count[a];
    c->cs.step[a] = count[a] > 1 ? (hi[a] - lo[a]) / (double)(count[a] - 1) : 0.0;
  }
  for (int a = d; a < kMaxD; ++a) c->cs.count[a] = 1;
  c->dist.grid_total = (long long)total;
  c->has_cand = true;
  candidates_changed(c, kind);
  return SBO_OK;
}

int sbo_candidates_grid(sbo_ctx* c, int d, const double* lo, const double* hi, const int64_t* count, int64_t first,
                        int64_t n_local) {
  return grid_set(c, d, lo, hi, count, first, n_local, kCandGrid);
}

int sbo_candidates_grid_sharded(sbo_ctx* c, int d, const double* lo, const double* hi, const int64_t* count,
                                int64_t* first_out, int64_t* n_local_out) {
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (d < 1 || d > SBO_MAX_D || !lo || !hi || !count) return fail(SBO_E_INVALID, "bad grid description");
  long long stride = 1;
  for (int a = 0; a < d - 1; ++a) {
    if (count[a] < 1) return fail(SBO_E_INVALID, "grid count must be >= 1");
    stride *= count[a];
  }
  if (count[d - 1] < 1) return fail(SBO_E_INVALID, "grid count must be >= 1");
  const long long planes = count[d - 1];
  const int W = c->dist.world, r = c->dist.rank;
  std::vector<long long> first_of(W + 1);
  for (int i = 0; i <= W; ++i) first_of[i] = (planes * i / W) * stride;
  int rc = grid_set(c, d, lo, hi, count, first_of[r], first_of[r + 1] - first_of[r], kCandGridSharded);
  if (rc) return rc;
  c->dist.first_of = first_of;
  if ((rc = ensure(c->dist.shard_first, sizeof(long long) * (W + 1)))) return rc;
  SBO_HIP(hipMemcpy(c->dist.shard_first.p, first_of.data(), sizeof(long long) * (W + 1), hipMemcpyHostToDevice));
  if (first_out) *first_out = first_of[r];
  if (n_local_out) *n_local_out = first_of[r + 1] - first_of[r];
  return SBO_OK;
}

}  // extern "C"

static int check_ready(sbo_ctx* c) {
  if (!c) return fail(SBO_E_INVALID, "ctx is NULL");
  if (!c->has_model) return fail(SBO_E_NO_MODEL, "sbo_model_set has not been called");
  if (!c->has_cand) return fail(SBO_E_NO_CANDIDATES, "no candidates resident");
  if (c->cs.d != c->mc.d) return fail(SBO_E_INVALID, "ERROR W and X_norm dimension should be same");  // GP_Safe.py:159
  return SBO_OK;
}

int sbo::posterior_enqueue(sbo_ctx* c, const PostRequest& req, PostOutcome* out) {
  PostOutcome none;
  if (!out) out = &none;
  *out = PostOutcome{};
  int rc = check_ready(c);
  if (rc) return rc;
  SBO_HIP(hipSetDevice(c->device));
  guard_audit_harvest(c, false);
  if ((rc = alloc_workspace(c))) return rc;
  // (a standing audit of the last sweep may not have taken its sample of mean / var yet: it is a few microseconds of work on its stream)
  if (c->audit.pending) SBO_HIP(hipStreamWaitEvent(c->stream, c->audit.ev[0], 0));
  if (c->cs.n_local > 0 && (rc = launch_posterior(c, req, *out))) return rc;
  c->posterior_valid = true;
  c->post_l0_missing = req.sweep_lean != 0;
  return SBO_OK;
}

extern "C" {

double sbo_algorithmic_flops(const sbo_ctx* c) {
  const double n = c->mc.n, d = c->mc.d, q = c->mc.q;
  return q * (n * n + (2 * d + 10) * n) * (double)c->cs.n_local;
}

int sbo_posterior_run(sbo_ctx* c) {
  int rc = check_ready(c);
  if (rc) return rc;
  SBO_HIP(hipSetDevice(c->device));
  SBO_HIP(hipEventRecord(c->ev[0], c->stream));
  PostOutcome out;
  if ((rc = posterior_enqueue(c, PostRequest{}, &out))) return rc;
  SBO_HIP(k1_stop(c, out));
  SBO_HIP(hipEventSynchronize(c->ev[1]));
  float ms = 0;
  SBO_HIP(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
  memset(&c->prof, 0, sizeof(c->prof));
  c->prof.posterior_ms = ms;
  c->prof.total_ms = ms;
  c->prof.posterior_flops = sbo_algorithmic_flops(c);
  c->prof.candidates = c->cs.n_local;
  c->prof.posterior_launches = c->cs.n_local > 0 ? 1 : 0;
  return SBO_OK;
}

int sbo_posterior_get(sbo_ctx* c, void* mean_out, void* var_out) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!c->posterior_valid && (rc = sbo_posterior_run(c))) return rc;
  const size_t es = c->dtype == SBO_F64 ? 8 : 4;
  const size_t bytes = es * (size_t)c->cs.n_local * c->mc.q;
  if (bytes == 0) return SBO_OK;
  DevBuf tmp;
  if ((rc = ensure(tmp, bytes))) return rc;
  for (int which = 0; which < 2; ++which) {
    void* dst = which ? var_out : mean_out;
    if (!dst) continue;
    rc = launch_soa_to_aos(c, which ? c->var.p : c->mean.p, tmp.p);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(dst, tmp.p, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(e, "copy posterior to host");
  }
  return SBO_OK;
}

int sbo_bounds(sbo_ctx* c, double b, int index, int kind, void* out) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (index < 0 || index >= c->mc.q) return fail(SBO_E_INVALID, "output index out of range");
  if (kind < SBO_MEAN || kind > SBO_VAR) return fail(SBO_E_INVALID, "bad bound kind");
  if (!out) return fail(SBO_E_INVALID, "out is NULL");
  if (!c->posterior_valid && (rc = sbo_posterior_run(c))) return rc;
  const size_t es = c->dtype == SBO_F64 ? 8 : 4;
  const size_t bytes = es * (size_t)c->cs.n_local;
  if (bytes == 0) return SBO_OK;
  DevBuf tmp;
  if ((rc = ensure(tmp, bytes))) return rc;
  rc = launch_bound(c, b, index, kind, tmp.p);
  if (!rc) {
    hipError_t e = hipMemcpyAsync(out, tmp.p, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = hip_fail(e, "copy bounds to host");
  }
  return rc;
}

int sbo_profile_get(sbo_ctx* c, sbo_profile* out) {
  if (!c || !out) return fail(SBO_E_INVALID, "NULL argument");
  *out = c->prof;
  out->posterior_kernel = c->last_k1;
  out->posterior_executed_flops = c->prof.posterior_launches ? c->last_k1_flops : 0.0;
  out->posterior_setup_ms = c->bl.setup_ms;
  guard_audit_harvest(c, false);
  out->guard_audit_samples = c->audit.samples;
  out->guard_audit_violations = c->audit.violations;
  out->guard_audit_worst = c->audit.worst;
  out->guard_audit_skipped = c->audit.skipped;
  // the guard band of the posterior that is resident (K1b measures it on the device: a small read-back, off the hot path)
  for (int o = 0; o < SBO_MAX_Q; ++o)
    out->guard_dm[o] = out->guard_dv[o] = out->guard_rl[o] = out->guard_analytic_dm[o] = out->guard_analytic_dv[o] = out->guard_probe_dm[o] = out->guard_probe_dv[o] = 0.0;
  if (c->gb.active && c->opt.guard_band && c->gb.buf.p && c->posterior_valid) {
    if (!c->gb.host_valid) {               // (once per plan: the profile is read after every sweep of a timing loop)
      GuardBand hb;
      if (c->gb.mirrored) {
        // (the plan's band kernel wrote a copy into the pinned block; the sweep whose posterior is valid has synchronised since)
        memcpy(&hb, c->h_back->guard_band, sizeof(hb));
      } else {
        SBO_HIP(hipSetDevice(c->device));
        SBO_HIP(hipMemcpyAsync(&hb, c->gb.buf.p, sizeof(hb), hipMemcpyDeviceToHost, c->stream));
        SBO_HIP(hipStreamSynchronize(c->stream));
      }
      for (int o = 0; o < SBO_MAX_Q; ++o) {
        c->gb.host[o] = hb.dm[o]; c->gb.host[SBO_MAX_Q + o] = hb.dv[o]; c->gb.host[2 * SBO_MAX_Q + o] = hb.rl[o];
        c->gb.host[3 * SBO_MAX_Q + o] = hb.an_m[o]; c->gb.host[4 * SBO_MAX_Q + o] = hb.an_v[o];
        c->gb.host[5 * SBO_MAX_Q + o] = hb.pr_m[o]; c->gb.host[6 * SBO_MAX_Q + o] = hb.pr_v[o];
      }
      c->gb.host_valid = true;
    }
    for (int o = 0; o < c->mc.q; ++o) {
      out->guard_dm[o] = c->gb.host[o];
      out->guard_dv[o] = c->gb.host[SBO_MAX_Q + o];
      out->guard_rl[o] = c->gb.host[2 * SBO_MAX_Q + o];
      out->guard_analytic_dm[o] = c->gb.host[3 * SBO_MAX_Q + o];
      out->guard_analytic_dv[o] = c->gb.host[4 * SBO_MAX_Q + o];
      out->guard_probe_dm[o] = c->gb.host[5 * SBO_MAX_Q + o];
      out->guard_probe_dv[o] = c->gb.host[6 * SBO_MAX_Q + o];
    }
  }
  return SBO_OK;
}

}  // extern "C"
