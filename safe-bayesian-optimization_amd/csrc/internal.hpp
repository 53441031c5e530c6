// internal.hpp -- shared declarations of libsafebo.so (host side + kernel argument blocks).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>
#include "../../include/safebo.h"

namespace sbo {

// The direct reference of the guard band (guard.hip: k_ref_list) keeps 16 cross-covariance vectors of npad doubles + 32 KB of partial
// sums in LDS: 160 KB at npad = 1024.  Larger models do not take the GEMM posteriors with a caller's matrix (they run K1g, whose
// factor is made on demand) -- ADVICE r04.
constexpr int kGuardRefMaxNpad = 1008;
constexpr int kMaxD = SBO_MAX_D;
constexpr int kMaxQ = SBO_MAX_Q;

// ---- The three small shared blocks, each laid out once.  A member is a region at a fixed offset with room for its largest writer (its pad:
// the region's size less the member's); the asserts fail the build when a region moves, overlaps the next one or is too small.  SweepScalars
// and GuardBand are defined later (sets.hip, device_common.hpp): their regions are bytes here, the assert on their size stands at the type.
// Recheck::list (sets_recheck.inc.hpp) = RcHead, then the list of flagged candidates.  A recheck reads back the part in front of gkeys.
struct RcScal {
  unsigned long long ulo_key, uhi_key, vmax_key;   // interval of u*, lower end of the largest variance over M
  long long count;                                 // length of the first list (k_rc_flag)
};
struct RcHead {
  RcScal sc;
  unsigned long long deferred;       // candidates a set phase deferred (RcExp, k_rc_gdefer) / contenders of an arg-min (k_rc_lflag)
  unsigned long long lmin_key;       // rc_argmin_contenders: min over the mask of the upper end of lcb_0
  unsigned long long all_ranks;      // rc_count_all: the largest `deferred` over the ranks (the collective's word)
  unsigned long long all_ranks_back; // ... and where that word lands in the pinned copy (on the device: unused)
  unsigned long long gkeys[kMaxQ];   // k_rc_gmax: per constraint, max over G_c of the lower end of var_0
  unsigned char pad[192 - sizeof(gkeys)];
};
static_assert(offsetof(RcHead, deferred) == 32 && offsetof(RcHead, lmin_key) == 40 && offsetof(RcHead, all_ranks) == 48 &&
              offsetof(RcHead, all_ranks_back) == 56 && offsetof(RcHead, gkeys) == 64 && sizeof(RcHead) == 256, "RcHead");
// The 4 KB device scalar block of lane 0 (SetLane::scal): one allocation, so that one read-back covers the scalars and the keys.
struct ScalBlock {
  unsigned char scalars[2048];                                                         // SweepScalars (sets.hip)
  double point[kMaxD]; unsigned char pad0[1024 - sizeof(point)];                       // the explore target / trust-region centre
  unsigned long long lip_keys[kMaxQ]; unsigned char pad1[928 - sizeof(lip_keys)];      // sbo_ctx::Lmax
  double comm_word; unsigned char pad2[96 - sizeof(comm_word)];                        // sbo_comm_barrier's all-reduce word
};
static_assert(offsetof(ScalBlock, point) == 2048 && offsetof(ScalBlock, lip_keys) == 3072 && offsetof(ScalBlock, comm_word) == 4000 &&
              sizeof(ScalBlock) == 4096, "ScalBlock");
// The 8 KB pinned landing block sbo_ctx::h_back: where the small device-to-host copies of a call land, and what the last kernel of a
// sweep or a plan's band kernel writes itself (`mirror`).  Its head is the image of ScalBlock's, up to the end of lip_keys.
struct PinnedBack {
  unsigned char scalars[2048], pad0[1024];                                             // SweepScalars (its first kScalHost bytes are read)
  unsigned long long lip_keys[kMaxQ]; unsigned char pad1[1024 - sizeof(lip_keys)];     // k_sweep_finals, k_arg_final_mirror, k_col_finals write
  int basis_info[8 * kMaxQ]; unsigned char pad2[512 - sizeof(basis_info)];             // K1b: 4 ints per axis basis (bilinear.hip)
  int build_bad[kMaxQ]; unsigned char pad3[256 - sizeof(build_bad)];                   // the model build's verdict per output (model.hip)
  int factor_bad[kMaxQ]; unsigned char pad4[256 - sizeof(factor_bad)];                 // the deferred factor chain's (factor_sync reads)
  RcHead rc;                                                                           // a recheck's counters (sets_recheck.inc.hpp)
  int tile_eff[4 * kMaxQ]; unsigned char pad5[1792 - sizeof(tile_eff)];                // K1b: the counts its kernels run to (k_cheb_trunc)
  unsigned long long audit[4]; unsigned char pad6[512 - sizeof(audit)];                // the standing audit's counters (guard.hip)
  unsigned char guard_band[512];                                                       // GuardBand, written by the plan's band kernel
};
static_assert(offsetof(PinnedBack, lip_keys) == offsetof(ScalBlock, lip_keys) && offsetof(PinnedBack, basis_info) == 4096 &&
              offsetof(PinnedBack, build_bad) == 4608 && offsetof(PinnedBack, factor_bad) == 4864 && offsetof(PinnedBack, rc) == 5120 &&
              offsetof(PinnedBack, tile_eff) == 5376 && offsetof(PinnedBack, audit) == 7168 && offsetof(PinnedBack, guard_band) == 7680 &&
              sizeof(PinnedBack) == 8192, "PinnedBack");

// Model constants handed to kernels by value (kernarg segment).  Everything is kept in double; the
// fp32 kernels round on use.  Rows a1/a4 of SURVEY.md section 8 (models/GP_Safe.py:236-245, 326-347).
struct ModelConst {
  int n, npad, d, dpad, q, factor;
  double X_mean[kMaxD], X_std[kMaxD], X_rstd[kMaxD];
  double Y_mean[kMaxQ], Y_std[kMaxQ];
  double sf2[kMaxQ];            // exp(2 h[d])                       GP_Safe.py:338
  double sn2[kMaxQ];            // exp(2 h[d+1]) + float32 eps       GP_Safe.py:229 (used by the model build / append only)
  double mp[kMaxQ];             // prior mean, -2 Y_mean/Y_std, [0]=0 GP_Safe.py:331-332
  double vinv[kMaxQ][kMaxD];    // ell^-1/2 = exp(-h[a])             GP_Safe.py:112
  double inv_ell[kMaxQ][kMaxD]; // 1/ell = exp(-2 h[a])
};

// Candidate description (explicit list or implicit tensor grid), by value.
struct CandSpec {
  int kind;        // 0 explicit points, 1 grid
  int d;
  int pts_dtype;   // SBO_F64 / SBO_F32 for explicit points
  int pad;
  const void* pts; // device pointer [n_local, d]
  long long n_local, first;
  double lo[kMaxD], hi[kMaxD], step[kMaxD];
  long long count[kMaxD];
};

// The four kinds of device resource a context holds, each freed by its holder's destructor and nowhere else.  Move-only (a copy
// would free twice); what merely points into another's memory is a plain pointer, not one of these.
struct DevBuf;
int ensure(DevBuf& b, size_t bytes);
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(DevBuf&& o) noexcept {      // (the one move: sbo_model_append swaps a grown factor in)
    if (this != &o) { reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};
// A device block that starts every sweep in a NEUTRAL state (zeros, or the neutral elements of its merges) without a fill per sweep:
// the last kernel of a sweep that reads the block puts it back, and the host only remembers whether that has happened.
//   * acquire(bytes, fill, key) is the one way to the block: it grows the buffer, runs `fill` (which enqueues, and may wait) when the
//     buffer grew, when the block is not known to be neutral, or when it was laid out for another `key`, and marks the block in use.
//     A new allocation is never taken for neutral.
//   * reset_enqueued() says that the kernel that resets the block has been enqueued behind its last reader -- or, where the caller
//     wants more, that the sweep it ran in has come through.  Which of the two a block uses is its owner's choice and stands at the
//     member; nobody else raises the flag.
//   * in_use() is for a sweep that may touch the block but runs none of its kernels' resets (no buffer is needed for it).
//   * A sweep that fails between acquire() and reset_enqueued() leaves the block in use: the next acquire() fills it again.  A failure
//     after reset_enqueued() leaves it neutral, which is right as long as what was enqueued runs (a failed call drains the streams).
struct ResetBuf {
  DevBuf buf;
  template <class Fill> int acquire(size_t bytes, Fill&& fill, long long key = 0) {
    const bool fresh = buf.bytes < bytes;
    if (int rc = ensure(buf, bytes)) return rc;
    const bool stale = fresh || !neutral_ || key != key_;
    neutral_ = false;
    key_ = key;
    return stale ? fill() : SBO_OK;
  }
  void reset_enqueued() { neutral_ = true; }
  void in_use() { neutral_ = false; }

 private:
  bool neutral_ = false;
  long long key_ = 0;
};
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  ~Event() { if (e) (void)hipEventDestroy(e); }
};
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  ~Stream() { if (s) (void)hipStreamDestroy(s); }
};
struct Pinned {
  void* p = nullptr;
  size_t bytes = 0;
  Pinned() = default;
  Pinned(const Pinned&) = delete;
  ~Pinned() { reset(); }
  void reset() { if (p) (void)hipHostFree(p); p = nullptr; bytes = 0; }
};

// Spatial index of an explicit candidate list (sets_index.inc.hpp): Morton order of the points, built at the first sweep that
// needs it and kept until the candidates change (option "list_index")
struct ListIndex {
  bool valid = false;
  bool built_now = false;        // built by the running sweep (its time goes into sbo_profile.list_index_build_ms)
  bool ran = false;              // the running sweep walked the index (its counters go into sbo_profile)
  long long n = 0;
  int d = 0;
  int perm_half = 0;             // which half of `vals` holds the sorted permutation
  DevBuf box;                    // bounding box (ord keys), kIdxBoxHead words
  DevBuf keys, vals, hist;       // radix sort: keys / values twice (ping-pong), per-tile digit counts
  DevBuf xs;                     // sorted coordinates, fp64 [n][d]
  DevBuf stats;                  // walk counters of the running sweep: leaf pairs, nodes skipped
  Event ev0, ev1;
};

// Column-word form of the masks of a 2-D grid (r05): word [s][i] holds the bits of column i (axis 0) for the 64 rows
// 64 s .. 64 s + 63 of axis 1 -- exactly what one 64 x 128 tile of the GEMM posterior (k_bpost) knows about a column, so the
// constraint's mean epilogue emits the S / U words itself (128 coalesced 8-byte stores per tile instead of 16384 byte
// stores), and every set-phase kernel of the column path (sets_colpath.inc.hpp) reads 1/8 of the bytes.  Usum[i]: bit s set
// iff Uw[s][i] != 0 (the carries of the column distance transform in two dependent loads).
struct ColBits {
  unsigned long long* Sw;
  unsigned long long* Uw;
  unsigned long long* Usum;
  unsigned long long* slots;   // [kColSlotFields][kColSlots]: the tiles' partial scalars, merged by atomics as the workgroups end
};
// One workgroup merging the 2 x 2048 partial rows of config H took 15 us at the head of the set phase.  Instead a tile's workgroup
// adds / maxes / mins its scalars into slot (tile mod 64) of each field (64 addresses per field: no queueing in L2), and whoever
// needs a scalar reduces 64 words with one load per lane.  The finals reset the block for the next sweep.
constexpr int kColSlots = 64;
enum ColSlotField { kSlotUmin = 0 /* min key of ucb_0 over S */, kSlotS, kSlotU, kSlotB /* counts */, kSlotVmin0, kSlotVmin1 /* min keys */,
                    kSlotRmax1 /* max key */, kSlotL0, kSlotL1 /* max of the gradient norms' bit patterns */,
                    kSlotRowMask /* word s: bit t set iff tile t of tile row s holds a safe candidate */,
                    kSlotSkip /* count: constraint tiles its enclosure proved unsafe, left unevaluated (r06) */,
                    kSlotSkipSafe /* count: constraint tiles its enclosure proved safe, left unevaluated (option k1_skip_safe) */,
                    kSlotResC, kSlotResO /* counts: constraint / objective tiles classified from their stored mean / var (option k1_resident) */,
                    kSlotCells /* count: 8 x 8 cells of those constraint tiles whose stored values were loaded (option k1_cells: k_bhead) */,
                    kColSlotFields };
__host__ __device__ inline bool col_slot_is_min(int f) { return f == kSlotUmin || f == kSlotVmin0 || f == kSlotVmin1; }
constexpr unsigned int kTlistUnsafe = 0x80000000u, kTlistSafe = 0x40000000u;          // flag bits of a tile-list entry (the tile: ent & 0xffffff)
constexpr unsigned char kSkipUnsafe = 1, kSkipSafe = 2;                                  // a tile's skip byte (bl_encl, behind the enclosures): 0 = evaluated
constexpr int kTlistShift = 5, kTlistShards = 1 << kTlistShift, kTlistHead = 32;     // PostExtra::tlist (the constraint's list; the objective's has one shard)
// what a k_bpost launch is told beyond its operands (r05: one launch per output on the column path)
struct PostExtra {
  int o0;        // first output of this launch (blockIdx.z counts from it)
  int q;         // outputs of the model (layout of the gradient gate's tables)
  int lean;      // 1: an objective tile without a safe candidate does not store its mean / var (nobody reads them)
  long long fstride; // fused classification of several constraints: stride of the S / U byte planes (constraint o writes plane o - 1; 0: one constraint, the masks themselves)
  int nograd;    // 1: the gradient phases (Lipschitz keys) run in a launch of their own (k_bpost<.., 3>, K1i's deferred gate): none here
  ColBits cb;    // Sw == nullptr: no bit words (byte masks or no classification at all)
  // lean >= 2, the constraint's launch (r06): the plan's enclosures of its mean / var, [tiles][128 cells of 8 x 8][m_lo, m_hi, v_lo, v_hi]
  // (k_bl_enclose), and one byte per tile that says whether the tile was left unevaluated; nullptr: every tile is evaluated
  const double* encl;
  uint8_t* skip;
  int skip_safe; // option k1_skip_safe: tiles the enclosures prove SAFE are left unevaluated as well (skip byte kSkipSafe)
  // lean >= 2, k1_sched (r07): nullptr, or the tile list of this launch, 2^tshift shards: a head of kTlistHead words per shard -- [0] =
  // entries at the front, [1] = entries at the back, the rest unused: a shard's counters have a cache line to themselves --, then room for
  // tcap entries per shard: the tile (by * tgx + bx) in bits 0..23, bit 31 = a constraint tile the list's kernel proved unsafe that still
  // runs the gradient phases, bit 30 = one it proved safe that does.  Workgroup i of a 1-D grid of tcap << tshift takes entry i >> tshift of shard i mod 2^tshift -- the front
  // entries upwards, then the back entries from the last one down -- and exits at once past both.  Tiles not in the list were written by
  // the list's kernels.
  const unsigned int* tlist;
  int tshift, tcap;
  int tgx, tgy;  // the tile grid (tiles per row, tile rows) behind the list
  // option k1_resident (BilinearPlan::lrows_ready / omap_dirty).  front_only: the launch takes the front entries of its list alone -- the
  // back ones belong to the light launch (k_bres).  omap: nullptr, or the plan's residency bytes of the objective's tiles: a workgroup of
  // the objective's launch that stores its tile raises the tile's byte.
  int front_only;
  uint8_t* omap;
};

// The operands of the GEMM posterior -- stage 1 (k_bstage1) and k_bpost -- as the plan that made them lays them out (K1b:
// bilinear_setup, K1i: interp_setup); launch_posterior_gemm launches on them.  Device pointers and per-output strides in elements.
// (The pointers are taken when the plan is built.  Only the two plan builders resize the bl_* buffers, and neither runs while the
// other's plan can still be launched: K1i's is built only while K1b's is invalid, K1b's only once K1i's is used or unusable.)
struct GemmOps {
  int sets = 1;          // stage 1: coefficient sets per output (grid z = sets q)
  int KB1 = 0;           // stage 1: k-blocks (the 16-blocks of axis 1)
  size_t sP1A = 0, sT4f = 0, sBt1 = 0;   // stage 1: per-set strides of its A operand (P1A), of T4f and of its output (BtA)
  double *BtA = nullptr, *P0f = nullptr, *VA = nullptr, *SBf = nullptr;
  size_t sBtA = 0, sP0f = 0, sVA = 0, sSBf = 0;
  int KB0 = 0, KS0 = 0, KBm = 0, KSm = 0, KBm2 = 0;   // k-blocks / k-steps of the variance phase; of the mean phases
  int ncs0 = 0, nrb = 0;   // 16-column strips of axis 0, 16-row blocks of the local lines
  int* eff = nullptr;    // device: the counts the kernels run to (k_cheb_trunc), followed by the truncation tails
  const double* gtmax = nullptr;              // device: largest gradient samples per k_bpost tile + slacks (k_bl_gradcoarse), or none
  const unsigned long long* gkey = nullptr;   // device: the grid's largest gradient samples
  bool band_ready = false;   // the guard band of this plan has been measured
  int imode = 0;         // k_bpost's K1i mode: four coefficient sets per output, the k-steps of every phase from eff
};

// K1b (bilinear.hip): device tables of the reduced-basis posterior on a 2-D grid, valid for one (model, candidates) pair
struct BilinearPlan {
  bool valid = false;    // built (or found unusable) for the current model and candidates
  bool usable = false;   // the bases qualified: the posterior runs as two GEMMs
  int r0u = 0;
  long long nlines_pad = 0;
  int r0[kMaxQ] = {0}, r1[kMaxQ] = {0};
  double setup_ms = 0.0;
  GemmOps ops;           // (eff: per-output counts; band_ready: guard.hip, guard_band_bilinear)
  // bl_encl holds the enclosures of the constraint's mean / var per 8 x 8 cell (k_bl_enclose, r06), recorded from a launch of this plan
  // that stored every tile, AND no posterior launch of another kind has written sbo_ctx::mean / var since.
  // vals_ready: on top of that, the constraint's regions of sbo_ctx::mean / var hold ON EVERY TILE the bits this plan's k_bpost computes
  // (a lean-2 sweep leaves the tiles it proves safe unevaluated, and k_col_decide reads their stored values: option k1_skip_safe).
  // WHO MAY WRITE THOSE REGIONS while the flags stand: K1b's column-path launches of this plan, nothing else.
  //   * Every posterior launch on the context passes through launch_posterior (posterior.hip), which drops both flags for every other
  //     family -- K1g, K1i, K1t, the generic kernels, an fp32 model's launches, whoever asked (a sweep, sbo_posterior_run, the guard) --;
  //     launch_posterior_gemm drops them for a K1b launch that is not on the column path (another epilogue: not relied on).
  //   * A new plan starts without them (bilinear_setup: a new model, new candidates, an option the plans are built with, among them
  //     `bilinear` itself), and so does a reallocation of mean / var (alloc_workspace).
  //   * The guard's recheck scatters exact values over the plan's at the candidates it lists (rc_refine): it drops vals_ready alone --
  //     nobody reads the stored values of a tile proved UNSAFE, so r06's skip stands --, and the next K1b column-path launch that
  //     evaluates and stores every tile (the recording one, or a lean-0 / lean-1 sweep) sets it again.
  // With encl_ready down the next K1b column-path launch evaluates and stores every tile and records the enclosures again, as after a
  // plan rebuild.  Whoever adds a writer of sbo_ctx::mean / var must call post_regions_written (or post_values_patched).
  bool encl_ready = false;
  bool vals_ready = false;
  // Option k1_resident: what a later sweep of the plan takes from memory instead of running the GEMM phases again (sbo_ctx::bl_res).
  // INVARIANT (the constraint's values): vals_ready, above -- k_bres<1> classifies a listed tile from its stored mean / var.
  // INVARIANT (lrows_ready): bl_res holds, per tile, the row of output 1 the plan's recording launch wrote into the Lipschitz partials
  // (the maximum of the tile's gradient phases and its coarse samples: operands, gate and k-order are the plan's, b and the band do not
  // enter).  Recorded by k_bl_enclose behind that launch; raised where encl_ready is raised and dropped wherever encl_ready is dropped.
  // INVARIANT (the residency bytes, bl_res behind the rows): a tile's byte stands only if the OBJECTIVE's mean / var of that tile hold the
  // bits a column-path launch of this plan stored, and nothing has written that region since.  Raised by the workgroups of k_bpost<1, 2>
  // that store their tile; omap_dirty says that the bytes must be cleared before the next column-path launch reads or raises one: a new
  // plan starts with it (bilinear_setup), post_regions_written and post_values_patched set it, a new buffer has it.
  bool lrows_ready = false;
  bool omap_dirty = true;
  // bl_BtA holds stage 1's images of THIS plan (k_bstage1 has been enqueued on its operands): launch_posterior_gemm runs stage 1 for
  // the plan's first launch only.  INVARIANT: stage 1 reads bl_P1A, bl_T4f and the counts `ops.eff` (in bl_cheb) and writes bl_BtA;
  // all four are written by the two plan builders and by nothing else -- bilinear_setup (k_cheb_tab<0>, k_cheb_t4f, k_cheb_trunc)
  // and interp_setup, which lays K1i's own tables into the same buffers -- and only those two resize them.  Both clear the flag, and
  // so does a K1i launch (its stage 1 overwrites bl_BtA).  Whoever adds a writer of one of the four must clear it as well.
  bool bt_ready = false;
};

// What one posterior launch is asked to do (posterior_enqueue).  A default request is a plain posterior run: every value and
// Lipschitz key, no classification, the approximating kernels wherever they qualify.
struct PostRequest {
  int fuse = 0;             // classification fused into K1b's mean epilogue (one-constraint sweeps): 0 no, 1 yes, 2 when the launch
                            // is large enough for it to pay (option fuse_classify = -1)
  double fuse_b = 0.0;      // ... at the sweep's confidence multiplier
  bool lmax_defer = false;  // K1b leaves its per-wave Lipschitz partials for the sweep's first small kernel to merge
  bool col = false;         // column path (sets_colpath.inc.hpp): the classification as column words, one launch per output
  int col_lean = 0;         // ... objective tiles without a safe candidate need not store mean / var (1), nor be evaluated (2)
  int sweep_lean = 0;       // a lean SafeOpt sweep: the objective's Lipschitz key L_0 (no sweep reads it) is not computed by K1t / K1i
  bool exact = false;       // no approximating posterior (K1b, K1i, K1t): the exact kernels only
};

// The column path's rows in sbo_ctx::cpart: field-major with `cap` rows to a field (the capacity the launcher laid cpart out with,
// sbo_ctx::cpart_cap), a row per tile -- the constraint's tiles first, then the objective's.  launch_posterior_gemm builds the view;
// the list kernels' launch lines and col_set_phase read it.
constexpr int kColRowRmax1 = 4 + kMaxQ + 1;    // the field of constraint 1's radius key (= kFuseRmax + 1 = kRowRmax + 1: asserted where those are defined)
struct ColPartRows {
  unsigned long long* base = nullptr;
  int cap = 0;
  int tiles = 0;                                   // constraint rows [0, tiles), objective rows [tiles, 2 tiles)
  int count() const { return 2 * tiles; }
  const unsigned long long* field(int f) const { return base + (size_t)f * cap; }
  const unsigned long long* tumin() const { return field(0); }                  // per constraint tile: key of the lower end of ucb_1 over its safe candidates
  const unsigned long long* tumax() const { return field(kColRowRmax1); }       // ... of the upper end (the tile's radius key)
  const unsigned long long* olmin() const { return field(1) + tiles; }          // per objective tile: key of the smallest lower bound of lcb_0 over its safe candidates
};

// What the launch reports back (filled by the launcher: all zero unless a GEMM posterior ran)
struct PostOutcome {
  bool col_active = false;     // the launch delivered the classification as column words (col_set_phase runs)
  bool col_forked = false;     // ... and the constraint's launch carried ColPath::ev[0]
  int col_lean = 0;            // ... at this lean level (non-zero: the objective's mean / var are incomplete)
  bool col_sched = false;      // ... and k_bl_sched_list2 ran behind the constraint's launch: the counters of the constraint's tile list are zero again
  int fuse_rows = 0;           // > 0: the kernel wrote S / U and that many partial rows at the head of cpart
  ColPartRows col_rows;        // col_active: those rows
  bool lmax_pending = false;   // the Lipschitz partials (lmax_per_out rows per output in bl_lpart) wait for the sweep to merge them
  int lmax_per_out = 0;
  bool stop_attached = false;  // the last kernel carries ev[1] as its stop event (no separate record, which costs a ~6 us bubble)
};

// K1i: the first sweep of a model by interpolation from Chebyshev nodes (bilinear.hip)
struct InterpPlan {
  bool valid = false;    // enqueued (or found not applicable) for model `serial` and the current grid
  bool usable = false;
  bool used = false;     // a sweep has run on it: the next one builds K1b's own plan
  unsigned long long serial = 0;
  GemmOps ops;           // (eff: per coefficient set, 4 per output)
  bool grad_deferred = false;                 // the gate's kernels run on stream3 beside the plan's tail: the posterior launches carry no
                                              // gradient phases, a launch of those alone follows the gate there (launch_posterior_gemm)
};

// K1t (tensor.hip): fp64 grids of three / four axes by Chebyshev interpolation from exact node values.  The plan keys itself on
// (model, first, nlocal, count, lo, hi): a new model or new candidates need not drop it, an option it is built with must
struct TensorPlan {
  DevBuf pts, vals, work, W0t, W1t, probe, scr;
  DevBuf gather;     // ranks > 1: this rank's slab of the node tensors | every rank's (all-gather)
  DevBuf W[SBO_MAX_D];
  size_t work_half = 0;
  double flops = 0.0;           // multiply-add flops of the last interpolation pass
  bool valid = false, usable = false;     // plan decided for (model, grid below) / it passed its accuracy probe
  unsigned long long model = 0;
  long long first = 0, nlocal = 0, count[4] = {0, 0, 0, 0};
  double lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
  int level[4] = {0, 0, 0, 0};
  int dn[4] = {0, 0, 0, 0};     // node counts of the plan in use
  DevBuf tail;             // [2 q][d] keys of the node tensors' coefficient tails per axis (k_t_fiber_tail)
  double band[7 * SBO_MAX_Q] = {0};   // the plan's guard band (dm | dv | rl | analytic dm | dv | probe dm | dv per output)
  int bump = 0;                 // ladder steps added to the first guess on this grid (a previous model's plan needed its second attempt)
  bool lean_probe = false;      // the plan's probe left out output 0's gradient (decided by a lean sweep): a full sweep probes it again
  void invalidate() { valid = false; }
};

// Guard band of the approximating posteriors K1b / K1t (device_common.hpp: GuardBand; guard.hip), as far as it belongs to the
// resident posterior
struct ResidentBand {
  bool active = false;          // the posterior in mean / var came from an approximating kernel; `buf` holds (or will hold, in stream order) its band
                                // (a fact about the resident arrays, kept between calls; what a running set phase makes of it: SetView in sets.hip)
  DevBuf buf;                   // GuardBand of the resident posterior
  long long first = 0;          // decisions the first pass of the running sweep left open
  bool mirrored = false;        // the plan's band kernel also wrote the block to pinned host memory (PinnedBack::guard_band): valid once a sweep has synchronised
  bool host_valid = false;      // `host` mirrors `buf` (read back on demand by sbo_profile_get; dropped when a plan writes the block)
  double host[7 * SBO_MAX_Q] = {0};   // dm | dv | rl | analytic dm | dv | largest probe deviation dm | dv
  DevBuf pts, vals;             // re-evaluation: coordinates and exact values of the listed candidates
  DevBuf part;                  // k_ref_list: per-column-chunk partial sums
  DevBuf probe;                 // K1b: probe indices / coordinates / reference values of the running plan
  unsigned long long plan_model = 0;   // K1b: the model whose band `buf` holds (0: none)
  long long plan_first = -1, plan_n = -1;
};

// Standing audit of the band (r05): behind every K1b / K1i posterior launch of a sweep a rotating sample of the candidates is
// re-evaluated with the reference formula on stream2 -- off the critical path -- and compared with what the posterior kernel
// stored: a deviation beyond the band is a VIOLATION of the claim the sweeps' exactness rests on (counted, reported in sbo_profile)
struct Audit {
  long long tick = 0;
  DevBuf pts, val, part, cnt;
  hipEvent_t ev[2]{};           // the sample has been taken (mean / var may be overwritten) / the audit has finished
  bool pending = false;
  unsigned long long offset = 0;
  long long samples = 0, violations = 0;
  long long skipped = 0;        // of samples: constraint samples on tiles a lean sweep left unevaluated (checked against the enclosure)
  double worst = 0.0;           // largest deviation seen, in units of the band
};

// Column path (r05, sets_colpath.inc.hpp): a one-rank SafeOpt sweep of a one-constraint model on a 2-D grid of whole
// 64 x 128 tiles asks (PostRequest::col) for the classification as column words; the GEMM posterior then runs one launch per
// output -- constraint first: S / U words, |S| per tile; objective second: u* and min var_0 over S from its own epilogue --
// and says so (PostOutcome::col_active).  The words stay resident for sbo_masks_get (masks_bits: expanded to bytes on demand).
struct ColPath {
  DevBuf S, U, M, G;                 // column words [H / 64][W]
  // The blocks a sweep's last reader resets (ResetBuf).  Each flag but the tile lists' is raised when the resetting kernel is ENQUEUED;
  // the lists' (sbo_ctx::bl_sched) only at the end of col_set_phase, once the sweep whose k_bl_sched_list2 reset them has come through.
  ResetBuf Usum;                     // [W]: zero; k_col_decide clears it (raised behind k_col_a, the chain's first launch)
  ResetBuf slots;                    // ColBits::slots: the neutral elements of its fields (a host array, copied and waited for); k_col_finals
  DevBuf img, bmin;                  // column distance image u16 [H][W], block minima u16 [H][W / 32]
  DevBuf cimg;                       // the same on the 8 x 8 cells
  ResetBuf cbmin;                    // ... 0xffff in the padding of its rows, keyed on the grid: k_col_a, its one writer, leaves the padding alone
  ResetBuf fin;                      // the objective's scalars, the finals' tickets and intermediate rows (4 KB): zero; k_col_finals' last workgroup of a slot resets its ticket
  hipEvent_t ev[3]{};      // fork (the constraint's posterior launch has finished) / join (the expander chain on stream3 has) /
                           // the chain's first kernel, which clears the M words, has finished (carried by k_col_a: the minimiser's M part waits for it)
  bool masks_bits = false;     // the masks of the last sweep live in the column words (byte buffers stale)
  bool G_bytes = false;        // ... except G, which the exhaustive recheck finished in byte form
};

// Several ranks: the communicator or the rehearsal transport, the buffers of the collectives, the sharding of the grid
struct MultiRank {
  void* comm = nullptr;  // ncclComm_t
  int world = 1, rank = 0;
  // rehearsal transport (tests on a 1-GPU box): collectives staged through host callbacks instead of RCCL
  sbo_relay_allreduce_fn relay_allreduce = nullptr;
  sbo_relay_allgather_fn relay_allgather = nullptr;
  void* relay_user = nullptr;
  long long comm_bytes = 0;   // collectives of the running sweep: bytes handed over (send side), calls, and -- option comm_events --
  int comm_calls = 0;         // an event pair per call (comm_ev, created on first use) whose elapsed times sbo_profile.comm_ms sums
  int comm_nev = 0;
  double comm_host_ms = 0.0;  // (relay transport: wall clock of the staged collectives)
  Event comm_ev[16];
  DevBuf Wfull;   // GoOSE: source weights of the whole grid (all-gathered), T [grid_total]
  DevBuf Uwin;    // U mask of the expander transform's window (own planes + halo), uint8
  long long uwin_first = 0, uwin_n = 0;   // flat range the window covers
  DevBuf ubits;                      // own U bits (gather_words words) followed by every rank's (all-gathered)
  long long gather_words = 0;        // words per rank in ubits
  DevBuf gather;  // all-gather receive buffer [world][max_local]
  DevBuf xch;     // small exchange buffers (C1 keys, C3 rows)
  DevBuf shard_first;  // device copy of first_of[]
  long long grid_total = 0; // candidates in the whole grid (all ranks)
  bool sharded = false;     // candidates were set with the canonical plane sharding
  std::vector<long long> first_of;   // [world + 1] flat offsets of the rank shards
  unsigned long long* h_c1 = nullptr;     // pinned host copy of the C1 keys (global u*, L, radius) of the running sweep
  bool c1_pending = false;                // the read-back of h_c1 has been enqueued (event ev[5]) but not yet waited for
  // Speculative halo (ranks > 1, option halo_spec): the host sizes the transform window of constraint c from the keys of the
  // PREVIOUS sweep (with a margin) instead of waiting for this sweep's; the device checks the guess against the keys it
  // gathered (SweepScalars::halo_short) and a short guess reruns the set phase the waiting way.  -1: no guess yet.
  long long halo_guess[SBO_MAX_Q] = {-1, -1, -1, -1, -1, -1, -1, -1};
  int halo_reruns = 0;            // set phases of the current sweep call discarded for a short window (global decision)
};

// fp32 models: an fp64 twin of the model (same arrays, double images) that re-evaluates the candidates the fp32 bounds
// cannot decide (option fp64_recheck); it borrows its owner's streams, events and h_back and holds explicit lists only
struct Recheck {
  sbo_ctx* shadow = nullptr;
  // the owner's model_serial the twin holds the model of (twin_current below): written when sbo_model_set builds the twin, advanced when
  // the twin has followed an accepted append, block append or removal; kNoSerial while it is ahead of its owner, inside such a call
  static constexpr unsigned long long kNoSerial = ~0ull;
  unsigned long long serial = kNoSerial;
  DevBuf mean, var;         // double [q][n_local]: the fp32 posterior widened, flagged entries replaced by fp64 values (what the recheck's set phases read)
  DevBuf list;              // RcHead, then the flagged candidate indices (long long)
  DevBuf refined;           // uint8 [n_local]: this candidate's entries of mean / var are fp64 values
  // the band of the resident fp32 posterior (sets_recheck.inc.hpp: rc_bands): max(1e-4 normalised, 16 x the largest |fp32 - fp64 twin| over
  // the probe candidates), measured when an fp32 sweep first meets this (model, candidate set); dropped by plans_invalidate
  DevBuf probe;             // probe indices (long long [kRcProbes]) behind 2 kMaxQ deviation keys
  bool band_valid = false;
  double band_dm[kMaxQ] = {}, band_dv[kMaxQ] = {};
  long long probe_round = 0;  // rotates the probe set of the standing audit
  void invalidate() { band_valid = false; }
  ~Recheck();               // deletes the twin (defined below sbo_ctx)
};

// robust sweep (robust.hip): per-control arrays of the last one, the mask of robust-safe controls, the split partials
struct Robust {
  DevBuf vals, mask, part;
  long long nc = 0;
  int q = 0;
  bool valid = false;   // sbo_robust_get may read `vals` (cleared by a model or candidate change)
  void invalidate() { valid = false; }
};

// sbo_model_loo (model.hip): what one call leaves per output, and the buffers every call reuses
struct LooSummary {
  double logdet, lpd, z_max;
  int z_argmax, outside;
};
struct Loo {
  DevBuf part;     // [q][ceil(ld / kLooRows)][ld] (ld: ResidentFactor::ld()) partial column sums of squares of the factor, one row per chunk of rows
  DevBuf out;      // LooSummary[kMaxQ] | resid [n][q] | var [n][q]
  Pinned h_out;    // ... and where the one copy of a call lands
};

// The resident fp64 factor of the model (model.hip): the lower factor M [q][ld][ld], row-major, with M^T M = invK, and alpha [q][a_ld]
// -- what the K1b table build, the O(n^2) readers (refine, lipschitz, batch, guard, loo) and the three model updates work on.
//   * Tight after a build: ld == n, a_ld == npad.  The first reserve() that has to grow it leaves a_ld == ld == the capacity (a
//     multiple of 128, at most SBO_MAX_N), and so it stays until the next build.
//   * Everything outside the n x n lower triangles and alpha's first n entries is zero: right of the diagonal in appended rows, and
//     all of the padding (reserve() copies into zeroed buffers, the commit kernels write whole rows, a removal writes a zeroed spare).
//   * The spare pair has the leading dimensions of the resident one.  A removal writes the factor without its row there and
//     adopt_spare() swaps the pairs: the outgoing pair is the next removal's spare.
// Readers take F() / alpha(); the mutable forms are for the kernels that build or commit an update.
struct ResidentFactor {
  const double *F() const { return (const double*)F_.p; }  const double *alpha() const { return (const double*)alpha_.p; }
  double *F_mut() { return (double*)F_.p; }                double *alpha_mut() { return (double*)alpha_.p; }
  double *spare_F() { return (double*)Fspare_.p; }         double *spare_alpha() { return (double*)aspare_.p; }
  int ld() const { return ld_; }                           int a_ld() const { return a_ld_; }
  bool present() const { return F_.p != nullptr && alpha_.p != nullptr; }
  int build(int n, int npad, int q);            // tight buffers for a model build (contents: the builder's)
  // Room for `rows` more rows.  A tight factor gets room for 256 more rows -- or for all of `rows`, if that is more --, a grown one that
  // does not fit grows again.  The copy keeps every value and is waited for; a call refused afterwards leaves the larger capacity behind.
  int reserve(sbo_ctx* c, int rows);
  int spare_ensure_zeroed(sbo_ctx* c);          // the spare pair, zeroed on the main stream (enqueued)
  void adopt_spare() { std::swap(F_.p, Fspare_.p); std::swap(F_.bytes, Fspare_.bytes); std::swap(alpha_.p, aspare_.p); std::swap(alpha_.bytes, aspare_.bytes); }

 private:
  DevBuf F_, alpha_, Fspare_, aspare_;
  int ld_ = 0, a_ld_ = 0;
};

}  // namespace sbo

struct sbo_ctx {
  // What sbo_init created, and it alone fills: the fp64 twin (Recheck::shadow) borrows the raw handles below and its `own` stays empty.
  // Declared first, so destroyed last: its pinned blocks, events, streams, after every buffer further down.  (The owners a plan or the twin
  // holds itself -- h_stage, h_bi_params, ev_bi_params, lx.ev0 / ev1, dist.comm_ev[] -- go among the buffers; every stream outlives them.)
  struct Owned {
    sbo::Stream stream, stream2, stream3, stream_audit, stream4;
    sbo::Event ev_factor, ev_w, ev[8], ev_join[SBO_MAX_Q], ev_col[3], ev_grad[4], ev_audit[2];
    sbo::Pinned h_c1, h_back;
  } own;
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;   // side stream: the K1b axis bases of a new model run next to its factorisation
  hipStream_t stream_audit = nullptr;   // lowest priority: the standing audit of the guard band (guard.hip) fills what the sweeps leave idle
  hipStream_t stream4 = nullptr;   // the deferred factorisation of a caller's invK (chol_async): off the critical path of a model change
  hipStream_t stream3 = nullptr;   // spare high-priority stream (drained with the others)
  int n_cu = 256;
  int decide_wg_per_cu = 1;        // workgroups of k_col_decide a CU holds at once (the occupancy query of sbo_init): sizes its persistent grid
  // What sbo_set_option steers (api.hip: one table row per key -- how the value is taken, its bounds, what it makes stale)
  struct Options {
    int chol_async = 1;
    int exact_lazy = 1;      // one-constraint SafeOpt sweeps on one rank: k_expander_exact only when the result block reports in-band candidates
    double cheb_tol = 4e-15; // ... relative size below which trailing coefficients are not run (option cheb_tol_e17, in units of 1e-17)
    int tensor_cheb = 1;             // 0 = always K1g
    int tensor_guess_pct = 100;      // (test hook): scales the first guess of the node counts; a short guess exercises the probe's second attempt
    int guard_band = 1;              // 1 count + re-evaluate exactly when the count is non-zero; 0 off; 2 re-evaluate on every sweep (test)
    int guard_audit = 1024;          // samples per audited sweep, 0 = off
    int guard_audit_every = 16;      // one sweep in this many is audited (the context's first one is)
    double audit_scale = 1.0;        // guard_audit_scale_ppm (tests): the audit compares against band x this -- a way to see it fire
    int set_lanes = 1;       // 0: all constraints on the main stream, one after the other
    int refine_lds = 1;   // (A/B checker): 1 sbo_refine stages M in LDS when it fits, 0 it always streams M's rows
    int lipschitz_lds = 1;  // (A/B checker): 1 sbo_lipschitz stages X_norm and the output's alpha in LDS when they fit, 0 it always streams them
    int list_index = -1;  // -1 the index for explicit lists above the exhaustive cap only, 0 never, 1 always
    int k1_sched = 1;             // 1 = K1b's two lean-2 column-path launches take their tiles from per-sweep lists; 0: one workgroup per tile
    int k1_resident = 1;          // 1 = the second and later lean-2 column-path sweeps of a plan classify from the stored mean / var (k_bres); 0: every sweep runs the GEMM phases
    int k1_skip_safe = 1;         // 1 = a lean-2 column-path sweep leaves the constraint tiles its enclosures prove SAFE unevaluated too; 0: the unsafe ones only
    int k1_cells = 1;             // 1 = on a resident plan (k_bres<1> would run) one launch decides the constraint's tiles and classifies the listed ones per 8 x 8 cell (k_bhead); 0: k_bl_sched_tiles1 + k_bres<1>
    int comm_events = 0;     // an event pair per collective (MultiRank::comm_ev) whose elapsed times sbo_profile.comm_ms sums
    int col_path = 1;        // 0 = never
    int col_overlap = 1;     // 1 = the expander chain runs on stream3 beside the objective's posterior launch; 0: one stream
    int col_queue = 128;     // open candidates a wave of k_col_decide queues in LDS before it flushes them to the scan list: 64 .. 128 (64: a flush before every append, the test of that path)
    int grad_defer = 1;          // 0 = K1i's gate stays in front of the posterior launch (r04)
    int halo_spec = 1;       // speculative halo (MultiRank::halo_guess)
    int scan_waves = 1;      // 1: candidates the coarse bounds leave open are scanned one wave each (0: by their own thread)
    int scan_blocks = 1;     // 0: step-by-step last-axis scans (A/B against the blocked form)
    int result_mirror = 1;   // SafeOpt sweeps on one rank: the last kernel writes the results into the pinned host block itself (0: a copy behind it)
    int set_fuse = 1;        // 2-D grids: independent set-phase kernels share launches (k_edt_axis0_pair, k_set_mid); 0: one launch each
    int fuse_classify = -1;  // one-constraint sweeps on the K1b path take their S / U bytes from the posterior kernel's mean epilogue: 1 always, 0 never, -1 (default) when the launch has at least four workgroups per CU (r03, sqrt-free sign tests: config H -40 us, config B +-0)
    int goose_pairs = 0;     // 1: GoOSE coverage by pruned pair evaluation on grids too (A/B against the transform)
    int phase_events = 0;    // 1: events between the set phases too (classify / expander / arg-reduce times in sbo_profile)
    int bilinear = 1;        // 1: fp64 2-D grids run the posterior as two GEMMs in a reduced basis when the bases qualify (K1b)
    int posterior_path = 0;  // 0 auto (separable tables on aligned grids), 1 force the generic exp() kernel
    int fp64_recheck = 1;    // fp32 models get an fp64 twin (Recheck::shadow); takes effect at the next sbo_model_set
    int comm_selftest = 0; // 1: a one-rank world still sends C1 / C2 / C3 through its communicator (test of the RCCL calls on one GPU)
  } opt;
  // model
  bool has_model = false;
  int dtype = SBO_F64;
  sbo::ModelConst mc{};
  sbo::DevBuf Fpk;     // [q][ntri*4*64] packed MFMA A-fragments of the contraction matrix
  sbo::DevBuf As;      // [q][npad][dpad]  X_norm * ell^-1/2
  sbo::DevBuf sqA;     // [q][npad]        sum_a As^2
  sbo::DevBuf alpha;   // [q][npad]        invK (Y_norm - mp)
  sbo::DevBuf Xn;      // [npad][dpad]     X_norm (for the mean gradient)
  sbo::DevBuf E0f;     // grid path: axis-0 kernel table in B-fragment order [q][tiles0][npad/4][64]
  sbo::DevBuf Er;      // grid path: tables of the remaining axes [q][sum_a count_a][npad]
  sbo::DevBuf AXg;     // grid path: alpha_j (1, Xn_j) rows in fragment-slot order [q][npad][1 + dpad]
  size_t fpk_stride = 0;  // elements per output in Fpk
  std::vector<double> h_Xnorm;   // host copies used by the exact-recheck / result decoding
  std::vector<double> h_Ynorm;   // [n][q], kept in step with h_Xnorm: sbo_expander_gain whitens the residuals itself (expander.hip)
  sbo::ResidentFactor factor;    // the fp64 lower factor M and alpha, with the spare pair of a removal
  sbo::DevBuf mwork;             // model build workspace (uploads, fp64 copies of the derived arrays, the factorisation's scratch)
  sbo::DevBuf appendbuf;         // model_append_stage's / model_append_block_stage's uploads and scratch (apart from mwork: a refused append leaves the uploaded invK in place)
  sbo::DevBuf removebuf;         // model_update_commit's per-row coefficients of a removal [q][3 factor.ld() + 1]
  sbo::Loo loo;                  // sbo_model_loo's scratch and landing area (the call reads the model and writes nothing else)
  // Caller's invK on a K1b-capable grid (option chol_async): the GEMM posterior's tables contract with invK itself -- packed
  // here as full matrix-core images, exactly the matrix of models/GP_Safe.py:341-343 -- so the reverse Cholesky factor M (needed
  // by the O(n^2) kernels K1g / K1 / K1c and by sbo_model_append only) is built on stream4 while the caller goes on; whoever
  // needs it calls factor_sync first, which also delivers the positive-definiteness verdict
  sbo::DevBuf invk_img;            // [q][npad / 16][npad / 16][256] A images of the full invK (fp64)
  bool invk_img_valid = false;
  bool invk_w_valid = false;       // the uploaded invK of the current model is still in the build workspace (images can be packed later)
  const double* invk_plain = nullptr;     // the caller's invK as uploaded, [q][n][n] (valid while invk_w_valid)
  bool factor_todo = false;        // the chain has not been enqueued yet (sbo_model_set does that last: model_factor_enqueue)
  bool factor_pending = false;     // the factor chain of the current model is (possibly) still running; ev_factor marks its end
  hipEvent_t ev_factor = nullptr, ev_w = nullptr;
  unsigned long long model_serial = 0;   // bumped by every sbo_model_set and by every accepted update (model_update_run: sbo_model_append, sbo_model_append_batch, sbo_model_remove)
  // K1b (bilinear.hip): the plan, its tables, and what its builders and launches keep between calls
  sbo::BilinearPlan bl;
  sbo::DevBuf bl_P0f, bl_P1A, bl_T4f, bl_BtA, bl_SBf, bl_VA, bl_small, bl_work, bl_cheb;
  sbo::DevBuf bl_basis;            // K1b: the 2 q axis bases (U, Chebyshev series, ranks) and the workspace of their kernel
  bool bl_basis_ok = false;        // bases enqueued for (bl_basis_serial, bl_basis_ab); their (ok, r, rc) records land in PinnedBack::basis_info
  unsigned long long bl_basis_serial = 0;
  double bl_basis_ab[4] = {0, 0, 0, 0};
  sbo::DevBuf bl_grad;  // K1b: which tiles run the gradient phases (per plan)
  sbo::DevBuf bl_lpart; // K1b: per-wave Lipschitz partials of k_bpost
  sbo::DevBuf bl_encl;  // K1b column path: per-cell enclosures of the constraint's posterior (per plan) + a skip byte per tile (per sweep)
  sbo::DevBuf bl_res;   // K1b column path, option k1_resident (per plan): [tiles] rows of output 1's Lipschitz partials | [tiles] residency bytes of the objective
  sbo::ResetBuf bl_sched;       // K1b column path, lean 2 (r07): the tile lists of the constraint's and the objective's launch (PostExtra::tlist); neutral: the
                                // counters of the constraint's list, at the head, are zero (k_bl_sched_list2; raised by col_set_phase at its end)
  sbo::Pinned h_stage;          // pinned staging of the K1b table build's single upload (the twin has one of its own)
  // what the last posterior launch leaves for the standing audit (guard.hip), cleared by every enqueue of a posterior (api.hip):
  struct K1AuditRecord {
    bool skip_armed = false;    // it could leave constraint tiles unevaluated: bl_encl's skip bytes are its record
    bool encl_check = false;    // a K1b column-path launch on a plan whose enclosures were recorded: what it stored lies inside them
    size_t encl_tiles = 0;      // tiles of the grid bl_encl was laid out for (the skip bytes sit behind 4 x 128 doubles per tile)
  } k1_audit;                   // (filled by col_enclosures, read by guard_audit_enqueue)
  // K1i plan (first sweep of a model)
  sbo::InterpPlan bi;
  sbo::DevBuf bi_params; // ... its per-model parameter block (device; the plan's kernels read it by pointer) and its pinned staging
  sbo::Pinned h_bi_params;
  sbo::Event ev_bi_params;   // the plan's copy of the block (and everything before it on the main stream) has run
  hipEvent_t ev_grad[4]{};     // K1i's deferred tail: fork (plan: the series are in place) / stage 1 has run / the keys are merged / the band is written
  bool grad_pending = false;   // a deferred gradient launch is in flight on stream3: whoever reads the Lipschitz partials elsewhere waits for ev_grad[2]
  sbo::TensorPlan tn;   // K1t plan (fp64 grids of three / four axes)
  sbo::ResidentBand gb;
  sbo::Audit audit;
  sbo::DevBuf list_scr;            // key scratch of launch_posterior_on_list
  // candidates
  bool has_cand = false;
  sbo::CandSpec cs{};
  sbo::DevBuf pts;
  // posterior workspace, SoA [q][n_local] of the model dtype
  sbo::DevBuf mean, var;
  bool posterior_valid = false;
  bool post_l0_missing = false;  // the resident posterior came from a lean sweep's launch: L_0 (Lmax[0]) was not computed
  int last_k1 = 0;               // kernel family of the last posterior launch (sbo_profile.posterior_kernel)
  double last_k1_tile_flops[2] = {0.0, 0.0};   // K1b: of that, the share of one 64 x 128 tile of output 0 / 1 (its variance and mean phases)
  double last_k1_flops = 0.0;    // matrix-core flops it issued
  unsigned long long* Lmax = nullptr;   // [kMaxQ] keys: max ||grad MEAN_i||_inf over the candidates -- a view: ScalBlock::lip_keys of lane[0].scal
  // set workspace
  sbo::DevBuf maskS, maskU, maskM, maskG, maskO;   // uint8 [n_local] (G/O: [(q-1)][n_local])
  sbo::DevBuf fitbuf, fitwork;   // hyper-parameter objective: inputs/outputs and the P x n x n factor workspace
  sbo::DevBuf refbuf;            // sbo_refine: seeds, candidates, their exact values and the results (refine.hip)
  sbo::DevBuf lipbuf;            // sbo_mean_grad / sbo_lipschitz: points, gradients, picks and the result block (lipschitz.hip)
  sbo::DevBuf batchbuf;          // sbo_batch_select: the scratch factor that grows with the picks, the pool, its variances and the state block (batch.hip)
  sbo::DevBuf expbuf;            // sbo_expander_gain: the points, their whitened vectors and posteriors, the partials and the results (expander.hip)
  sbo::DevBuf pathbuf;           // sbo_sample_paths: the draws, the B operand (scaled weights, then the update coefficients), the points, the values, the partials and the result block (paths.hip)
  sbo::DevBuf jointbuf;          // sbo_posterior_joint: the points, their whitened vectors, the covariance, the matrix that is factored in place, the draws, the partials and the result block (joint.hip)
  // What one per-constraint chain of the set phase enqueues on and scribbles in.  Lane 0 is the main stream's: everything before
  // the fork and after the join, every sweep of a model with one constraint and every sweep on several ranks uses it alone.  With
  // two or more constraints on one rank the chains are independent, so every other constraint goes to lane 1: stream2, its own
  // scratch, and a snapshot of the scalar block that k_classify_final writes (the chains only write its recheck / scan counters;
  // the finals merge them).  The chain's functions take the lane as a parameter (sets.hip); no field here changes to select one --
  // nor to say which posterior arrays, band or refinement lists a set phase works on: a recheck hands those down the same way (SetView).
  struct SetLane {
    hipStream_t stream = nullptr;  // not owned: sbo_ctx::stream (lane 0) / stream2 (lane 1), set where those are created (api.hip)
    sbo::DevBuf dist2, dist2b;     // double [n_local] distance-transform scratch (x2 for ping-pong)
    sbo::DevBuf coarse;            // coarse U mask + its distance transform (expander pre-decision)
    sbo::DevBuf blockmin;          // per-block minima along the last axis (blocked last-axis scans)
    sbo::DevBuf blockmax;          // per-block largest source weight along axis 0 (blocked axis-0 pass of the power transform)
    sbo::DevBuf scanlist;          // candidates left open by the coarse expander decision (wave-per-candidate scan)
    sbo::DevBuf amb;               // ambiguous-index list for the exact recheck
    sbo::DevBuf gw;                // GoOSE: source weights (ucb_c on sources, -inf elsewhere), T [max shard]
    sbo::DevBuf runmeta;           // GoOSE: per-run bounding boxes / radii of the coverage search
    sbo::DevBuf lxtree;            // list index: this sweep's boxes of U members / sorted U mask, or GoOSE's sorted weights and masks
    // small device scalar block (keys, counters, arg-reduce results), 4 KB.  Lane 0's is THE block of the sweep, laid out as a
    // ScalBlock (scal_block below); lane 1's holds a snapshot of its SweepScalars alone
    sbo::DevBuf scal;
    bool amb_clean = false;        // the recheck / scan counters of `scal` are still zero (no k_reset_amb needed)
  } lane[2];
  sbo::DevBuf partial; // arg-reduce per-block partials
  sbo::ListIndex lx;    // spatial index of an explicit list (sets_index.inc.hpp); a sweep's hierarchy on it: SetLane::lxtree
  sbo::DevBuf cpart;   // per-workgroup partials of k_classify, field-major [kClassifyRow][cpart_cap]
  int cpart_cap = 0;   // row capacity the last writer of cpart laid its rows out with
  int host_syncs = 0;  // host waits on the device inside the running sweep call (sbo_profile.host_syncs)
  sbo::DevBuf fuseS, fuseU;   // [(q - 1)][N] byte planes of a fused classification of several constraints (r05)
  sbo::ColPath col;
  sbo::MultiRank dist;
  sbo::PinnedBack* h_back = nullptr;      // pinned host landing block (the twin borrows its owner's)
  int last_sweep = 0;  // 1 safeopt, 2 goose (what the masks hold)
  bool masks_valid = false;
  // profile
  sbo_profile prof{};
  hipEvent_t ev[8]{};
  hipEvent_t ev_join[SBO_MAX_Q]{};   // phase marks of the fp32 recheck; fork / join marks of the plan builders and of the lanes
  bool is_shadow = false;   // this context is the fp64 twin of an fp32 model's (Recheck::shadow of its owner)
  sbo::Recheck recheck;
  sbo::Robust rob;
};

inline sbo::Recheck::~Recheck() { delete shadow; }

namespace sbo {
// the sweeps take their multi-rank path (pack, collective, unpack, host merge): more than one rank, or the self-test
inline bool multi_rank(const sbo_ctx* c) { return c->dist.world > 1 || c->opt.comm_selftest; }
// the fp64 twin is the resident model's: an fp32 model, a twin with a model, built for (or brought along to) this model_serial.  A twin
// left behind by an earlier model -- an fp64 model set since, or an fp32 one under fp64_recheck = 0 -- takes part in nothing: no sweep
// rechecks against it, no append or removal reaches it
inline bool twin_current(const sbo_ctx* c) {
  return c->dtype == SBO_F32 && c->recheck.shadow && c->recheck.shadow->has_model && c->recheck.serial == c->model_serial;
}
inline ScalBlock* scal_block(const sbo_ctx* c) { return (ScalBlock*)c->lane[0].scal.p; }
// the guard band of the resident posterior of an fp64 model (device_common.hpp: GuardBand), when an approximating kernel (K1b / K1i / K1t)
// wrote it and option guard_band is on; nullptr: the values are the exact kernels'
struct GuardBand;
inline const GuardBand* resident_band(const sbo_ctx* c) {
  return (c->gb.active && c->opt.guard_band && c->gb.buf.p) ? (const GuardBand*)c->gb.buf.p : nullptr;
}
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);
int ensure(DevBuf& b, size_t bytes);
hipError_t stream_wait(const sbo_ctx* c, hipStream_t st);   // hipStreamSynchronize, polling first (option spin_wait)
void release(DevBuf& b);
void drain_streams(sbo_ctx* c);
int col_decide_resident(int* wg_per_cu);   // sets.hip: the runtime's occupancy of k_col_decide, workgroups per CU
int factor_sync(sbo_ctx* c);      // wait for a deferred factorisation (sbo_ctx::factor_pending); SBO_E_INVALID when invK was not positive definite   // after a failed call: wait for whatever it left on the main and side streams

// What the calls that only read the resident model do once their arguments are checked (sbo_refine*, sbo_mean_grad, sbo_lipschitz,
// sbo_batch_select, sbo_model_loo): no model -> SBO_E_NO_MODEL, `need_f64` and an fp32 model -> SBO_E_UNSUPPORTED ("<who> needs an
// fp64 model"), then the device is selected and a deferred factor chain waited for (which also delivers the verdict on a caller's invK).
// model_reader_check is the first half alone, for a call that needs d and q to check its arguments before it waits.
int model_reader_check(const sbo_ctx* c, const char* who, bool need_f64);
int model_reader_begin(sbo_ctx* c, const char* who, bool need_f64);
// what the point calls ask of a caller's array before anything is copied
inline bool all_finite(const double* p, size_t count) {
  for (size_t t = 0; t < count; ++t)
    if (!std::isfinite(p[t])) return false;
  return true;
}

// Hands out consecutive blocks of one buffer, each at a multiple of `align` bytes.  A layout is one sequence of take() calls, run
// once on a null base for the size and once on the buffer for the pointers.  `floor`: the least alignment of every block.
struct Carve {
  unsigned char* base;
  size_t off = 0, floor = 1;
  template <class T> void take(T*& p, size_t count, size_t align = alignof(T)) {
    align = align > floor ? align : floor;
    off = (off + align - 1) / align * align;
    p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += sizeof(T) * count;
  }
};
// the two passes of `layout` (Carve -> the offset it ends at) over a buffer that grows to hold it
template <class F> int carve(DevBuf& buf, F&& layout, size_t floor = 1) {
  const size_t bytes = layout(Carve{nullptr, 0, floor});
  if (int rc = ensure(buf, bytes)) return rc;
  if (layout(Carve{(unsigned char*)buf.p, 0, floor}) != bytes) return fail(SBO_E_INVALID, "a scratch layout changed between its two passes");
  return SBO_OK;
}

// f(std::integral_constant<int, D>{}) for the padded input dimension D = 2, 4 or 8 (ModelConst::dpad): a launch line is written once,
// as a generic lambda `[&](auto D) { ... k<D()> ... }`
template <class F> auto with_dpad(int dpad, F&& f) {
  switch (dpad) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}
// S paths or draws in padded columns, 16 | 32 | 64 (S = 1 does not pay for 64), and f(std::integral_constant<int, Spad / 16>)
inline int spad_of(int S) { return S <= 16 ? 16 : S <= 32 ? 32 : 64; }
template <class F> auto with_spad(int Spad, F&& f) {
  switch (Spad) {
    case 16: return f(std::integral_constant<int, 1>{});
    case 32: return f(std::integral_constant<int, 2>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

// the posterior inside a sweep, without synchronisation or timing (api.hip); `out` (nullptr: not wanted) is reset first
int posterior_enqueue(sbo_ctx* c, const PostRequest& req, PostOutcome* out);
// the K1 stop event ev[1] behind a posterior enqueue: the last kernel carried it, or a record of its own
inline hipError_t k1_stop(sbo_ctx* c, const PostOutcome& out) { return out.stop_attached ? hipSuccess : hipEventRecord(c->ev[1], c->stream); }

// launchers implemented in the .hip files -----------------------------------------------------
int launch_posterior(sbo_ctx* c, const PostRequest& req, PostOutcome& out);
int launch_bound(sbo_ctx* c, double b, int index, int kind, void* dev_out);
int model_build(sbo_ctx* c, const double* const* host_invK, const double* X_norm, const double* Y_norm);
int model_prep(sbo_ctx* c, const double* X_norm);
// fit.hip: the DE of every output side by side and, with polish != 0, a projected BFGS from every output's DE best; x / nll are
// what a model is built from (the polished point where it is strictly lower).  Arguments are the caller's to check.
struct FitBatchResult {
  double x[kMaxQ][kMaxD + 2], de_x[kMaxQ][kMaxD + 2], nll[kMaxQ], de_nll[kMaxQ];
  int generations[kMaxQ], polish_status[kMaxQ], polish_evals[kMaxQ], polished[kMaxQ];
  int host_syncs;                 // read-backs the host waited for: one per convergence check and the final one
  double de_ms, polish_ms;        // host clock: upload + search up to its last check | polish + result read-back
};
int fit_batch(sbo_ctx* c, int n, int d, int q, const double* X_norm, const double* Y_norm, int P, const double* lo, const double* hi,
              const double* init_pop, const uint64_t* seeds, int maxiter, double tol, double atol, int polish, int polish_maxiter,
              double ftol, double gtol, FitBatchResult& out);
int model_factor_enqueue(sbo_ctx* c);
int model_pack_invk(sbo_ctx* c);         // images of the caller's invK for the K1b tables, when the grid arrived after the model   // the deferred factor chain of a caller's invK, behind everything on the critical path
// An update of the resident model, staged: computed into scratch and accepted by the device, nothing of the model written yet (a grown
// capacity keeps every value).  `rows`: +1 (one appended row), +k (a block), -1 (row `index` leaves).  The operands are what the commit
// kernel of its kind reads (appendbuf, laid out once by the stage function); `serial` / `ld`: the model and factor it was staged against.
struct ModelUpdate {
  int rows = 0, index = -1, ld = 0;
  unsigned long long serial = 0;
  const double *rho = nullptr, *scratch = nullptr, *sk = nullptr;     // one row: k_model_append_commit
  const double *U = nullptr, *G = nullptr, *w = nullptr;               // a block: k_append_commit
};
// One row (x_norm_new [d], y_norm_new [q]): the cross-covariances on the host, k_model_append, one wait for the verdict; SBO_E_INVALID
// when an output's s <= 0.  A block (x_norm_new [k][d], y_norm_new [k][q]): the five block kernels, one wait;
// SBO_E_INVALID when a Schur pivot is not > 0.  A removal cannot be refused on the device: its update is model_update_staged(c, -1, index).
int model_append_stage(sbo_ctx* c, const double* x_norm_new, const double* y_norm_new, ModelUpdate& u);
int model_append_block_stage(sbo_ctx* c, int k, const double* x_norm_new, const double* y_norm_new, ModelUpdate& u);
ModelUpdate model_update_staged(const sbo_ctx* c, int rows, int index = -1);
// Writes a staged update into the resident factor / alpha (enqueued, not waited for; mc.n still the old n) and drops the images of a
// caller's invK, which follow no update.  SBO_E_INVALID when the model or its factor moved since the update was staged.
int model_update_commit(sbo_ctx* c, const ModelUpdate& u);
// leave-one-out diagnostics of the resident factor / alpha; waited for: *host then points at LooSummary[kMaxQ] | resid [n][q] | var [n][q]
// (the arrays only with `arrays`)
int model_loo(sbo_ctx* c, double b, bool arrays, const unsigned char** host);
int model_repack(sbo_ctx* c);
bool bilinear_applicable(const sbo_ctx* c);
int bilinear_basis_enqueue(sbo_ctx* c, hipStream_t st, bool force_big);
bool interp_applicable(const sbo_ctx* c);
int interp_setup(sbo_ctx* c);
int guard_probe_gradients(sbo_ctx* c, hipStream_t st, double* ppts, double* grad_out, const sbo::ModelConst* mcp = nullptr);
int bilinear_setup(sbo_ctx* c);
int launch_posterior_gemm(sbo_ctx* c, bool interp, const PostRequest& req, PostOutcome& out);   // on the operands of K1i's plan (interp) or of K1b's
// What a change makes stale.  Every entry point and every option handler (api.hip) calls exactly one of the three functions below
// and writes no validity flag itself; where the cases differ, the reason stands here.
// Both GEMM-posterior plans, the posterior and the fp32 band: a new model, new candidates, or an option the plans are built with.
// (Not K1t's plan: it keys itself on the model's serial and the grid, tensor_applicable compares them.)
// Somebody other than a K1b column-path launch of the resident plan writes (or is about to write) sbo_ctx::mean / var: the stored
// values of the constraint are no longer the plan's on every tile (BilinearPlan::encl_ready).
inline void post_regions_written(sbo_ctx* c) { c->bl.encl_ready = c->bl.vals_ready = c->bl.lrows_ready = false; c->bl.omap_dirty = true; }
// ... single candidates of it are overwritten with other values (the guard's exact recheck): see BilinearPlan::vals_ready
inline void post_values_patched(sbo_ctx* c) { c->bl.vals_ready = false; c->bl.omap_dirty = true; }
inline void plans_invalidate(sbo_ctx* c) {
  c->bl.valid = false;
  c->bi.valid = false;
  c->posterior_valid = false;
  c->recheck.invalidate();
}
// sbo_model_set (before it touches the resident model) and model_update_run (api.hip: the driver of sbo_model_append, sbo_model_append_batch
// and sbo_model_remove, once the rows are in place: a refused or failed update leaves everything as it was).  The factor and invK flags are
// the model builder's own (model.hip: model_build, model_update_commit).
inline void model_changed(sbo_ctx* c) {
  c->masks_valid = false;
  c->rob.invalidate();
  plans_invalidate(c);
}
enum CandKind { kCandPoints, kCandGrid, kCandGridSharded };
inline void candidates_changed(sbo_ctx* c, CandKind kind) {
  if (kind == kCandPoints) c->lx.valid = false;          // (a grid leaves the index of the last list alone: only a list reads it, and every list drops it)
  else for (auto& g : c->dist.halo_guess) g = -1;        // (points: the halo guess is a property of grids)
  c->dist.sharded = kind == kCandGridSharded;
  c->rob.invalidate();
  plans_invalidate(c);
  c->masks_valid = false;
}
enum OptEffect {
  kOptNothing,     // read where it is used
  kOptPlans,       // the GEMM plans are built with it
  kOptPlansBand,   // guard_band: every plan measures its band when it is built -- K1t's too, which no model or grid change needs to drop
  kOptTensor,      // K1t's plan and the posterior it may have written
  kOptInterp,      // grad_defer: K1i's plan is laid out for it; K1b's is not, and a resident posterior stays what it is
  kOptPosterior    // posterior_path: another exact kernel sums in another order -- the posterior and an fp32 model's band, but no plan
};
inline void option_changed(sbo_ctx* c, OptEffect effect) {
  switch (effect) {
    case kOptNothing: break;
    case kOptPlans: plans_invalidate(c); break;
    case kOptPlansBand: plans_invalidate(c); c->tn.invalidate(); break;
    case kOptTensor: c->tn.invalidate(); c->posterior_valid = false; break;
    case kOptInterp: c->bi.valid = false; break;
    case kOptPosterior: c->posterior_valid = false; c->recheck.invalidate(); break;
  }
}
bool tensor_applicable(const sbo_ctx* c);
int launch_posterior_tensor(sbo_ctx* c, const PostRequest& req, bool* declined);
int launch_posterior_on_axes(sbo_ctx* c, int d, const long long* count, const double* axc, double* mean_out, double* var_out, double* grad_out,
                             unsigned long long* lmax);
// the exact posterior of the generic kernel on an explicit fp64 list [N][d] (device), into caller-given arrays [q][N]
int launch_posterior_on_list(sbo_ctx* c, const double* pts, long long N, double* mean_out, double* var_out);
// paths.hip: the preparation of sbo_sample_paths for a caller that evaluates the paths itself (sbo_refine_paths, refine.hip).
// paths_check_draws: the refusals of the draws (ranges, output, finite entries).  paths_prepare_list: the draws' device copies, the
// B operand and the packed per-path image in sbo_ctx::pathbuf, with room for a list of m points -- valid until the next call that
// carves pathbuf.  paths_eval_list: sbo_sample_paths' own evaluator (k_path_main) on pts -> vals, so a value of (point, path) is the
// bit pattern sbo_sample_paths returns there.  Everything is enqueued on c->stream; the caller waits.
struct PathDraws {
  int output, S, F;
  const double *omega, *phase, *weights, *noise;   // the caller's [F][d], [F], [S][F], [S][n]
  std::vector<double> omega_padded;                // (the host image the upload reads: it lives until the caller's wait)
};
struct PathImage {
  const double* Bt;        // [S][F + n]: path s' scaled weights, then c_s
  const double *om, *ph;   // [KF][dpad], [KF]
  const double *B, *As, *sq;   // the evaluator's operands: B [KF + KN][Spad], the scaled observations and their squares
  double *pts, *vals;     // the caller's list [m][d] and its values [m][S]
  int F, S, output;
  long long m;
};
int paths_check_draws(const sbo_ctx* c, const PathDraws& dr);
int paths_prepare_list(sbo_ctx* c, PathDraws& dr, long long m, PathImage* img);
int paths_eval_list(sbo_ctx* c, const PathImage& img);
// guard.hip: the exact evaluator that the band of the resident posterior was measured against, on a list; K1b's band (device,
// enqueued behind the first posterior launch of a plan); a host-known band (K1t) or "none" (exact kernels)
int guard_exact_list(sbo_ctx* c, const double* pts, long long N, double* mean_out, double* var_out);
int guard_exact_grad_list(sbo_ctx* c, const double* pts, long long N, double* grad_out /* [q][d][N] */);
int guard_probe_reference(sbo_ctx* c, hipStream_t side, double** ref_m, double** ref_v, const sbo::ModelConst* mcp = nullptr);       // -> gb.probe: [q][P] each; K1b's own values follow at + 2 q P
// what K1b's band kernel needs to carry the axis bases' truncation through the posterior formula (guard.hip: k_gb_band)
struct GbAnalytic {
  const double* axis_eps;   // [2 q][2]: largest of the last four Chebyshev coefficients of the axis factors | sqrt(rc) x largest residual row norm of the basis
  const double* alpha;      // [q][a_ld]
  int a_ld, n;
  int rc[sbo::kMaxQ][2];         // Chebyshev degree of the axis factors
  const double* Xn;         // [n][dpad] normalised observations, and the normalised interval of each grid axis (a0, b0, a1, b1)
  int dpad, pad;
  double ab[4];
  const double* ref_g;      // [q][2][P] exact gradient components of the mean at the probe points (a lower bound on the Lipschitz keys)
};
int guard_band_from_probes(sbo_ctx* c, const double* pm, const double* pv, const double* ref_m, const double* ref_v, const double* tail, const GbAnalytic& an);
int guard_band_host(sbo_ctx* c, const double* dm, const double* dv, const double* rl, const double* parts = nullptr /* analytic dm | dv | probe dm | dv, kMaxQ each */);
int guard_audit_enqueue(sbo_ctx* c, const PostOutcome& out);   // behind the posterior launch of a sweep (out.col_lean: the objective's values are incomplete)
void guard_audit_harvest(sbo_ctx* c, bool wait);         // collect a finished audit's counts (wait: block until it has finished)
}  // namespace sbo

#define SBO_HIP(x)                                                   \
  do {                                                               \
    hipError_t e__ = (x);                                            \
    if (e__ != hipSuccess) return sbo::hip_fail(e__, #x);            \
  } while (0)
