/*
 * safebo.h -- C ABI of libsafebo.so: the MI355X (gfx950) candidate-sweep engine for
 * SafeOpt / GoOSE safe Bayesian optimisation.
 *
 * The reference project (dleeim/Safe-Bayesian-Optimization) is pure Python/JAX and has no
 * FFI seam of its own; the seam this library sits behind is the one SURVEY.md section 8(b) names:
 *
 *   state crossing the seam  = the `inference_datasets` dict      models/GP_Safe.py:16-23, 236-245
 *                              + `bound`, `b`                     models/SafeOpt.py:12-13
 *   calls replaced           = GP.GP_inference (batched)          models/GP_Safe.py:310-352
 *                              BO.mean / ucb / lcb (batched)      models/SafeOpt.py:29-45, test/test_SafeOpt.py:337
 *                              BO.Minimizer / BO.Expander         models/SafeOpt.py:53-66, 90-124
 *                              BO.minimize_obj_lcb / Target /
 *                              explore_safeset                    models/GoOSE.py:63-67, 80-119
 *
 * Conventions
 *   - every entry point returns an int status (SBO_OK == 0, errors < 0) and never throws;
 *     sbo_last_error() returns a thread-local message for the last failing call.
 *   - host pointers are borrowed for the duration of the call only (the library copies);
 *     arrays are C-contiguous, row-major.  Model arrays are always passed as double; the
 *     `dtype` tag selects the arithmetic the kernels run in (the arrays are rounded once on upload).
 *   - one sbo_ctx per process and per GPU (one process per GPU, ranks joined with sbo_comm_init);
 *     a ctx is single-caller; calls return after the device work they issued has completed unless
 *     the entry point says "asynchronous".
 *   - flat candidate index g: for grids, axis 0 is the fastest axis
 *     (jnp.meshgrid 'xy' + ravel, test/test_SafeOpt.py:325-334); indices reported in results are
 *     GLOBAL flat indices (shard offset included).
 *   - there is no CPU fallback: without a HIP device sbo_init fails with SBO_E_HIP.
 */
#ifndef SAFEBO_H
#define SAFEBO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBO_ABI_VERSION 3
#define SBO_MAX_D 8        /* input dimension limit (reference problems use d = 2)          */
#define SBO_MAX_Q 8        /* modelled outputs: objective + constraints                      */
#define SBO_MAX_N 2048     /* observations                                                   */

enum sbo_status {
  SBO_OK = 0,
  SBO_E_INVALID = -1,         /* bad argument (maps to ValueError, as models/GP_Safe.py:134-137) */
  SBO_E_NOMEM = -2,
  SBO_E_HIP = -3,             /* HIP runtime error / no device                                   */
  SBO_E_NO_MODEL = -4,        /* sweep before sbo_model_set                                      */
  SBO_E_NO_CANDIDATES = -5,   /* sweep before sbo_candidates_*                                   */
  SBO_E_EMPTY_SAFE_SET = -6,  /* S_t is empty on this candidate set (all ranks)                  */
  SBO_E_COMM = -7,            /* RCCL error                                                      */
  SBO_E_UNSUPPORTED = -8
};

enum sbo_dtype { SBO_F64 = 0, SBO_F32 = 1 };

/* which matrix the variance contraction uses */
enum sbo_factor {
  SBO_FACTOR_INVK = 0,  /* caller's invK (models/GP_Safe.py:231-232): alpha = invK (y - mp) uses it as given, the
                           variance uses its triangular factor M (M^T M = invK):  k^T invK k = ||M k||^2        */
  SBO_FACTOR_CHOL = 1   /* library builds K + (sn2 + float32 eps) I = L L^T itself and contracts with M = L^-1:
                           var = sf2 - || L^-1 k ||^2  (used when invK == NULL)                            */
};

enum sbo_bound_kind { SBO_MEAN = 0, SBO_UCB = 1, SBO_LCB = 2, SBO_VAR = 3 };

enum sbo_mask {
  SBO_MASK_S = 0,   /* safe set                 models/SafeOpt.py:57-59                                   */
  SBO_MASK_U = 1,   /* "fully unsafe" witnesses models/SafeOpt.py:73-77, 109                              */
  SBO_MASK_M = 2,   /* potential minimisers     models/SafeOpt.py:62                                      */
  SBO_MASK_G = 3,   /* expanders G_c  (index c = 1..q-1)  models/SafeOpt.py:85-88, 111                    */
  SBO_MASK_O = 4    /* GoOSE optimistic set O_c (c = 1..q-1)  models/GoOSE.py:93-101                      */
};

typedef struct sbo_ctx sbo_ctx;

typedef struct sbo_sweep_opts {
  double b;                        /* confidence multiplier beta, models/SafeOpt.py:13                    */
  int32_t reference_quirk_L_index; /* 1: every constraint uses L_{q-1} (models/SafeOpt.py:110 loop leak);
                                      0: constraint c uses L_c                                            */
  int32_t want_masks;              /* 1: keep S/U/M/G (or O) masks in HBM for sbo_masks_get               */
  int32_t posterior_ready;         /* 1: reuse mean/var of the last sbo_posterior_run on these candidates */
  int32_t lean;                    /* the caller wants the sweep's result only -- sets, indices, counts, u*, the constraints' L.  1: the
                                      sweep may leave mean / var unwritten where no later stage of it reads them (the objective on posterior
                                      tiles without a safe candidate: u*, M and the arg-max reductions are over S only,
                                      models/SafeOpt.py:47-66); 2: it need not even evaluate them there (the result is the same), nor
                                      the constraint on the posterior tiles whose enclosure (per plan, from its first full evaluation)
                                      proves every candidate unsafe at this b and outside the guard band (sbo_profile.k1_tiles_skipped;
                                      one-constraint column path, from the plan's second sweep on), nor -- option "k1_skip_safe" -- on
                                      the tiles it proves safe throughout (k1_tiles_skipped_safe): there the set phase reads what the
                                      plan's first full evaluation stored, so any other writer of the resident posterior (another
                                      posterior kernel, sbo_posterior_run, a model / grid / option change) makes the next sweep of the
                                      plan evaluate and record everything again.  A later lean 2 sweep of a plan READS what an
                                      earlier one stored (option "k1_resident"): the constraint's listed tiles and the objective's
                                      tiles whose stored mean / var are the plan's are classified from memory, whatever b -- the
                                      posterior does not depend on it (sbo_profile.k1_tiles_resident_c / _o).  A lean
                                      SafeOpt sweep of a model with constraints reports L[0] = 0: the objective's Lipschitz key is read by
                                      no sweep of the reference (its expanders use the constraints' keys, models/SafeOpt.py:110,
                                      models/GoOSE.py:100), and the interpolating posteriors then leave its gradient fields out.
                                      sbo_posterior_get / sbo_bounds / a posterior_ready sweep behind a lean sweep run K1 again.  0 (the
                                      default): the whole posterior is evaluated and stays resident, as models/GP_Safe.py:310-352 returns it */
} sbo_sweep_opts;

typedef struct sbo_safeopt_result {
  /* Minimizer(): argmax_{M_t} var_0, returns (x, sqrt(var_0))           models/SafeOpt.py:53-66          */
  int64_t minimizer_index;
  double  minimizer_x[SBO_MAX_D];
  double  minimizer_std;
  /* Expander(): per constraint argmax_{G_c} var_0, most uncertain kept   models/SafeOpt.py:90-124         */
  int64_t expander_index_c[SBO_MAX_Q];   /* [c-1], -1 when G_c is empty; -1 past entry q-2 as well         */
  double  expander_std_c[SBO_MAX_Q];     /* [c-1], 0 when G_c is empty; 0 past entry q-2 (count_G too)     */
  int32_t expander_best_c;               /* constraint index of the kept expander, 0 when none            */
  int64_t expander_index;
  double  expander_x[SBO_MAX_D];
  double  expander_std;
  int32_t choose_minimizer;              /* std_min > std_exp, test/test_SafeOpt.py:153                   */
  double  u_star;                        /* min_{S_t} ucb_0, models/SafeOpt.py:47-51, 61                  */
  double  L[SBO_MAX_Q];                  /* max over candidates of ||grad MEAN_i||_inf, SafeOpt.py:79-83  */
  int64_t count_S, count_U, count_M;
  int64_t count_G[SBO_MAX_Q];            /* [c-1]                                                         */
  int64_t n_exact_rechecks;              /* expander decisions that fell in the +1e-8 ambiguity band and
                                            were re-decided by exhaustive evaluation                      */
  /* Guard band of an approximating posterior kernel (K1b: Chebyshev core, K1t: Chebyshev-node interpolation; zero for the exact
   * kernels): decisions of the first pass that the band +- (sbo_profile.guard_dm, guard_dv) left open; when non-zero the
   * candidates concerned were re-evaluated by the exact kernel and the set phase ran again, so that every mask and index
   * returned is that of the exact posterior                                                                              */
  int64_t guard_band;                    /* decisions inside the band on the first pass (0: the first pass is the result)  */
  int64_t guard_rechecks;                /* candidates re-evaluated by the exact kernel                                     */
  int32_t guard_passes;                  /* set-phase passes of the re-evaluation (0: none was needed)                      */
  int32_t reserved_g;
} sbo_safeopt_result;

typedef struct sbo_goose_result {
  int64_t safe_min_index;                /* argmin_{S_t} lcb_0            models/GoOSE.py:63-67            */
  double  safe_min_x[SBO_MAX_D];
  double  safe_min_lcb;
  int64_t target_index_c[SBO_MAX_Q];     /* per constraint argmin_{O_c} lcb_0, -1 when empty   :82-112;
                                            -1 past entry q-2 as well                                      */
  double  target_lcb_c[SBO_MAX_Q];       /* [c-1], +inf when O_c is empty; 0 past entry q-2 (count_O too) */
  int32_t target_best_c;
  int64_t target_index;
  double  target_x[SBO_MAX_D];
  double  target_lcb;
  int64_t explore_index;                 /* argmin_{S_t} ||x - target||_2  models/GoOSE.py:116-119        */
  double  explore_x[SBO_MAX_D];
  int32_t choose_safe_min;               /* min_safe_lcb <= target_lcb, test/test_GoOSE.py:158            */
  double  L[SBO_MAX_Q];
  int64_t count_S, count_U;
  int64_t count_O[SBO_MAX_Q];
  int64_t n_exact_rechecks;              /* candidates decided by the exhaustive reference predicate (expanders + coverage) */
  int64_t guard_band, guard_rechecks;    /* as in sbo_safeopt_result                                                        */
  int32_t guard_passes, reserved_g;
} sbo_goose_result;

typedef struct sbo_tr_result {
  int64_t index;                 /* argmin_{S_t and ||x - x_0|| <= r} lcb_0, -1 when that set is empty (models/GP_TR.py:43-51) */
  double  x[SBO_MAX_D];
  double  lcb;
  int64_t count_S, count_T;      /* |S_t|, |S_t intersected with the ball|                                                  */
  int64_t guard_band, guard_rechecks;    /* as in sbo_safeopt_result                                                        */
  int32_t guard_passes, reserved_g;
} sbo_tr_result;

/* StableOpt's robust min-max on a joint (xc, d) grid (models/StableOpt.py:139-164): axes 0 .. n_control_axes - 1 of the resident grid
 * are the controls xc, the rest the disturbance d (the slow axes: every disturbance point is one contiguous plane of the control
 * sub-grid).  Flat indices of xc / d are those of the two sub-grids (axis 0 / axis n_control_axes the fastest).                        */
typedef struct sbo_robust_result {
  int64_t index;                 /* argmin over robust-safe xc (min_d lcb_c >= 0 for every constraint c) of max_d bound_0; -1: none    */
  double  xc[SBO_MAX_D];
  double  value;                 /* min over robust-safe xc of max_d bound_0 (+inf when index == -1)                                    */
  int64_t worst_d_index;         /* argmax_d bound_0(xc*, d), ties -> lowest index (-1 when index == -1)                                */
  double  worst_d[SBO_MAX_D];
  int64_t candidate_index;       /* global flat index of (xc*, d*) on the joint grid                                                   */
  int64_t count_control, count_disturbance, count_safe;   /* |xc grid|, |d grid|, robust-safe controls                                 */
  int64_t guard_band, guard_rechecks;    /* as in sbo_safeopt_result; the re-evaluation reruns the exact kernel on the whole grid (rechecks
                                            = this rank's candidates)                                                                   */
  int32_t guard_passes, reserved_g;
} sbo_robust_result;

/* per-kernel device time of the last sweep / posterior call, measured with HIP events on the
 * library's stream (feeds bench.py's roofline.achieved) */
typedef struct sbo_profile {
  double posterior_ms;     /* K1: fused cross-covariance + contraction + mean/var                          */
  double classify_ms;      /* K3: bounds, S/U masks, u* (with "set_fuse" the merge of the partials and the M mask
                              ride in the expander's first launches and are counted there)  (these three: 0 unless option */
  double expander_ms;      /* K4: distance transform + G_c / O_c decisions  "phase_events" is 1 -- an event  */
  double argreduce_ms;     /* K5: masked arg-max / arg-min                   costs a ~6 us bubble per record) */
  double comm_ms;          /* RCCL collectives (option "comm_events": an event pair around every call -- bubbles, so off by default) */
  double total_ms;         /* first launch to last completion                                              */
  double posterior_flops;  /* algorithmic flops of the K1 launch(es): q (n^2 + (2d+10) n) per candidate    */
  int64_t candidates;      /* candidates swept by this rank                                                */
  int32_t posterior_launches;
  int32_t posterior_kernel;      /* which K1 ran last: 1 generic, 2 generic chunked, 3 separable tables (K1g), 4 bilinear GEMMs (K1b),
                                    5 Chebyshev-node interpolation on 3-D / 4-D grids (K1t), 6 the same two GEMMs as 4 on coefficients
                                    interpolated from exactly evaluated Chebyshev nodes: a model's first sweep on a 2-D grid (K1i) */
  double posterior_executed_flops; /* matrix-core flops the last K1 launch(es) actually issued (K1b: far below the algorithmic count) */
  double posterior_setup_ms;     /* host time of the last per-(model, grid) table build of K1b, 0 when none was needed        */
  int64_t fp64_rechecks;         /* dtype SBO_F32 SafeOpt sweeps: candidates whose fp32 bounds could not decide S / U / u* / M / the
                                    minimiser and were re-evaluated in fp64 (option "fp64_recheck"); 0 otherwise                  */
  double recheck_ms;             /* device time of that step (band reductions, flagging, fp64 posterior of the list, scatter)    */
  double set_phase_ms;           /* K1 stop event -> end of the sweep: what the set phase (K3-K5 + collectives) adds to K1          */
  int32_t host_syncs;            /* host waits on the device inside the last sweep call (1 = the result read-back only)          */
  int32_t comm_calls;            /* collectives of the last sweep; comm_ms is their event-timed sum when option "comm_events" is 1 */
  int64_t comm_bytes;            /* multi-rank sweeps: bytes this rank handed to the collectives of the last sweep (send side)     */
  /* guard band of the posterior kernel that ran last (un-normalised units; zero for the exact kernels K1 / K1c / K1g)             */
  double guard_dm[SBO_MAX_Q], guard_dv[SBO_MAX_Q], guard_rl[SBO_MAX_Q];   /* |mean - exact|, |var - exact|, relative band of L       */
  double guard_ms;               /* device + host time of the last sweep's re-evaluation (0: none was needed)                      */
  int32_t halo_reruns;           /* multi-rank: set phases run again because SOME rank's speculative halo window was too narrow
                                    (the decision is global; host_syncs / comm_* include the discarded pass)                        */
  int32_t set_path;              /* set phase of the last SafeOpt sweep: 0 byte masks, 1 column words written by the GEMM posterior (r05)    */
  /* Standing audit of the guard band (r05; option "guard_audit" = samples per sweep, default 4096): behind every SafeOpt sweep on K1b /
   * K1i with a caller's invK, a rotating sample of the candidates is re-evaluated with the reference formula (models/GP_Safe.py:341-343)
   * on a side stream and compared with what the posterior kernel stored.  Cumulative over the context's life (a finished audit is
   * collected by the next call): value pairs compared, pairs whose |difference| exceeded the band (guard_dm / guard_dv) -- the claim
   * every mask and index rests on: must stay 0 --, and the largest deviation seen in units of the band.                             */
  int64_t guard_audit_samples, guard_audit_violations;
  double guard_audit_worst;
  /* What the band is made of (r05, K1b / K1i): the ANALYTIC part -- the truncations the plan makes, carried through the posterior formula
   * (csrc/guard.hip: k_gb_band; csrc/bilinear.hip: k_gb_band_i) -- and the largest deviation seen at the plan's 144 probe points, which
   * only CHECKS it: guard_dm = analytic + rounding floor, or 1e300 (plan not trusted, every sweep re-evaluates exactly) when
   * 4 x probe exceeds that.  Zero for the exact kernels and for K1t (whose band is 16 x 2048 probes, measured).                       */
  double guard_analytic_dm[SBO_MAX_Q], guard_analytic_dv[SBO_MAX_Q], guard_probe_dm[SBO_MAX_Q], guard_probe_dv[SBO_MAX_Q];
  /* r06: posterior tiles (64 x 128 candidates) of the constraint that the last sweep left unevaluated -- a lean 2 sweep on the column
   * path (set_path 1) whose plan's per-cell enclosures of mean / var prove every candidate of the tile unsafe and outside the band.  */
  int64_t k1_tiles_skipped;
  /* ... and those it left unevaluated because the enclosures prove every candidate of the tile SAFE and outside the band (option
   * "k1_skip_safe"): every S bit, no U bit, the stored mean / var of the plan's recording sweep stand for the tile's values.          */
  int64_t k1_tiles_skipped_safe;
  /* Option "k1_resident": posterior tiles the last sweep classified from the mean / var an earlier sweep of the plan stored, without
   * running the GEMM phases again -- in the constraint's launch (the listed, evaluated tiles) and in the objective's (the tiles with a
   * safe candidate whose stored values are the plan's).  Zero unless the sweep was a lean 2 sweep on the column path of a plan whose
   * enclosures are recorded.                                                                                                        */
  int64_t k1_tiles_resident_c, k1_tiles_resident_o;
  /* Option "k1_cells": 8 x 8 cells of the k1_tiles_resident_c tiles whose stored mean / var the last sweep loaded and classified
   * candidate by candidate -- the cells the plan's enclosures prove neither safe nor unsafe at that sweep's b and band; the other cells
   * of those tiles got their bits from the proof.  Zero when the sweep did not take that path (then every cell of a resident tile is
   * loaded: 128 x k1_tiles_resident_c).                                                                                              */
  int64_t k1_cells_evaluated;
  /* of guard_audit_samples: samples on tiles of either kind, where the audit checks the reference values against the tile's enclosure
   * (widened by the band) instead of the stored ones -- on a proved-safe tile also the stored values, which must lie inside the
   * enclosure bit for bit.  Cumulative, as guard_audit_samples.                                                                      */
  int64_t guard_audit_skipped;
  /* Spatial index of an explicit list (option "list_index"; zero when the last sweep did not use it): device time of building its
   * sorted order (Morton keys, radix sort, sorted copy of the points) when the last sweep built it, 0 when it reused it; the
   * (candidate, U point) pairs the expander walk evaluated at its leaves, and the nodes whose box it skipped, summed over the
   * constraints.  GoOSE's coverage search on the sorted order does not count pairs.                                                */
  double list_index_build_ms;
  int64_t list_index_leaf_pairs, list_index_nodes_skipped;
  /* Band of the last sweep of a dtype SBO_F32 model (option "fp64_recheck"): the half-widths, per output and in un-normalised units,
   * within which that sweep took the fp32 mean / variance to lie of the fp64 values -- max(1e-4 normalised, 16 x the largest deviation the
   * fp64 twin measured at the probe candidates of this (model, candidate set)).  Zero for fp64 models and with the recheck off.    */
  double fp32_band_dm[SBO_MAX_Q], fp32_band_dv[SBO_MAX_Q];
} sbo_profile;

/* ---- library / context ------------------------------------------------------------------- */
int sbo_version(void);
const char* sbo_last_error(void);
int sbo_device_count(int* count);
int sbo_init(int device_id, sbo_ctx** out);
int sbo_shutdown(sbo_ctx* ctx);
int sbo_synchronize(sbo_ctx* ctx);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ---------------------------------------- */
#define SBO_COMM_ID_BYTES 128
int sbo_comm_unique_id(void* id_out /* SBO_COMM_ID_BYTES, filled on rank 0 and sent to peers */);
/* world_size == 1 with id == NULL: no communicator (the collectives are identities and are skipped); with an id a
 * one-rank RCCL communicator is built all the same (see option "comm_selftest").  On failure the context stays
 * single-rank and usable. */
int sbo_comm_init(sbo_ctx* ctx, int world_size, int rank, const void* id);
int sbo_comm_barrier(sbo_ctx* ctx);
/* Rehearsal transport for test rigs where the ranks cannot form an RCCL communicator (e.g. two ranks sharing
 * the one GPU of a test box, which RCCL refuses): the same collectives, staged through host memory and carried
 * by caller-supplied functions (the tests use torch.distributed/gloo).  elem: 0 = uint64, 1 = double;
 * op: 0 = sum, 1 = max, 2 = min.  Not a production path: RCCL over xGMI is. */
typedef int (*sbo_relay_allreduce_fn)(void* user, void* buf, int64_t count, int elem, int op);
typedef int (*sbo_relay_allgather_fn)(void* user, const void* send, void* recv, int64_t bytes_per_rank);
int sbo_comm_init_relay(sbo_ctx* ctx, int world_size, int rank, sbo_relay_allreduce_fn allreduce,
                        sbo_relay_allgather_fn allgather, void* user);

/* ---- model state = inference_datasets (models/GP_Safe.py:236-245) -------------------------- */
/* hypopt is [d+2, q]: rows 0..d-1 = log ell_a, row d = log sigma_f, row d+1 = log sigma_n, consumed as
 * exp(2 h) (models/GP_Safe.py:338).  invK is q stacked [n, n] matrices or NULL (see sbo_factor).
 * kernel must be "RBF" (models/GP_Safe.py:159-162), anything else is SBO_E_INVALID. */
int sbo_model_set(sbo_ctx* ctx, int dtype, const char* kernel, int n, int d, int q,
                  const double* X_mean, const double* X_std, const double* Y_mean, const double* Y_std,
                  const double* X_norm, const double* Y_norm, const double* hypopt, const double* invK);

/* The same with invK as the reference holds it: `invKopt`, a list of q separate [n, n] arrays (models/GP_Safe.py:231-232,
 * 244) -- no stacking copy on the host.  invK_list == NULL as above. */
int sbo_model_set_list(sbo_ctx* ctx, int dtype, const char* kernel, int n, int d, int q, const double* X_mean,
                       const double* X_std, const double* Y_mean, const double* Y_std, const double* X_norm,
                       const double* Y_norm, const double* hypopt, const double* const* invK_list);

/* The same with the prior mean given: mean_prior[q] in normalised units (models/GP_Robust.py:322-324 uses zero for every output).
 * mean_prior == NULL behaves exactly like sbo_model_set_list (GP_Safe's prior: 0 for the objective, -2 Y_mean / Y_std otherwise). */
int sbo_model_set_prior(sbo_ctx* ctx, int dtype, const char* kernel, int n, int d, int q, const double* X_mean,
                        const double* X_std, const double* Y_mean, const double* Y_std, const double* X_norm,
                        const double* Y_norm, const double* hypopt, const double* const* invK_list, const double* mean_prior);

/* ---- candidates (resident in HBM until replaced) ------------------------------------------- */
/* One more observation (normalised coordinates / outputs, the caller's frozen X_mean, X_std, Y_mean, Y_std) under the
 * hyper-parameters of the last sbo_model_set: the lower factor gains one row and alpha is updated in O(n^2) on the
 * device.  SURVEY.md 8(f) rank 2 -- an opt-in fast path; the reference itself refits and renormalises on every sample
 * (models/GP_Safe.py:283-304).  Fails with SBO_E_UNSUPPORTED at n = SBO_MAX_N (or when the resident factor cannot grow),
 * with SBO_E_INVALID for a non-finite x_norm_new / y_norm_new or when the new row leaves some output's K + sn2 I without a
 * positive pivot (s = kappa - k^T invK k <= 0).  On any error the model is as before the call: n, the factor, alpha and
 * everything a posterior or a sweep reads are unchanged. */
int sbo_model_append(sbo_ctx* ctx, const double* x_norm_new, const double* y_norm_new);

/* k observations in one block update: x_norm_new [k][d] and y_norm_new [k][q], normalised with the frozen
 * constants of the last sbo_model_set, enter in call order as observations n .. n + k - 1 and n becomes n + k; every later call sees
 * the larger model.  The result is the model k calls of sbo_model_append would leave (a lower factor with positive diagonal is
 * unique), but the two triangular products run as (n x n) (n x k) block products over the whole chip, followed by one k x k Schur
 * complement with its Cholesky, one verdict read-back, one re-pack of the factor images and one invalidation of the plans.  All
 * or nothing: every output's update is computed and checked before anything of the model is written; on any error n, the factor,
 * alpha and everything a posterior or a sweep reads are bit for bit as before (a grown capacity of the factor may stay).  Fails
 * with SBO_E_INVALID for NULL pointers, k < 1, k > SBO_MAX_APPEND, a non-finite coordinate or output, or a Schur pivot that is not
 * > 0 on some output (the message names the output and the row of the block); with SBO_E_UNSUPPORTED when n + k > SBO_MAX_N (no
 * row is appended, not even a prefix); with SBO_E_NO_MODEL without a model.  Waits first for a deferred factorisation.
 * Deterministic: the same model and the same rows give the same bits.  Multi-rank: the model is replicated, every rank makes the
 * same call, nothing is communicated. */
#define SBO_MAX_APPEND 64
int sbo_model_append_batch(sbo_ctx* ctx, int k, const double* x_norm_new /* [k][d] */, const double* y_norm_new /* [k][q] */);

/* The counterpart of sbo_model_append: observation `index` (0-based, in the order of X_norm as set and appended) leaves the resident model.  The
 * hyper-parameters, the normalisation constants and the prior mean stay frozen, the remaining observations keep their order
 * (row i > index becomes row i - 1) and n becomes n - 1; the lower factor and alpha are updated in O(n^2) on the device
 *  and no [n, n] matrix crosses the bus.  Every later call -- posterior, sweeps, refinement, an append,
 * another removal -- sees the (n - 1)-row model; a sliding window of recent data is a removal of index 0 followed by an
 * append.  Not the reference's behaviour either (it refits).  Fails with SBO_E_INVALID for an index outside [0, n) or for
 * n == 1 (a model holds at least one observation) and with SBO_E_NO_MODEL without a model; on any error the model is as
 * before the call.  Multi-rank: the model is replicated, every rank makes the same call, nothing is communicated (as for
 * sbo_model_append). */
int sbo_model_remove(sbo_ctx* ctx, int index);

/* Leave-one-out diagnostics of the resident model: is the frozen model still calibrated on its own data,
 * and which observation fits worst?  With P = invK, the prediction of observation i from all the others has the residual
 * e_i = y_i - mu_-i = alpha_i / P_ii and the variance v_i = 1 / P_ii (noise included); P_ii is a column sum of squares of the
 * resident lower factor M (M^T M = invK), so one pass over the triangle on the device gives every e_i and v_i in O(n^2) and
 * O(n q) bytes come back -- no [n, n] matrix is formed or crosses the bus.  Everything is in normalised units and fp64 whatever
 * the model dtype.  resid_out / var_out: [n][q] as in sbo_posterior_get, rows in the order of X_norm as set, appended and
 * removed; each of the three outputs may be NULL.  `outside` counts |z_i| > b, the test every safe set rests on
 * (|y - mean| <= b sqrt(var)).  The reference's NLL form (models/GP_Safe.py:169-192) is r^T alpha + logdet with
 * r = Y_norm - mean prior: since alpha_i = e_i / v_i, a caller forms it from these outputs and its own Y_norm (the library keeps
 * no copy of Y_norm).  The call is read-only: model, plans, caches, guard band and options are as before, and a posterior or
 * sweep after it equals one before it bit for bit; two calls on the same model return the same bits.  It waits for a deferred
 * factorisation first, so a caller's invK that is not positive definite gives SBO_E_INVALID here as elsewhere.  SBO_E_INVALID
 * also for a NULL ctx and for b not finite or < 0; SBO_E_NO_MODEL without a model.  Multi-rank: the model is replicated, any
 * rank may call, nothing is communicated. */
typedef struct sbo_model_loo_result {
  int32_t n, q;
  double  logdet[SBO_MAX_Q];    /* log det(K_o + sn2_o I) = -2 sum_i log M_o[i][i]                          */
  double  lpd[SBO_MAX_Q];       /* sum_i log N(y_i | mu_-i, v_i) = -1/2 sum_i (log(2 pi v_i) + e_i^2 / v_i) */
  double  z_max[SBO_MAX_Q];     /* max_i |z_i|,  z_i = e_i / sqrt(v_i) = alpha_i / sqrt(P_ii)               */
  int32_t z_argmax[SBO_MAX_Q];  /* its index; ties -> lowest index                                          */
  int32_t outside[SBO_MAX_Q];   /* #{ i : |z_i| > b }                                                       */
} sbo_model_loo_result;

int sbo_model_loo(sbo_ctx* ctx, double b, double* resid_out /* [n][q] or NULL */, double* var_out /* [n][q] or NULL */,
                  sbo_model_loo_result* result /* or NULL */);

/* explicit list: points[N, d] of doubles (dtype SBO_F64) or floats (SBO_F32); first_index = global flat
 * index of points[0] (shard offset). */
int sbo_candidates_points(sbo_ctx* ctx, const void* points, int points_dtype, int64_t n_local, int d,
                          int64_t first_index);
/* implicit tensor grid: x_a(i) = lo_a + i (hi_a - lo_a)/(count_a - 1), last = hi_a; this rank sweeps the
 * flat range [first_index, first_index + n_local). No HBM bytes are read for candidates. */
int sbo_candidates_grid(sbo_ctx* ctx, int d, const double* lo, const double* hi, const int64_t* count,
                        int64_t first_index, int64_t n_local);

/* same grid, sharded over the ranks of sbo_comm_init by whole hyper-planes of the slowest axis (rank r owns
 * planes [r P / W, (r+1) P / W)); returns this rank's flat range.  Required for multi-rank sweeps. */
int sbo_candidates_grid_sharded(sbo_ctx* ctx, int d, const double* lo, const double* hi, const int64_t* count,
                                int64_t* first_index_out, int64_t* n_local_out);

/* ---- hot path ------------------------------------------------------------------------------ */
/* K1: GP_inference for every local candidate; mean/var stay in HBM. */
int sbo_posterior_run(sbo_ctx* ctx);
/* copy out as [n_local, q] arrays of the model dtype (either pointer may be NULL) */
int sbo_posterior_get(sbo_ctx* ctx, void* mean_out, void* var_out);
/* batched BO.mean/ucb/lcb(points, index): out[n_local] of the model dtype (runs K1 if needed) */
int sbo_bounds(sbo_ctx* ctx, double b, int index, int kind, void* out);
/* full SafeOpt / GoOSE iteration on the resident candidates */
int sbo_sweep_safeopt(sbo_ctx* ctx, const sbo_sweep_opts* opts, sbo_safeopt_result* result);
int sbo_sweep_goose(sbo_ctx* ctx, const sbo_sweep_opts* opts, sbo_goose_result* result);
/* trust-region acquisition of models/GP_TR.py:43-51 on the resident candidates: x_0[d] centre, r radius */
int sbo_sweep_tr(sbo_ctx* ctx, const sbo_sweep_opts* opts, const double* x_0, double r, sbo_tr_result* result);
/* Robust min-max of models/StableOpt.py:139-152 on the resident grid (sbo_candidates_grid / _sharded; a point list is SBO_E_INVALID):
 * kind (SBO_MEAN / SBO_UCB / SBO_LCB) is the objective's bound, the constraints always use their LCB.  n_control_axes in [1, d - 1].
 * fp64 models only (SBO_F32: SBO_E_UNSUPPORTED -- an fp32 posterior with an fp64 recheck is not implemented here).  opts.lean and
 * opts.reference_quirk_L_index are ignored, opts.want_masks too (the masks of the last SafeOpt / GoOSE sweep stay as they were);
 * opts.posterior_ready is honoured.  sbo_profile: posterior_ms, argreduce_ms (reduction over d + mask + arg-min), guard_ms, total_ms. */
int sbo_sweep_robust(sbo_ctx* ctx, const sbo_sweep_opts* opts, int n_control_axes, int kind, sbo_robust_result* result);
/* the per-control arrays of the last robust sweep: f_out[Nc] = max_d bound_0, g_out[q - 1][Nc] = min_d lcb_c; either may be NULL */
int sbo_robust_get(sbo_ctx* ctx, double* f_out, double* g_out);
/* BO.explore_safeset(target) for a target of the caller's choosing (models/GoOSE.py:116-119): the candidate of the LAST sweep's safe set
 * closest to target[d] (scipy cdist's Euclidean distance, ties -> lowest flat index); x_out[SBO_MAX_D] may be NULL.
 * SBO_E_EMPTY_SAFE_SET when S_t is empty.  (sbo_sweep_goose answers the same question for its own target in its result.) */
int sbo_explore_safeset(sbo_ctx* ctx, const double* target, int64_t* index_out, double* x_out);
/* uint8 mask [n_local] of the last sweep (opts.want_masks); c is the constraint index for G / O */
int sbo_masks_get(sbo_ctx* ctx, int which, int c, uint8_t* out);

/* ---- model fit ------------------------------------------------- */
/* negative_loglikelihood (models/GP_Safe.py:169-192) for P hyper-parameter vectors at once:
 * hyper[P, d+2] rows = (log ell_0.., log sigma_f, log sigma_n); X_norm[n, d]; y[n] = one column of Y_norm;
 * out[p] = y^T K_p^-1 y + log|K_p| with K_p = sf2 exp(-1/2 D) + (sn2 + 1e-8) I (+inf if not positive definite).
 * This is the objective SciPy DE evaluates at models/GP_Safe.py:224, one population per call. */
int sbo_nll_batch(sbo_ctx* ctx, int n, int d, const double* X_norm, const double* y, int P, const double* hyper,
                  double* out);

/* The whole differential-evolution search of that objective on the device (models/GP_Safe.py:205-224: SciPy DE, default
 * best1bin strategy, mutation dithered in [0.5, 1), recombination 0.7; deferred updating here).  init_pop[P, d+2] is the
 * initial population (SciPy uses a Latin hypercube over the bounds lo / hi [d+2]); stops after maxiter generations or when
 * std(energies) <= atol + tol |mean(energies)|.  best_x[d+2], *best_energy, *generations are written on return; the
 * caller may polish best_x (SciPy does, with L-BFGS-B). */
int sbo_fit_de(sbo_ctx* ctx, int n, int d, const double* X_norm, const double* y, int P, const double* lo, const double* hi,
               const double* init_pop, uint64_t seed, int maxiter, double tol, double atol, double* best_x, double* best_energy,
               int* generations);

/* NLL and its analytic gradient for P hyper-parameter vectors (the jac = grad(NLL) of models/GP_Classic.py:219-226):
 * nll_out[p] is bit for bit sbo_nll_batch's out[p]; grad_out[p, d+2] = dNLL/dh with Q = K^-1 - alpha alpha^T, Kf = K's noise-free
 * part: sum_ik Q_ik Kf_ik (x_ia - x_ka)^2 / W_a (a < d), 2 sum_ik Q_ik Kf_ik, 2 sn2 tr Q.  A member whose factor fails gets
 * +inf and a NaN gradient.  Needs 8 (n d + 4 n) bytes of LDS <= 150 KiB (SBO_E_UNSUPPORTED above). */
int sbo_nll_grad_batch(sbo_ctx* ctx, int n, int d, const double* X_norm, const double* y, int P, const double* hyper,
                       double* nll_out, double* grad_out);

/* per-start outcome of sbo_fit_local */
enum sbo_fit_status {
  SBO_FIT_FTOL = 0,        /* |f_k - f_k+1| < ftol after an accepted step                  */
  SBO_FIT_GTOL = 1,        /* ||projected gradient||_inf <= gtol                           */
  SBO_FIT_MAXITER = 2,     /* maxiter accepted steps                                       */
  SBO_FIT_LINESEARCH = 3,  /* no Armijo point along steepest descent                       */
  SBO_FIT_NOT_PD = 4       /* the clipped start has no factor (or no finite gradient)      */
};

/* GP_Classic's multistart fit (models/GP_Classic.py:194-240) in one launch: for every output o < q (column o of Y_norm[n, q]) and
 * every start s < P (starts[P, d+2], shared by all outputs), a projected BFGS on the box [lo, hi]^(d+2) with Armijo backtracking
 * along the projection arc, one workgroup per (o, s).  best_x[q, d+2] / best_nll[q]: the lowest NLL per
 * output, ties to the lowest start.  Optional (NULL allowed): x_out[q, P, d+2], nll_out[q, P], iters_out / evals_out [q, P],
 * pgnorm_out[q, P] (projected-gradient inf-norm at the result, NaN for SBO_FIT_NOT_PD), status_out[q, P] (sbo_fit_status). */
int sbo_fit_local(sbo_ctx* ctx, int n, int d, int q, const double* X_norm, const double* Y_norm, int P, const double* starts,
                  const double* lo, const double* hi, int maxiter, double ftol, double gtol, double* best_x, double* best_nll,
                  double* x_out, double* nll_out, int* iters_out, int* evals_out, double* pgnorm_out, int* status_out);

/* sbo_fit_de for q outputs side by side: column o of Y_norm[n, q] is searched with seeds[o] from the shared init_pop[P, d+2], one
 * launch per generation for all outputs (one workgroup per member and output) and one read-back of the q P energies per convergence
 * check (every 8th generation and the last).  Output o comes out bit for bit as sbo_fit_de gives it for that column and seed:
 * best_x[q, d+2], best_energy[q], generations[q] (may be NULL).  An output that has converged is frozen while the others go on. */
int sbo_fit_de_batch(sbo_ctx* ctx, int n, int d, int q, const double* X_norm, const double* Y_norm, int P, const double* lo,
                     const double* hi, const double* init_pop, const uint64_t* seeds, int maxiter, double tol, double atol,
                     double* best_x, double* best_energy, int* generations);

/* ---- fit and build in one call ------------------------------------------ */
typedef struct sbo_fit_opts {
  int32_t  P, maxiter;                 /* DE population (>= 4) and generation limit                          */
  double   tol, atol;                  /* DE stop: std(E) <= atol + tol |mean(E)|                            */
  uint64_t seed;                       /* output o searches with seed + o                                    */
  int32_t  polish, polish_maxiter;     /* 1: projected BFGS from every output's DE best; <= 0: 10000 steps   */
  double   polish_ftol, polish_gtol;   /* <= 0: float32 eps, 1e-8                                            */
  double   lo[SBO_MAX_D + 2], hi[SBO_MAX_D + 2];   /* the box of the search and of the polish, [d+2] used    */
} sbo_fit_opts;

typedef struct sbo_fit_report {
  double  de_nll[SBO_MAX_Q], nll[SBO_MAX_Q];        /* best NLL after the DE / after the polish (what the model uses) */
  int32_t generations[SBO_MAX_Q], polish_status[SBO_MAX_Q] /* sbo_fit_status, -1 without a polish */, polish_evals[SBO_MAX_Q],
          polished[SBO_MAX_Q];                      /* 1: the polished point was strictly lower and replaced the DE's  */
  double  de_ms, polish_ms, build_ms, total_ms;     /* host clock around each phase                                   */
  int32_t host_syncs, reserved;                     /* read-backs the fit waited for: one per convergence check + 1    */
} sbo_fit_report;

/* From normalised data to a resident, sweepable model (models/GP_Safe.py:194-245 without the host in the middle): the DE of
 * sbo_fit_de_batch for all q outputs (output o with opts->seed + o, from init_pop[P, d+2]), with opts->polish one sbo_fit_local-style
 * projected BFGS per output from its DE best on the same box -- kept only where its NLL is strictly lower --, then the model build of
 * sbo_model_set_prior(..., hypopt_out, invK_list = NULL, mean_prior) (SBO_FACTOR_CHOL).  hypopt_out[d+2, q] is written in the layout
 * sbo_model_set takes; report may be NULL.  No [n, n] matrix crosses the bus in either direction.  The fit runs in fp64 whatever
 * dtype says; dtype tags the built model.  Status codes as sbo_fit_de / sbo_fit_local / sbo_model_set give them; an output whose
 * whole final population has no finite NLL is SBO_E_INVALID.  A failure before the build leaves the resident model untouched; a
 * failure of the build behaves as sbo_model_set's.  Deterministic; no collectives (every rank fits its replicated data). */
int sbo_model_fit(sbo_ctx* ctx, int dtype, const char* kernel, int n, int d, int q, const double* X_mean, const double* X_std,
                  const double* Y_mean, const double* Y_std, const double* X_norm, const double* Y_norm, const double* mean_prior,
                  const sbo_fit_opts* opts, const double* init_pop, double* hypopt_out, sbo_fit_report* report);

/* ---- local refinement of an acquisition optimum off the grid ------------ */
/* per-seed outcome of sbo_refine */
enum sbo_refine_status {
  SBO_REFINE_CONVERGED = 0,        /* the barrier path reached its floor with a small projected gradient; the point was accepted  */
  SBO_REFINE_MAX_EVAL = 1,         /* max_eval evaluations ran out; the best accepted point is returned                           */
  SBO_REFINE_NO_PROGRESS = 2,      /* no iterate passed the exact check (or the solver could not start): the seed is returned     */
  SBO_REFINE_INFEASIBLE_SEED = 3,  /* the seed fails the S predicate (box, ball, lcb_c >= 0, finite): returned unchanged, never best */
  SBO_REFINE_ON_BOUNDARY = 4       /* the seed is feasible with some lcb_c == 0 or on the ball's sphere: returned unchanged        */
};

typedef struct sbo_refine_opts {
  double   b;                      /* confidence multiplier, as sbo_sweep_opts.b                                                 */
  int32_t  objective;              /* output index o in [0, q)                                                                   */
  int32_t  kind;                   /* SBO_MEAN / SBO_UCB / SBO_LCB / SBO_VAR of output o                                         */
  int32_t  maximize;               /* 0: minimise, 1: maximise                                                                   */
  uint32_t constraint_mask;        /* bit c (1 <= c < q): enforce lcb_c(x) >= 0; bit 0 must be clear                             */
  double   lo[SBO_MAX_D], hi[SBO_MAX_D];   /* box (finite, lo <= hi); seeds outside it are infeasible, not clipped            */
  int32_t  use_ball;               /* 1: also ||x - x_0||_2 <= r (no 1e-8 shift, as sbo_sweep_tr)                                */
  int32_t  max_eval;               /* posterior + gradient evaluations per seed; <= 0: 400; at most min(20000, max(400, 4e9 / n^2)) */
  double   x_0[SBO_MAX_D], r;      /* ball centre and radius (use_ball: finite, r > 0)                                           */
  double   tol;                    /* projected-gradient inf-norm of the barrier function, box-scaled; <= 0: 1e-9                */
} sbo_refine_opts;

typedef struct sbo_refine_result {
  int64_t best;                    /* seed whose returned point has the best objective (ties: lowest index), -1 if none usable   */
  double  best_x[SBO_MAX_D], best_value;
  int64_t evaluations;             /* posterior + gradient evaluations, summed over seeds                                        */
  int32_t converged;               /* seeds with SBO_REFINE_CONVERGED                                                            */
  int32_t reserved;
} sbo_refine_result;

/* Refine each seed[n_seeds][d] to a local optimum of `kind` of output `objective` over {x in the box, lcb_c(x) >= 0 for every c in
 * constraint_mask, ||x - x_0|| <= r when use_ball}: one workgroup per seed, a projected BFGS on a log-barrier function of the exact
 * fp64 posterior (the model's factor M with M^T M = invK).  Every returned point is re-evaluated by the exact list evaluator -- the
 * values sbo_bounds gives there -- and is feasible under the sweep's S predicate and no worse than its seed (the seed itself at
 * worst).  x_out[n_seeds][d], value_out[n_seeds] (the exact objective at the returned point) and status_out[n_seeds]
 * (sbo_refine_status) may be NULL.  Deterministic.  Does not touch the resident candidates, posterior, masks, guard band or audit;
 * no collectives (every rank refines on its replicated model).  fp64 models only (SBO_F32: SBO_E_UNSUPPORTED). */
int sbo_refine(sbo_ctx* ctx, const sbo_refine_opts* opts, int64_t n_seeds, const double* seeds, double* x_out, double* value_out,
               int32_t* status_out, sbo_refine_result* result);

/* ---- the set-valued steps refined off the grid ----------------------------- */
/* objective kind of sbo_refine_sets beside SBO_MEAN .. SBO_VAR: the squared distance ||x - target||^2, minimised (the value
 * reported is the Euclidean distance) */
#define SBO_REFINE_DIST 4

typedef struct sbo_refine_sets_opts {
  double   b;                      /* confidence multiplier, as sbo_sweep_opts.b                                                 */
  int32_t  pair;                   /* 0: the variable is one point x; 1: a pair (x, x'), which needs 2 d <= SBO_MAX_D            */
  int32_t  objective;              /* output index o in [0, q) (unused by SBO_REFINE_DIST)                                       */
  int32_t  kind;                   /* SBO_MEAN / SBO_UCB / SBO_LCB / SBO_VAR of output o, or SBO_REFINE_DIST                     */
  int32_t  objective_point;        /* 0: the bound is taken at x; 1: at x' (pair mode)                                           */
  int32_t  maximize;               /* 0: minimise, 1: maximise (SBO_REFINE_DIST: 0)                                              */
  uint32_t safe_mask;              /* bit c (1 <= c < q): lcb_c(x) >= 0                                                          */
  uint32_t unsafe_mask;            /* bit c (1 <= c < q): lcb_c(x') <= 0 -- x' in the sweeps' U when every constraint is set; pair mode */
  int32_t  use_level;              /* 1: also lcb_{level_output}(x) <= level (M_t: output 0, level u*)                           */
  int32_t  level_output;
  int32_t  use_link;               /* 1: also ucb_{link_output}(x) - L ||x - x' + 1e-8||_2 >= 0 (1e-8 added per component); pair mode */
  int32_t  link_output;            /* a constraint output in [1, q)                                                              */
  int32_t  use_ball;               /* 1: also ||x - x_0||_2 <= r, as sbo_refine_opts                                             */
  int32_t  max_eval;               /* as sbo_refine_opts; a pair costs two evaluations, and the count is in evaluations of one point */
  int32_t  reserved;
  double   level, L;               /* finite; L >= 0 is the caller's Lipschitz constant (the one the sweep used: sbo_*_result.L)  */
  double   lo[SBO_MAX_D], hi[SBO_MAX_D];   /* box of x and of x'                                                              */
  double   x_0[SBO_MAX_D], r;
  double   target[SBO_MAX_D];      /* SBO_REFINE_DIST: the point t                                                               */
  double   tol;                    /* as sbo_refine_opts                                                                         */
} sbo_refine_sets_opts;

typedef struct sbo_refine_sets_result {
  int64_t best;                    /* as sbo_refine_result                                                                       */
  double  best_x[SBO_MAX_D], best_xp[SBO_MAX_D], best_value;   /* best_xp: x' of the best pair (zeros in single mode)            */
  int64_t evaluations;             /* posterior + gradient evaluations of one point, summed over seeds                           */
  int32_t converged;
  int32_t reserved;
} sbo_refine_sets_result;

/* sbo_refine's solver on the problems of the set-valued steps (models/SafeOpt.py:53-124, models/GoOSE.py:80-119): each seed
 * seeds[n_seeds][d] -- in pair mode with its partner seeds_p[n_seeds][d] -- moves to a local optimum of the objective over
 * {x (and x') in the box; lcb_c(x) >= 0, c in safe_mask; lcb_c(x') <= 0, c in unsafe_mask; lcb_o(x) <= level; the link; the ball}.
 * The exact check is sbo_refine's: seeds and iterates are evaluated by the list evaluator (both points of a pair) and every term is
 * judged there with the sweeps' closed predicates; a returned x (pair) satisfies every term and its exact objective is no worse
 * than its seed's, the seed itself at worst.  A seed that fails a term is SBO_REFINE_INFEASIBLE_SEED, a feasible seed with a term of
 * exactly zero slack SBO_REFINE_ON_BOUNDARY; both come back unchanged.  x_out[n_seeds][d], xp_out[n_seeds][d] (pair mode),
 * value_out[n_seeds] and status_out[n_seeds] may be NULL; seeds_p is read in pair mode only.  Pair mode with 2 d > SBO_MAX_D:
 * SBO_E_UNSUPPORTED.  Otherwise as sbo_refine: deterministic, fp64 models only, no collectives, nothing resident is touched. */
int sbo_refine_sets(sbo_ctx* ctx, const sbo_refine_sets_opts* opts, int64_t n_seeds, const double* seeds, const double* seeds_p,
                    double* x_out, double* xp_out, double* value_out, int32_t* status_out, sbo_refine_sets_result* result);

/* ---- StableOpt's robust min-max refined off the grid ----------------------- */
#define SBO_ROBUST_MAX_SCEN 8      /* scenarios (disturbance points) the outer approximation holds at a time */

typedef struct sbo_refine_robust_opts {
  double  b;                       /* confidence multiplier, as sbo_sweep_opts.b                                                 */
  int32_t kind;                    /* SBO_MEAN / SBO_UCB / SBO_LCB of output 0; the constraints always use their LCB             */
  int32_t n_control_axes;          /* axes 0 .. nxc - 1 of a point are the controls xc, the rest the disturbance d (sbo_sweep_robust);
                                      in [1, d - 1], and nxc + 1 <= SBO_MAX_D (the solver's variables are (xc, t))               */
  int32_t max_rounds;              /* separation rounds; <= 0: 6                                                                 */
  int32_t max_scenarios;           /* <= 0: SBO_ROBUST_MAX_SCEN, which is also the most                                          */
  int32_t max_eval;                /* posterior + gradient evaluations of one point over the whole call; <= 0: the ceiling
                                      min(20000, max(400, 4e9 / n^2)) of sbo_refine_opts.max_eval, which also caps a given value */
  int32_t reserved;
  double  lo[SBO_MAX_D], hi[SBO_MAX_D];   /* joint box: controls, then disturbances (finite, lo <= hi)                          */
  int64_t count_d[SBO_MAX_D];      /* check grid of the disturbance box: points per disturbance axis (>= 1), [d - nxc] used; the
                                      points are sbo_candidates_grid's (lo + i step, the last one hi), axis 0 of d the fastest   */
  double  tol;                     /* as sbo_refine_opts (<= 0: 1e-9); also the separation tolerance in units of Y_std           */
} sbo_refine_robust_opts;

typedef struct sbo_refine_robust_result {
  int32_t status;                  /* sbo_refine_status                                                                          */
  int32_t rounds, scenarios;       /* separation rounds run; scenarios held at the end (the rows of scenarios_out that are set)  */
  int32_t reserved;
  int64_t evaluations;             /* posterior + gradient evaluations of one point: outer steps and polishes                    */
  double  xc[SBO_MAX_D];           /* the returned control (the seed unless the refined one passed the exact check)              */
  double  value, seed_value;       /* max over C of bound_0(xc, .) / the same at the seed                                        */
  double  worst_d[SBO_MAX_D];      /* the arg-max of value: first occurrence, grid order, then scenarios                         */
  double  g_min[SBO_MAX_Q];        /* [c]: min over C of lcb_c(xc, .), c = 1 .. q - 1; entry 0 and entries >= q are 0            */
  double  gap;                     /* the last separation's largest violation of the outer solution, in Y_std units (>= 0)       */
} sbo_refine_robust_result;

/* min over xc of max over d of bound_0(xc, d) subject to min over d of lcb_c(xc, d) >= 0 for every constraint c, xc and d in the box,
 * from one seed xc_seed[nxc] (the winner of sbo_sweep_robust), by outer approximation over a scenario set D of at most max_scenarios
 * disturbance points.  A round separates at the current xc -- the exact values on {xc} x (check grid), their arg-max of bound_0 and
 * arg-min of every lcb_c (ties: lowest index) each polished over d by sbo_refine's solver with xc held, kept when no better for the
 * caller than its grid seed, and entered into D when it violates the outer solution by more than tol Y_std (first round: always;
 * D full: the scenario of largest slack is replaced) -- and then minimises t over (xc, t) subject to bound_0(xc, d_k) <= t and
 * lcb_c(xc, d_k) >= 0 for every d_k in D by the projected BFGS on a log barrier (one workgroup).  It ends when a separation adds
 * nothing (SBO_REFINE_CONVERGED), at max_rounds / max_eval (SBO_REFINE_MAX_EVAL), or when the outer step cannot move.
 * Exact check: with C = the check grid followed by the scenarios held at the end, the seed and the final xc are evaluated on
 * {xc} x C by the list evaluator (the values sbo_bounds gives there).  The final xc is returned only when it lies in the box,
 * every g_min[c] >= 0 and value <= seed_value; otherwise the seed with SBO_REFINE_NO_PROGRESS.  A seed with some min over C of
 * lcb_c < 0 is SBO_REFINE_INFEASIBLE_SEED (the grid winner is not robust-safe off the grid), one with a minimum of exactly 0
 * SBO_REFINE_ON_BOUNDARY; both come back unchanged with their g_min.  scenarios_out[SBO_ROBUST_MAX_SCEN][d - nxc] may be NULL.
 * q = 1 (no constraints) is served.  Deterministic; fp64 models only (SBO_F32: SBO_E_UNSUPPORTED); nxc + 1 > SBO_MAX_D:
 * SBO_E_UNSUPPORTED; nothing resident is touched, no collectives; at most one host wait per round and one at the end. */
int sbo_refine_robust(sbo_ctx* ctx, const sbo_refine_robust_opts* opts, const double* xc_seed, double* scenarios_out,
                      sbo_refine_robust_result* result);

/* ---- the mean's gradient at a list, and its bound maximised over the box ---- */
/* d MEAN_o / d x_a = Y_std_o sum_j alpha_oj k_j (X_ja - xn_a) / ell_a / X_std_a (DESIGN.md section 12's formula, on the resident fp64
 * alpha and X_norm) at points[n_points][d]: grad_out[n_points][q][d], infnorm_out[n_points][q] = max_a |.|; either may be NULL, not
 * both.  The value at a point does not depend on n_points or on the point's place in the list, bit for bit: every sum runs over the
 * observations in their order, whatever the launch shape, and two calls return the same bits.  Waits first for a deferred
 * factorisation (one that fails: SBO_E_INVALID).  Reads the model only: candidates, posterior, masks, plans, guard band, audit
 * counters and options are untouched, and a sweep behind the call equals one before it bit for bit.  No collectives (the model is
 * replicated: any rank may call).  fp64 models only (SBO_F32: SBO_E_UNSUPPORTED); n_points < 1: SBO_E_INVALID. */
int sbo_mean_grad(sbo_ctx* ctx, int64_t n_points, const double* points, double* grad_out, double* infnorm_out);

typedef struct sbo_lipschitz_opts {
  uint32_t output_mask;            /* bit o (o < q): bound output o; 0: every output                                              */
  int32_t  top;                    /* seeds refined per (output, axis, sign); <= 0: 4; at most 16                                 */
  int32_t  max_eval;               /* evaluations (value + Hessian row) per problem; <= 0: 200; at most 2000                      */
  int32_t  reserved;
  double   tol;                    /* projected-gradient inf-norm in span units of the objective scaled by the output's L_seed;
                                      <= 0: 1e-9                                                                                  */
  double   lo[SBO_MAX_D], hi[SBO_MAX_D];   /* the box (finite, lo <= hi; an axis of span 0 is held)                               */
} sbo_lipschitz_opts;

typedef struct sbo_lipschitz_result {
  double  L[SBO_MAX_Q];            /* the bound found; 0 for outputs not asked for                                                */
  double  L_seed[SBO_MAX_Q];       /* max over the usable seeds, before any refinement                                            */
  double  x[SBO_MAX_Q][SBO_MAX_D]; /* where L[o] is attained                                                                      */
  int32_t axis[SBO_MAX_Q], sign[SBO_MAX_Q];   /* L[o] = sign * dMEAN_o/dx_axis at x[o]; sign is +1 or -1                          */
  int64_t seeds_used, evaluations; /* seeds inside the box; evaluations summed over the problems                                  */
  int32_t problems, converged;     /* solver problems run / ended at tol                                                          */
} sbo_lipschitz_result;

/* L[o] ~ max over the box of ||grad MEAN_o||_inf (models/SafeOpt.py:79-83, models/GoOSE.py:74-78: maximize_infnorm_mean_grad, there by
 * SciPy DE) as a multistart local search from seeds[n_seeds][d].  Seeds that are non-finite or outside the box are skipped, not
 * clipped (none left: SBO_E_INVALID).  Stage 1 evaluates every usable seed with sbo_mean_grad's kernel and keeps, for each asked
 * output o, axis a of span > 0 and sign s, the `top` seeds of largest s g_a (ties: the lowest seed index).  Stage 2 runs one solver
 * problem per kept seed, all in one launch and one workgroup each: maximise s g_a(x) over the box by a projected BFGS in the metric of
 * the spans on F = -s g_a / L_seed[o], with row a of the mean's Hessian as its gradient (max_x ||grad||_inf = max_{a,s} max_x s g_a(x),
 * and every inner problem is smooth); it stops at tol, at max_eval, when an accepted step changes F by no more than rounding, or when a
 * line search fails with H reset.  Exact check: the final iterate of
 * every problem is evaluated again by stage 1's kernel, and L[o] is the largest |g_a| over the usable seeds and those final points, all
 * axes (ties: the lowest axis, then sign +, then seeds before iterates, then the lowest index).  Hence L[o] >= L_seed[o] always, lo <=
 * x[o] <= hi, and L[o] is bit for bit the infnorm_out sbo_mean_grad gives at x[o].  L is a lower bound of the supremum, attained inside
 * the box -- as the reference's DE gives one; it is NOT a certificate: a basin no seed reaches is missed.  Deterministic; one host wait.
 * Otherwise as sbo_mean_grad: waits for a deferred factorisation, reads the model only, no collectives, fp64 models only.
 * SBO_E_INVALID: n_seeds < 1, top > 16, max_eval > 2000, a box that is not finite with lo <= hi, output_mask bits at or above q. */
int sbo_lipschitz(sbo_ctx* ctx, const sbo_lipschitz_opts* opts, int64_t n_seeds, const double* seeds /* [n_seeds][d] */,
                  sbo_lipschitz_result* result);

/* ---- a greedy batch of k points under hallucinated observations (GP-BUCB) ---- */
#define SBO_MAX_BATCH 64
typedef struct sbo_batch_opts {
  int32_t output;      /* whose variance is maximised, 0 .. q-1                                                                    */
  int32_t k;           /* picks wanted, 1 .. SBO_MAX_BATCH                                                                          */
  int32_t n_pending;   /* points conditioned on first and never picked; n_pending + k <= SBO_MAX_BATCH                              */
  int32_t reserved;
  double  min_std;     /* stop before a pick whose conditional std (un-normalised) is < min_std; >= 0, finite                       */
} sbo_batch_opts;

typedef struct sbo_batch_result {
  int32_t n_selected, reserved;
  int64_t index[SBO_MAX_BATCH];   /* into pool, in pick order; -1 past n_selected                                                  */
  double  std[SBO_MAX_BATCH];     /* sqrt of the conditional variance the pick had when picked, times Y_std[output]                */
} sbo_batch_result;

/* Pick j of the batch is the arg-max over pool[m][d] (raw coordinates, as for sbo_mean_grad and sbo_candidates_points) of the
 * posterior variance of `output` conditioned on the data, on pending[n_pending][d] (raw coordinates; in their order, first) and on
 * picks 0 .. j-1 -- possible before any of them is measured, because a GP's posterior variance does not depend on the observed values.
 * fp64 on the resident fp64 factor whatever the model dtype, as sbo_model_loo.  With the resident lower factor M (M^T M =
 * inv(K + sn2 I)): v_0(x) = sf2 - ||M k_x||^2, k_x with the expanded distance of the reference (GP_Safe.py:119); v is not clipped
 * inside the recursion.  Conditioning on a point z is the step sbo_model_append would take for it: with c(x) the current posterior
 * covariance of x and z and s = v(z) + sn2 (kappa = sf2 + sn2 on the diagonal of the new row), v(x) <- v(x) - c(x)^2 / s.  Ties go
 * to the lowest index; a pool point may be picked again (with noise its variance stays positive).  std[j] = sqrt(max(0, v)) Y_std[output];
 * var_out[m] (may be NULL) is the pool's variance after the last conditioning -- every pick made is conditioned on --: max(0, v) Y_std^2.
 * The value computed for a pool point does not depend on m or on the point's place in the list, bit for bit: every sum over the
 * observations and the earlier picks runs in index order, two identical pool rows hold identical bits (the lower index wins), and two
 * calls return the same bits.  Waits first for a deferred factorisation (one that fails: SBO_E_INVALID).  Reads the model only -- the
 * growing factor is a scratch copy --: candidates, posterior, masks, plans, guard band, audit counters and options are untouched, and a
 * sweep behind the call equals one before it bit for bit.  One host wait.  No collectives (the model is replicated: any rank may call).
 * SBO_E_INVALID: a NULL ctx, opts, pool or result; m < 1 (or > 2^28); output outside [0, q); k < 1; n_pending < 0, or > 0 with a NULL
 * pending; k + n_pending > SBO_MAX_BATCH; a non-finite coordinate; min_std negative or non-finite; a conditioning step with s <= 0.
 * SBO_E_NO_MODEL without a model.  On any error the result is zeroed, its indices -1. */
int sbo_batch_select(sbo_ctx* ctx, const sbo_batch_opts* opts, int64_t m, const double* pool /* [m][d] */,
                     const double* pending /* [n_pending][d] or NULL */, double* var_out /* [m] or NULL */, sbo_batch_result* result);

/* ---- expanders by hallucinated optimistic observations (the SafeOpt paper's G_t) ---- */
#define SBO_EXPANDER_MAX_POINTS  65536            /* sources, and targets, of one call; longer target lists: several calls (counts add)      */
#define SBO_EXPANDER_MAX_SCRATCH 4294967296ULL    /* bytes of the whitened vectors of one call: (ms + mt) * ldt * #constraints * 8, ldt = n
                                                     rounded up to a multiple of 32                                                          */
typedef struct sbo_expander_opts {
  double   b;                 /* finite, >= 0                                                                                              */
  uint32_t constraint_mask;   /* bit c (1 <= c < q): constraint c takes part; 0: every constraint 1 .. q-1; bit 0 or bits >= q: SBO_E_INVALID */
  int32_t  reserved;
} sbo_expander_opts;

/* Source g of sources[ms][d] (raw coordinates, as for sbo_batch_select) is an expander when, were it measured at its optimistic value
 * ucb_c(g) on every masked constraint c, the GP would certify some target of targets[mt][d]: count_out[g] > 0.  No Lipschitz constant
 * enters (the rule the sweeps evaluate, SURVEY.md Appendix A, is the reference's and is untouched).  Normalised units, per masked c,
 * with the resident lower factor M_c (M_c^T M_c = inv(K_c + sn2_c I)), t_p = M_c k_c(X, p) with the expanded distance of the reference
 * (GP_Safe.py:115-119), mu_c(p) = mp_c + k_c(X, p) . alpha_c, taken as mp_c + t_p . (M_c (y_c - mp_c)) -- the call rests on the factor
 * and the data, so an append and the removal of that row give back its bits --, and v_c(p) = sf2_c - ||t_p||^2 (not clipped):
 *   s = v_c(g) + sn2_c              (kappa = sf2 + sn2 on the diagonal of the new row, as sbo_model_append)
 *   cov = k_c(x, g) - t_x . t_g
 *   mu' = mu_c(x) + cov b sqrt(max(0, v_c(g))) / s      (the observation at g is ucb_c(g): its residual is b sqrt(v))
 *   v'  = v_c(x) - cov^2 / s
 *   z_c(x | g) = mu' - b sqrt(max(0, v')) + Y_mean[c] / Y_std[c]     (>= 0 <=> the raw lcb of c at x, with g added, is >= 0)
 *   Z(x | g) = min over the masked c of z_c(x | g)
 * count_out[g] = #{x : Z(x | g) >= 0}; margin_out[g] (may be NULL) = max_x Z(x | g) and witness_out[g] (may be NULL) its target index,
 * ties to the lowest index, a NaN never taken (none left: margin NaN, witness -1).  fp64 on the resident fp64 factor whatever the
 * model dtype, as sbo_batch_select.  Stage 1 forms t, mu and v of every point (O((ms + mt) n^2)); stage 2 takes t_x . t_g of all pairs
 * on the matrix cores in 64 x 64 tiles (O(ms mt n) per constraint) with the formulas above as its epilogue; no [ms][mt] array exists.
 * The value of a pair does not depend on ms, mt or the points' places in their lists; per-source partials are combined in workgroup
 * order, there are no atomics, and two calls return the same bits.  Waits first for a deferred factorisation (one that fails:
 * SBO_E_INVALID).  Reads the model only: candidates, posterior, masks, plans, guard band, audit counters and options are untouched, and
 * a sweep behind the call equals one before it bit for bit.  One host wait.  No collectives (the model is replicated: any rank may call).
 * SBO_E_INVALID: a NULL ctx, opts, sources, targets or count_out; ms < 1 or mt < 1; b negative or non-finite; q < 2; a bad mask; a
 * non-finite coordinate; s <= 0 on some source and masked constraint.  SBO_E_NO_MODEL without a model.  SBO_E_UNSUPPORTED: ms or mt above
 * SBO_EXPANDER_MAX_POINTS, or whitened vectors above SBO_EXPANDER_MAX_SCRATCH.  On any error the outputs are cleared: counts 0, margins
 * NaN, witnesses -1. */
int sbo_expander_gain(sbo_ctx* ctx, const sbo_expander_opts* opts, int64_t ms, const double* sources /* [ms][d] */, int64_t mt,
                      const double* targets /* [mt][d] */, int64_t* count_out /* [ms] */, double* margin_out /* [ms] or NULL */,
                      int64_t* witness_out /* [ms] or NULL */);

/* ---- posterior sample paths for Thompson sampling (pathwise conditioning) ---- */
#define SBO_MAX_PATHS        64
#define SBO_MAX_FEATURES     8192
#define SBO_PATHS_MAX_POINTS 16777216          /* 2^24 points of one call; longer pools: several calls with the same draws               */
#define SBO_PATHS_MAX_VALUES 4294967296ULL     /* bytes of values_out: m * n_paths * 8                                                    */
typedef struct sbo_paths_opts {
  int32_t output;      /* 0 .. q-1                                                       */
  int32_t n_paths;     /* S, 1 .. SBO_MAX_PATHS                                          */
  int32_t n_features;  /* F, 1 .. SBO_MAX_FEATURES                                       */
  int32_t maximize;    /* 0: per path the arg-min over the points, 1: the arg-max        */
} sbo_paths_opts;
typedef struct sbo_paths_result {
  int64_t index[SBO_MAX_PATHS];   /* into points; -1 past n_paths, and when every value of the path is NaN */
  double  value[SBO_MAX_PATHS];   /* the path's value there, un-normalised; NaN where index is -1         */
} sbo_paths_result;

/* S joint draws from the posterior of one output, as functions, evaluated at points[m][d] (raw coordinates, as for sbo_batch_select),
 * at O(F + n) per point and path (Matheron's rule: a random-feature draw from the prior plus a data-dependent update; Wilson et al.,
 * "Efficiently sampling functions from Gaussian process posteriors", 2020).  The library draws nothing: omega [F][d], weights [S][F]
 * and noise [S][n] are the caller's standard normal numbers, phase [F] is uniform on [0, 2 pi); the library applies the
 * hyper-parameters, so the call is deterministic and the same draws in two calls are the same functions (a long pool can be chunked).
 * Normalised units, output o, ell_a = exp(2 h_a), u(p)_a = xn(p)_a / sqrt(ell_a), k the reference's expanded distance
 * (GP_Safe.py:115-119), sn2 as sbo_batch_select's s = v + sn2, M the resident lower factor (M^T M = inv(K + sn2 I)):
 *   phi_f(p)   = sqrt(2 sf2 / F) cos(omega_f . u(p) + phase_f)
 *   prior_s(p) = sum_f weights[s][f] phi_f(p)
 *   r_s[j]     = (Y_norm[j][o] - mp) - prior_s(X_j) - sqrt(sn2) noise[s][j]
 *   c_s        = M^T (M r_s)
 *   f_s(p)     = mp + prior_s(p) + sum_j k(X_j, p) c_s[j]
 *   value      = Y_mean[o] + Y_std[o] f_s(p)
 * With weights = 0 and noise = 0, f_s is the posterior mean.  c_s rests on the factor and the data, not on the resident alpha: an
 * append and the removal of that row give back the call's bits.  values_out [m][S] (may be NULL) receives every value; result->index[s]
 * / value[s] the arg-min (maximize = 1: the arg-max) of path s over the points and the value there, ties to the lowest index, a NaN
 * never taken.  One set of F features fixes the prior's kernel to within O(1 / sqrt(F)): the paths' variance differs from the
 * posterior's by that much.  fp64 on the resident fp64 factor whatever the model dtype.  The value of (point, path) does not depend on
 * m, on the point's place in the list or on the other paths: every sum over features and observations runs in an order fixed by (F, n)
 * alone, two identical rows hold identical bits, per-path partials are combined in workgroup order, there are no atomics, and two calls
 * return the same bits.  Waits first for a deferred factorisation (one that fails: SBO_E_INVALID).  Reads the model only: candidates,
 * posterior, masks, plans, guard band, audit counters and options are untouched, and a sweep behind the call equals one before it bit
 * for bit.  One host wait.  No collectives (the model is replicated: any rank may call).
 * SBO_E_INVALID: a NULL ctx, opts, omega, phase, weights, noise, points or result; m < 1 or m > SBO_PATHS_MAX_POINTS; n_paths or
 * n_features out of range; output outside [0, q); maximize not 0 or 1; a non-finite entry of the five input arrays.  SBO_E_NO_MODEL
 * without a model.  SBO_E_UNSUPPORTED: values_out given and m * S * 8 > SBO_PATHS_MAX_VALUES.  On any error the result is cleared
 * (indices -1, values NaN) and values_out is not written. */
int sbo_sample_paths(sbo_ctx* ctx, const sbo_paths_opts* opts, const double* omega /* [F][d] */, const double* phase /* [F] */,
                     const double* weights /* [S][F] */, const double* noise /* [S][n] */, int64_t m,
                     const double* points /* [m][d], raw coordinates */, double* values_out /* [m][S] or NULL */,
                     sbo_paths_result* result);

/* ---- sample-path optima refined off the grid ---- */
#define SBO_REFINE_PATHS_MAX_STARTS 64
typedef struct sbo_refine_paths_opts {
  double   b;                 /* confidence multiplier of the constraints, as sbo_refine_opts.b                               */
  int32_t  output;            /* the paths' output, 0 .. q-1                                                                  */
  int32_t  n_paths;           /* S, 1 .. SBO_MAX_PATHS                                                                        */
  int32_t  n_features;        /* F, 1 .. SBO_MAX_FEATURES                                                                     */
  int32_t  n_starts;          /* K seeds per path, 1 .. SBO_REFINE_PATHS_MAX_STARTS                                           */
  int32_t  maximize;          /* 0: minimise every path, 1: maximise                                                          */
  uint32_t constraint_mask;   /* bit c (1 <= c < q): lcb_c(x) >= 0; bit 0 must be clear; 0: the box only                      */
  int32_t  max_eval;          /* path + constraint evaluations per problem; as sbo_refine_opts.max_eval (default and ceiling)  */
  int32_t  reserved;
  double   lo[SBO_MAX_D], hi[SBO_MAX_D];   /* box (finite, lo <= hi); seeds outside it are infeasible, not clipped           */
  double   tol;               /* as sbo_refine_opts.tol                                                                       */
} sbo_refine_paths_opts;
typedef struct sbo_refine_paths_result {
  int64_t best[SBO_MAX_PATHS];            /* per path the start whose returned point is best (ties: lowest), -1: none usable / past S */
  double  best_x[SBO_MAX_PATHS][SBO_MAX_D], best_value[SBO_MAX_PATHS];   /* zeros / NaN where best is -1 */
  int64_t evaluations;                    /* summed over all S * K problems */
  int32_t converged, reserved;            /* problems with SBO_REFINE_CONVERGED */
} sbo_refine_paths_result;

/* Problem (s, k) moves seeds[s][k] to a local optimum of path f_s over {x in the box, lcb_c(x) >= 0 for every c in constraint_mask}.
 * f_s is the function sbo_sample_paths defines for the same draws (omega, phase, weights, noise: see there; the library applies the
 * feature scale, the hyper-parameters and c_s = M^T (M r_s)), and both calls share one preparation.  One workgroup per problem runs
 * sbo_refine's solver -- the projected BFGS and its barrier stages -- on the path's value and analytic gradient (O(F + n) per
 * evaluation; with an empty mask nothing else is evaluated) and the constraints' exact fp64 posterior.  Then, as in sbo_refine, the
 * seed and the problem's final and best-objective iterates are judged under exact values: the constraints by the exact list evaluator
 * with the sweeps' closed predicates, the path by sbo_sample_paths' own evaluator.  So every returned point is feasible under the
 * values sbo_bounds gives there, value_out[s][k] is bit for bit the entry values_out[.][s] sbo_sample_paths returns for the same draws
 * at x_out[s][k], and it is no worse than the same figure at the seed (the seed itself at worst).  A seed outside the box or with a
 * non-finite coordinate is SBO_REFINE_INFEASIBLE_SEED, returned unchanged (value NaN where non-finite).  status_out: sbo_refine_status.
 * x_out [S][K][d], value_out [S][K], status_out [S][K] may be NULL.  Deterministic, no atomics: the result of problem (s, k) depends on
 * S, the draws and its own seed, not on K or the other seeds.  Reads the model only, one host wait, no collectives.
 * SBO_E_INVALID: a NULL ctx, opts, omega, phase, weights, noise, seeds or result; n_paths, n_features, n_starts or output out of range;
 * maximize not 0 or 1; bit 0 of the mask set or a bit at or above q; a non-finite draw; a bad box, b or tol.  SBO_E_NO_MODEL without a
 * model; SBO_E_UNSUPPORTED on an fp32 model.  On any error the result is cleared (best -1, values NaN, points and counts zero) and no
 * output array is written. */
int sbo_refine_paths(sbo_ctx* ctx, const sbo_refine_paths_opts* opts, const double* omega /* [F][d] */, const double* phase /* [F] */,
                     const double* weights /* [S][F] */, const double* noise /* [S][n] */, const double* seeds /* [S][K][d] */,
                     double* x_out /* [S][K][d] or NULL */, double* value_out /* [S][K] or NULL */, int32_t* status_out /* [S][K] or NULL */,
                     sbo_refine_paths_result* result);

/* ---- the posterior of a point list as a multivariate normal ---- */
#define SBO_JOINT_MAX_POINTS 2048          /* m of one call: the m x m images are 32 MiB each */
typedef struct sbo_joint_opts {
  int32_t output;     /* 0 .. q-1 */
  int32_t n_draws;    /* S, 0 .. SBO_MAX_PATHS */
  int32_t noise;      /* 0: covariance of the latent f; 1: of a new observation y (adds sn2 on the diagonal) */
  int32_t maximize;   /* 0: per draw the arg-min over the points, 1: the arg-max */
  double  jitter;     /* >= 0, finite; in units of sf2; added to the diagonal of the matrix that is factored, and only there */
} sbo_joint_opts;
typedef struct sbo_joint_result {
  int64_t index[SBO_MAX_PATHS];  /* -1 past n_draws */
  double  value[SBO_MAX_PATHS];  /* un-normalised; NaN where index is -1 */
  double  pivot_min;             /* smallest pivot / its diagonal entry met by the factorisation (NaN when none ran) */
  int64_t pivot_row;             /* its row (-1 when none ran) */
} sbo_joint_result;

/* Mean vector, full covariance and S exact joint draws of one output at points[m][d] (raw coordinates, as for sbo_batch_select),
 * m <= SBO_JOINT_MAX_POINTS.  Normalised units, with the conventions of sbo_expander_gain above (t_p = M k(X, p), sn2 as there):
 *   mu(p)    = mp + t_p . (M (y - mp))
 *   C(p, p') = k(p, p') - t_p . t_p'       (k with the smaller of the two squared norms first in the expanded distance: symmetric bit for bit)
 *   A        = C + (noise sn2 + jitter sf2) I = L L^T,  L lower with a positive diagonal
 *   f_s      = mu + L z_s,   z [S][m] the caller's standard normal numbers (NULL exactly when S = 0): the library draws nothing
 * mean_out [m] = Y_mean + Y_std mu; cov_out [m][m] = Y_std^2 (C + noise sn2 I), symmetric bit for bit, the jitter not in it; chol_out
 * [m][m] = Y_std L in full, zeros above the diagonal -- the matrix that is factored is cov_out's image plus Y_std^2 jitter sf2 on its
 * diagonal, so no scaling stands behind the factorisation --; draws_out [m][S], draws_out[p][s] = Y_mean + Y_std f_s(p); every array may
 * be NULL.  result->index[s] / value[s]: the arg-min (maximize = 1: the arg-max) of draw s over the points and the value there, ties to
 * the lowest index, a NaN never taken.  The factorisation (blocked, right-looking, panels of 64 columns) runs only when S > 0 or
 * chol_out is given; a pivot that is not above 2^-40 times its diagonal entry of A fails the call (the message names the row): a
 * jitter of 1e-8 never trips that on a positive semi-definite C, a duplicated point with jitter 0 and noise 0 always does.
 * result->pivot_min / pivot_row: the smallest pivot relative to its diagonal entry, and its row (the lowest on a tie).
 * fp64 on the resident fp64 factor whatever the model dtype.  C(i, j) depends on the two points and the model alone, rows 0 .. r of L on
 * the first r + 1 points alone; every sum runs in an order fixed by the element's place and n, per-draw partials are combined in
 * workgroup order, there are no atomics, and two calls return the same bits.  Waits first for a deferred factorisation of the model
 * (one that fails: SBO_E_INVALID).  Reads the model only: candidates, posterior, masks, plans, guard band, audit counters and options
 * are untouched, and a sweep behind the call equals one before it bit for bit.  One host wait.  No collectives (the model is replicated:
 * any rank may call).
 * SBO_E_INVALID: a NULL ctx, opts, points or result; z NULL with S > 0 or given with S = 0; m < 1; output, n_draws, noise or maximize out
 * of range; jitter negative or non-finite; a non-finite coordinate or z entry; a failed pivot.  SBO_E_NO_MODEL without a model.
 * SBO_E_UNSUPPORTED: m > SBO_JOINT_MAX_POINTS.  On any error the result is cleared (indices -1, values and pivot_min NaN, pivot_row -1)
 * and no output array is written. */
int sbo_posterior_joint(sbo_ctx* ctx, const sbo_joint_opts* opts, int64_t m, const double* points /* [m][d], raw coordinates */,
                        const double* z /* [S][m] standard normals, NULL iff S == 0 */, double* mean_out /* [m] or NULL */,
                        double* cov_out /* [m][m] or NULL */, double* chol_out /* [m][m] or NULL */, double* draws_out /* [m][S] or NULL */,
                        sbo_joint_result* result);

/* ---- plant evaluation ------------------------------------------ */
/* The reference's William-Otto reactor (problems/WilliamOttoReactor_Problem.py:19-93), noise-free, for n input rows
 * u[n, 2] = (Fb, Tr): out[n, 3] = (get_objective, get_constraint1, get_constraint2), each the steady state of the six
 * mass balances reached from x0 = 0.1 (the reference calls scipy fsolve once per point and output). */
int sbo_plant_wo(sbo_ctx* ctx, int64_t n, const double* u, double* out);

/* ---- measurement --------------------------------------------------------------------------- */
int sbo_profile_get(sbo_ctx* ctx, sbo_profile* out);
/* Diagnostics / test knobs (every default is the measured-best path; DESIGN.md "Options" has the A/B record of each):
 *   "posterior_path"   0 auto | 1 generic single-phase kernel (K1) | 2 generic chunked kernel (K1c)
 *   "bilinear"         1: fp64 2-D grids run the posterior as two GEMMs on Chebyshev coefficients -- a model's first sweep with a caller's
 *                      invK from exactly evaluated nodes (K1i), later sweeps from the reduced-basis plan (K1b) when the bases qualify;
 *                      2: K1b's plan from the first sweep on; 0: K1g
 *   "cheb_tol_e17"     K1b / K1i: coefficients below this x 1e-17 of the largest are not run (default 400 = 4e-15)
 *   "tensor_cheb"      1: fp64 3-D / 4-D grids interpolate the exact posterior from a tensor grid of Chebyshev nodes (K1t); 0: K1g
 *   "tensor_guess_pct" K1t test hook: scales the first guess of the node counts (a short guess exercises the probe's retry)
 *   "fuse_classify"    one-constraint K1b sweeps take S / U from the posterior's mean epilogue: 1 | 0 | -1 auto (default)
 *   "chol_async"       1: a caller's invK is contracted as given by K1b and its reverse Cholesky factor built off the critical path
 *   "scan_blocks"      1: blocked last-axis scans of the distance transforms; 0: step by step (A/B checker)
 *   "scan_waves"       1: open candidates of the verdict kernels are listed and scanned by groups of 16 lanes (8 | 32 | 64: lanes); 0: own thread
 *   "goose_pairs"      1: GoOSE coverage by pruned pair evaluation on grids too (A/B checker of the power transform)
 *   "col_path"         1 (auto): one-constraint SafeOpt sweeps of one rank on 2-D grids of whole 64 x 128 posterior tiles -- at least four tiles
 *                      per CU and output -- run their set phase on column words written by the GEMM posterior's epilogue
 *                      (sets_colpath.inc.hpp); 2: on every grid of that shape; 0: the byte-mask pipeline (A/B checker)
 *   "grad_defer"       first sweep of a model on fp64 2-D grids (K1i): where the Lipschitz keys' gradient phases run.  0: inside the posterior
 *                      launches, behind the gate's kernels (r04); 1 (default): in a launch of their own on a side stream beside the posterior
 *                      launches -- behind the gate on large grids, on every tile without a gate on small ones; 2: always without, 3: always with
 *   "k1_sched"         1: lean-2 sweeps on that path launch the constraint's and the objective's GEMM posterior over lists of the tiles they
 *                      evaluate, built per sweep (tiles left out are written by the lists' kernels); 0: one workgroup per tile (A/B checker)
 *   "k1_skip_safe"     1: lean-2 sweeps on that path also leave unevaluated the constraint tiles the plan's enclosures prove safe at this
 *                      sweep's b (sbo_profile.k1_tiles_skipped_safe); 0: only the tiles proved unsafe (A/B checker)
 *   "k1_resident"      1: from a plan's second lean-2 sweep on that path on (k1_sched 1, enclosures recorded), the tiles whose stored mean /
 *                      var are the plan's are classified from memory without their GEMM phases, and the constraint's Lipschitz rows come
 *                      from the plan's record (sbo_profile.k1_tiles_resident_c / _o); 0: every sweep runs the GEMM phases (A/B checker)
 *   "k1_cells"         1: where k1_resident classifies the constraint's listed tiles from memory, one launch decides every tile and classifies
 *                      the others per 8 x 8 cell -- a cell its enclosure proves safe or unsafe takes its bits from the proof, only the rest
 *                      load their stored values (sbo_profile.k1_cells_evaluated); 0: the tile-list kernel and the per-tile launch (A/B checker)
 *   "col_overlap"      1: on that path the expander chain (distance transform, verdicts) runs on a second stream beside the objective's
 *                      posterior launch and the M part of the minimiser; 0: every kernel on the main stream
 *   "set_fuse"         1: 2-D grids of one rank share launches between independent set-phase kernels; 0: one launch per kernel
 *   "set_lanes"        1: constraints of a one-rank sweep alternate between two streams; 0: one after the other
 *   "exact_lazy"       1: one-constraint sweeps launch the exhaustive recheck only when in-band verdicts were listed; 2: always that late path (test); 0: eager
 *   "result_mirror"    1: the last kernel of a one-rank sweep writes the result block into pinned host memory; 0: a copy behind it
 *   "phase_events"     1: events between the set phases too (sbo_profile.classify_ms / expander_ms / argreduce_ms; ~6 us bubble each)
 *   "halo_spec"        1: ranks > 1 size their transform windows from the previous sweep's keys (device-checked); 0: wait for this sweep's
 *   "comm_events"      1: an event pair around every collective (sbo_profile.comm_ms)
 *   "comm_selftest"    1: a one-rank communicator still sends C1 / C2 / C3 through RCCL (results must not change)
 *   "fp64_recheck"     1: fp32 models re-evaluate in fp64 every candidate that the band of their posterior cannot decide -- measured per (model,
 *                      candidate set) by the fp64 twin at 256 probe candidates, never under 1e-4 normalised (sbo_profile.fp32_band_dm / _dv);
 *                      0: masks of the fp32 posterior.  Read by sbo_model_set, which builds the twin: a change takes effect at the next one.  A
 *                      twin is its model's alone (it follows that model's appends and removals); once another model is set it takes no part
 *   "guard_audit"      samples per audited sweep of the standing audit of the guard band (sbo_profile.guard_audit_*; default 1024); 0: off
 *   "guard_audit_scale_ppm" test hook: the audit compares against the band x value / 1e6 (default 1000000); setting it clears the counts
 *   "guard_audit_every" one sweep in this many carries an audit (default 16; the first sweep after setting it does).  An audit shares
 *                      the card with the sweep it follows (~35 us of config H's set phase at 1024 samples, n = 512): 1 audits every sweep
 *   "refine_lds"       1 (default): sbo_refine / sbo_refine_sets / sbo_refine_robust stage the used outputs' triangles of M in LDS when they fit 144 KiB; 0: it always streams
 *                      M's rows from L2 (the tier of larger models; results are bit-identical either way)
 *   "lipschitz_lds"    1 (default): sbo_lipschitz's solver stages X_norm and its output's alpha in LDS when they fit 144 KiB; 0: it always streams
 *                      them from L2 (results are bit-identical either way)
 *   "list_index"       explicit candidate lists: expander sets (SafeOpt, GoOSE's source filter) and GoOSE's coverage search on a spatial
 *                      index of the list (Morton order, boxes of the U members; verdicts identical to the exhaustive ones).  -1 (default):
 *                      only for lists above 2097152 candidates, where the exhaustive expander sets are refused; 1: at any size (A/B checker);
 *                      0: never (lists above the cap: SBO_E_UNSUPPORTED for expander sets).  One rank only
 *   "guard_band"       1: sweeps on an approximating posterior (K1b / K1i / K1t) count the decisions inside its band and re-evaluate exactly
 *                      when there are any; 0: masks of the approximating posterior as they come; 2: the re-evaluation on every sweep (test) */
int sbo_set_option(sbo_ctx* ctx, const char* key, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* SAFEBO_H */
