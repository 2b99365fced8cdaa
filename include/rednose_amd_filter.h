/*
 * rednose_amd_filter.h -- the C ABI of a generated rednose_amd filter library (lib{name}.so).
 *
 * Every symbol is prefixed with the filter name chosen at gen_code() time, exactly like the reference
 * (/root/reference/rednose/helpers/ekf_sym.py:149-171).  This header documents the ABI with the macro
 * RN_FN(name, sym) == name##_##sym; the concrete per-model prototype lists that gen_code writes next to
 * each library are committed for the shipped models as include/kinematic.h, include/kinematic6.h and
 * include/live.h, and tests/test_abi.py checks that each library exports every symbol they declare.
 *
 * Conventions
 *   - fp64 everywhere, dense row-major: x is D doubles, P is E x E, z is Z, R is Z x Z
 *     (/root/reference/rednose/templates/ekf_c.c:4-6,39-44).
 *   - in-place semantics of the reference are kept: x and P are updated in place, z is overwritten with the
 *     residual y = z - h(x) (ekf_c.c:118-120); Q, R, ea are read-only; no allocation crosses the boundary.
 *   - section 1 takes HOST pointers and one filter (the reference's existing ABI, run as a batch of one on
 *     the GPU); section 2 takes DEVICE pointers and n filters laid out as the natural batch of the same
 *     buffers: x (n, D), P (n, E, E), z (n, Z), R (Z, Z) shared or (n, Z, Z), contiguous, 16-byte aligned.
 *   - section 2 functions are asynchronous on `stream` (a hipStream_t passed as void*, NULL = default
 *     stream) and return 0 on success or a status (1 HIP error, 2 bad argument, 3 misaligned pointer); the
 *     reference returns void and asserts (/root/reference/rednose/helpers/ekf_sym.cc:13,25-27,204).
 *     {name}_last_error() / {name}_last_error_string() report the last failure of the calling thread,
 *     including failures inside the void section-1 functions.
 *   - there is no CPU implementation behind any of these symbols.
 *
 * Asymmetric covariances.  The reference never symmetrises P: its predict and update multiply with both halves, and its
 * innovation covariance S = H P H^T + R is solved as a general matrix (ekf_c.c:24,100-101,115) -- a P that is not exactly
 * symmetric (its own Joseph form leaves ~1e-12 of asymmetry after a few thousand steps) is a legal input.  What each entry
 * point does with one (tests/test_gpu_asymmetric.py feeds SPD + a skew part through every one of them):
 *   - step-granular entry points -- the section-1 functions, batch_predict, batch_update_k, batch_predict_update_k, their
 *     _masked twins, batch_maha_k -- follow the reference entry for entry: both halves of P, S factored as a general matrix
 *     (L D U, no pivoting).  Same input, same result as the oracle to 1e-10 of the row maximum, symmetric or not.
 *   - batch_run keeps P in registers for T steps with arithmetic that uses P = P^T (one transposition per predict, the gain
 *     taken from the rows).  It reads (P + P^T) / 2 of the caller's matrix, ONCE, when the state enters the registers; the
 *     result is the reference's on THAT matrix, to rounding.  Against the reference run on the asymmetric matrix itself the
 *     difference is first order in (P - P^T) / 2, like any perturbation of P0 of that size.  The final P and the covariance
 *     trace come back symmetric to rounding (lane-per-filter models: exactly).
 *     WHICH MODE IS THE REFERENCE'S: the step-granular one.  A caller that needs the reference's result for a T-step schedule on a
 *     covariance with a skew part walks the schedule with batch_predict_update_k -- BatchedEKF.run(..., exact=True) does exactly that
 *     (trace, flags and residuals included; tests/test_gpu_asymmetric.py::test_run_exact_is_the_reference_on_the_asymmetric_matrix_itself:
 *     1e-10 against the oracle on the asymmetric matrix); batch_run is the fast path for covariances that are symmetric up to
 *     rounding, which is every covariance a filter produces itself.
 *   - batch_rts factors the predicted covariance by Cholesky and keeps Pk1_n - Pk1_k as a packed triangle.  It reads the
 *     LOWER triangle (diagonal included) of every covariance it is given -- Pf[k], P_last -- mirrored, for the gain Ck and
 *     the correction Ck (Pk1_n - Pk1_k) Ck^T; the filtered covariance itself enters the sum as given:
 *     Ps[k] = Pf[k] + correction.  On a trace written by batch_run (symmetric to rounding) that is the reference's
 *     rts_smooth to rounding.  (The reference's own backward step is triangle-dependent on such input too: its gain comes from
 *     scipy.linalg.solve(..., assume_a='pos'), i.e. LAPACK posv on ONE triangle of Pk1_k, ekf_sym.py:677.)
 *
 * Elementary functions of the model's expressions.  sqrt, reciprocals and negative half-integer powers are evaluated from the
 * hardware seeds with Newton steps (within an ulp or two of libm; IEEE answers kept at 0 and infinity).  sin / cos of one
 * argument come from one in-line routine accurate to 2e-16 ABSOLUTE for |a| <= 2^45 rad; beyond that (neighbouring doubles are
 * 0.008 rad apart there), and for NaN / inf, both are NaN -- the reference's libm returns the sine of the exact double instead.
 * A filter whose state drives a trigonometric argument that far comes back non-finite and is flagged (flag bit 1), not silently wrong.
 * The opt-out: a library generated under RN_TUNE=exact_math=1 uses IEEE division / sqrt and the library's sin / cos (full range) in
 * every kernel.  Measured against such a build (tests/test_gpu_live.py, profiles/r5_live_fast_vs_ieee.json): single calls of the live
 * filter agree to 1e-17 of the row maximum, a free-running 84-step stream to 3.4e-13 on P.
 */
#ifndef REDNOSE_AMD_FILTER_H
#define REDNOSE_AMD_FILTER_H

#include <stdint.h>

#define RN_FN(name, sym) name##_##sym

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------
 * Section 1 -- the reference's scalar ABI, unchanged signatures (HOST pointers, one filter)
 * Each call runs as a batch of one on the GPU and returns when its results are in the caller's buffers: the arguments are packed
 * into one pinned host buffer that is mapped into the device's address space, the kernel works on it in place, the call waits for
 * the null stream (one launch + one wait: 15-25 us per call on an MI355X; thread-safe: one mutex per library).  Errors are recorded
 * ({name}_last_error / _last_error_string) and leave the caller's buffers untouched -- without a HIP device every call does that.
 * --------------------------------------------------------------------------------------------------- */
#define RN_DECLARE_SCALAR_ABI(name)                                                                              \
  /* replaces {name}_predict, ekf_sym.py:162-165 -> predict(), ekf_c.c:8-33 */                                     \
  void RN_FN(name, predict)(double *in_x, double *in_P, double *in_Q, double dt);                                  \
  /* sympy routine wrappers, ekf_sym.py:155-161 (typedefs in rednose/helpers/ekf.h:21-25) */                      \
  void RN_FN(name, f_fun)(double *state, double dt, double *out);        /* next nominal state, D            */   \
  void RN_FN(name, F_fun)(double *state, double dt, double *out);        /* error-state transition, E x E    */   \
  void RN_FN(name, err_fun)(double *nom_x, double *delta_x, double *out);    /* inject error, D              */   \
  void RN_FN(name, inv_err_fun)(double *nom_x, double *true_x, double *out); /* extract error, E             */   \
  void RN_FN(name, H_mod_fun)(double *state, double *out);               /* d nominal / d error, D x E       */

/* per observation kind k (the integer is part of the symbol):
 *   replaces {name}_update_{k}, ekf_sym.py:149-152 -> update<Z,3,MAHA>(), ekf_c.c:37-121 */
/* one per gen_code global_var v: void {name}_set_{v}(double x)  -- ekf_sym.py:166-171; writes a device global */

#define RN_DECLARE_SCALAR_KIND(name, k)                                                                          \
  void RN_FN(name, update_##k)(double *in_x, double *in_P, double *in_z, double *in_R, double *in_ea);             \
  void RN_FN(name, h_##k)(double *state, double *ea, double *out);       /* predicted observation, Z         */   \
  void RN_FN(name, H_##k)(double *state, double *ea, double *out);       /* observation Jacobian, Z x D      */

/* ---------------------------------------------------------------------------------------------------
 * Section 2 -- batched entry points (DEVICE pointers, n independent filters) -- new with this engine.
 * They replace n sequential calls of the section-1 functions made by the reference's orchestrators
 * (EKFSym::predict / ::update, /root/reference/rednose/helpers/ekf_sym.cc:196-219).
 * --------------------------------------------------------------------------------------------------- */
#define RN_DECLARE_BATCH_ABI(name)                                                                               \
  void RN_FN(name, dims)(int *dims);                  /* dims[0..2] = DIM, EDIM, MEDIM (ekf_sym.py:122-124) */     \
  int RN_FN(name, num_kinds)(void);                                                                              \
  void RN_FN(name, kinds)(int *out);                  /* observation kinds, EKF::kinds (ekf.h:18)            */   \
  int RN_FN(name, kind_zdim)(int kind);               /* Z of a kind, -1 if unknown                          */   \
  int RN_FN(name, kind_maha)(int kind);               /* 1 if generated with the Mahalanobis gate            */   \
  int RN_FN(name, kind_eadim)(int kind);              /* extra arguments per observation of a kind (0: `ea` ignored) */ \
  void RN_FN(name, msckf_dims)(int *dims);            /* dim_main, dim_main_err, dim_augment, dim_augment_err, N (ekf_sym.py:57-73) */ \
  int RN_FN(name, last_error)(void);                                                                             \
  const char *RN_FN(name, last_error_string)(void);                                                              \
  void RN_FN(name, clear_error)(void);                                                                           \
  /* P <- F P F^T + dt Q, x <- f(x, dt) for n filters; dt_vec (n) may be NULL => scalar dt for all;            \
   * norm_quats != 0 renormalises the quaternion slices given to gen_code (EKFSym::normalize_quaternions,      \
   * ekf_sym.cc:69-77,207) */                                                                                  \
  int RN_FN(name, batch_predict)(double *x, double *P, const double *Q, const double *dt_vec, double dt,         \
                                 int64_t n, int norm_quats, void *stream);                                       \
  /* the same for the filters with active[i] != 0 only (see RN_DECLARE_BATCH_KIND_MASKED) */                     \
  int RN_FN(name, batch_predict_masked)(double *x, double *P, const double *Q, const double *dt_vec, double dt,  \
                                        int64_t n, int norm_quats, const uint8_t *active, void *stream);

/* fused multi-step run and offline smoothing (SURVEY.md 8b "proposed new batched exports") */
#define RN_DECLARE_BATCH_RUN(name)                                                                               \
  int RN_FN(name, zmax)(void);                        /* largest Z over the kinds: row stride of z in batch_run  */  \
  int RN_FN(name, run_unroll)(void);                  /* steps per iteration of batch_run's loop (instruction accounting) */ \
  int RN_FN(name, has_tri_trace)(void);               /* 1: the library has RN_DECLARE_BATCH_TRI's entry points (packed-triangle covariance trace) */ \
  int RN_FN(name, has_batch_run)(void);               /* 0: the fused kernel of this model did not fit the register file -- batch_run \
                                                         returns 4 (unsupported); walk the schedule with batch_predict_update_k */ \
  int RN_FN(name, predict_identity_at_dt0)(void);     /* 1: predict(dt = 0) is the identity on (x, P) for this model (f(x, 0) == x, F(x, 0) == I \
                                                         symbolically): a batch_run step with dt = 0 is an update alone -- the n observations of one  \
                                                         EKFSym::predict_and_update_batch call (ekf_sym.cc:172-180) can be one launch */ \
  /* T predict+update steps in ONE launch, x and P resident on chip between steps.  kinds (T) int32, dts (T),   \
   * R (T, zmax*zmax; the leading Z*Z entries of row t are that step's row-major R) and z (T, n, zmax; in: z,   \
   * out: y) are DEVICE arrays; the schedule is shared by all filters.  flags (T, n), trace_x (T, n, D) and      \
   * trace_P (T, n, E, E) -- the FILTERED pair after each step, i.e. Estimate.xk/Pk of ekf_sym.h:32-42 -- may be  \
   * NULL.  ea (T, n, EA) DEVICE array or NULL: per filter and step extra arguments of the kinds that take them (EA = the   \
   * largest kind_eadim; MSCKF feature tracks: the landmark); augment (T) int32 DEVICE array or NULL: non-zero = MSCKF window \
   * shift after that step (EKF_sym.augment, ekf_sym.py:365-391,527-528).  Replaces T calls of                              \
   * EKFSym::predict_and_update_batch (ekf_sym.cc:158-194). */                                                              \
  int RN_FN(name, batch_run)(double *x, double *P, const double *Q, const int32_t *kinds, const double *dts,       \
                             int64_t T, double *z, const double *R, int64_t n, int norm_quats, uint8_t *flags,    \
                             double *trace_x, double *trace_P, const double *ea, const int32_t *augment,          \
                             void *stream);                                                                       \
  /* Rauch-Tung-Striebel backward pass over a filtered trace; replaces the Python-only EKF_sym.rts_smooth        \
   * (/root/reference/rednose/helpers/ekf_sym.py:651-690).  xs/Ps may alias xf/Pf.  norm_quats: bit 0 = renormalise the   \
   * recomputed predicted states (as the forward pass did), bit 1 = the reference's norm_quats (smoothed states).       \
   * x_last (n, D) / P_last (n, E, E), both optional (NULL): the PREDICTED pair of the last step, which the reference     \
   * returns verbatim as the newest smoothed estimate (estimates[-1][0], [2], ekf_sym.py:658-659); NULL = recomputed from  \
   * the filtered pair of step T-2 (exact unless an MSCKF window shift happened in between).  MSCKF models: only the     \
   * main block / main states are smoothed, the rest of each filtered estimate passes through (ekf_sym.py:675-686). */    \
  int RN_FN(name, batch_rts)(const double *xf, const double *Pf, const double *ts, int64_t T, const double *Q,     \
                             int64_t n, int norm_quats, double *xs, double *Ps, const double *x_last,             \
                             const double *P_last, void *stream);

/* Packed-triangle trace (libraries with {name}_has_tri_trace() == 1: lane-group models of 13 .. 22 error states, e.g. live): the filtered
 * covariance trace between the forward and the backward pass as LOWER TRIANGLES packed row-major -- entry (i, j <= i) of a covariance at
 * i (i + 1) / 2 + j, E (E + 1) / 2 doubles per record instead of E * E.  Nothing is lost against batch_run + batch_rts: the fused run's covariance
 * is symmetric by contract and batch_rts reads lower triangles only (see "Asymmetric covariances" above).  batch_run_tri: trace_P is
 * (T, n, E (E + 1) / 2), everything else as batch_run.  batch_rts_tri: Pf, Ps and P_last are packed, everything else as batch_rts (Ps may alias
 * Pf).  batch_tri_unpack / batch_tri_pack convert `count` records to / from full symmetric matrices (pack takes the lower triangle). */
#define RN_DECLARE_BATCH_TRI(name)                                                                               \
  int RN_FN(name, batch_run_tri)(double *x, double *P, const double *Q, const int32_t *kinds, const double *dts,   \
                                 int64_t T, double *z, const double *R, int64_t n, int norm_quats, uint8_t *flags, \
                                 double *trace_x, double *trace_P, const double *ea, const int32_t *augment,       \
                                 void *stream);                                                                    \
  int RN_FN(name, batch_rts_tri)(const double *xf, const double *Pf, const double *ts, int64_t T, const double *Q,  \
                                 int64_t n, int norm_quats, double *xs, double *Ps, const double *x_last,          \
                                 const double *P_last, void *stream);                                              \
  int RN_FN(name, batch_tri_unpack)(const double *tri, double *full, int64_t count, void *stream);                 \
  int RN_FN(name, batch_tri_pack)(const double *full, double *tri, int64_t count, void *stream);

/* MSCKF models only (gen_code msckf_params): window shift of EKF_sym.augment (ekf_sym.py:365-391) on n filters, in place */
#define RN_DECLARE_BATCH_MSCKF(name)                                                                             \
  int RN_FN(name, batch_augment)(double *x, double *P, int64_t n, void *stream);

/* feature-track kinds of an MSCKF model additionally export the reference's extra-argument Jacobian:
 *   void {name}_He_{k}(double *state, double *ea, double *out)   -- Z x 3, ekf_sym.py:110-113; their updates project the
 *   residual, H and R on the left null space of it (ekf_c.c:66-76) and write Z - 3 residual rows back into z (the last 3 entries of
 *   z pass through).  BASIS of that residual: the reference writes A^T (z - h) with A = Hea^T.fullPivLu().kernel() (ekf_c.c:71-73,120),
 *   a basis that is not orthonormal; these kernels use an ORTHONORMAL basis Q of the same space (Householder QR of Hea).  x and P do
 *   not depend on the choice (tested to 1e-10); the residuals are related by y_ref = (A^T Q) y, and the quantity that does not
 *   depend on the basis agrees: |y|^2 = y_ref^T (A^T A)^-1 y_ref = |projection of z - h on the null space|^2
 *   (tests/test_gpu_msckf.py::test_both_kinds_vs_oracle_strict checks it against the reference's A for every filter). */
#define RN_DECLARE_BATCH_KIND(name, k)                                                                           \
  /* update only.  ea: (n, kind_eadim) extra arguments, one row per filter (NULL when the kind takes none).    \
   * flags (n bytes, may be NULL): bit0 = Mahalanobis gate fired (R inflated, ekf_c.c:88-94),                  \
   * bit1 = non-finite state after the update, bit2 = null-space projection failed (rank-deficient extra-argument  \
   * Jacobian; the measurement is ignored like in ekf_sym.py:589-591) */                                        \
  int RN_FN(name, batch_update_##k)(double *x, double *P, double *z, const double *R, int r_per_filter,          \
                                    const double *ea, int64_t n, int norm_quats, uint8_t *flags, void *stream);  \
  /* Mahalanobis distance d2 = y^T (He P He^T + R)^-1 y of an observation, nothing modified; replaces the Python-only \
   * EKF_sym.maha_test (/root/reference/rednose/helpers/ekf_sym.py:626-649) for n filters */                      \
  int RN_FN(name, batch_maha_##k)(const double *x, const double *P, const double *z, const double *R,            \
                                  int r_per_filter, const double *ea, int64_t n, double *d2, void *stream);      \
  /* fused predict + update: ONE launch, state crosses HBM once (EKFSym::predict_and_update_batch with a       \
   * single observation, ekf_sym.cc:158-194) */                                                                \
  int RN_FN(name, batch_predict_update_##k)(double *x, double *P, const double *Q, const double *dt_vec,         \
                                            double dt, double *z, const double *R, int r_per_filter,             \
                                            const double *ea, int64_t n, int norm_quats, uint8_t *flags,         \
                                            void *stream);                                                       \
  /* the same launch also writing the call's CHECKPOINT -- what EKFSym::checkpoint keeps of a call (ekf_sym.cc:142-156, 191): \
   * ckpt_z (n, Z) the observations as they came (z itself leaves as the residuals), ckpt_x (n, D) / ckpt_P (n, E, E) the   \
   * filtered pair; DEVICE, 16-byte aligned, distinct from x / P / z.  One launch and 1.5 x the bytes of the plain step      \
   * instead of the step plus three copies (2 x the bytes, four launches) */                                    \
  int RN_FN(name, batch_predict_update_##k##_ckpt)(double *x, double *P, const double *Q, const double *dt_vec,  \
                                                   double dt, double *z, const double *R, int r_per_filter,      \
                                                   const double *ea, int64_t n, int norm_quats, uint8_t *flags,  \
                                                   double *ckpt_x, double *ckpt_P, double *ckpt_z, void *stream);

/* Per-filter timelines.  Every filter of the reference is its own instance with its own filter_time and its own rewind ring
 * (EKFSym::predict_and_update_batch / rewind, /root/reference/rednose/helpers/ekf_sym.cc:83-156); a batch fed from n INDEPENDENT
 * logs therefore needs calls that advance only SOME filters, each by its own dt.  The `_masked` twins of the step-granular entry
 * points take `active` (n bytes, DEVICE): filters with active[i] == 0 pass through untouched -- x, P and z[i] leave exactly as
 * they came -- and get flags[i] = 16 (bit 4); the others see the plain entry point's arithmetic with dt_vec[i].  active == NULL is
 * the plain entry point.  (Bit 5 of the orchestrators' flags, "observation too old for this filter's ring, ignored"
 * -- ekf_sym.cc:87-94 -- is set on the host side: BatchedEKF / EKFSymBatch.) */
/* Checkpoint rings of per-filter timelines: `rec` doubles of record i of a flat DEVICE array (row stride flat_stride) <-> entry
 * slot[i] of filter i in a ring laid out (K, n, ring_stride), for the filters with active[i] != 0 (NULL: all); to_ring != 0
 * stores, 0 loads.  One launch moves one array of a checkpoint (x: D, P: E * E, z: Z of the kind into a ring of stride zmax) for
 * the whole batch, every filter at its own ring position -- the batched form of EKFSym::checkpoint / ::rewind's state copy
 * (ekf_sym.cc:119-156), whose lists are per filter instance. */
#define RN_DECLARE_BATCH_RING(name)                                                                              \
  int RN_FN(name, batch_ring_copy)(double *ring, int64_t ring_stride, double *flat, int64_t flat_stride,          \
                                   int64_t rec, const int32_t *slot, const uint8_t *active, int64_t n,            \
                                   int to_ring, void *stream);                                                    \
  /* flags[i] = value for the filters with mask[i] != 0 (both n bytes, DEVICE): how an orchestrator marks the filters whose observation was  \
   * too old for their ring (bits 4 | 5) on the stream, without moving the flag bytes through the host */          \
  int RN_FN(name, batch_flags_set)(uint8_t *flags, const uint8_t *mask, int value, int64_t n, void *stream);

/* Per-filter timelines with the in-order bookkeeping ON THE DEVICE: the filters' times ft (n doubles, NaN = not started) and their
 * rings stay in device memory, and a call in which no filter is late costs the host one integer.  All pointers are DEVICE pointers, both
 * calls are asynchronous on `stream`, status codes as in section 2.
 *
 * batch_timeline_plan is PURE -- it writes only its outputs, never ft or a ring.  Per filter i, with active == NULL meaning all:
 *   inactive                               dt_out = 0,                          act_out = 0, late_out = 0
 *   active, ft NaN or t >= ft              dt_out = isnan(ft) ? 0 : t - ft,     act_out = 1, late_out = 0
 *   active, t < ft  (late)                 dt_out = 0,                          act_out = 0, late_out = 1, counted in *n_late
 * dt_out / act_out are the dt_vec / active of the `_masked` entry points below.  *n_late (one int32) ACCUMULATES, one vector atomic per
 * wavefront with a late filter: zero it before the call or compare with its value before.  It may be pinned host memory mapped
 * into the device (hipHostMallocMapped: readable after one wait for the stream), or device memory followed by a 4-byte copy.
 * z_keep (may be NULL): z_count doubles of z_src copied aside, for the checkpoint -- the step overwrites z with the residuals.
 *
 * batch_timeline_push is the whole checkpoint of a call (EKFSym::checkpoint, ekf_sym.cc:142-156, for n instances) in ONE launch, to
 * be enqueued behind the step.  For every filter with act[i] != 0: ft[i] = t[i]; its ring advances --
 *   full = length >= K;  head = full ? (head + 1) % K : head;  length = full ? length : length + 1;  slot = (head + length - 1) % K
 * -- and entry `slot` takes t[i], x[i] (D), P[i] (E * E), kind, nobs and the call's nobs observations AS THEY CAME: observation j of
 * filter i is read at z_obs + i * z_stride_f + j * z_stride_o (Z of the kind; strides in doubles), its noise at R + i * r_stride_f +
 * j * r_stride_o (Z * Z; r_per_filter == 0: shared by the filters, r_stride_f ignored), its extra arguments (kinds that take them)
 * at ea + i * ea_stride_f + j * ea_stride_o.  Ring layout, K entries per filter: ring_t (K, n), ring_x (K, n, D), ring_P (K, n, E, E),
 * ring_kind / ring_nobs (K, n) int32, ring_z (K, n, nmax, zmax), ring_R (K, n, nmax, zmax, zmax), ring_ea (K, n, nmax, eamax) with
 * zmax = {name}_zmax() and eamax = max(1, largest {name}_kind_eadim); ring_head / ring_length (n) int64.  Only the Z / Z x Z / EA
 * leading entries of an observation's slots are written.  1 <= nobs <= nmax.  K == 0 (ring pointers NULL): only ft is written. */
#define RN_DECLARE_BATCH_TIMELINE(name)                                                                          \
  int RN_FN(name, batch_timeline_plan)(const double *t, const uint8_t *active, const double *ft, int64_t n,       \
                                       double *dt_out, uint8_t *act_out, uint8_t *late_out, int32_t *n_late,      \
                                       const double *z_src, double *z_keep, int64_t z_count, void *stream);       \
  int RN_FN(name, batch_timeline_push)(const double *t, const uint8_t *act, double *ft, const double *x,          \
                                       const double *P, int64_t n, int64_t K, int64_t nmax, double *ring_t,       \
                                       double *ring_x, double *ring_P, int32_t *ring_kind, int32_t *ring_nobs,    \
                                       double *ring_z, double *ring_R, double *ring_ea, int64_t *ring_head,       \
                                       int64_t *ring_length, int kind, int nobs, const double *z_obs,             \
                                       int64_t z_stride_f, int64_t z_stride_o, const double *R, int r_per_filter, \
                                       int64_t r_stride_f, int64_t r_stride_o, const double *ea,                  \
                                       int64_t ea_stride_f, int64_t ea_stride_o, void *stream);

/* A DIFFERENT OBSERVATION KIND PER FILTER IN ONE LAUNCH.  N independent filters receive, at a tick, whatever kind their sensor produced
 * (updates.at(kind), /root/reference/rednose/helpers/ekf_sym.cc:196-219); with the per-kind entry points such a tick is one `_masked`
 * launch per kind present, each moving the state of ALL filters through HBM.  Here filter i gets predict(dt[i]) and the update of
 * kinds[i] in one launch: the arithmetic of batch_predict_update_{kinds[i]}_masked, the state crossing HBM once.
 *   {name}_has_step_kinds() == 1: the library has the kernel.  0: MSCKF models, models with a kind that takes extra arguments or has 7 or
 *   more rows, or a kernel that did not fit the register file -- the three entry points then return status 4 and nothing is launched.
 * Buffers (DEVICE, 16-byte aligned like everywhere): kinds (n) int32; z (n, zmax), zmax = {name}_zmax(): the first Z entries of row i are
 * read and overwritten by the residual, the rest of the row passes through bit for bit; R: r_per_filter != 0 -> (n, zmax * zmax), the
 * leading Z * Z entries of row i are filter i's row-major R (batch_run's convention); r_per_filter == 0 -> a table (num_kinds, zmax * zmax)
 * with one such row per kind in the order of {name}_kinds(); dt_vec / dt, active, flags, norm_quats as in the `_masked` entry points.
 * Per filter: active[i] == 0 -> x, P and the z row untouched, flag 16; active and kinds[i] a kind of the model -> stepped, flags as the
 * per-kind entry points; active and any other kinds[i] -> untouched like an inactive filter (no predict either), flag 8.
 * batch_timeline_push_kinds is batch_timeline_push for such a call: kinds (n) in place of (kind, nobs) -- one observation per filter, an
 * entry that is not a kind of the model skips its filter --, z_obs (n, zmax) the observations as they came, R as above. */
#define RN_DECLARE_BATCH_KINDS(name)                                                                             \
  int RN_FN(name, has_step_kinds)(void);                                                                         \
  int RN_FN(name, batch_predict_update_kinds)(double *x, double *P, const double *Q, const double *dt_vec,        \
                                              double dt, const int32_t *kinds, double *z, const double *R,        \
                                              int r_per_filter, int64_t n, int norm_quats, uint8_t *flags,        \
                                              const uint8_t *active, void *stream);                               \
  int RN_FN(name, batch_update_kinds)(double *x, double *P, const int32_t *kinds, double *z, const double *R,     \
                                      int r_per_filter, int64_t n, int norm_quats, uint8_t *flags,                \
                                      const uint8_t *active, void *stream);                                       \
  int RN_FN(name, batch_timeline_push_kinds)(const double *t, const uint8_t *act, double *ft, const double *x,    \
                                             const double *P, int64_t n, int64_t K, int64_t nmax, double *ring_t, \
                                             double *ring_x, double *ring_P, int32_t *ring_kind,                  \
                                             int32_t *ring_nobs, double *ring_z, double *ring_R, double *ring_ea, \
                                             int64_t *ring_head, int64_t *ring_length, const int32_t *kinds,      \
                                             const double *z_obs, const double *R, int r_per_filter,              \
                                             void *stream);

/* THE FUSED RUN WITH A SCHEDULE PER FILTER: N recorded logs replayed in ONE launch.  batch_run keeps x and P on chip for T steps but shares
 * its schedule among the filters; batch_predict_update_kinds gives every filter its own kind and dt but moves the whole state through HBM at
 * every tick.  Here filter i walks its own column of kinds (T, n) int32 and dts (T, n) with x and P resident in registers.
 *   {name}_has_batch_run_pf() == 1: the library has the kernel (both kernel families, up to 64 error states).  0: MSCKF models, models
 *   with a kind that takes extra arguments, models without batch_run, or a kernel that did not fit the register file -- batch_run_pf then
 *   returns status 4 and nothing is launched (walk the schedule with batch_predict_update_kinds).
 * All pointers are DEVICE pointers; alignment rules, status codes and argument checks are those of batch_run; T == 0 or n == 0 is a no-op
 * that returns 0.  z (T, n, zmax) in: z, out: y; R is the per-kind table of batch_predict_update_kinds with r_per_filter == 0: (num_kinds,
 * zmax * zmax), one row per kind in the order of {name}_kinds(), the leading Z * Z entries of a row are that kind's row-major R.  flags
 * (T, n), trace_x (T, n, D), trace_P (T, n, E, E) may be NULL.  Per entry (t, i):
 *   kinds[t, i] <= 0 (idle)   filter i is not touched at step t, no predict; dts[t, i] is ignored; the z row passes through bit for bit; flag 16
 *   a kind of the model       predict(dts[t, i]), renormalisation as in batch_run, then the update of that kind: the first Z entries of the z row
 *                             become the residual, the rest of the row passes through; flags as in batch_run, the gate bit included
 *   any other value           untouched like an idle entry, flag 8 (the rule of batch_predict_update_kinds, not batch_run's "predict, then flag 8")
 * trace_x / trace_P row (t, i) is filter i's pair after step t -- for an idle or flag-8 entry the pair it had: the trace is dense.  The
 * covariance is read as (P + P^T) / 2 as the state enters the registers, like batch_run (see "Asymmetric covariances" above).  A filter
 * without a stepped entry in the whole schedule is NOT written back: its x and P leave bit for bit as they came (the `_masked` rule). */
#define RN_DECLARE_BATCH_RUN_PF(name)                                                                            \
  int RN_FN(name, has_batch_run_pf)(void);                                                                       \
  int RN_FN(name, batch_run_pf)(double *x, double *P, const double *Q, const int32_t *kinds, const double *dts,   \
                                int64_t T, double *z, const double *R, int64_t n, int norm_quats, uint8_t *flags, \
                                double *trace_x, double *trace_P, void *stream);

/* THE SMOOTHER WITH A SCHEDULE PER FILTER: the backward pass over the dense trace batch_run_pf writes, N ragged logs in ONE launch.
 *   {name}_has_batch_rts_pf() == 1: the library has the kernel (every library with batch_rts whose model has no MSCKF window).  0: MSCKF
 *   models, libraries without batch_rts, or a kernel that did not fit the register file -- batch_rts_pf then returns status 4 and nothing is
 *   launched.
 * All pointers are DEVICE pointers; alignment rules, status codes, the norm_quats bits and aliasing (xs == xf, Ps == Pf allowed) are those of
 * batch_rts; T == 0 or n == 0 is a no-op that returns 0.  xf (T, n, D) / Pf (T, n, E, E): the dense trace (the row of an entry that did not step
 * its filter is the pair the filter already had).  dts (T, n): the forward dt of every entry.  act (T, n): 1 where entry (t, i) stepped filter
 * i -- its kind is a kind of the model, whether or not the gate rejected the update --, 0 for idle and unknown-kind entries, where dts is
 * ignored.  Per filter i, with m its last entry with act == 1, backward step k relates rows k and k + 1:
 *   act[k + 1, i] == 0   no predict happened between the two rows: the predicted pair of k + 1 IS the filtered pair of k and Ck = I -- for
 *                        every model, also where predict(0) is not the identity (an idle entry is not a predict(0))
 *   act[k + 1, i] == 1   the step of batch_rts with dt = dts[k + 1, i] (the identity-gain path for dt == 0 where the model has it)
 *   start                the smoothed pair of row m is the PREDICTED pair of entry m (the reference's estimates[-1][0], [2]): recomputed from
 *                        row m - 1 and dts[m, i], or row i of x_last / P_last when those are passed; step m - 1 therefore sees
 *                        Pk1_n - Pk1_k = 0, as the reference's second-newest estimate does.  m == 0 and nothing passed: the filtered pair
 *                        passes through (the T == 1 rule of batch_rts)
 *   rows behind m        and every row of a filter without an act entry leave bit for bit as they came (copied, or in place rewritten with
 *                        the same bits)
 *   rows before the filter's first act entry f: step f - 1 is an ordinary full step with dts[f, i] -- it smooths the pair the filter started
 *                        from --, the rows before it follow by identity steps.  (The reference has no counterpart: its estimates begin with
 *                        the first observation.)
 * Covariances are read as lower triangles, mirrored (see "Asymmetric covariances" above). */
#define RN_DECLARE_BATCH_RTS_PF(name)                                                                            \
  int RN_FN(name, has_batch_rts_pf)(void);                                                                       \
  int RN_FN(name, batch_rts_pf)(const double *xf, const double *Pf, const double *dts, const uint8_t *act,       \
                                int64_t T, const double *Q, int64_t n, int norm_quats, double *xs, double *Ps,   \
                                const double *x_last, const double *P_last, void *stream);

/* THE SAME RUN WITH A NOISE MATRIX PER LOG ENTRY.  A recorded log carries the noise of each observation (a GNSS fix with the receiver's
 * reported variance, an odometry frame with its own standard deviation); batch_run_pf knows one R per kind for the whole run.  Here
 * every entry (t, i) brings its own R, as every predict_and_update_batch(t, kind, z, R) call of the reference does.
 *   {name}_has_batch_run_pf_r() == 1: the library has the kernel.  0: a library without batch_run_pf, or one whose kernel did not fit the
 *   register file -- batch_run_pf_r then returns status 4 and nothing is launched (walk the schedule with batch_predict_update_kinds and
 *   r_per_filter != 0, one step's rows at a time).
 * Every argument is batch_run_pf's, and so are the status codes, the argument checks (NULL -> 2, misaligned -> 3, T == 0 or n == 0 a no-op
 * that returns 0, no device -> 1), the alignment rules, the flag rules 16 / 8, the dense trace, (P + P^T) / 2 at entry, and "a filter that
 * no entry stepped is not written back".  What differs is R:
 *   R is a DEVICE array (T, n, zmax * zmax), 16-byte aligned.  The leading Z * Z doubles of row (t, i) are the row-major R of entry (t, i),
 *   Z being the Z of kinds[t, i]: R + t * n * zmax * zmax is exactly the `r_per_filter != 0` buffer of batch_predict_update_kinds for step t.
 *   The rest of a row is never used, and neither are the rows of idle entries (kinds[t, i] <= 0) and of entries with an unknown kind
 *   (flag 8): such doubles may hold anything, NaN included, and nothing of them reaches x, P, y, the flags or the trace.  The R of an entry
 *   is symmetric positive definite, like the rows of the table. */
#define RN_DECLARE_BATCH_RUN_PF_R(name)                                                                          \
  int RN_FN(name, has_batch_run_pf_r)(void);                                                                     \
  int RN_FN(name, batch_run_pf_r)(double *x, double *P, const double *Q, const int32_t *kinds, const double *dts, \
                                  int64_t T, double *z, const double *R, int64_t n, int norm_quats,               \
                                  uint8_t *flags, double *trace_x, double *trace_P, void *stream);

/* THE SAME RUN WITH A DIAGONAL NOISE PER LOG ENTRY.  The noise a recorded log carries is almost always diagonal (np.diag(std**2), a
 * variance per component); as full (Z, Z) matrices it costs batch_run_pf_r Z * Z doubles per entry where Z would do.  Here every entry
 * (t, i) brings the Z variances of its observation.
 *   {name}_has_batch_run_pf_rd() == 1: the library has the kernel.  0: a library without batch_run_pf, or one whose kernel did not fit the
 *   register file -- batch_run_pf_rd then returns status 4 and nothing is launched (expand the rows to (Z, Z) matrices and call
 *   batch_run_pf_r, or walk the schedule as described there).  Not tied to has_batch_run_pf_r(): a row is zmax doubles, not zmax * zmax.
 * Every argument is batch_run_pf_r's, and so are the status codes, the argument checks (NULL -> 2, misaligned -> 3, T == 0 or n == 0 a
 * no-op that returns 0, no device -> 1), the alignment rules, the flag rules 16 / 8, the dense trace, (P + P^T) / 2 at entry, and "a filter
 * that no entry stepped is not written back".  What differs is R:
 *   R is a DEVICE array (T, n, zmax), 16-byte aligned at its base.  The leading Z doubles of row (t, i) are the diagonal of the noise of
 *   entry (t, i) -- variances, positive --, Z being the Z of kinds[t, i]; the off-diagonal entries are zero by definition.  The rest of a
 *   row is never read, and neither are the rows of idle entries (kinds[t, i] <= 0) and of entries with an unknown kind (flag 8): such
 *   doubles may hold anything, NaN included, and nothing of them reaches x, P, y, the flags or the trace.
 * The run is batch_run_pf_r on the matrices diag(row), to rounding. */
#define RN_DECLARE_BATCH_RUN_PF_RD(name)                                                                          \
  int RN_FN(name, has_batch_run_pf_rd)(void);                                                                     \
  int RN_FN(name, batch_run_pf_rd)(double *x, double *P, const double *Q, const int32_t *kinds, const double *dts, \
                                   int64_t T, double *z, const double *R, int64_t n, int norm_quats,               \
                                   uint8_t *flags, double *trace_x, double *trace_P, void *stream);

/* THE SAME RUN FOR MSCKF MODELS: extra arguments per entry (a feature track's landmark) and a window shift per filter.  N camera logs,
 * each with its own feature tracks and its own keyframe times, in one launch.
 *   {name}_has_batch_run_pf_ea() == 1: the library has the kernel (MSCKF models with a fused run).  0: every other library --
 *   batch_run_pf_ea then returns status 4 and nothing is launched (batch_run_pf serves the models without a window; walk the schedule
 *   with batch_predict_update_{k}_masked and batch_augment_masked otherwise).  has_batch_run_pf() stays 0 for MSCKF models.
 * x .. trace_P are batch_run_pf's arguments (R: one row of zmax * zmax doubles per kind), and so are the status codes, the argument checks
 * (NULL -> 2, `ea` included; misaligned -> 3, T == 0 or n == 0 a no-op that returns 0, no device -> 1), the flag rules 16 / 8, the dense
 * trace, (P + P^T) / 2 at entry, "a filter that no entry stepped is not written back", and z: rows of idle entries and the columns beyond
 * Z pass through; a feature-track kind writes Z - 3 residual rows in the reference's basis (above), as batch_run does.
 *   ea is a DEVICE array (T, n, EA), EA the largest {name}_kind_eadim: the leading doubles of row (t, i) are the extra arguments of entry
 *   (t, i).  Only the rows of entries whose kind takes extra arguments are read; the others may hold anything, NaN included.
 *   augment is a DEVICE array (T, n) of int32, or NULL (no shifts): augment[t, i] != 0 shifts the window of filter i (batch_augment) after
 *   its entry t.  Ignored at entries that did not step the filter (idle, unknown kind).  An entry whose null-space projection was rank
 *   deficient (flag 4: the measurement is ignored) still shifts, as in batch_run.  trace row (t, i) is the estimate BEFORE that shift.
 * The step-granular half, exported beside batch_augment by MSCKF libraries only (no macro of its own, like nothing else here that
 * only some libraries have apart from RN_DECLARE_BATCH_MSCKF):
 *   int {name}_batch_augment_masked(double *x, double *P, const uint8_t *active, int64_t n, void *stream);
 * batch_augment on the filters with active[i] != 0, the others untouched bit for bit; active == NULL: every filter. */
#define RN_DECLARE_BATCH_RUN_PF_EA(name)                                                                          \
  int RN_FN(name, has_batch_run_pf_ea)(void);                                                                     \
  int RN_FN(name, batch_run_pf_ea)(double *x, double *P, const double *Q, const int32_t *kinds, const double *dts, \
                                   int64_t T, double *z, const double *R, int64_t n, int norm_quats,               \
                                   uint8_t *flags, double *trace_x, double *trace_P, const double *ea,             \
                                   const int32_t *augment, void *stream);

/* Per-filter timelines, THE LATE OBSERVATION ON THE DEVICE: the rewind of every filter batch_timeline_plan found late, each in its own ring
 * (EKF_sym.rewind and the too-old test in front of it, the reference's ekf_sym.py:418-438, 464-471), and the gather of the
 * overtaken entries, one replay position of all rewound filters at a time, into the buffers batch_predict_update_kinds and
 * batch_timeline_push_kinds take (the fast-forward, ekf_sym.py:477-479).  DEVICE pointers, asynchronous on `stream`, status codes as in
 * section 2; n == 0 is a no-op.  Ring layout as in batch_timeline_push; K >= 1.
 *
 * batch_rewind_locate.  late / dt_out / act_out (n) are the plan's buffers; x, P, ft the filters' state and times; rep_slot / rep_n (n) int32,
 * drop_out (n) bytes; counts: two int32, ZEROED by the caller on the stream before the call.  With L = ring_length[i] and H = ring_head[i]
 * (both clamped: 0 <= H < K, 0 <= L <= K) and T[j] = ring_t[((H + j) % K) * n + i], j < L, per filter i:
 *   late[i] == 0                                      drop_out = 0, rep_n = 0, nothing else of the filter is touched
 *   L == 0, t < T[0] or t < T[L-1] - max_rewind_age   too old: drop_out = 1, rep_n = 0, counts[1] += 1 (a vector atomic); nothing else changes
 *                                                     (the plan left act_out = 0, dt_out = 0: the filter sits this call out)
 *   otherwise, ix = #{j < L: T[j] <= t}               (bisect_right; 1 <= ix <= L) x[i], P[i] <- entry (H + ix - 1) % K; ft = T[ix-1];
 *                                                     dt_out = t - T[ix-1]; act_out = 1; rep_slot = (H + ix) % K; rep_n = L - ix;
 *                                                     ring_length = ix; drop_out = 0; counts[0] = max(counts[0], rep_n) (a vector atomic)
 * batch_rewind_fetch, replay position q >= 0.  Per filter i with rep_n[i] > q, e = ((rep_slot[i] + q) % K) * n + i: t_out = ring_t[e];
 * dt_out = t_out - t_prev[i]; kinds_out = ring_kind[e]; act_out = 1, or 0 where that is not a kind of the model; the entry's FIRST observation
 * row (zmax doubles) to z_out (n, zmax) and again to z_keep (n, zmax) -- the step overwrites z_out with the residual, the checkpoint wants the
 * observation --; its noise, zmax x zmax in the ring, compacted to the leading Z * Z doubles (row-major) of row i of R_out (n, zmax * zmax):
 * r_per_filter != 0 of batch_predict_update_kinds.  Every other filter: act_out = 0, dt_out = 0, kinds_out = 0, t_out = t_prev[i], its z and
 * R rows untouched.  t_prev is the call's own t for q == 0 and the previous fetch's t_out after that -- never ft, which the push of the
 * position before may not have written yet.
 *
 * ORDER of a late call on the one stream: plan -> locate -> fetch(0) -> the call's own step (the plan's dt / act: rewound and in-order filters
 * together) -> its push -> for q = 0 .. counts[0] - 1: fetch(q + 1) into a second buffer set, batch_predict_update_kinds and
 * batch_timeline_push_kinds on the current set.  Every entry is fetched before a launch overwrites its slot: the call's own push writes the
 * slot of replay position 0, the push behind position q the slot of position q + 1.  A push evicts only on a full ring -- here the last
 * replay's push at most, and it takes the filter's oldest entry, never a replay entry (ix >= 1). */
#define RN_DECLARE_BATCH_REWIND(name)                                                                            \
  int RN_FN(name, batch_rewind_locate)(const uint8_t *late, const double *t, int64_t n, int64_t K, double *ring_t, \
                                       double *ring_x, double *ring_P, int64_t *ring_head, int64_t *ring_length,  \
                                       double max_rewind_age, double *x, double *P, double *ft, double *dt_out,   \
                                       uint8_t *act_out, int32_t *rep_slot, int32_t *rep_n, uint8_t *drop_out,    \
                                       int32_t *counts, void *stream);                                            \
  int RN_FN(name, batch_rewind_fetch)(const int32_t *rep_slot, const int32_t *rep_n, int64_t q,                   \
                                      const double *t_prev, int64_t n, int64_t K, int64_t nmax, double *ring_t,   \
                                      int32_t *ring_kind, double *ring_z, double *ring_R, double *t_out,          \
                                      double *dt_out, int32_t *kinds_out, uint8_t *act_out, double *z_out,        \
                                      double *z_keep, double *R_out, void *stream);

#define RN_DECLARE_BATCH_KIND_MASKED(name, k)                                                                  \
  int RN_FN(name, batch_update_##k##_masked)(double *x, double *P, double *z, const double *R, int r_per_filter,  \
                                             const double *ea, int64_t n, int norm_quats, uint8_t *flags,         \
                                             const uint8_t *active, void *stream);                                \
  int RN_FN(name, batch_predict_update_##k##_masked)(double *x, double *P, const double *Q, const double *dt_vec, \
                                                     double dt, double *z, const double *R, int r_per_filter,     \
                                                     const double *ea, int64_t n, int norm_quats, uint8_t *flags, \
                                                     const uint8_t *active, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* REDNOSE_AMD_FILTER_H */
