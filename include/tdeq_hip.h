/*
 * tdeq_hip.h — C-ABI of libtdeq_hip.so, the MI355X (gfx950) explicit Runge–Kutta hot path.
 *
 * The reference (rtqichen/torchdiffeq v0.2.5) has no native boundary: every function below replaces a
 * group of eager ATen calls inside one reference Python function (cited per entry point as
 * torchdiffeq/_impl/<file>:<lines>).  The host solver (torchdiffeq_amd/solvers.py) is the only caller.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types cross the boundary.
 *   - every entry point returns an int: 0 on success, a hipError_t (>0) from the launch, or a
 *     TDEQ_E* (<0) for argument errors.  Nothing throws or aborts across the ABI.
 *   - all device buffers are BORROWED: owned by the caller, contiguous, kept alive until the stream
 *     reaches the launch.  No allocation, no hipDeviceSynchronize, no global mutable state.
 *   - launches are asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream).
 *   - `dtype`: TDEQ_F32 or TDEQ_F64 = element type T of every state-sized buffer.
 *   - coefficient arithmetic follows the reference's rounding: c_j = fl_T(fl_T(coef_j) * fl_T(dt)),
 *     products and sums in T, no FMA contraction (rk_common.py:79,89,201-205; interp.py:17-21).
 *   - `dt` may be negative: a solve in decreasing time passes sign*dt and keeps the raw func outputs
 *     in k_j, which is bit-identical to the reference's `_ReverseFunc(mul=-1)` wrapper (misc.py:158-165).
 *   - host arrays (`k`, `coef`, segment tables) are read during the call and copied into the kernel
 *     argument block; they need not outlive the call.
 *   - state buffers whose address is 16-byte aligned take the 16 B/lane vector path; otherwise a
 *     scalar path is used (same results).
 *
 * Segments.  A state vector may consist of several logical segments (tuple states, the adjoint's
 * [y | adj_y | params | vjp_t]).  Segment s starts at element chunk_start[s]*chunk and holds numel[s]
 * valid elements; the space up to the next segment start is padding that the norm kernels ignore.
 * `chunk` (elements) must be a multiple of TDEQ_CHUNK_QUANTUM.  n_seg==1 with chunk_start={0}
 * is the plain unpadded tensor case.
 */
#ifndef TDEQ_HIP_H
#define TDEQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDEQ_ABI_VERSION 35
#define TDEQ_F32 0
#define TDEQ_F64 1
/* interleaved (re, im) complex states — accepted by the NORM entry points only (tdeq_error_norm, tdeq_error_norm_partial[_ctrl],
 * tdeq_init_norms, tdeq_init_scaled): segment tables, chunk and counts are then in complex elements and T below is the
 * real type; every other entry point is linear with real coefficients and takes the state's real view (2n elements of
 * TDEQ_F32 / TDEQ_F64).  |z| = hypot(re, im), z / real = z * (1 / real): torchdiffeq/_impl/misc.py:80-82 as ATen rounds it. */
#define TDEQ_C64 2
#define TDEQ_C128 3
/* bfloat16 / float16 states (r05).  The reference integrates them in their own precision (misc.py:185-187,
 * rk_common.py:61-65): every ATen op computes in float32 and rounds its result to the storage type, a `torch.sum` over a
 * tableau row accumulates the rounded products in float32 and rounds once.  Accepted by the entry points of the
 * host-driven step — tdeq_stage_combine, tdeq_stage_combine_fill, tdeq_stage_combine_err, tdeq_error_norm,
 * tdeq_init_norms, tdeq_init_scaled, tdeq_dense_eval, tdeq_dense_eval_multi, tdeq_interp_fit, tdeq_rk4_38_stage,
 * tdeq_lerp, tdeq_fixed_stage, tdeq_weighted_sum — with exactly that rounding (tdeq_kernels_lp.hpp), and by the
 * look-ahead pair tdeq_error_norm_partial_ctrl (err_partial MUST be NULL: the whole error row in `k` / `coef`, 1..14
 * terms — a row is rounded once, there is no partial sum to continue; the controller forms the ratio, the next step and
 * its stage times in the state's type; `state_in_dev` as for fp32) + tdeq_stage_combine_sel, and by tdeq_stage_combine_dev
 * (captured steps; err_out must be NULL); every other entry point returns TDEQ_EINVAL for them.  Scalars: `dt`, tableau weights, `slope`, tolerances are rounded to the
 * storage type where the reference holds them as 0-dim tensors of the state's type or as FIRST operands, and taken at
 * float32 where ATen takes a Python number as SECOND operand of `*` (rk4's 1/3, `* dt`; tdeq_init_norms' rtol).
 * The norm entry points report per segment the sum of fl(|q|^2) — for a segment of ONE element |q| itself (the adjoint's
 * norms take their time component as `t.abs()`, adjoint.py:250, and the caller squares it with the same rounding). */
#define TDEQ_BF16 4
#define TDEQ_F16 5
#define TDEQ_MAX_TERMS 14      /* dopri8: 13 stages + FSAL slot (dopri8.py:5-70) */
#define TDEQ_MAX_SUM_TERMS 8    /* tdeq_weighted_sum */
#define TDEQ_MAX_DENSE_OUTPUTS 16 /* tdeq_dense_eval_multi */
#define TDEQ_MAX_SEGMENTS 4096
#define TDEQ_INLINE_SEGMENTS 16  /* segment tables up to this size travel in the kernel arguments */
#define TDEQ_CHUNK_QUANTUM 1024

#define TDEQ_EINVAL (-1)       /* bad argument (null pointer, n_terms out of range, bad dtype ...) */
#define TDEQ_EWORKSPACE (-2)   /* workspace too small */

/* Segment table entry (host memory, passed to the norm entry points). */
typedef struct tdeq_segment {
    int64_t chunk_start;   /* first chunk of the segment                        */
    int64_t numel;         /* valid elements in the segment                     */
    double rtol;           /* per-segment tolerances (misc.py:115-123 tuple tol) */
    double atol;
} tdeq_segment;

/*
 * Step-controller parameters of ONE adaptive trial step (host memory, copied into the kernel arguments).
 * Everything is a host double, as in the host loop (torchdiffeq_amd/solvers.py); the reference keeps the same
 * quantities as 0-dim fp64 device tensors (rk_common.py:186-194).
 */
#define TDEQ_MAX_STAGE_TIMES 16
typedef struct tdeq_step_ctrl {
    double t0;          /* start of the trial step, solver (ascending) time                                  */
    double dt;          /* its size, > 0, after the min_step / max_step clamp (rk_common.py:268-271)          */
    double safety;      /* misc.py:85-95 `_optimal_step_size` parameters (rk_common.py:172-174)               */
    double ifactor;
    double dfactor;
    double exponent;    /* 1 / order                                                                          */
    double min_step;
    double max_step;
    double time_sign;   /* +1, or -1 for a decreasing-time solve: user time = sign * solver time (misc.py:158-165) */
    double alpha[TDEQ_MAX_STAGE_TIMES];   /* stage abscissae of the tableau, already rounded to T (rk_common.py:201) */
    uint32_t alpha_is_one;                /* bit i set: stage i is evaluated at t1 with Perturb.PREV (rk_common.py:72-75) */
    int32_t n_times;    /* number of stages (func evaluations per step), 1..TDEQ_MAX_STAGE_TIMES               */
    int32_t n_norm_seg; /* leading segments that enter the max of the mixed norm (seminorm: adjoint.py:267-270) */
    int32_t leading_abs; /* 16-bit states only: segment 0, if it holds ONE element, enters the max as |x| itself instead of
                            its rms — the adjoint norms take their time component as `t.abs()` (adjoint.py:250, 273); for
                            fp32 / fp64 the two are the same number and the field is ignored */
} tdeq_step_ctrl;

/* ABI version of the loaded library (== TDEQ_ABI_VERSION). */
int tdeq_abi_version(void);

/* Bytes of device workspace the norm entry points need for a state of n_chunks chunks. */
size_t tdeq_workspace_bytes(int64_t n_chunks);

/*
 * Stage accumulate:  out = y0 + sum_j c_j * k_j ,  c_j = fl_T(fl_T(coef_j) * fl_T(dt)).
 * Replaces `yi = y0 + torch.sum(k[..., :i+1] * (beta_i * dt), dim=-1)` (rk_common.py:79), the
 * non-FSAL solution combine (rk_common.py:83-85) and `y1 = y0 + h0 * f0` of the initial-step
 * heuristic (misc.py:65).  Structural zeros of the tableau row are skipped by the caller.
 * 1 <= n_terms <= TDEQ_MAX_TERMS.  `out` may alias nothing it reads.
 */
int tdeq_stage_combine(void* out, const void* y0, const void* const* k, const double* coef,
                       int n_terms, double dt, int64_t n, int dtype, void* stream);

/*
 * Measurement hook: tdeq_stage_combine whose launch updates two caller-created hipEvent_t (enable-timing) with the
 * dispatch's own begin and end timestamps (hipExtLaunchKernelGGL), so that hipEventElapsedTime(start, stop) is the
 * kernel's duration as a profiler reports it — not the event -> launch -> event bracket, which adds ≈3 µs of
 * marker cost.  Same kernel, same results; 16-byte aligned buffers only (others take the plain launch and leave the
 * events untouched).  Used by bench.py for the live roofline figure of the dominant kernel.
 */
int tdeq_stage_combine_timed(void* out, const void* y0, const void* const* k, const double* coef, int n_terms,
                             double dt, int64_t n, int dtype, void* stream, void* start_event, void* stop_event);

/*
 * tdeq_stage_combine for the FIRST stage of a step (n_terms 1 or 2, n >= 1) that also stores `n_fill` (<= 16)
 * scalars, converted to T, at fill_dst[0..n_fill): the stage times `ti = t0 + alpha_i * dt` (rk_common.py:72-78)
 * that the following func evaluations read as 0-dim tensors.  Saves the separate tdeq_fill_scalars launch at the
 * latency-critical start of a step; results are identical to the two separate calls.
 */
int tdeq_stage_combine_fill(void* out, const void* y0, const void* const* k, const double* coef, int n_terms,
                            double dt, int64_t n, int dtype, void* fill_dst, const double* fill_vals, int n_fill,
                            void* stream);

/*
 * Embedded error estimate + tolerance scaling + per-segment sum of squares, fused:
 *   err = sum_j fl_T(coef_j*dt) * k_j                       (rk_common.py:89)
 *   tol = atol + rtol * max(|y0|, |y1|)                      (misc.py:81)
 *   out_sumsq[s]  = sum over segment s of (err/tol)^2        (misc.py:22-23, 30-33, 82; fp64 accumulate)
 *   out_nonfinite[s] = number of non-finite elements of y0/y1 seen in segment s (rk_common.py:287)
 * The caller finishes sqrt(sumsq/numel) and the max over segments on the host.
 * `out_sumsq` / `out_nonfinite` (n_seg doubles each) may be device memory or pinned host memory.
 * `scaled_out` (optional, may be NULL): if given, err/tol is also stored per element (padding of a
 * segmented layout zero-filled) so that a user-supplied norm callable can reduce it.
 * `segs` is the host segment table; for n_seg > TDEQ_INLINE_SEGMENTS the caller also passes
 * `segs_dev`, a device copy of the same n_seg records (made once per solve), else it may be NULL.
 */
int tdeq_error_norm(void* scaled_out, const void* y0, const void* y1, const void* const* k,
                    const double* coef, int n_terms, double dt, const tdeq_segment* segs,
                    const void* segs_dev, int n_seg, int64_t chunk, int64_t n_chunks,
                    double* out_sumsq, double* out_nonfinite, void* workspace,
                    size_t workspace_bytes, int dtype, void* stream);

/*
 * tdeq_error_norm for PER-ELEMENT tolerances: `rtol` / `atol` tensors that broadcast against the state (misc.py:80-82 —
 * the reference needs no code for it) or tuple tolerances with vector entries (flat vectors, misc.py:115-123).  A
 * dimensioned tolerance is a device vector of fp64 (the time dtype of rk_common.py:186-187) over the flat, padded state;
 * the other one may be 0-dim (`*_vec` NULL, value in `*_scalar`); at least one must be dimensioned.  Promotion as ATen
 * does it: rtol[i] * max(|y0|,|y1|) in fp64 when rtol is dimensioned, in T (rtol cast to T) when it is 0-dim; the sum
 * with atol, err / tol and the sum of squares in fp64.  The segment table's rtol / atol are ignored.
 * `err_partial` (nullable, ABI 20): the error row's leading run as tdeq_stage_combine_err summed it —
 * err = (err_partial + c_0 k_0) + ... over the n_terms >= 0 remaining stages, as tdeq_error_norm_partial; NULL: the whole row
 * from k (n_terms >= 1).
 */
int tdeq_error_norm_vec(const void* err_partial, const void* y0, const void* y1, const void* const* k, const double* coef,
                        int n_terms, double dt, const double* rtol_vec, double rtol_scalar, const double* atol_vec, double atol_scalar,
                        const tdeq_segment* segs, const void* segs_dev, int n_seg, int64_t chunk, int64_t n_chunks,
                        double* out_sumsq, double* out_nonfinite, void* workspace, size_t workspace_bytes, int dtype,
                        void* stream);

/*
 * tdeq_error_norm_vec whose finalize step also runs the step controller on the device (as tdeq_error_norm_partial_ctrl
 * does for scalar tolerances): the error ratio in fp64 — the promoted type of the reference's quotient and norm when a
 * tolerance is dimensioned —, accept flag, next step size, and the next trial step's stage times in T; `out_ctrl`,
 * `ctrl_dev`, `next_times` as there.  Lets the look-ahead first stage (tdeq_stage_combine_sel) follow.
 * state_in_dev != 0 (ABI 21, hipGraph mode, as for tdeq_error_norm_partial_ctrl): the trial step's (t0, dt) and the step
 * size the error row's coefficients are multiplied by live in ctrl_dev; `dt` is ignored and c = fl_T(fl_T(coef) * T(dt))
 * is formed on the device — captured trial steps with per-element tolerances.
 */
int tdeq_error_norm_vec_ctrl(const void* err_partial, const void* y0, const void* y1, const void* const* k,
                             const double* coef, int n_terms, double dt,
                             const double* rtol_vec, double rtol_scalar, const double* atol_vec, double atol_scalar,
                             const tdeq_segment* segs, const void* segs_dev, int n_seg, int64_t chunk, int64_t n_chunks,
                             double* out_sumsq, double* out_nonfinite, const tdeq_step_ctrl* ctrl, double* out_ctrl,
                             double* ctrl_dev, void* next_times, int state_in_dev, void* workspace, size_t workspace_bytes,
                             int dtype, void* stream);

/*
 * Fused pair for the END of a trial step (same results as tdeq_stage_combine + tdeq_error_norm, fewer bytes):
 *   tdeq_stage_combine_err   the step's last combine (last stage row, or the c_sol combine of a non-FSAL pair)
 *                            also stores  err_out = (e_0 k_0 + e_1 k_1) + ...,  e_j = fl_T(fl_T(err_coef_j)*fl_T(dt)),
 *                            the partial embedded error over the SAME stages, left to right (rk_common.py:89);
 *   tdeq_error_norm_partial  err = (err_partial + c_0 k_0) + ... over the 0..2 remaining stages (for an FSAL
 *                            pair: the last stage slot only), then tolerance scaling, per-segment sums and the
 *                            non-finite census exactly as tdeq_error_norm.
 * The caller uses the pair only when the fused stages are a leading run of the error row's non-zero entries, so
 * the left-to-right sum order (and therefore every bit of err) is unchanged.  Traffic per dopri5 step:
 * 40 -> 37 words per element (7+1 and 4 instead of 7 and 8); dopri8: 105 -> 98.
 */
int tdeq_stage_combine_err(void* out, void* err_out, const void* y0, const void* const* k, const double* coef,
                           const double* err_coef, int n_terms, double dt, int64_t n, int dtype, void* stream);
int tdeq_error_norm_partial(const void* err_partial, const void* y0, const void* y1, const void* const* k,
                            const double* coef, int n_terms, double dt, const tdeq_segment* segs,
                            const void* segs_dev, int n_seg, int64_t chunk, int64_t n_chunks, double* out_sumsq,
                            double* out_nonfinite, void* workspace, size_t workspace_bytes, int dtype,
                            void* stream);

/*
 * Carried partial sums (r03).  Every tableau row re-reads all earlier stages: row i of `_runge_kutta_step`
 * (rk_common.py:69-81) is  y_i = y0 + ((c_i0 k_0 + c_i1 k_1) + ... + c_ii k_i), summed left to right, so the stages a
 * LATER row r needs from k_0..k_i are in registers while row i is being formed.  This entry point makes ONE pass over
 * `n_terms` stage streams and produces up to TDEQ_MAX_MULTI_OUT outputs from them:
 *
 *     s_o    = [acc_in +] sum over the set bits j of mask_o, ascending, of  fl_T(fl_T(coef_o[j]) * fl_T(dt)) * k_j
 *     out_o  = add_y0_o ? y0 + s_o : s_o
 *
 * Output 0 is the row's own stage input; a further output with add_y0 = 0 is the left-to-right PREFIX of a later
 * row's sum (a "carried" partial sum), which that row's launch continues through `acc_in` (output 0 only) over the
 * stages computed since — it then reads acc_in, the new stages and y0 instead of every earlier stage; a further
 * output with add_y0 = 1 is a later stage input that needs no newer stage at all (dopri8 row 12, whose weight on
 * k_11 is zero: dopri8.py:5-70) and is finished here.  The partial embedded error of tdeq_stage_combine_err is the
 * same thing (add_y0 = 0, continued by tdeq_error_norm_partial).  Rounding sequence = the one of tdeq_stage_combine
 * (first product not added to a zero, structural zeros skipped — not multiplied —, products and sums rounded
 * separately in T), so every output is BIT-IDENTICAL to the row-by-row kernels; only the bytes change:
 * dopri8 98 -> 75 words per element and step (13 launches instead of 14), dopri5 37 -> 35 (tableaus.carry_plan).
 * 1 <= n_terms <= TDEQ_MAX_TERMS, 1 <= n_out <= TDEQ_MAX_MULTI_OUT, every mask non-zero and within n_terms bits;
 * `acc_in` may be NULL.  Outputs may alias nothing that is read.
 */
#define TDEQ_MAX_MULTI_OUT 4
/* streaming launches whose streams add up to more than this many MiB use non-temporal loads and stores (tdeq_abi.hip
 * stream_policy; TDEQ_NT_THRESHOLD_MB overrides, TDEQ_COMBINE_POLICY=0..3 forces one policy) */
#define TDEQ_NT_THRESHOLD_DEFAULT_MB 512
typedef struct tdeq_multi_out {
    void* out;                      /* T[n]                                                                   */
    double coef[TDEQ_MAX_TERMS];    /* fp64 tableau weights of this output's row over the n_terms streams       */
    uint32_t mask;                  /* bit j set: stream j takes part in this output's sum                      */
    int32_t add_y0;                 /* 1: out = y0 + sum (a finished stage input); 0: out = sum (a partial sum) */
} tdeq_multi_out;
int tdeq_stage_combine_multi(const tdeq_multi_out* outs, int n_out, const void* y0, const void* acc_in,
                             const void* const* k, int n_terms, double dt, int64_t n, int dtype, void* stream);
/* hipGraph mode: the step size is ctrl_dev[1] (sign * T(dt), maintained by tdeq_error_norm_partial_ctrl with
 * state_in_dev = 1), read on the device; c = fl_T(fl_T(coef) * T(dt)) as above, same bits as the host-dt entry point. */
int tdeq_stage_combine_multi_dev(const tdeq_multi_out* outs, int n_out, const void* y0, const void* acc_in,
                                 const void* const* k, int n_terms, const double* ctrl_dev, int64_t n, int dtype,
                                 void* stream);
/* Measurement hook, as tdeq_stage_combine_timed: the dispatch stamps the two events with its own begin / end. */
int tdeq_stage_combine_multi_timed(const tdeq_multi_out* outs, int n_out, const void* y0, const void* acc_in,
                                   const void* const* k, int n_terms, double dt, int64_t n, int dtype, void* stream,
                                   void* start_event, void* stop_event);

/*
 * Device-resident step controller + look-ahead first stage.  The accept/reject LOOP stays on the host; what
 * moves to the device is the scalar decision of one trial step, so that the next trial step's first stage
 * (and the func evaluation behind it) can be enqueued BEFORE the host has read the decision back — the
 * poll -> controller -> launch latency of the host leaves the critical path.
 *
 *   tdeq_error_norm_partial_ctrl   = tdeq_error_norm_partial (same partial kernel, same per-segment sums in the
 *       same order) whose finalize step, one workgroup, also runs the reference's controller on the sums:
 *         ratio  = max_s sqrt(sumsq_s / numel_s) over the first n_norm_seg segments, rounded to T
 *                                                                                (misc.py:22-33, 80-82)
 *         accept = ratio <= 1, overridden by dt > max_step -> reject, dt <= min_step -> accept
 *                                                                                (rk_common.py:324-330)
 *         dt_next = clamp(_optimal_step_size(dt, ratio, safety, ifactor, dfactor, order), min_step, max_step)
 *                                                                                (misc.py:85-95, rk_common.py:353)
 *         next trial step: t0' = accept ? t0 + dt : t0 ; dt' = dt_next (min_step if non-finite);
 *         stage times t_i = t0' + alpha_i dt' in T, or nextafter(t1, t1 - 1) with t1 = T(t0' + dt') for alpha_i == 1
 *         (Perturb.PREV), times the time sign                                    (rk_common.py:72-78, misc.py:174-197)
 *       Outputs: out_sumsq / out_nonfinite as tdeq_error_norm_partial; out_ctrl[4] = {accept (0/1), dt_next,
 *       ratio, t0'} (device or pinned host memory, read by the host loop); ctrl_dev[4] = {accept, sign * T(dt'),
 *       t0', dt'} (device memory, read by tdeq_stage_combine_sel and by the hipGraph-mode kernels);
 *       next_times[n_times] (device memory, element type T) = the 0-dim time tensors the next trial step hands to
 *       func.  More than TDEQ_INLINE_SEGMENTS segments (segs_dev required, as for tdeq_error_norm): the sums come
 *       from the parallel per-segment finalize launch and the one-workgroup controller runs on them (one launch
 *       more; same sums, same decision).  state_in_dev != 0 (hipGraph mode, below): ctrl->t0 / ctrl->dt and
 *       the `dt` argument are ignored — the trial step's (t0, dt) are ctrl_dev[2..3] and the error coefficients are
 *       scaled by ctrl_dev[1], all left there by the previous call (or by the host before the first one).
 *       copy_last_k (ABI 21, nullable; fp32 / fp64 states, n_terms >= 1): the last remaining stage k[n_terms - 1] — the
 *       step's f1 = f(t1, y1) for an FSAL pair — is ALSO written to this buffer by the norm launch, which has the
 *       stream in registers: a captured trial step whose next step must read f1 from a buffer of its own (func's output
 *       buffer cannot be chosen) saves the N-word copy node.
 *
 *   tdeq_stage_combine_sel   first stage of the next trial step, launched before the host knows `accept`:
 *         (y, f) = accept ? (y_acc, f_acc) : (y_rej, f_rej) ;  out = y + fl_T(fl_T(coef) * T(dt')) * f
 *       i.e. tdeq_stage_combine with one term on the pair the controller selected (accepted: the new state and
 *       its FSAL derivative; rejected: the old pair, rk_common.py:335-361) and the controller's dt'.
 *       Bit-identical to the host-driven tdeq_stage_combine call it replaces.
 */
int tdeq_error_norm_partial_ctrl(const void* err_partial, const void* y0, const void* y1, const void* const* k,
                                 const double* coef, int n_terms, double dt, const tdeq_segment* segs,
                                 const void* segs_dev, int n_seg, int64_t chunk, int64_t n_chunks, double* out_sumsq,
                                 double* out_nonfinite, const tdeq_step_ctrl* ctrl, double* out_ctrl, double* ctrl_dev,
                                 void* next_times, int state_in_dev, void* copy_last_k, void* workspace,
                                 size_t workspace_bytes, int dtype, void* stream);
int tdeq_stage_combine_sel(void* out, const void* y_acc, const void* f_acc, const void* y_rej, const void* f_rej,
                           double coef, const double* ctrl_dev, int64_t n, int dtype, void* stream);

/*
 * The controller alone, on per-segment sums that already sit in DEVICE memory — the lock-step mode of a batch-sharded
 * solve (no counterpart in the reference, which has no distributed code): every rank runs tdeq_error_norm_partial
 * into device buffers, the n_seg sums (+ non-finite counters) are all-reduced over the ranks ON THE DEVICE (RCCL over
 * xGMI, no host round trip), and this entry point then takes the same decision on every rank:
 *   ratio = max_s sqrt(sums[s] / segs[s].numel) over the first n_norm_seg segments — `segs[s].numel` must hold the
 *   GLOBAL element counts (summed over the ranks) — then accept / dt_next / next stage times exactly as
 *   tdeq_error_norm_partial_ctrl.  sums / nonfinite are mirrored to out_sumsq / out_nonfinite (device or pinned host
 *   memory) for the host's bookkeeping; the other outputs as tdeq_error_norm_partial_ctrl.  Only `numel` of the
 *   segment table is read (segs_dev required beyond TDEQ_INLINE_SEGMENTS segments).
 */
int tdeq_step_controller(const double* sums, const double* nonfinite, const tdeq_segment* segs, const void* segs_dev,
                         int n_seg, double* out_sumsq, double* out_nonfinite, const tdeq_step_ctrl* ctrl,
                         double* out_ctrl, double* ctrl_dev, void* next_times, int state_in_dev, int dtype,
                         void* stream);

/*
 * hipGraph mode of the adaptive solvers (small states, where a trial step is launch-latency-bound): ONE captured
 * graph = one trial step (S func evaluations, S + 4 launches) is replayed until the solve ends; the step size
 * lives in device memory (ctrl_dev, maintained by tdeq_error_norm_partial_ctrl with state_in_dev = 1) and the
 * state in static buffers.
 *   tdeq_stage_combine_dev  tdeq_stage_combine (err_out == NULL) or tdeq_stage_combine_err with
 *                           c_j = fl_T(fl_T(coef_j) * T(dt)), dt = ctrl_dev[1] read on the device; same operation
 *                           order, same results as the host-dt entry points (from 2^17 elements on with the same
 *                           unrolled, 16-byte-per-lane streams; below, one run-time-term kernel: launch-bound anyway).
 *   tdeq_step_commit        if ctrl_dev[0] (accept): (y_prev, f_prev) <- (y_cur, f_cur); (y_cur, f_cur) <- (y1, f1)
 *                           — the accepted state becomes the next trial's base (rk_common.py:335-352) and the
 *                           previous pair stays available for the dense output of the step just taken.
 *                           For callers that keep ONE captured graph and let the device select the pair.  The package's
 *                           own host (solvers._GraphStep, r03) no longer needs it: it reads the decision after every
 *                           replay anyway and alternates between two graphs over ping-pong buffers instead (no copy).
 */
int tdeq_stage_combine_dev(void* out, void* err_out, const void* y0, const void* const* k, const double* coef,
                           const double* err_coef, int n_terms, const double* ctrl_dev, int64_t n, int dtype,
                           void* stream);
int tdeq_step_commit(void* y_prev, void* f_prev, void* y_cur, void* f_cur, const void* y1, const void* f1,
                     const double* ctrl_dev, int64_t n, int dtype, void* stream);

/*
 * Initial-step norms (Hairer II.4 as in misc.py:36-77), scale = atol + |y0| * rtol:
 *   mode 0:  out_sumsq[s]          = sum (a / scale)^2           (a = y0 -> d0 ; misc.py:55)
 *            out_sumsq[n_seg + s]  = sum (b / scale)^2           (b = f0 -> d1 ; misc.py:56)
 *   mode 1:  out_sumsq[s]          = sum ((a - b) / scale)^2     (a = f1, b = f0 -> d2*h0 ; misc.py:68)
 * out_nonfinite[s] counts non-finite elements of yscale (the state) per segment.
 */
int tdeq_init_norms(int mode, const void* a, const void* b, const void* yscale,
                    const tdeq_segment* segs, const void* segs_dev, int n_seg, int64_t chunk,
                    int64_t n_chunks, double* out_sumsq, double* out_nonfinite, void* workspace, size_t workspace_bytes,
                    int dtype, void* stream);

/*
 * tdeq_init_norms with PER-ELEMENT tolerances (ABI 21): `rtol_vec` / `atol_vec` = fp64 device vectors over the flat (padded)
 * state, or NULL with the 0-dim value in `rtol_scalar` / `atol_scalar` (at least one vector) — what misc.py:50-56,68
 * computes by broadcasting when the caller's tolerances are tensors (rk_common.py:186-187 makes them W = fp64 tensors).
 * Promotion as ATen applies it: |y| * rtol[i] in fp64 for a dimensioned rtol, in T for a 0-dim one; the sum with atol,
 * the quotients and the sums of squares in fp64; (a - b) of mode 1 in T.  fp32 / fp64 states; outputs as tdeq_init_norms.
 */
int tdeq_init_norms_vec(int mode, const void* a, const void* b, const void* yscale, const double* rtol_vec,
                        double rtol_scalar, const double* atol_vec, double atol_scalar, const tdeq_segment* segs,
                        const void* segs_dev, int n_seg, int64_t chunk, int64_t n_chunks, double* out_sumsq,
                        double* out_nonfinite, void* workspace, size_t workspace_bytes, int dtype, void* stream);

/*
 * The quotients of tdeq_init_norms MATERIALISED, for a user-supplied norm callable (the reference hands its `norm`
 * to _select_initial_step too, rk_common.py:217 -> misc.py:55-56,68):
 *   mode 0: out0 = a / scale, out1 = b / scale          mode 1: out0 = (a - b) / scale      (out1 may be NULL)
 * element-wise over the segments; the padding of a segmented layout is zero-filled.
 */
int tdeq_init_scaled(int mode, const void* a, const void* b, const void* yscale, const tdeq_segment* segs,
                     const void* segs_dev, int n_seg, int64_t chunk, int64_t n_chunks, void* out0, void* out1,
                     int dtype, void* stream);

/*
 * Dense output, fused fit + evaluate (rk_common.py:363-369 + interp.py:1-48):
 *   y_mid = y0 + sum_j fl_T(coef_j*dt) * k_j ; quartic [e,d,c,b,a] from (y0,y1,y_mid,f0,f1,dt);
 *   out = e + x d + x^2 c + x^3 b + x^4 a, with x already rounded to T by the caller.
 * f0 / f1 are the first / last stage slots (k[...,0], k[...,-1]).
 */
int tdeq_dense_eval(void* out, const void* y0, const void* y1, const void* f0, const void* f1,
                    const void* const* k, const double* coef, int n_terms, double dt, double x,
                    int64_t n, int dtype, void* stream);

/*
 * tdeq_dense_eval for n_x (1..TDEQ_MAX_DENSE_OUTPUTS) output times that fall inside the SAME accepted step — the
 * reference calls _interp_evaluate once per output time (solvers.py:28-35 -> rk_common.py:243-250): the quartic is
 * fitted once per element and evaluated at x[0..n_x); row q is written at out + q*out_stride elements (the rows of
 * the solution tensor).  (8 + n_x) words per element instead of 9*n_x, one launch instead of n_x; each row is
 * bit-identical to the single-output call.
 */
int tdeq_dense_eval_multi(void* out, int64_t out_stride, const void* y0, const void* y1, const void* f0,
                          const void* f1, const void* const* k, const double* coef, int n_terms, double dt,
                          const double* x, int n_x, int64_t n, int dtype, void* stream);

/*
 * Dense-output fit only: writes the 5 interpolation coefficients [e,d,c,b,a] contiguously into
 * `coeffs` (5*n elements; interp.py:17-22).  Used by odeint_dense-style consumers ("next" row).
 */
int tdeq_interp_fit(void* coeffs, const void* y0, const void* y1, const void* f0, const void* f1,
                    const void* const* k, const double* coef, int n_terms, double dt, int64_t n,
                    int dtype, void* stream);

/*
 * rk4 "3/8 rule" stages (rk_common.py:110-118, solvers.py:115), dt already in T:
 *   stage 1: out = y0 + (dt*k1)*(1/3)
 *   stage 2: out = y0 + dt*(k2 - k1*(1/3))
 *   stage 3: out = y0 + dt*((k1 - k2) + k3)
 *   stage 4: out = y0 + (((k1 + 3*(k2+k3)) + k4)*dt)*0.125
 * Unused k pointers may be NULL.
 */
int tdeq_rk4_38_stage(int stage, void* out, const void* y0, const void* k1, const void* k2,
                      const void* k3, const void* k4, double dt, int64_t n, int dtype, void* stream);

/*
 * hipGraph mode of the fixed-grid rk4 solver (small states, where a step is launch-latency-bound): ONE captured
 * graph — four func evaluations, four tdeq_rk4_38_stage_dev launches, tdeq_grid_commit, tdeq_grid_advance — is
 * replayed once per grid interval; everything that changes between steps lives in device memory.
 *   tdeq_rk4_38_stage_dev  tdeq_rk4_38_stage with dt read from *dt_dev (device double holding sign*dt).
 *   tdeq_grid_advance      *counter += 1 (=: c); t0 = grid[c], t1 = grid[c+1], dt = t1 - t0 in the grid's dtype
 *                          (solvers.py:110-112); times_out[0..4) = the stage times t0, t0 + dt/3, t0 + 2dt/3, t1 of
 *                          the 3/8 rule (rk_common.py:110-118) cast to the state dtype, perturbed at both ends if
 *                          `perturb` (fixed-grid option, misc.py:174-197), times `sign`; *dt_out = sign * dt.
 *                          Nothing is written when c + 1 >= n_grid.  Start with *counter = -1.
 *   tdeq_grid_commit       solution[(*counter + 1) * row_stride + i] = y_new[i] and y_cur[i] = y_new[i], i < n: the
 *                          step's result becomes output row c + 1 and the next step's state (solvers.py:113-127
 *                          with the grid equal to the output times).
 */
int tdeq_rk4_38_stage_dev(int stage, void* out, const void* y0, const void* k1, const void* k2, const void* k3,
                          const void* k4, const double* dt_dev, int64_t n, int dtype, void* stream);
int tdeq_grid_advance(const void* grid, int grid_dtype, int64_t n_grid, int64_t* counter, int perturb, double sign,
                      void* times_out, double* dt_out, int state_dtype, void* stream);
int tdeq_grid_commit(void* solution, int64_t row_stride, void* y_cur, const void* y_new, const int64_t* counter,
                     int64_t n, int dtype, void* stream);
/*
 * hipGraph mode of the OTHER explicit fixed-grid methods (r03: euler, midpoint, heun2, heun3; fixed_grid.py:6-60,
 * rk_common.py:121-157) — the same scheme as tdeq_grid_advance / tdeq_rk4_38_stage_dev with the method described by data:
 *   tdeq_grid_advance_stages  counter += 1; t0 = grid[c], t1 = grid[c+1], dt = t1 - t0 in the grid's dtype; stage time i
 *                             = t1 if (mode_i & 1) else t0 + dt * fl_G(frac_i)  (t0 itself for frac_i = 0), cast to the
 *                             state dtype, perturbed to the NEXT (mode_i & 2) / PREVIOUS (mode_i & 4) representable value
 *                             when `perturb`, times `sign`; dt_out = sign * dt.  1 <= n_times <= 4.
 *   tdeq_fixed_stage_dev      tdeq_fixed_stage with the step size read from device memory (*dt_dev, rounded to T).
 * Euler's and midpoint's stages are tdeq_stage_combine_dev (whose ctrl_dev[1] is this dt_out).  Same operation order as the
 * host-dt entry points, so a captured step replays the eager step bit for bit.
 */
int tdeq_grid_advance_stages(const void* grid, int grid_dtype, int64_t n_grid, int64_t* counter, int perturb, double sign,
                             const double* frac, const int* mode, int n_times, void* times_out, double* dt_out,
                             int state_dtype, void* stream);
int tdeq_fixed_stage_dev(int mode, void* out, const void* y0, const void* const* k, const double* w, int n_terms,
                         const double* dt_dev, int64_t n, int dtype, void* stream);

/* Fixed-grid output interpolation  out = y0 + slope*(y1 - y0)  (solvers.py:175-181). */
int tdeq_lerp(void* out, const void* y0, const void* y1, double slope, int64_t n, int dtype,
              void* stream);

/*
 * Low-order fixed-grid Runge–Kutta stages with the reference's operation order (euler / midpoint use
 * tdeq_stage_combine, which is bit-identical for their single-term forms).  w_j and dt rounded to T:
 *   mode 0: out = y0 + dt * ((k0*w0 + k1*w1) + ...)   `y0 + dt * (k1*a31 + k2*a32)`, and y1 = y0 + dy with
 *                                                    dy = `dt * (k1*b1 + k2*b2 [+ k3*b3])`
 *                                                    (rk_common.py:139,140,156,157; solvers.py:115)
 *   mode 1: out = y0 + (dt * k0) * w0                 `y0 + dt * k1 * a21` (rk_common.py:138,156); n_terms == 1
 * 1 <= n_terms <= 4; structural zeros are skipped by the caller (heun2 / heun3, fixed_grid.py:32-60).
 */
int tdeq_fixed_stage(int mode, void* out, const void* y0, const void* const* k, const double* w, int n_terms,
                     double dt, int64_t n, int dtype, void* stream);

/*
 * out = (x0*w0 + x1*w1) + ... (left to right, w_j rounded to T), 1 <= n_terms <= TDEQ_MAX_SUM_TERMS.
 * Cubic Hermite output interpolation of the fixed-grid solvers,
 * `h00*y0 + h10*dt*f0 + h01*y1 + h11*dt*f1` (solvers.py:166-173), with the scalar products formed by the host.
 */
int tdeq_weighted_sum(void* out, const void* const* x, const double* w, int n_terms, int64_t n, int dtype,
                      void* stream);

/*
 * Backward helpers of the differentiable plain `odeint`.  Every elementwise entry
 * point above computes out = sum_m w_m(dt, x) * X_m, so the vector-Jacobian product the reference obtains
 * from autograd over its eager ops (incl. `_UncheckedAssign.backward`, rk_common.py:31-40) is:
 *   grad X_m = w_m * g                            tdeq_scale_many: g is read once, n_out tensors are written
 *   grad s   = sum_m dw_m/ds * <g, X_m>           tdeq_multi_dot: out[m] = <g, x_m> in fp64 (device memory),
 *                                                 for the time-like scalars s = dt, x when `t` requires grad
 * 1 <= n_out, n_x <= TDEQ_MAX_TERMS.  tdeq_multi_dot needs tdeq_dots_workspace_bytes(n, n_x) bytes of device
 * workspace; n == 0 yields zeros.
 */
int tdeq_scale_many(void* const* outs, const void* g, const double* w, int n_out, int64_t n, int dtype,
                    void* stream);
size_t tdeq_dots_workspace_bytes(int64_t n, int n_x);
int tdeq_multi_dot(const void* g, const void* const* x, int n_x, int64_t n, double* out, void* workspace,
                   size_t workspace_bytes, int dtype, void* stream);

/*
 * Pack the pieces of a tuple-valued func output into ONE flat segmented state with one launch:
 *   out[chunk_start[s]*chunk + i] = scale[s] * src[s][i]   for i < numel[s];   padding and src[s] == NULL -> 0
 * over n_chunks*chunk elements of `out`.  Replaces `torch.cat([f_.reshape(-1) for f_ in f])` of _TupleFunc
 * (misc.py:137-145) and, for the adjoint's augmented dynamics (adjoint.py:72-105), also the `-adj_y` negation (:95),
 * the zeros_like of absent gradients (:99-103) and _ReverseFunc's multiply (misc.py:158-165): scale[s] is +1 or -1,
 * so every product is exact.  src[s]: contiguous, element type T, numel[s] elements.  1 <= n_seg <=
 * TDEQ_INLINE_SEGMENTS, chunk_start[0] == 0 and strictly increasing, numel[s] <= room of segment s.
 */
int tdeq_pack_segments(void* out, const void* const* src, const int64_t* chunk_start, const int64_t* numel,
                       const double* scale, int n_seg, int64_t chunk, int64_t n_chunks, int dtype, void* stream);

/* Writes n_vals scalars (converted to T) to consecutive elements of dst (stage times for func). */
int tdeq_fill_scalars(void* dst, const double* vals, int n_vals, int dtype, void* stream);

/*
 * Adams–Bashforth(–Moulton) multistep steps of the fixed-grid solvers `explicit_adams`, `implicit_adams`
 * (= `fixed_adams`), fixed_adams.py:164-228.  f_hist[j] = func output at t_{n-j} (newest first, separate
 * contiguous tensors — the reference's deque `prev_f`), 1 <= n_terms <= TDEQ_MAX_TERMS (the reference uses 3..11).
 *
 * tdeq_adams_predict — one pass over the history:
 *   dy    = (cb_0*f_0 + cb_1*f_1) + ...       `_dot_product(dt * bashforth_coeffs, prev_f)` (:205); the caller passes
 *                                             cb_j = dt*b_j formed in fp64, rounded to T here (0-dim fp64 x T tensor)
 *   y_out = y0 + dy                           (:213 / solvers.py:115)
 *   delta = T(dt) * ((cm_0*f_0 + cm_1*f_1) + ...)   `dt * _dot_product(moulton_coeffs[1:], prev_f)` (:210), cm_j = m_{j+1}
 * dy_out / delta_out / cm are given together (implicit method) or all NULL (explicit method).
 *
 * tdeq_adams_correct — one corrector iteration and its convergence test in one pass (:212-216, :189-192):
 *   compute != 0:  dy = T(c)*f + delta (c = dt*m_0 formed in fp64 by the caller), dy_out = dy, y_out = y0 + dy
 *   compute == 0:  dy is read from dy_out (test only; y_out, f, delta, y0 unused)
 *   out_count[s]      = number of elements of segment s with NOT (|dy_old - dy| / (atol_s + rtol_s*max(|dy_old|,|dy|)) < 1)
 *                       — `_has_converged` (l-inf norm of the error ratio < 1, misc.py:80-82) <=> all counts are 0
 *   out_nonfinite[s]  = number of non-finite elements of dy in segment s
 * Segment table, workspace (tdeq_workspace_bytes(n_chunks)) and result placement as for tdeq_error_norm; n = number of
 * elements of every buffer (>= the end of the last segment; the padding of a segmented state is written, not counted).
 */
int tdeq_adams_predict(void* y_out, void* dy_out, void* delta_out, const void* y0, const void* const* f_hist,
                       const double* cb, const double* cm, int n_terms, double dt, int64_t n, int dtype,
                       void* stream);
int tdeq_adams_correct(void* y_out, void* dy_out, const void* f, const void* delta, const void* dy_old,
                       const void* y0, double c, int compute, const tdeq_segment* segs, const void* segs_dev,
                       int n_seg, int64_t chunk, int64_t n_chunks, int64_t n, double* out_count,
                       double* out_nonfinite, void* workspace, size_t workspace_bytes, int dtype, void* stream);

/*
 * ---- Per-row step control (since ABI 22; torchdiffeq_amd/rowwise.py `odeint_rowwise`) ----
 * The state is [n_rows, row_len] row-major (fp32 / fp64 only); every row is its own IVP with its own step controller.
 * Per-row device vectors (length n_rows) carry the controller state; the entry points below read and update them.
 *
 * tdeq_row_partials     fp64 partials per row of the row reductions (1 for rows up to 1024 16-byte elements); the
 *                       reduction buffer `part` holds 3 * n_rows * that many doubles.  A function of (row_len, dtype)
 *                       only: a row is reduced the same way in a batch of any size.
 * tdeq_row_combine      tdeq_stage_combine_multi with the step size of each element's row: coefficient
 *                       fl_T(fl_T(coef) * dts[r]), dts = sign * T(dt_r).  Rows with active[r] == 0 read no stage:
 *                       outputs with add_y0 get y0, the others 0.
 * tdeq_row_reduce       mode 0: the embedded error [partial +] sum_j fl_T(fl_T(coef_j) dts[r]) k_j and per row the fp64 sum
 *                       of (err / (atol + rtol max(|y0|, |y1|)))^2 and the count of non-finite y0 / y1 entries (inactive
 *                       rows: 0).  mode 1 / 2: tdeq_init_norms' MODE 0 / 1 per row with a = y1, b = partial, y = y0.
 * tdeq_row_control      per row: the sums of `part` -> mode 0: error ratio, accept / reject, next dt, output range, counters;
 *                       mode 1: h0 of the initial-step heuristic (dts_out = sign * T(h0), times_out[0] = time of f(t0 + h0));
 *                       mode 2: first step = min(100 h0, h1); mode 3: dt given, non-finite census only.  Then, for rows still
 *                       active (modes 0, 2, 3), the next trial step: dt clamp, dts_out, stage times times_out[n_times, n_rows]
 *                       and the row's error code (2 max_num_steps, 1 dt underflow, 3 non-finite y).  status[0] = active
 *                       rows, status[1] = smallest row with a non-zero code (0x7fffffff: none).
 * tdeq_row_dense_commit for each row whose trial step was accepted: the quartic dense output at output times
 *                       out_lo[r] .. out_hi[r] - 1 into sol[j, r, :], then y0 <- y1, f0 <- f1.
 */
typedef struct tdeq_row_state {
    double* t0;            /* [n_rows] start of the next trial step (solver time)                     */
    double* tprev;         /* [n_rows] start of the last accepted step                                */
    double* dt;            /* [n_rows] size of the next trial step                                    */
    double* h0;            /* [n_rows] initial-step heuristic                                         */
    const double* tgrid;   /* [n_out, n_rows] output times (solver time)                              */
    int32_t* active;
    int32_t* accepted;
    int32_t* out_lo;
    int32_t* out_hi;
    int32_t* next_out;
    int32_t* since;        /* trial steps since the row last reached an output time                   */
    int32_t* bad_y;
    int32_t* code;
    int64_t* n_acc;
    int64_t* n_rej;
    double* ratio;         /* [n_rows] last error ratio                                               */
    int32_t* status;       /* [2]; [3] for tdeq_row_control_points                                    */
    int64_t n_rows;
    int64_t row_len;
    int64_t max_num_steps;
    int32_t n_out;
    int32_t order;         /* the solver's order - 1 (initial-step heuristic)                         */
} tdeq_row_state;

int64_t tdeq_row_partials(int64_t row_len, int dtype);
int tdeq_row_combine(const tdeq_multi_out* outs, int n_out, const void* y0, const void* acc_in, const void* const* k,
                     int n_terms, const void* dts, const int32_t* active, int64_t n_rows, int64_t row_len, int dtype,
                     void* stream);
int tdeq_row_reduce(int mode, const void* y0, const void* y1, const void* partial, const void* const* k,
                    const double* coef, int n_terms, const void* dts, const int32_t* active, double rtol, double atol,
                    int64_t n_rows, int64_t row_len, double* part, size_t part_bytes, int dtype, void* stream);
int tdeq_row_control(int mode, const double* part, const tdeq_step_ctrl* ctrl, const tdeq_row_state* st,
                     void* dts_out, void* times_out, int dtype, void* stream);
int tdeq_row_dense_commit(void* sol, void* y0, const void* y1, void* f0, const void* f1, const void* const* k,
                          const double* coef, int n_terms, const void* dts, const tdeq_row_state* st, int dtype,
                          void* stream);

/*
 * ---- Backward of the row-linear operations (ABI 23; torchdiffeq_amd/rowwise_autodiff.py, `differentiable=True`) ----
 * Every state-sized operation of a rowwise trial step is out[r, :] = sum_m w_m[r] X_m[r, :] with one weight per row.
 *
 * tdeq_row_scale_many   outs[m][r, e] = w[m * n_rows + r] * g[r, e] (one rounding), m < n_out <= TDEQ_MAX_TERMS; `w` is a
 *                       device [n_out, n_rows] tensor of the state type; g is read once.
 * tdeq_row_multi_dot    out[m * n_rows + r] = sum_e g[r, e] * x[m][r, e] accumulated in fp64, m < n_x <= TDEQ_MAX_TERMS,
 *                       with the reduction geometry of tdeq_row_reduce: a row's dot has the same bits in a batch of
 *                       any size.  Rows of more than one partial (tdeq_row_partials) need a workspace of
 *                       tdeq_row_dots_workspace_bytes (0 for short rows: `workspace` may then be NULL); 16-byte aligned
 *                       tensors whenever row_len is a multiple of 16 / sizeof(T).
 * n_rows == 0: no-op.  row_len == 0: scale_many is a no-op, multi_dot writes zeros.
 */
int tdeq_row_scale_many(void* const* outs, int n_out, const void* g, const void* w, int64_t n_rows, int64_t row_len,
                        int dtype, void* stream);
size_t tdeq_row_dots_workspace_bytes(int64_t n_rows, int64_t row_len, int n_x, int dtype);
int tdeq_row_multi_dot(const void* g, const void* const* x, int n_x, int64_t n_rows, int64_t row_len, double* out,
                       void* workspace, size_t workspace_bytes, int dtype, void* stream);

/*
 * ---- Compaction of a rowwise batch (ABI 24; `odeint_rowwise(compact=...)`) ----
 * tdeq_row_gather               dst[m][q, e] = src[m][idx[q], e] for q < n_idx, e < row_len, m < n_src (1 .. 4), all in one
 *                               launch; a copy of bits.  16-byte elements when row_len is a multiple of 16 / sizeof(T) and
 *                               every pointer is 16-byte aligned, scalar elements otherwise.  Every idx[q] must be a row of
 *                               every src[m]; dst[m] holds n_idx rows and must not overlap any src.  n_idx == 0: no-op.
 * tdeq_row_dense_commit_mapped  tdeq_row_dense_commit for a compacted batch: the state tensors and `st` hold st->n_rows
 *                               compact rows, `sol` is [n_out, sol_rows, row_len], and the outputs of compact row r go to
 *                               sol[j, row_map[r], :] (0 <= row_map[r] < sol_rows); y0 <- y1, f0 <- f1 at the compact index.
 */
int tdeq_row_gather(void* const* dst, const void* const* src, int n_src, const int32_t* idx, int64_t n_idx,
                    int64_t row_len, int dtype, void* stream);
int tdeq_row_dense_commit_mapped(void* sol, const int32_t* row_map, int64_t sol_rows, void* y0, const void* y1, void* f0,
                                 const void* f1, const void* const* k, const double* coef, int n_terms, const void* dts,
                                 const tdeq_row_state* st, int dtype, void* stream);

/*
 * ---- Per-row tolerances of the row reductions (ABI 25; `odeint_rowwise(rtol=[B], atol=[B])`) ----
 * tdeq_row_reduce_tol   tdeq_row_reduce with a tolerance pair per row: `rtol_rows`, `atol_rows` are device vectors
 *                       [n_rows] of the state type (already rounded to it), and row r is reduced with rtol_rows[r],
 *                       atol_rows[r] in every mode.  Same argument checks (a NULL tolerance pointer: TDEQ_EINVAL), same
 *                       geometry, same layout of `part`, same element arithmetic: with rtol_rows[r] = T(rtol) and
 *                       atol_rows[r] = T(atol) for every r it writes the bits of tdeq_row_reduce(rtol, atol), and a row's
 *                       words do not depend on the tolerances of the other rows.  Per-element tolerances inside a row are
 *                       not offered.
 */
int tdeq_row_reduce_tol(int mode, const void* y0, const void* y1, const void* partial, const void* const* k,
                        const double* coef, int n_terms, const void* dts, const int32_t* active, const void* rtol_rows,
                        const void* atol_rows, int64_t n_rows, int64_t row_len, double* part, size_t part_bytes, int dtype,
                        void* stream);

/*
 * ---- Per-row terminal events (ABI 26; torchdiffeq_amd/rowwise_event.py `odeint_rowwise_event`) ----
 * tdeq_row_event_detect  after tdeq_row_control(mode 0), one lane per row.  `g1` [n_rows] of the state type holds the event
 *                        value at the end of each row's trial step, `sign0` [n_rows] the row's starting sign, sign(g) =
 *                        (g > 0) - (g < 0) (0 for a NaN).  A row with accepted[r] && !fired[r] && sign(g1[r]) != sign0[r]
 *                        fires: fired[r] = fired_now[r] = 1, lo[r] = tprev[r], hi[r] = t0[r]; if it is still active,
 *                        active[r] = 0, status[0] -= 1 and `dts` [n_rows] / `times` [n_times, n_rows] — the buffers the
 *                        controller just wrote for the next trial step — are frozen as for a finished row (0 and
 *                        time_sign * T(t0[r])).  Every other row gets fired_now[r] = 0 and nothing else.  `ctrl` gives
 *                        n_times and time_sign.
 * tdeq_row_event_fit     for the rows with fired_now[r]: the quartic of the step (y0, y1, f0, f1, the mid-point stages `k`
 *                        with fl_T(fl_T(coef_j) * dts[r])) as tdeq_row_dense_commit forms it, its coefficients e, d, c, b, a
 *                        stored at q[j, r, :] of a [5, n_rows, row_len] buffer.  Other rows are neither read nor written.
 *                        Runs before the commit, which overwrites y0 and f0.
 * tdeq_row_event_eval    out[r, :] = the quartic q[:, r, :] at x[r] (`x` [n_rows] of the state type) for the rows with
 *                        mask[r]; other rows of `out` are untouched.
 * 16-byte elements when row_len is a multiple of 16 / sizeof(T) and every state-sized pointer is 16-byte aligned, scalar
 * elements otherwise.  n_rows == 0: no-op.
 */
int tdeq_row_event_detect(const void* g1, const int32_t* sign0, const tdeq_step_ctrl* ctrl, const tdeq_row_state* st,
                          void* dts, void* times, int32_t* fired, int32_t* fired_now, double* lo, double* hi, int dtype,
                          void* stream);
int tdeq_row_event_fit(void* q, const int32_t* fired_now, const void* y0, const void* y1, const void* f0, const void* f1,
                       const void* const* k, const double* coef, int n_terms, const void* dts, int64_t n_rows,
                       int64_t row_len, int dtype, void* stream);
int tdeq_row_event_eval(void* out, const void* q, const void* x, const int32_t* mask, int64_t n_rows, int64_t row_len,
                        int dtype, void* stream);

/*
 * ---- Compaction of an event solve (ABI 27; `odeint_rowwise_event(compact=...)`) ----
 * The stopped rows leave the batch; the quartics stay in a buffer of all the original rows, read by the bisection after
 * their rows have left.
 * tdeq_row_event_fit_mapped   tdeq_row_event_fit for a compacted batch: the state tensors, `dts` and `fired_now` hold n_rows
 *                             compact rows, `q` is [5, q_rows, row_len], and the quartic of compact row r with fired_now[r]
 *                             goes to q[j, row_map[r], :] (0 <= row_map[r] < q_rows, no row named twice; q_rows >= n_rows).
 *                             The same arithmetic; other rows of q are neither read nor written.
 * tdeq_row_event_eval_mapped  the quartics of an index list, no mask: for i < n_idx, out[dst_map ? dst_map[i] : i, :] = the
 *                             quartic q[:, src_map[i], :] at x[i] (`x` [n_idx] of the state type).  `q` is [5, q_rows,
 *                             row_len], `out` [out_rows, row_len]; 0 <= src_map[i] < q_rows, 0 <= dst_map[i] < out_rows (no
 *                             row named twice), and with dst_map == NULL out_rows >= n_idx.  Other rows of `out` are
 *                             untouched.
 * 64-bit offsets; the stride of q's leading dimension is q_rows * row_len.  16-byte elements when row_len is a multiple of
 * 16 / sizeof(T) and every state-sized pointer is 16-byte aligned (every row start of q and out is then aligned too),
 * scalar elements otherwise.  A NULL pointer (dst_map excepted), a negative size, no row of q or out with work to do, or a
 * dtype other than TDEQ_F32 / TDEQ_F64: TDEQ_EINVAL before any launch.  n_rows == 0 / n_idx == 0: no-op.
 */
int tdeq_row_event_fit_mapped(void* q, const int32_t* row_map, int64_t q_rows, const int32_t* fired_now, const void* y0,
                              const void* y1, const void* f0, const void* f1, const void* const* k, const double* coef,
                              int n_terms, const void* dts, int64_t n_rows, int64_t row_len, int dtype, void* stream);
int tdeq_row_event_eval_mapped(void* out, const int32_t* dst_map, int64_t out_rows, const void* q, const int32_t* src_map,
                               int64_t q_rows, const void* x, int64_t n_idx, int64_t row_len, int dtype, void* stream);

/*
 * ---- Per-row dense output (ABI 28; torchdiffeq_amd/rowwise_dense.py `odeint_rowwise_dense`) ----
 * The piecewise quartic of a whole rowwise solve: one segment per accepted step of each row.  During the solve the
 * quartics go to CHUNKS — `q` [5, cap, row_len] of the state type, per-slot metadata `slot_row` / `slot_ord` (int32 [cap]),
 * `slot_ta` / `slot_tb` (double [cap], solver time) and a device `counter` (int32 [2] = {slots taken, a row found no slot});
 * after it every chunk is packed into `coeffs` [5, n_seg, row_len], row r's segments contiguous and in step order at
 * offsets[r] .. offsets[r + 1] - 1.
 * tdeq_row_dense_slots   after tdeq_row_control(mode 0), one lane per row of `st`.  A row with accepted[r] takes the slot
 *                        s = (old counter[0]) + (its rank among the accepted rows of the launch): a ballot prefix inside a
 *                        wave, one atomicAdd per wave — unique, inside [old counter[0], old counter[0] + accepted rows), in
 *                        arrival order (no contract).  With s < cap: slot_row[s] = row_map ? row_map[r] : r, slot_ord[s] =
 *                        n_acc[r] - 1 (the controller has counted the step), slot_ta[s] = tprev[r], slot_tb[s] = t0[r],
 *                        slot[r] = s, mask[r] = 1.  With s >= cap nothing is written at s, counter[1] = 1, slot[r] = -1,
 *                        mask[r] = 0.  Every other row: slot[r] = -1, mask[r] = 0.  The quartic then goes to the chunk by
 *                        tdeq_row_event_fit_mapped(q = chunk, row_map = slot, fired_now = mask), which reads row_map[r] of
 *                        the rows with fired_now[r] only and needs cap >= n_rows.  cap + n_rows must fit an int32.
 * tdeq_row_dense_pack    dst[p, dest[s], :] = src[p, s, :] for s < n_used and the 5 planes p: a copy of bits.  `dst` is
 *                        [5, dst_rows, row_len], `src` [5, src_rows, row_len], `dest` a device int64 [n_used] with
 *                        0 <= dest[s] < dst_rows and no row named twice (not checked: it lives on the device); n_used <=
 *                        src_rows.  16-byte elements when row_len is a multiple of 16 / sizeof(T) and both bases are 16-byte
 *                        aligned, scalar elements otherwise.  Other rows of dst are untouched.
 * tdeq_row_dense_search  one lane per query i = j * n_rows + r of `tq` [n_q, n_rows] (double, solver time).  With t0[r] <=
 *                        tq <= t1[r] (and a row that has a segment): seg[i] = the first s in offsets[r] .. offsets[r + 1] - 1
 *                        with tq <= seg_tb[s], the row's last segment if there is none (it may end beyond t1[r]), found by
 *                        bisection; x[i] = T((tq - seg_ta[s]) / (seg_tb[s] - seg_ta[s])), the quotient formed in fp64.  A
 *                        breakpoint belongs to the earlier step (x = 1), tq = t0[r] to the first (x = 0).  Any other query,
 *                        a NaN included: seg[i] = offsets[r], x[i] = NaN, and status[0] (int32, preset to INT32_MAX by the
 *                        caller) is lowered to i — a minimum inside the wave, one atomicMin per wave that has one.
 *                        0 <= offsets[r] <= offsets[r + 1] <= n_seg; 1 <= n_seg <= INT32_MAX, n_q * n_rows < INT32_MAX.
 *                        The values are then tdeq_row_event_eval_mapped(out [n_q * n_rows, row_len], dst_map = NULL,
 *                        q = coeffs, src_map = seg, x).
 * 64-bit offsets.  A NULL pointer (row_map excepted), a negative size, a size beyond the stated limits or a dtype other than
 * TDEQ_F32 / TDEQ_F64: TDEQ_EINVAL before any launch.  n_rows == 0 / n_used == 0 / n_q == 0: no-op.
 */
int tdeq_row_dense_slots(const tdeq_row_state* st, const int32_t* row_map, int64_t cap, int32_t* counter, int32_t* slot_row,
                         int32_t* slot_ord, double* slot_ta, double* slot_tb, int32_t* slot, int32_t* mask, void* stream);
int tdeq_row_dense_pack(void* dst, int64_t dst_rows, const void* src, int64_t src_rows, const int64_t* dest, int64_t n_used,
                        int64_t row_len, int dtype, void* stream);
int tdeq_row_dense_search(const double* tq, int64_t n_q, const int64_t* offsets, const double* seg_ta, const double* seg_tb,
                          int64_t n_seg, const double* t0, const double* t1, int64_t n_rows, int32_t* seg, void* x,
                          int32_t* status, int dtype, void* stream);

/*
 * ---- Calculus on the per-row dense record (ABI 31; `RowDenseOutput.derivative` / `.antiderivative` / `.integral`) ----
 * Linear functionals of the piecewise quartic y(x) = e + d x + c x^2 + b x^3 + a x^4 of `coeffs` [5, n_seg, row_len] (planes
 * e, d, c, b, a), per element.  `seg_ta` / `seg_tb` are the segment ends in SOLVER time, `time_sign` is +1 for an ascending
 * and -1 for a descending solve (true time = time_sign * solver time), so every result is with respect to TRUE time.  Nothing
 * is contracted.
 * tdeq_row_dense_prefix  `prefix` [n_seg, row_len] double: the EXCLUSIVE prefix of the whole-segment integrals of each row, in
 *                        solver time.  With h_s = seg_tb[s] - seg_ta[s] (fp64), the coefficients converted to double and
 *                            J_s(x) = (((((a*0.2)*x + b*0.25)*x + c*(1.0/3.0))*x + d*0.5)*x + e) * x * h_s
 *                        every product and sum rounded once in fp64, I_s = J_s(1.0) — the same expression — and
 *                        prefix[offsets[r]] = 0, prefix[s + 1] = prefix[s] + I_s for s + 1 < offsets[r + 1], added LEFT TO
 *                        RIGHT: one lane per (row, element) walks the row's segments in order.  That order is the contract (a
 *                        row's bits depend neither on n_rows nor on the backend); a row with many segments runs serially.
 *                        0 <= offsets[r] <= offsets[r + 1] <= n_seg (the walk is clamped to the record).
 * tdeq_row_dense_calc    for i < n_idx, out[i, :] (of the state type T) from the segment seg[i] and the fraction x[i] (T) that
 *                        tdeq_row_dense_search wrote for query tq[i]; an out-of-range query is marked by x[i] = NaN and gives
 *                        a row of NaN.  mode
 *                        TDEQ_DENSE_DERIVATIVE      in T:  tot = d + (c + c) * x;  xp = x * x;  tot = tot + (T(3) * b) * xp;
 *                                                   xp = xp * x;  tot = tot + (T(4) * a) * xp;  out = tot / w  with
 *                                                   w = T(time_sign * (seg_tb[s] - seg_ta[s])), the difference in fp64.  At a
 *                                                   breakpoint (x = 1 of the earlier segment) that is the LEFT derivative.
 *                                                   `prefix`, `tq`, `seg2`, `x2`, `tq2` are not read (may be NULL).
 *                        TDEQ_DENSE_ANTIDERIVATIVE  in fp64: x64 = (tq[i] - seg_ta[s]) / h_s, NOT rounded to T,
 *                                                   F64 = time_sign * (prefix[s, :] + J_s(x64)),  out = T(F64): one rounding
 *                                                   to T.  The integral from t0[r] in true time; 0 at tq = t0[r].
 *                        TDEQ_DENSE_INTEGRAL        out = T(F64 of (seg2[i], x2[i], tq2[i]) - F64 of (seg[i], x[i], tq[i])),
 *                                                   the difference in fp64: the integral from tq to tq2.  Either end out of
 *                                                   range gives NaN.
 *                        0 <= seg[i], seg2[i] < n_seg (not checked: they live on the device; the search guarantees it).
 * 64-bit offsets; 16-byte elements when row_len is a multiple of 16 / sizeof(T) and `out`, `coeffs` and `prefix` are 16-byte
 * aligned, scalar elements otherwise.  A NULL pointer that the mode reads, a negative size, n_seg > INT32_MAX, a mode or
 * time_sign other than those named, or a dtype other than TDEQ_F32 / TDEQ_F64: TDEQ_EINVAL before any launch.  n_rows == 0 /
 * n_seg == 0 (prefix) / n_idx == 0: no-op.
 */
#define TDEQ_DENSE_DERIVATIVE 0
#define TDEQ_DENSE_ANTIDERIVATIVE 1
#define TDEQ_DENSE_INTEGRAL 2
int tdeq_row_dense_prefix(double* prefix, const void* coeffs, const int64_t* offsets, const double* seg_ta,
                          const double* seg_tb, int64_t n_seg, int64_t n_rows, int64_t row_len, int dtype, void* stream);
int tdeq_row_dense_calc(void* out, int mode, const void* coeffs, int64_t n_seg, const double* seg_ta, const double* seg_tb,
                        const double* prefix, double time_sign, const int32_t* seg, const void* x, const double* tq,
                        const int32_t* seg2, const void* x2, const double* tq2, int64_t n_idx, int64_t row_len, int dtype,
                        void* stream);

/*
 * ---- Extrema of the per-row dense record over a time window (ABI 32; `RowDenseOutput.maximum` / `.minimum`) ----
 * tdeq_row_dense_extremum  for i < n_idx and every element of the row: the largest (TDEQ_DENSE_MAXIMUM) or smallest
 *                          (TDEQ_DENSE_MINIMUM) value of the piecewise quartic on the closed window between the queries tq[i]
 *                          and tq2[i], and the time at which that element attains it.  (seg, x, tq) and (seg2, x2, tq2) are
 *                          what tdeq_row_dense_search wrote for the two ends (both of one row of the record); their order
 *                          does not matter.  `values` [n_idx, row_len] of the state type T, `times` [n_idx, row_len] double in
 *                          TRUE time.  The extremum is over the left-continuous record on the window together with the RIGHT
 *                          limits at the breakpoints p with lo <= p < hi (lo, hi the window's ends in solver time): the walk
 *                          below enters the segment that starts at p at x = 0, so a state impulse at p inside the window or at
 *                          its near end counts, one at its far end does not, and the time reported for a right limit is p.
 *                          THE ARITHMETIC IS THE CONTRACT.  Everything is fp64, one rounded operation per written operation,
 *                          nothing contracted; only + - * /, comparisons and fabs (no sqrt, no transcendental).  Per element:
 *                          Ends.    (segA, tqa), (segB, tqb) = the two ends, swapped if tq2[i] < tq[i], so tqa <= tqb.  If x[i]
 *                                   or x2[i] is NaN (an out-of-range end): values = NaN, times = NaN.
 *                          Walk.    s = segA .. segB in order; ta_s = seg_ta[s], tb_s = seg_tb[s], h_s = tb_s - ta_s,
 *                                   xlo = (s == segA) ? (tqa - ta_s) / h_s : 0.0,  xhi = (s == segB) ? (tqb - ta_s) / h_s : 1.0
 *                                   (the fractions of the antiderivative, not rounded to T).
 *                          Polynomials, the coefficients converted T -> double (exact):
 *                                   p(x)  = e + x*(d + x*(c + x*(b + x*a)))
 *                                   g(x)  = d + x*((c+c) + x*(3*b + x*(4*a)))
 *                                   g1(x) = (c+c) + x*(6*b + x*(12*a))
 *                                   x1 = (-b) / (4*a), the root of g1', when a != 0.
 *                          bisect(phi, lo, hi), with neg(v) = (v < 0): if phi(lo) == 0 or phi(hi) == 0 (that end is a
 *                                   candidate already) or neg(phi(lo)) == neg(phi(hi)) there is no root.  Otherwise at most 64
 *                                   rounds of: mid = 0.5 * (lo + hi); stop if mid == lo || mid == hi; if phi(mid) == 0 the root
 *                                   is mid; else mid replaces the end whose neg it shares.  After the rounds the root is lo if
 *                                   fabs(phi(lo)) <= fabs(phi(hi)), else hi.  (An exact zero is treated alike for phi and -phi:
 *                                   the minimum of a record is minus the maximum of the record with negated coefficients, at
 *                                   the same time, bit for bit but for the sign of a zero value.)
 *                          Isolation.  The pieces of g1 are bounded by [xlo, x1, xhi], x1 only if xlo < x1 < xhi; bisect g1 on
 *                                   each piece (at most 2 roots).  The pieces of g are bounded by xlo, those roots and xhi;
 *                                   bisect g on each piece (at most 3 roots).  Every bound of a piece of g and every root of g
 *                                   is a candidate: at most 7 evaluations of p per segment.
 *                          Selection.  Candidates are visited in increasing x, segments in order; the first candidate sets the
 *                                   best, a later one replaces it only if strictly greater (maximum) / strictly smaller
 *                                   (minimum): a tie goes to the candidate met first in the direction of the solve.  A NaN
 *                                   candidate value makes values and times NaN.  values = T(best): one rounding.
 *                          Time of a candidate x of segment s:  tqa if s == segA and x == xlo;  else tqb if s == segB and
 *                                   x == xhi;  else ta_s if x == 0;  else tb_s if x == 1 (the stored bits);  else ta_s + x * h_s.
 *                                   times = time_sign * that.
 *                          (Equal x give equal p(x), so a repeated candidate never replaces anything and an implementation may
 *                          visit repeats or skip them.)
 *                          One lane per (query, 16-byte element) walks its segments serially; no workspace, nothing cached.
 *                          0 <= seg[i] , seg2[i] < n_seg (the walk is clamped to the record).  16-byte elements when row_len
 *                          is a multiple of 16 / sizeof(T) and `values`, `times` and `coeffs` are 16-byte aligned, scalar
 *                          elements otherwise.  A NULL pointer, `which` or time_sign other than those named, a negative
 *                          size, n_seg > INT32_MAX or a dtype other than TDEQ_F32 / TDEQ_F64: TDEQ_EINVAL before any launch.
 *                          n_idx == 0 or row_len == 0: no-op.
 */
#define TDEQ_DENSE_MAXIMUM 0
#define TDEQ_DENSE_MINIMUM 1
int tdeq_row_dense_extremum(void* values, double* times, int which, const void* coeffs, int64_t n_seg, const double* seg_ta,
                            const double* seg_tb, double time_sign, const int32_t* seg, const void* x, const double* tq,
                            const int32_t* seg2, const void* x2, const double* tq2, int64_t n_idx, int64_t row_len, int dtype,
                            void* stream);

/*
 * ---- Level crossings of the per-row dense record over a time window (ABI 33; `RowDenseOutput.crossings` / `.time_above`) ----
 * tdeq_row_dense_level     for i < n_idx (a query of row i % n_rows; n_idx is a multiple of n_rows) and every element of the
 *                          row: how often the piecewise quartic crosses `level[row, el]` (`level` [n_rows, row_len] of the state
 *                          type T) on the window between the queries tq[i] and tq2[i], the times of the first and the last
 *                          crossing, and for how long the element is ABOVE the level.  (seg, x, tq), (seg2, x2, tq2) as for
 *                          tdeq_row_dense_extremum; their order does not matter.  `count` int32, `first`, `last`, `time_above`
 *                          double, all [n_idx, row_len]; `first` and `last` in TRUE time, `time_above` a duration >= 0.
 *                          THE ARITHMETIC IS THE CONTRACT.  Everything is fp64, one rounded operation per written operation,
 *                          nothing contracted; only + - * /, comparisons and fabs.  Per element:
 *                          Ends, Walk, xlo, xhi, Polynomials, bisect, Isolation: those of tdeq_row_dense_extremum, exactly.
 *                                   The candidates of a segment are the extremum's — xlo, the roots of g1 that bound pieces,
 *                                   the roots of g, xhi — in increasing x; between two neighbours the quartic is monotone up
 *                                   to what the isolation leaves.  (A repeated candidate changes nothing.)
 *                          Level function.  lev = double(level[row, el]);  phi(x) = (e + x*(d + x*(c + x*(b + x*a)))) - lev
 *                                   (the extremum's p, then one subtraction);  above(x) = phi(x) > 0, strict: a value equal to
 *                                   the level is not above.
 *                          State machine.  Candidates are visited in increasing x, segments in order.  The first candidate of
 *                                   the window (xlo of segA) sets state = above; if it is above, t_up = tqa.  Every later
 *                                   candidate v — the first candidate of each later segment, which is the RIGHT limit at a
 *                                   breakpoint, included — is compared with state; a difference is a crossing, after which
 *                                   state = above(v).
 *                          Location of a crossing.  Between two candidates u < v of one segment: z = u if phi(u) == 0, else
 *                                   v if phi(v) == 0, else bisect(phi, u, v), which always finds a root there.  At the first
 *                                   candidate of a later segment: that candidate, whose time is the breakpoint — a state
 *                                   impulse at p that lifts the element over the level is a crossing at p.
 *                          Time tz of a crossing z of segment s: the extremum's rule for a candidate — tqa if s == segA and
 *                                   z == xlo;  else tqb if s == segB and z == xhi;  else ta_s if z == 0;  else tb_s if z == 1
 *                                   (the stored bits);  else ta_s + z * h_s.
 *                          Accumulation per crossing.  count += 1;  first is set by the first crossing, last by every one;  an
 *                                   up-crossing (state becomes above) sets t_up = tz;  a down-crossing does
 *                                   total = total + (tz - t_up).  After the last segment, if state: total = total + (tqb -
 *                                   t_up).  Durations are added left to right in solver time; that order is the contract.
 *                          Outputs.  first = time_sign * tz of the first crossing, last = time_sign * tz of the last one, NaN
 *                                   when count == 0;  time_above = total (solver-time differences: the same number for an
 *                                   ascending and a descending solve).  A NaN phi at any candidate (a NaN level included), or
 *                                   an out-of-range end (x[i] or x2[i] NaN): count = -1, first = last = time_above = NaN.
 *                          The answer is exact ON THE RECORD, and the record is discontinuous at rounding level at every
 *                          breakpoint: p_s(1) and p_{s+1}(0) may differ in their last bits, and a level inside that gap is
 *                          crossed once more at the breakpoint (and back on the way).  A value that touches the level without
 *                          passing it (phi == 0 at a candidate, not above on both sides) is no crossing; one that comes down
 *                          to the level exactly and rises again is two crossings at the same time.
 *                          One lane per (query, 16-byte element) walks its segments serially; no workspace, nothing cached.
 *                          0 <= seg[i], seg2[i] < n_seg (the walk is clamped to the record).  16-byte elements when row_len
 *                          is a multiple of 16 / sizeof(T), `coeffs`, `level`, `first`, `last` and `time_above` are 16-byte
 *                          aligned and `count` is aligned to its word of 16 / sizeof(T) int32; scalar elements otherwise, with
 *                          the same bits.  A NULL pointer, n_rows <= 0 with n_idx > 0, n_idx no multiple of n_rows, a
 *                          negative size, n_seg > INT32_MAX, a time_sign other than +1 / -1 or a dtype other than TDEQ_F32 /
 *                          TDEQ_F64: TDEQ_EINVAL before any launch.  n_idx == 0 or row_len == 0: no-op.
 */
int tdeq_row_dense_level(int32_t* count, double* first, double* last, double* time_above, const void* level, int64_t n_rows,
                         const void* coeffs, int64_t n_seg, const double* seg_ta, const double* seg_tb, double time_sign,
                         const int32_t* seg, const void* x, const double* tq, const int32_t* seg2, const void* x2,
                         const double* tq2, int64_t n_idx, int64_t row_len, int dtype, void* stream);

/*
 * ---- Area above and below a level over a time window (ABI 34; `RowDenseOutput.exposure` / `.area_above` / `.area_below`) ----
 * tdeq_row_dense_exposure  for i < n_idx (a query of row i % n_rows; n_idx is a multiple of n_rows) and every element of the
 *                          row: the integral of max(y - level, 0) and of max(level - y, 0) of the piecewise quartic over the
 *                          window between the queries tq[i] and tq2[i], and for how long the element is ABOVE the level.
 *                          `level` [n_rows, row_len] of the state type T; (seg, x, tq), (seg2, x2, tq2) as for
 *                          tdeq_row_dense_extremum; their order does not matter.  `area_above`, `area_below` of T,
 *                          `time_above` double, all [n_idx, row_len]; the areas are durations times state units, >= 0.
 *                          THE ARITHMETIC IS THE CONTRACT.  Everything is fp64, one rounded operation per written operation,
 *                          nothing contracted; only + - * /, comparisons and fabs.  Per element:
 *                          Ends, Walk, xlo, xhi, Polynomials, bisect, Isolation, Level function, State machine, Location and
 *                                   Time of a crossing: those of tdeq_row_dense_level, exactly, so `time_above` is that
 *                                   function's `time_above`, bit for bit (its `total`, t_up and tz).
 *                          Area function.  el = e - lev, one subtraction;
 *                                       K(x) = (((((a*0.2)*x + b*0.25)*x + c*(1.0/3.0))*x + d*0.5)*x + el) * x * h_s
 *                                   — J_s of tdeq_row_dense_prefix with e replaced by el: the integral of y - level from the
 *                                   segment's start to x, in solver time.
 *                          Accumulation.  A_up = A_dn = 0.  A piece q is added under a state st:  A_up = A_up + q if st is
 *                                   above, else A_dn = A_dn - q.  For every candidate v that is not the first of its segment,
 *                                   with u the previous candidate of that segment:  without a crossing between them, add
 *                                   K(v) - K(u) under the current state;  with a crossing at z (the z of Location above, u or v
 *                                   themselves included), add K(z) - K(u) under the old state, then K(v) - K(z) under the new
 *                                   one.  The first candidate of a later segment (the right limit at a breakpoint) adds
 *                                   nothing: a state impulse flips the state there with zero width.  The window's first
 *                                   candidate adds nothing either.  Pieces are added in the order of the walk; that order is
 *                                   the contract.  (K(u) may be carried over from the previous visit: the same expression.)
 *                          Outputs.  area_above = T(A_up < 0 ? 0 : A_up), area_below = T(A_dn < 0 ? 0 : A_dn): one rounding
 *                                   each (a piece next to a crossing may carry the wrong sign at rounding level);  time_above =
 *                                   total.  All three are sums of solver-time pieces: the same numbers for an ascending and a
 *                                   descending solve, and `time_sign` changes nothing.  A NaN phi at any candidate (a NaN level
 *                                   included), or an out-of-range end (x[i] or x2[i] NaN): all three outputs NaN.
 *                          area_above - area_below is the integral of y - level over the window up to rounding; like the
 *                          crossings the answer is exact ON THE RECORD.  One lane per (query, 16-byte element) walks its
 *                          segments serially; no workspace, nothing cached.  0 <= seg[i], seg2[i] < n_seg (the walk is
 *                          clamped to the record).  16-byte elements when row_len is a multiple of 16 / sizeof(T) and `coeffs`,
 *                          `level`, `area_above`, `area_below` and `time_above` are 16-byte aligned; scalar elements otherwise,
 *                          with the same bits.  Refusals and no-ops are those of tdeq_row_dense_level: a NULL pointer,
 *                          n_rows <= 0 with n_idx > 0, n_idx no multiple of n_rows, a negative size, n_seg > INT32_MAX, a
 *                          time_sign other than +1 / -1 or a dtype other than TDEQ_F32 / TDEQ_F64: TDEQ_EINVAL before any
 *                          launch.  n_idx == 0 or row_len == 0: no-op.
 */
int tdeq_row_dense_exposure(void* area_above, void* area_below, double* time_above, const void* level, int64_t n_rows,
                            const void* coeffs, int64_t n_seg, const double* seg_ta, const double* seg_tb, double time_sign,
                            const int32_t* seg, const void* x, const double* tq, const int32_t* seg2, const void* x2,
                            const double* tq2, int64_t n_idx, int64_t row_len, int dtype, void* stream);

/*
 * ---- The times of all crossings of a level over a time window (ABI 35; `RowDenseOutput.crossing_times`) ----
 * tdeq_row_dense_level_times  for i < n_idx (a query of row i % n_rows; n_idx is a multiple of n_rows) and every element of
 *                          the row: the times of the first K = max_count RISING and of the first K FALLING crossings of
 *                          `level[row, el]` on the window between the queries tq[i] and tq2[i], and how many crossings of
 *                          each direction the window holds.  `level` [n_rows, row_len] of the state type T; (seg, x, tq),
 *                          (seg2, x2, tq2) as for tdeq_row_dense_extremum; their order does not matter.  `n_rising`,
 *                          `n_falling` int32 [n_idx, row_len]; `rising`, `falling` double [K, n_idx, row_len] in TRUE time.
 *                          THE ARITHMETIC IS THE CONTRACT.  Per element:
 *                          Ends, Walk, xlo, xhi, Polynomials, bisect, Isolation, Level function, State machine, Location and
 *                                   Time of a crossing: those of tdeq_row_dense_level, exactly: the crossings are that
 *                                   function's crossings, in its order, with its tz.
 *                          Direction.  Rising is defined in TRUE time: y goes from <= level to > level as true time
 *                                   increases.  The walk runs in solver time, so a crossing after which the state is above is
 *                                   rising when time_sign > 0 and falling when time_sign < 0:
 *                                   rising = (state becomes above) == (time_sign > 0).
 *                          Lists.  Each direction has a counter n, 0 at the start.  A crossing at tz of that direction:  if
 *                                   n < K, list[n, i, el] = time_sign * tz;  then n += 1.  So a list holds the first K
 *                                   crossings of its direction in the order of the walk — the direction of the solve:
 *                                   decreasing true time when time_sign < 0 — and the counting continues past K.  After the
 *                                   walk the slots min(n, K) .. K - 1 of both lists are NaN and n_rising, n_falling are the
 *                                   two counters; n_rising + n_falling is the `count` of tdeq_row_dense_level.
 *                          NaN.  A NaN phi at any candidate (a NaN level included), or an out-of-range end (x[i] or x2[i]
 *                                   NaN): n_rising = n_falling = -1 and all K slots of both lists NaN.
 *                          Every slot of the four outputs is written and nothing else.  The remarks of tdeq_row_dense_level
 *                          on the record (the rounding-level gap at a breakpoint, a touch, a state impulse) hold unchanged.
 *                          One lane per (query, 16-byte element) walks its segments serially and stores a located time at
 *                          once, as one 8-byte store; no workspace, nothing cached.  0 <= seg[i], seg2[i] < n_seg (the walk is
 *                          clamped to the record).  16-byte elements when row_len is a multiple of 16 / sizeof(T), `coeffs`
 *                          and `level` are 16-byte aligned and `n_rising`, `n_falling` are aligned to their word of
 *                          16 / sizeof(T) int32; scalar elements otherwise, with the same bits.  `rising` and `falling` put no
 *                          condition on the form.  Refusals and no-ops are those of tdeq_row_dense_level, plus max_count < 1 or
 *                          max_count > 65535: TDEQ_EINVAL before any launch.
 */
int tdeq_row_dense_level_times(int32_t* n_rising, int32_t* n_falling, double* rising, double* falling, int64_t max_count,
                               const void* level, int64_t n_rows, const void* coeffs, int64_t n_seg, const double* seg_ta,
                               const double* seg_tb, double time_sign, const int32_t* seg, const void* x, const double* tq,
                               const int32_t* seg2, const void* x2, const double* tq2, int64_t n_idx, int64_t row_len,
                               int dtype, void* stream);

/*
 * ---- Per-row step options (ABI 29; `min_step`, `max_step`, `step_t`, `jump_t` of the rowwise family) ----
 * tdeq_row_control_points  tdeq_row_control with step bounds per row and with points per row: `step_t` (times a step of
 *                          the row must end on) and `jump_t` (times where func is discontinuous), rk_common.py:223-241,
 *                          289-309, 343-352 row by row.  Every mode clamps with the row's min_step[r] / max_step[r] (NULL:
 *                          the scalar of `ctrl`), and mode 0 accepts with them.  After the clamp and the error checks of a
 *                          prepared step (modes 0, 2, 3, rows still active), with p = step_t[next_step[r], r] for a row with
 *                          step_count[r] >= 1: t0 < p < t0 + dt cuts the step, dt = p - t0 and the step ends at p; then the
 *                          same test with jump_t on the step so far, and a jump point wins.  on_point[r] = 0 / 1 / 2 (not
 *                          cut / step point / jump point, 0 for a row not active), and for a cut step clip_t[r] = p,
 *                          dt[r] = p - t0, dts_out[r] = sign * T(dt), the stage of abscissa 1 at sign * prev_T(T(p)), the
 *                          others at sign * (T(t0) + alpha_T T(dt)).  Mode 0 ends an accepted step with on_point[r] != 0 at
 *                          t0[r] = clip_t[r] (the point's bits, not t0 + dt), then moves next_step[r] (on_point 1) or
 *                          next_jump[r] (on_point 2) on by one unless it is the row's last index, and writes for EVERY row
 *                          jumped[r] = the accepted step ended on a jump point, jump_times[r] (state type) = sign *
 *                          next_T(T(t0[r])) where jumped, sign * T(t0[r]) elsewhere: the times of the one evaluation of
 *                          func that refreshes f0 of the rows that jumped.  st->status holds THREE words: the two of
 *                          tdeq_row_control and status[2] = rows with jumped[r] in this launch (0 in the other modes).
 *                          Tables are [n_points, n_rows] doubles in solver time, each column sorted ascending and padded
 *                          with +inf; a NULL table is absent (its count / index vectors are then not read).  0 <=
 *                          next[r] < count[r] <= n_points for a row with points.  With both tables and both bound
 *                          vectors NULL every vector of `st`, dts_out and times_out get the bits of tdeq_row_control.
 * tdeq_row_select          dst[r, e] = src[r, e] for the rows with mask[r] != 0 (int32 [n_rows]), e < row_len: a copy of
 *                          bits; no other row is read or written.  16-byte elements when row_len is a multiple of
 *                          16 / sizeof(T) and both bases are 16-byte aligned, scalar elements otherwise.
 * State impulses at jump points (ABI 30; `jump_dy` of the rowwise family):
 * tdeq_row_control_points  with pts->jump_hit != NULL the jump table is tested with t0 < p <= t0 + dt: a prepared step
 *                          that lands on the point exactly is a step onto it: on_point 2, clip_t = p, dt[r] unchanged
 *                          (p - t0 may round above dt and above max_step); step_t keeps the open test.  Mode 0 writes
 *                          jump_hit[r] = next_jump[r] before it is moved on, for the rows with jumped[r] only.
 *                          jump_hit and jump_closed = 1 go together, and both need jump_t: one without the other, or
 *                          without the table, is TDEQ_EINVAL.  With both zero (the zeroed tail of an ABI-29 block)
 *                          every output is that of ABI 29.
 * tdeq_row_impulse         for the rows with jumped[r] != 0: o = row_map ? row_map[r] : r, k = dy_index[jump_hit[r] * n_orig
 *                          + o]; k >= 0: y[r, e] += dy[(k * dy_rows + (dy_rows == 1 ? 0 : o)) * row_len + e], one addition in
 *                          the state's type.  dy_index is int32 [K', n_orig] (sorted position of a point in the row's column
 *                          -> the caller's k; -1: none), dy_rows is 1 or n_orig, row_map NULL for a batch that was never
 *                          compacted.  No other row of y or dy is read or written.  16-byte elements when row_len is a
 *                          multiple of 16 / sizeof(T) and y and dy are 16-byte aligned, scalar elements otherwise.
 * 64-bit offsets.  A NULL pointer other than those named, a negative size or a dtype other than TDEQ_F32 / TDEQ_F64:
 * TDEQ_EINVAL before any launch.  n_rows == 0: no-op (the status words are still reset).
 */
typedef struct tdeq_row_points {
    const double* step_t;       /* [n_step, n_rows] or NULL                                             */
    const double* jump_t;       /* [n_jump, n_rows] or NULL                                             */
    const int32_t* step_count;  /* [n_rows] points of each row                                          */
    const int32_t* jump_count;
    int32_t* next_step;         /* [n_rows] index of the row's next point                               */
    int32_t* next_jump;
    double* clip_t;             /* [n_rows] end of a prepared step that was cut                         */
    int32_t* on_point;          /* [n_rows] 0 not cut, 1 at a step point, 2 at a jump point             */
    const double* min_step;     /* [n_rows] or NULL                                                     */
    const double* max_step;     /* [n_rows] or NULL                                                     */
    int32_t* jumped;            /* [n_rows] mode 0                                                      */
    void* jump_times;           /* [n_rows] of the state type, mode 0                                   */
    int32_t n_step;             /* rows of the step_t table                                             */
    int32_t n_jump;
    int32_t* jump_hit;          /* [n_rows] or NULL: mode 0, position of the jump point a row ended on  */
    int32_t jump_closed;        /* 1 with jump_hit: the jump table is tested with p <= t0 + dt          */
} tdeq_row_points;

int tdeq_row_control_points(int mode, const double* part, const tdeq_step_ctrl* ctrl, const tdeq_row_state* st,
                            const tdeq_row_points* pts, void* dts_out, void* times_out, int dtype, void* stream);
int tdeq_row_select(void* dst, const void* src, const int32_t* mask, int64_t n_rows, int64_t row_len, int dtype,
                    void* stream);
int tdeq_row_impulse(void* y, const void* dy, int64_t dy_rows, const int32_t* dy_index, int64_t n_orig,
                     const int32_t* jump_hit, const int32_t* jumped, const int32_t* row_map /* or NULL */, int64_t n_rows,
                     int64_t row_len, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TDEQ_HIP_H */
