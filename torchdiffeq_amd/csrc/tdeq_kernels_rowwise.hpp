// tdeq_kernels_rowwise.hpp — gfx950 device code of `odeint_rowwise` (torchdiffeq_amd/rowwise.py): a batch of B
// independent IVPs of L elements each, one step controller PER ROW.
//
// The state is [B, L] row-major.  Every per-row quantity lives in a device vector of length B: the time t0[B] and step
// size dt[B] (fp64, the reference's time type W), sign * T(dt) of the running trial step (T[B]), the stage times handed
// to func ([n_stages, B] of T), the active flag, the counters and an error code.  The host reads back two words per
// trial step (active rows, first row in error), three in a solve with per-row step options (rows that jumped).
//
// The arithmetic of every element is that of the whole-batch kernels in tdeq_kernels.hpp with the row's own step
// size: coefficients fl_T(fl_T(a_j) * T(dt_r)), left-to-right sums, -ffp-contract=off.  Rows that have finished
// (`active[r] == 0`) read none of their stage streams (func's output for them is ignored, NaN or not): the stage
// combine writes their y0 unchanged, the reductions report zeros, the controller leaves them alone.
//
// Reductions are batch-invariant: how a row is reduced depends on L only (never on B or on the row's position), so
// a row's error ratio has the same bits in a batch of any size.
//   short rows (nv <= kRowWaveMax 16-byte elements):  G = power of two <= 64 lanes per row, each lane its strided
//                                                      elements in order, then a butterfly over the G lanes
//   long rows:                                         nch chunks of `chunk` elements per row, one workgroup per
//                                                      (row, chunk) -> fp64 partial; the controller adds a row's
//                                                      partials with one wave in a fixed order.  A long row of ONE
//                                                      chunk (kRowWaveMax < nv <= chunk) takes the same chunk kernels;
//                                                      its single partial sits where a short row's does
//
// The per-row step options (`min_step`, `max_step` as [B] vectors, `step_t`, `jump_t`, `jump_dy`) are the controller's
// POINTS / IMPULSE instantiations — the step rule is stated once, see "Per-row controller" — plus two streaming kernels:
//   row_select_kernel        dst[r, :] = src[r, :] for the rows of a mask: how the re-evaluated f0 of the rows that jumped
//                            is taken, and nothing of any other row.
//   row_impulse_kernel       y[r, :] += dy[k, row, :] for the rows of the same mask (`jump_dy`): the state impulse of the
//                            jump point the row's step ended on, k looked up from the position the controller reported.
#pragma once

#include "tdeq_kernels.hpp"

namespace tdeq {

constexpr int kRowWaveMax = 64 * 16;      // short-row limit in E elements (16 per lane at G = 64)

// ------------------------------------------------------------------------------------------------
// Row stage combine with carried partial sums (the rowwise form of stage_combine_multi_kernel):
//   s_o = [acc_in +] sum_{j in mask_o, ascending} fl_T(c_o[j] * dts[r]) * k_j ;  out_o = add_y0_o ? y0 + s_o : s_o
// Inactive rows: out_o = y0 (add_y0) or 0, no stage is read.
// ------------------------------------------------------------------------------------------------
template <typename T, int NT>
struct RowMultiArgs {
    const T* y0;
    const T* acc_in;                  // nullable: prefix of output 0's sum
    const T* k[NT];
    T* out[kMaxMultiOut];
    T c[kMaxMultiOut][NT];            // fl_T(coef)
    uint32_t mask[kMaxMultiOut];
    uint32_t add_y0;
    int n_out;
    const T* dts;                     // [B] sign * T(dt_r)
    const int32_t* active;            // [B]
    int64_t row_len;                  // L, in units of the element type E of the launch
    int64_t n;                        // B * L elements of T
};

template <typename T, int NT, typename E>
__device__ __forceinline__ void row_multi_elem(const RowMultiArgs<T, NT>& a, int64_t i, int64_t r) {
    const E y = reinterpret_cast<const E*>(a.y0)[i];
    if (!a.active[r]) {
        E zero = y;
        zero = zero - y;              // (0 for a finite y0; the value is never read for a finished row)
#pragma unroll
        for (int o = 0; o < kMaxMultiOut; ++o)
            if (o < a.n_out) reinterpret_cast<E*>(a.out[o])[i] = ((a.add_y0 >> o) & 1u) ? y : zero;
        return;
    }
    const T dtT = a.dts[r];
    E kk[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) kk[j] = reinterpret_cast<const E*>(a.k[j])[i];
    const bool has_acc = a.acc_in != nullptr;
    E acc0 = y;
    if (has_acc) acc0 = reinterpret_cast<const E*>(a.acc_in)[i];
#pragma unroll
    for (int o = 0; o < kMaxMultiOut; ++o) {
        if (o < a.n_out) {
            const uint32_t m = a.mask[o];
            bool started = (o == 0) && has_acc;
            E s = acc0;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                if ((m >> j) & 1u) {
                    const T cj = a.c[o][j] * dtT;          // fl_T(fl_T(coef) * T(dt_r))
                    const E p = kk[j] * cj;
                    s = started ? s + p : p;
                    started = true;
                }
            }
            reinterpret_cast<E*>(a.out[o])[i] = ((a.add_y0 >> o) & 1u) ? y + s : s;
        }
    }
}

// VEC: L % (16 / sizeof(T)) == 0 and every buffer 16-byte aligned, so a 16-byte element never straddles two rows.
template <typename T, int NT, bool VEC>
__global__ __launch_bounds__(kBlock) void row_combine_kernel(const RowMultiArgs<T, NT> a) {
    using E = typename std::conditional<VEC, typename VecOf<T>::type, T>::type;
    constexpr int LV = VEC ? VecOf<T>::L : 1;
    const int64_t ne = a.n / LV;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < ne; i += stride)
        row_multi_elem<T, NT, E>(a, i, i / a.row_len);
}

// ------------------------------------------------------------------------------------------------
// Row reductions.  MODE 0: embedded error  e = [partial +] sum_j fl_T(c_j * dts[r]) * k_j, then
//   acc0 += (e / (atol + rtol * max(|y0|, |y1|)))^2, bad += !finite(y0) || !finite(y1)      (tol_accumulate)
// MODE 1 / 2: the initial-step norms of init_elem (a = y0 or f1, b = f0, y = y0 for the scale).
// rtol, atol: the two scalars of the argument block, or with ROWTOL the row's own (RowRedTolArgs) — in every mode.
// Results: part[q * (B * nch) + r * nch + c], q = 0, 1 sums, q = 2 the non-finite count.
// ------------------------------------------------------------------------------------------------
template <typename T, int NT>
struct RowRedArgs {
    const T* y0;                      // MODE 0: y0; MODE 1/2: the scale state y
    const T* y1;                      // MODE 0: y1; MODE 1/2: a
    const T* partial;                 // MODE 0, nullable; MODE 1/2: b
    const T* k[NT > 0 ? NT : 1];
    T c[NT > 0 ? NT : 1];
    const T* dts;
    const int32_t* active;
    T rtol, atol;
    int64_t row_len;                  // in E units
    int64_t n_rows;
    int64_t chunk;                    // long rows: E units per workgroup
    int nch;                          // chunks per row (1 for short rows and for long rows of one chunk)
    int group;                        // short rows: lanes per row (power of two <= 64)
    double* part;
};

// The per-row form (ROWTOL) serves `odeint_rowwise` with [B] tolerance vectors: row r is reduced with rtol_rows[r],
// atol_rows[r] (already rounded to T by the caller) in place of the two scalars of the block, which it does not read.
// The element arithmetic, the geometry and the layout of `part` are those of the plain form.
template <typename T, int NT>
struct RowRedTolArgs : RowRedArgs<T, NT> {
    const T* rtol_rows;               // [n_rows]
    const T* atol_rows;               // [n_rows]
};

template <typename T, int NT, bool ROWTOL>
using RowRedArgsOf = typename std::conditional<ROWTOL, RowRedTolArgs<T, NT>, RowRedArgs<T, NT>>::type;

template <typename T, int NT, int MODE, bool PARTIAL, typename E>
__device__ __forceinline__ void row_red_elem(const RowRedArgs<T, NT>& a, const T (&cc)[NT > 0 ? NT : 1], T rtol, T atol,
                                             int64_t i, double (&acc)[3]) {
    constexpr int LV = sizeof(E) / sizeof(T);
    if constexpr (MODE == 0) {
        E e;
        if constexpr (PARTIAL) e = reinterpret_cast<const E*>(a.partial)[i];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const E p = reinterpret_cast<const E*>(a.k[j])[i] * cc[j];
            if (PARTIAL || j > 0) e = e + p;
            else e = p;
        }
        const E v0 = reinterpret_cast<const E*>(a.y0)[i], v1 = reinterpret_cast<const E*>(a.y1)[i];
        if constexpr (LV == 1) {
            tol_accumulate<T>(e, v0, v1, rtol, atol, acc[0], acc[2]);
        } else {
#pragma unroll
            for (int q = 0; q < LV; ++q) tol_accumulate<T>(e[q], v0[q], v1[q], rtol, atol, acc[0], acc[2]);
        }
    } else {
        const E yv = reinterpret_cast<const E*>(a.y0)[i];
        const E av = reinterpret_cast<const E*>(a.y1)[i];
        const E bv = reinterpret_cast<const E*>(a.partial)[i];
        if constexpr (LV == 1) {
            init_elem<T, MODE - 1>(rtol, atol, av, bv, yv, acc);
        } else {
#pragma unroll
            for (int q = 0; q < LV; ++q) init_elem<T, MODE - 1>(rtol, atol, av[q], bv[q], yv[q], acc);
        }
    }
}

template <typename T, int NT>
__device__ __forceinline__ void row_coefs(const RowRedArgs<T, NT>& a, int64_t r, T (&cc)[NT > 0 ? NT : 1]) {
    const T dtT = a.dts ? a.dts[r] : (T)1;
#pragma unroll
    for (int j = 0; j < NT; ++j) cc[j] = a.c[j] * dtT;
}

// the row's two tolerances: the block's scalars, or (ROWTOL) one load each per row, the same address for every lane that
// serves the row
template <typename T, int NT, bool ROWTOL>
__device__ __forceinline__ void row_tols(const RowRedArgsOf<T, NT, ROWTOL>& a, int64_t r, T& rtol, T& atol) {
    if constexpr (ROWTOL) {
        rtol = a.rtol_rows[r];
        atol = a.atol_rows[r];
    } else {
        rtol = a.rtol;
        atol = a.atol;
    }
}

// short rows: `group` lanes per row, 256 / group rows per workgroup
template <typename T, int NT, int MODE, bool PARTIAL, bool VEC, bool ROWTOL>
__global__ __launch_bounds__(kBlock) void row_reduce_wave_kernel(const RowRedArgsOf<T, NT, ROWTOL> a) {
    using E = typename std::conditional<VEC, typename VecOf<T>::type, T>::type;
    const int g = a.group;
    const int lane = threadIdx.x & (g - 1);
    const int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / g;
    double acc[3] = {0.0, 0.0, 0.0};
    const bool live = r < a.n_rows && (MODE != 0 || a.active[r]);
    if (live) {
        T cc[NT > 0 ? NT : 1];
        row_coefs<T, NT>(a, r, cc);
        T rtol, atol;
        row_tols<T, NT, ROWTOL>(a, r, rtol, atol);
        const int64_t base = r * a.row_len;
        for (int64_t e = lane; e < a.row_len; e += g) row_red_elem<T, NT, MODE, PARTIAL, E>(a, cc, rtol, atol, base + e, acc);
    }
    // butterfly over the group's lanes (the same tree for every row; lanes of other groups are never mixed in)
    for (int off = g >> 1; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] += __shfl_xor(acc[q], off, kWave);
    }
    if (lane == 0 && r < a.n_rows) {
        const int64_t nb = a.n_rows;
        a.part[r] = acc[0];
        a.part[nb + r] = acc[1];
        a.part[2 * nb + r] = acc[2];
    }
}

// long rows: one workgroup per (row, chunk)
template <typename T, int NT, int MODE, bool PARTIAL, bool VEC, bool ROWTOL>
__global__ __launch_bounds__(kBlock) void row_reduce_chunk_kernel(const RowRedArgsOf<T, NT, ROWTOL> a) {
    using E = typename std::conditional<VEC, typename VecOf<T>::type, T>::type;
    __shared__ double red[3 * (kBlock / kWave)];
    const int64_t b = blockIdx.x;
    const int64_t r = b / a.nch, c = b - r * a.nch;
    double acc[3] = {0.0, 0.0, 0.0};
    if (MODE != 0 || a.active[r]) {
        T cc[NT > 0 ? NT : 1];
        row_coefs<T, NT>(a, r, cc);
        T rtol, atol;
        row_tols<T, NT, ROWTOL>(a, r, rtol, atol);
        const int64_t lo = c * a.chunk;
        const int64_t hi = lo + a.chunk < a.row_len ? lo + a.chunk : a.row_len;
        const int64_t base = r * a.row_len;
#pragma unroll 2
        for (int64_t e = lo + threadIdx.x; e < hi; e += kBlock)
            row_red_elem<T, NT, MODE, PARTIAL, E>(a, cc, rtol, atol, base + e, acc);
    }
    block_sum<3>(acc, red);
    if (threadIdx.x == 0) {
        const int64_t nb = a.n_rows * a.nch;
        a.part[b] = acc[0];
        a.part[nb + b] = acc[1];
        a.part[2 * nb + b] = acc[2];
    }
}

// ------------------------------------------------------------------------------------------------
// Per-row controller.  One lane per row (short rows) or one wave per row (long rows: the wave adds the row's nch
// partials, lane q taking q, q + 64, ... in order, then the wave's shuffle tree).  MODE:
//   0  trial step: error ratio -> accept / reject, next dt, output range, counters      (norm_finalize_ctrl_kernel)
//   1  initial step, first half: d0, d1 -> h0; dts = sign * T(h0), stage time of f(t0 + h0)   (_select_initial_step)
//   2  initial step, second half: d2 -> h1 -> dt = min(100 h0, h1)
//   3  dt given (first_step): only the non-finite census of y0 (the MODE 1 reduction) and the set-up below
// After modes 0 (rows still active), 2 and 3: the next trial step's dt clamp, sign * T(dt) and stage times, and the
// error checks the host raises for (code 2: max_num_steps, 1: dt underflow, 3: non-finite y).
//
// POINTS (a solve with `min_step` / `max_step` as [B] vectors, `step_t` or `jump_t`) is a compile-time flag of the
// controller, as ROWTOL is of the row reductions: false is the controller without them, with the two scalar bounds of
// `c`, and its block is RowCtrlArgs.  true takes the row's own bounds and the row's own points: times a step must end on
// (`step_t`) and times where func is discontinuous (`jump_t`).  A prepared step that would pass the row's next point is
// cut short at it (rk_common.py:289-309); an accepted cut step ends on the point's own bits and moves the row's index
// (rk_common.py:343-352); mode 0 also reports which rows ended on a jump point and the time vector of the one extra
// evaluation of func that follows.
// IMPULSE (POINTS with `jump_dy`) tests the jump table with `t0 < p <= t0 + dt` — a step that lands on a point exactly
// is a step onto it, or the row's index would stick there and the dose and every later one be lost; such a step keeps
// its dt (it ends on the point's bits already) — and an accepted step onto a jump point writes jump_hit[r], the
// position of the point in the row's sorted column.
// ------------------------------------------------------------------------------------------------
struct RowCtrlArgs {
    const double* part;               // [3][B * nch]
    int nch;
    int tkind;                        // 0 = fp64, 1 = fp32
    int mode;
    tdeq_step_ctrl c;                 // safety, ifactor, dfactor, exponent, min_step, max_step, time_sign, alpha[], n_times
    tdeq_row_state st;                // the [B] vectors of the solve; status: [2] = {active rows, first row in error}
    void* dts_out;                    // [B] of T: sign * T(dt) of the next trial step (mode 1: sign * T(h0))
    void* times;                      // [n_times, B] of T (mode 1: row 0 = the time of f(t0 + h0))
};

struct RowCtrlPointsArgs : RowCtrlArgs {      // st.status: [3], the third word = rows that jumped in this launch
    tdeq_row_points pts;              // tables sorted per row and padded with +inf; a null table or bound vector: none
};

template <bool POINTS>
using RowCtrlArgsOf = typename std::conditional<POINTS, RowCtrlPointsArgs, RowCtrlArgs>::type;

// stage time i of a step from t0 of size dt that ends at t1 (rk_common.py:72-78): ctl_stage_time with the end given
template <typename T>
__device__ __forceinline__ T row_stage_time_to(const tdeq_step_ctrl& c, double t0, double dt, double t1, int i) {
    T tt;
    if ((c.alpha_is_one >> i) & 1u) tt = ctl_prev((T)t1);
    else tt = (T)t0 + (T)c.alpha[i] * (T)dt;
    return (T)c.time_sign * tt;
}

// the row's next point of one table inside the prepared step (t0, t0 + dt), or no cut (rk_common.py:292-296); CLOSED:
// inside (t0, t0 + dt]
template <bool CLOSED = false>
__device__ __forceinline__ bool row_point_inside(const double* table, const int32_t* count, const int32_t* next, int64_t r,
                                                 int64_t n_rows, double t0, double dt, double& p) {
    if (!table || count[r] < 1) return false;
    p = table[(int64_t)next[r] * n_rows + r];
    if (CLOSED) return t0 < p && p <= t0 + dt;
    return t0 < p && p < t0 + dt;
}

// The next trial step of an active row (rk_common.py:266-287) with the row's bounds [lo, hi]; with POINTS the step is
// then cut short at the row's next step point and at its next jump point, which wins (rk_common.py:289-309).  Returns
// code != 0.
template <typename T, bool POINTS, bool IMPULSE>
__device__ __forceinline__ bool row_prepare(const RowCtrlArgsOf<POINTS>& a, int64_t r, double lo, double hi) {
    const tdeq_step_ctrl& c = a.c;
    const tdeq_row_state& s = a.st;
    double dt = s.dt[r];
    if (!__builtin_isfinite(dt)) dt = lo;
    dt = ctl_clamp(dt, lo, hi);
    const double t0 = s.t0[r];
    int code = 0;
    if (s.bad_y[r]) code = 3;
    if (!(t0 + dt > t0)) code = 1;
    if (s.since[r] >= s.max_num_steps) code = 2;
    double t1 = 0.0;
    int on = 0;
    if constexpr (POINTS) {
        const tdeq_row_points& q = a.pts;
        double p;
        if (row_point_inside(q.step_t, q.step_count, q.next_step, r, s.n_rows, t0, dt, p)) {
            on = 1;
            t1 = p;
            dt = p - t0;
        }
        if (row_point_inside<IMPULSE>(q.jump_t, q.jump_count, q.next_jump, r, s.n_rows, t0, dt, p)) {
            on = 2;
            t1 = p;
            // (a step that lands on the point keeps its size: p - t0 may round above dt, hence above max_step, and a step
            //  above the ceiling is never accepted)
            if (!IMPULSE || p < t0 + dt) dt = p - t0;
        }
        q.on_point[r] = on;
        if (on) q.clip_t[r] = t1;
    }
    s.dt[r] = dt;
    static_cast<T*>(a.dts_out)[r] = (T)dt * (T)c.time_sign;
    for (int i = 0; i < c.n_times; ++i)
        static_cast<T*>(a.times)[i * s.n_rows + r] = on ? row_stage_time_to<T>(c, t0, dt, t1, i) : ctl_stage_time<T>(c, t0, dt, i);
    s.code[r] = code;
    return code != 0;
}

// a finished row: func keeps being evaluated at the end t0 of its last accepted step, on its frozen state
template <typename T>
__device__ __forceinline__ void row_freeze(void* dts, void* times, int n_times, int64_t n_rows, double time_sign, double t0,
                                           int64_t r) {
    static_cast<T*>(dts)[r] = (T)0;
    const T tt = (T)time_sign * (T)t0;
    for (int i = 0; i < n_times; ++i) static_cast<T*>(times)[i * n_rows + r] = tt;
}

// sqrt(mean) of a row, rounded to T (misc.py:22-33 with one segment)
__device__ __forceinline__ double row_norm(double sum, int64_t numel, int tkind) {
    const double v = __builtin_sqrt(sum / (double)numel);
    return tkind == 1 ? (double)(float)v : v;
}

// returns: the row is active after this launch, (code != 0), and with POINTS: its accepted step ended on a jump point
template <typename T, bool POINTS, bool IMPULSE>
__device__ __forceinline__ void row_control(const RowCtrlArgsOf<POINTS>& a, int64_t r, double s0, double s1, double sb,
                                            bool& live, bool& err, bool& jump) {
    const tdeq_step_ctrl& c = a.c;
    const tdeq_row_state& s = a.st;
    double lo = c.min_step, hi = c.max_step;          // the bounds of row r
    if constexpr (POINTS) {
        if (a.pts.min_step) lo = a.pts.min_step[r];
        if (a.pts.max_step) hi = a.pts.max_step[r];
    }
    const bool was_live = s.active[r] != 0;
    live = was_live;
    err = false;
    jump = false;
    if (a.mode == 0) {
        double t_now = s.t0[r];
        if (live) {
            const double ratio = row_norm(s0, s.row_len, a.tkind);
            const double step_t0 = t_now, step_dt = s.dt[r];
            bool accept = ratio <= 1.0;
            if (step_dt > hi) accept = false;
            if (step_dt <= lo) accept = true;
            double dt_next;
            if (ratio == 0.0) {
                dt_next = step_dt * c.ifactor;
            } else {
                const double dfactor = ratio < 1.0 ? 1.0 : c.dfactor;
                const double scaled = c.safety / pow(ratio, c.exponent);
                dt_next = step_dt * ctl_nan_min(c.ifactor, ctl_nan_max(scaled, dfactor));
            }
            dt_next = ctl_clamp(dt_next, lo, hi);
            s.ratio[r] = ratio;
            s.since[r] += 1;
            s.accepted[r] = accept ? 1 : 0;
            if (accept) {
                t_now = step_t0 + step_dt;
                int on = 0;
                if constexpr (POINTS) {
                    on = a.pts.on_point[r];
                    if (on) t_now = a.pts.clip_t[r];              // a cut step ends on the point's own bits
                }
                s.tprev[r] = step_t0;
                s.t0[r] = t_now;
                s.n_acc[r] += 1;
                const int out_lo = s.next_out[r];
                int out_hi = out_lo;
                while (out_hi < s.n_out && s.tgrid[(int64_t)out_hi * s.n_rows + r] <= t_now) ++out_hi;
                s.out_lo[r] = out_lo;
                s.out_hi[r] = out_hi;
                s.next_out[r] = out_hi;
                if (out_hi > out_lo) s.since[r] = 0;
                s.bad_y[r] = sb != 0.0 ? 1 : 0;
                if constexpr (POINTS) {
                    const tdeq_row_points& q = a.pts;
                    if (on == 1 && q.next_step[r] != q.step_count[r] - 1) q.next_step[r] += 1;
                    if (on == 2) {
                        if (IMPULSE) q.jump_hit[r] = q.next_jump[r];
                        if (q.next_jump[r] != q.jump_count[r] - 1) q.next_jump[r] += 1;
                        jump = true;
                    }
                }
                if (out_hi >= s.n_out) {
                    live = false;
                    s.active[r] = 0;
                }
            } else {
                s.n_rej[r] += 1;
            }
            s.dt[r] = dt_next;
        } else {
            s.accepted[r] = 0;
        }
        if constexpr (POINTS) {
            a.pts.jumped[r] = jump ? 1 : 0;
            static_cast<T*>(a.pts.jump_times)[r] = (T)c.time_sign * (jump ? ctl_next((T)t_now) : (T)t_now);
        }
    } else if (a.mode == 1) {
        // _select_initial_step (misc.py:36-77) in T: d0 = ||y0 / scale||, d1 = ||f0 / scale||
        const T d0 = (T)row_norm(s0, s.row_len, a.tkind), d1 = (T)row_norm(s1, s.row_len, a.tkind);
        T h0;
        if (d0 < (T)1e-5 || d1 < (T)1e-5) h0 = (T)1e-6;
        else h0 = ((T)0.01 * d0) / d1;
        h0 = h0 < (T)0 ? -h0 : h0;
        s.h0[r] = (double)h0;
        s.dt[r] = (double)d1;                 // parked for mode 2; no step is prepared before it
        s.bad_y[r] = sb != 0.0 ? 1 : 0;
        static_cast<T*>(a.dts_out)[r] = (T)((double)h0 * c.time_sign);
        static_cast<T*>(a.times)[r] = (T)c.time_sign * (T)(s.t0[r] + (double)h0);
        return;
    } else if (a.mode == 2) {
        const T h0 = (T)s.h0[r];
        const T d1 = (T)s.dt[r];              // (parked by mode 1)
        const T d2n = (T)row_norm(s0, s.row_len, a.tkind);
        T d2 = d2n / h0;
        d2 = d2 < (T)0 ? -d2 : d2;
        T h1;
        // (Python's max / min on host scalars: max(a, b) = b if b > a else a, min(a, b) = b if b < a else a)
        if (d1 <= (T)1e-15 && d2 <= (T)1e-15) {
            const T small = (T)1e-6, v = h0 * (T)1e-3;
            h1 = v > small ? v : small;
        } else {
            const T m = d2 > d1 ? d2 : d1;
            const T q = ((T)1 / m) * (T)0.01;           // `0.01 / x` = x.reciprocal() * 0.01 (_scalars.rdiv)
            const double e = 1.0 / (double)(s.order + 1);
            if (e == 0.5) h1 = sizeof(T) == 4 ? (T)__builtin_sqrtf((float)q) : (T)__builtin_sqrt((double)q);   // ATen's sqrt
            else h1 = (T)pow((double)q, e);                                                    // raised in double (_scalars.power)
        }
        h1 = h1 < (T)0 ? -h1 : h1;
        const T big = (T)100 * h0;
        const T fs = h1 < big ? h1 : big;
        s.dt[r] = (double)fs;
    } else {
        s.bad_y[r] = sb != 0.0 ? 1 : 0;
    }
    if (live) {
        err = row_prepare<T, POINTS, IMPULSE>(a, r, lo, hi);
    } else {
        row_freeze<T>(a.dts_out, a.times, c.n_times, s.n_rows, c.time_sign, s.t0[r], r);
        // (a row that had finished before a trial step is only frozen again: its on_point stays as it is)
        if constexpr (POINTS) if (was_live || a.mode != 0) a.pts.on_point[r] = 0;
    }
}

template <typename T, bool WAVE, bool POINTS, bool IMPULSE>
__global__ __launch_bounds__(kBlock) void row_ctrl_kernel(const RowCtrlArgsOf<POINTS> a) {
    static_assert(POINTS || !IMPULSE, "IMPULSE is a variant of POINTS");
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t n_rows = a.st.n_rows;
    int64_t r;
    double s0 = 0.0, s1 = 0.0, sb = 0.0;
    const int64_t np = n_rows * a.nch;
    if (WAVE) {
        r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;
        if (r < n_rows) {
            for (int64_t q = lane; q < a.nch; q += kWave) {
                s0 += a.part[r * a.nch + q];
                s1 += a.part[np + r * a.nch + q];
                sb += a.part[2 * np + r * a.nch + q];
            }
        }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        sb = wave_sum(sb);
    } else {
        r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        if (r < n_rows) {
            s0 = a.part[r];
            s1 = a.part[np + r];
            sb = a.part[2 * np + r];
        }
    }
    bool live = false, err = false, jump = false;
    if (r < n_rows && (!WAVE || lane == 0)) {
        row_control<T, POINTS, IMPULSE>(a, r, s0, s1, sb, live, err, jump);
        if (err) atomicMin(a.st.status + 1, (int32_t)r);
    }
    // the active-row count, and with POINTS the count of rows that jumped: one atomic per wave each
    const uint64_t m = __ballot(live ? 1 : 0);
    if (lane == 0 && m) atomicAdd(a.st.status, (int32_t)__popcll(m));
    if constexpr (POINTS) {
        const uint64_t mj = __ballot(jump ? 1 : 0);
        if (lane == 0 && mj) atomicAdd(a.st.status + 2, (int32_t)__popcll(mj));
    }
}

// ------------------------------------------------------------------------------------------------
// Dense output + commit of the accepted rows (rk_common.py:243-250, 335-352, interp.py:25-48): the quartic of the step
// at every output time in (tprev_r, t0_r] — out_lo[r] .. out_hi[r] - 1 — written to solution[j, r, :], then
// y0 <- y1 and f0 <- f1 (FSAL) for the row.  Rows without an accepted step are not touched.
// ------------------------------------------------------------------------------------------------
template <typename T, int NT>
struct RowDenseArgs {
    T* sol;                           // [n_out, B, L]
    T* y0;                            // updated in place
    const T* y1;
    T* f0;                            // updated in place
    const T* f1;
    const T* k[NT];
    T c[NT];                          // fl_T(c_mid)
    const T* dts;                     // sign * T(dt) of the step just taken
    const double* tgrid;
    const double* tprev;
    const double* t1;
    const int32_t* accepted;
    const int32_t* out_lo;
    const int32_t* out_hi;
    int64_t row_len;                  // E units
    int64_t n_rows;
    int64_t n;                        // B * L elements of T
};

// The mapped form (MAPPED) serves a compacted batch (`odeint_rowwise(compact=...)`): the state holds n_rows compact rows,
// the solution keeps all sol_rows original ones, and output j of compact row r goes to sol[j, row_map[r], :]; y0 and f0
// are committed at the compact index.  The plain form is the arithmetic and the addressing it always was.
template <typename T, int NT>
struct RowDenseMappedArgs : RowDenseArgs<T, NT> {
    const int32_t* row_map;           // [n_rows] solution row of each compact row
    int64_t sol_rows;                 // rows of sol: [n_out, sol_rows, L]
};

template <typename T, int NT, bool VEC, bool MAPPED, typename Args>
__device__ __forceinline__ void row_dense_commit_body(const Args& a) {
    using E = typename std::conditional<VEC, typename VecOf<T>::type, T>::type;
    constexpr int LV = VEC ? VecOf<T>::L : 1;
    const int64_t ne = a.n / LV;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < ne; i += stride) {
        const int64_t r = i / a.row_len;
        if (!a.accepted[r]) continue;
        const E y1 = reinterpret_cast<const E*>(a.y1)[i];
        const E f1 = reinterpret_cast<const E*>(a.f1)[i];
        const int lo = a.out_lo[r], hi = a.out_hi[r];
        if (hi > lo) {                // (a step without an output time moves 4 words: y1, f1 in, y0, f0 out)
            const E y0 = reinterpret_cast<const E*>(a.y0)[i];
            DenseArgs<T, NT> d;
            const T dtT = a.dts[r];
#pragma unroll
            for (int j = 0; j < NT; ++j) d.c[j] = a.c[j] * dtT;      // fl_T(fl_T(mid_j) * T(dt)) — rk_common.py:365-366
            d.dt = dtT;
            E kk[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) kk[j] = reinterpret_cast<const E*>(a.k[j])[i];
            const E f0 = reinterpret_cast<const E*>(a.f0)[i];
            const Quartic<T, E> q = fit_one<T, NT, E>(d, y0, y1, f0, f1, kk);
            const double ta = a.tprev[r], tb = a.t1[r];
            for (int j = lo; j < hi; ++j) {
                const T x = (T)((a.tgrid[(int64_t)j * a.n_rows + r] - ta) / (tb - ta));   // interp.py:39-40 in W, then T
                if constexpr (MAPPED) {
                    const int64_t at = ((int64_t)j * a.sol_rows + (int64_t)a.row_map[r]) * a.row_len + (i - r * a.row_len);
                    reinterpret_cast<E*>(a.sol)[at] = eval_one<T, E>(q, x);
                } else {
                    reinterpret_cast<E*>(a.sol + (int64_t)j * a.n)[i] = eval_one<T, E>(q, x);
                }
            }
        }
        reinterpret_cast<E*>(a.y0)[i] = y1;
        reinterpret_cast<E*>(a.f0)[i] = f1;
    }
}

template <typename T, int NT, bool VEC>
__global__ __launch_bounds__(kBlock) void row_dense_commit_kernel(const RowDenseArgs<T, NT> a) {
    row_dense_commit_body<T, NT, VEC, false>(a);
}

template <typename T, int NT, bool VEC>
__global__ __launch_bounds__(kBlock) void row_dense_commit_mapped_kernel(const RowDenseMappedArgs<T, NT> a) {
    row_dense_commit_body<T, NT, VEC, true>(a);
}

// ------------------------------------------------------------------------------------------------
// Row gather (the repack of `odeint_rowwise(compact=...)`): dst[m][q, :] = src[m][idx[q], :] for m < NS, one launch
// for up to kMaxGather tensors.  A copy of bits: no arithmetic touches a value.  NS is a template parameter so that the
// pointer arrays of the argument block are indexed by constants (a runtime index would put the block into scratch).
// ------------------------------------------------------------------------------------------------
constexpr int kMaxGather = 4;

template <int NS>
struct RowGatherArgs {
    void* dst[NS];
    const void* src[NS];
    const int32_t* idx;               // [n_idx] source row of each output row
    int64_t row_len;                  // E units
    int64_t ne;                       // n_idx * row_len
};

template <typename E, int NS>
__global__ __launch_bounds__(kBlock) void row_gather_kernel(const RowGatherArgs<NS> a) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.ne; i += stride) {
        const int64_t q = i / a.row_len;
        const int64_t from = (int64_t)a.idx[q] * a.row_len + (i - q * a.row_len);
#pragma unroll
        for (int m = 0; m < NS; ++m) static_cast<E*>(a.dst[m])[i] = static_cast<const E*>(a.src[m])[from];
    }
}

// ------------------------------------------------------------------------------------------------
// Row select: dst[r, :] = src[r, :] where mask[r] != 0.  A copy of bits; a row outside the mask is neither read nor
// written (its src may hold anything, NaN included).
// ------------------------------------------------------------------------------------------------
struct RowSelectArgs {
    void* dst;
    const void* src;
    const int32_t* mask;              // [n_rows]
    int64_t row_len;                  // E units
    int64_t ne;                       // n_rows * row_len
};

template <typename E>
__global__ __launch_bounds__(kBlock) void row_select_kernel(const RowSelectArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.ne; i += stride) {
        if (a.mask[i / a.row_len]) static_cast<E*>(a.dst)[i] = static_cast<const E*>(a.src)[i];
    }
}

// ------------------------------------------------------------------------------------------------
// Row impulse: y[r, :] += dy[k, o or 0, :] where jumped[r] != 0, with o = row_map[r] (null: r) the row's original index and
// k = dy_index[jump_hit[r], o] the user's entry of the point the step ended on (k < 0: none).  One addition in the state's
// type.  A row outside the mask is neither read nor written, and of `dy` only the rows that are added are read: 3 words per
// element of a row that jumped, none for any other.
// ------------------------------------------------------------------------------------------------
struct RowImpulseArgs {
    void* y;                          // [n_rows, row_len]
    const void* dy;                   // [K, dy_rows, row_len]
    const int32_t* dy_index;          // [K', n_orig]: sorted position -> k, -1 none
    const int32_t* jump_hit;          // [n_rows]
    const int32_t* jumped;            // [n_rows]
    const int32_t* row_map;           // [n_rows] or null
    int64_t dy_rows;                  // 1 or n_orig
    int64_t n_orig;
    int64_t row_len;                  // E units
    int64_t ne;                       // n_rows * row_len
};

template <typename E>
__global__ __launch_bounds__(kBlock) void row_impulse_kernel(const RowImpulseArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.ne; i += stride) {
        const int64_t r = i / a.row_len;
        if (!a.jumped[r]) continue;
        const int64_t o = a.row_map ? a.row_map[r] : r;
        const int64_t k = a.dy_index[(int64_t)a.jump_hit[r] * a.n_orig + o];
        if (k < 0) continue;
        const int64_t src = (k * a.dy_rows + (a.dy_rows == 1 ? 0 : o)) * a.row_len + (i - r * a.row_len);
        static_cast<E*>(a.y)[i] = static_cast<E*>(a.y)[i] + static_cast<const E*>(a.dy)[src];
    }
}

// ------------------------------------------------------------------------------------------------
// Backward of the row-linear operations (differentiable odeint_rowwise, rowwise_autodiff.py).  Every state-sized
// operation of a rowwise trial step is out[r, :] = sum_m w_m[r] X_m[r, :], so its VJP is
//   grad X_m[r, :] = w_m[r] * g[r, :]                       row_scale_many_kernel: g read once, NT tensors written
//   grad s_r = sum_m dw_m/ds[r] * <g[r, :], X_m[r, :]>      row_dot_*_kernel: fp64 dots per row, g read once
// for a per-row scalar s (the first step size).
// ------------------------------------------------------------------------------------------------
template <typename T, int NT>
struct RowScaleArgs {
    T* out[NT];
    const T* g;
    const T* w;                       // [NT, B]
    int64_t n_rows;
    int64_t row_len;                  // in E units
    int64_t n;                        // B * L elements of T
};

// Pure streaming: 1 word read + NT written per element.  A lane keeps its row's NT weights in registers and fetches
// them again only when its grid-stride walk enters another row.
template <typename T, int NT, bool VEC>
__global__ __launch_bounds__(kBlock) void row_scale_many_kernel(const RowScaleArgs<T, NT> a) {
    using E = typename std::conditional<VEC, typename VecOf<T>::type, T>::type;
    constexpr int LV = VEC ? VecOf<T>::L : 1;
    const int64_t ne = a.n / LV;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t r_held = -1;
    T w[NT];
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < ne; i += stride) {
        const E g = reinterpret_cast<const E*>(a.g)[i];
        const int64_t r = i / a.row_len;
        if (r != r_held) {
#pragma unroll
            for (int j = 0; j < NT; ++j) w[j] = a.w[(int64_t)j * a.n_rows + r];
            r_held = r;
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) reinterpret_cast<E*>(a.out[j])[i] = g * w[j];
    }
}

template <typename T, int NT>
struct RowDotArgs {
    const T* g;
    const T* x[NT];
    int64_t row_len;                  // in E units
    int64_t n_rows;
    int64_t chunk;                    // long rows: E units per workgroup
    int nch;                          // chunks per row (1 for short rows and for long rows of one chunk)
    int group;                        // short rows: lanes per row (power of two <= 64)
    double* out;                      // nch == 1: [NT, B] results; else [NT, B * nch] partials
};

template <typename T, int NT, typename E>
__device__ __forceinline__ void row_dot_elem(const RowDotArgs<T, NT>& a, int64_t i, double (&acc)[NT]) {
    constexpr int LV = sizeof(E) / sizeof(T);
    const E gv = reinterpret_cast<const E*>(a.g)[i];
    E xv[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) xv[j] = reinterpret_cast<const E*>(a.x[j])[i];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        if constexpr (LV == 1) {
            acc[j] += (double)gv * (double)xv[j];
        } else {
#pragma unroll
            for (int q = 0; q < LV; ++q) acc[j] += (double)gv[q] * (double)xv[j][q];
        }
    }
}

// short rows: the geometry of row_reduce_wave_kernel
template <typename T, int NT, bool VEC>
__global__ __launch_bounds__(kBlock) void row_dot_wave_kernel(const RowDotArgs<T, NT> a) {
    using E = typename std::conditional<VEC, typename VecOf<T>::type, T>::type;
    const int g = a.group;
    const int lane = threadIdx.x & (g - 1);
    const int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / g;
    double acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = 0.0;
    if (r < a.n_rows) {
        const int64_t base = r * a.row_len;
        for (int64_t e = lane; e < a.row_len; e += g) row_dot_elem<T, NT, E>(a, base + e, acc);
    }
    for (int off = g >> 1; off > 0; off >>= 1) {
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] += __shfl_xor(acc[j], off, kWave);
    }
    if (lane == 0 && r < a.n_rows) {
#pragma unroll
        for (int j = 0; j < NT; ++j) a.out[(int64_t)j * a.n_rows + r] = acc[j];
    }
}

// long rows: one workgroup per (row, chunk), the geometry of row_reduce_chunk_kernel
template <typename T, int NT, bool VEC>
__global__ __launch_bounds__(kBlock) void row_dot_chunk_kernel(const RowDotArgs<T, NT> a) {
    using E = typename std::conditional<VEC, typename VecOf<T>::type, T>::type;
    __shared__ double red[NT * (kBlock / kWave)];
    const int64_t b = blockIdx.x;
    const int64_t r = b / a.nch, c = b - r * a.nch;
    double acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = 0.0;
    const int64_t lo = c * a.chunk;
    const int64_t hi = lo + a.chunk < a.row_len ? lo + a.chunk : a.row_len;
    const int64_t base = r * a.row_len;
    for (int64_t e = lo + threadIdx.x; e < hi; e += kBlock) row_dot_elem<T, NT, E>(a, base + e, acc);
    block_sum<NT>(acc, red);
    if (threadIdx.x == 0) {
        const int64_t nb = a.n_rows * a.nch;
#pragma unroll
        for (int j = 0; j < NT; ++j) a.out[(int64_t)j * nb + b] = acc[j];
    }
}

// out[j, r] = the row's nch partials added by one wave in a fixed order (as row_ctrl_kernel adds a long row's norms)
struct RowDotFinalizeArgs {
    const double* part;               // [n_x, B * nch]
    int nch;
    int n_x;
    int64_t n_rows;
    double* out;                      // [n_x, B]
};

__global__ __launch_bounds__(kBlock) void row_dot_finalize_kernel(const RowDotFinalizeArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;
    const int64_t np = a.n_rows * a.nch;
    for (int j = 0; j < a.n_x; ++j) {
        double s = 0.0;
        if (r < a.n_rows)
            for (int64_t q = lane; q < a.nch; q += kWave) s += a.part[(int64_t)j * np + r * a.nch + q];
        s = wave_sum(s);
        if (lane == 0 && r < a.n_rows) a.out[(int64_t)j * a.n_rows + r] = s;
    }
}

}  // namespace tdeq
