// tdeq_kernels_rowwise_steps.hpp — gfx950 device code of the per-row step options of the rowwise family
// (torchdiffeq_amd/rowwise.py: `min_step`, `max_step` as [B] vectors, `step_t`, `jump_t`).
//
//   row_ctrl_points_kernel   the per-row controller (row_ctrl_kernel) with the row's own step bounds and the row's own
//                            points: times a step must end on (`step_t`) and times where func is discontinuous
//                            (`jump_t`).  A prepared step that would pass the row's next point is cut short at it
//                            (rk_common.py:289-309); an accepted cut step ends on the point's own bits and moves the
//                            row's index (rk_common.py:343-352).  In mode 0 it also reports which rows ended on a jump
//                            point and the time vector of the one extra evaluation of func that follows.
//   row_select_kernel        dst[r, :] = src[r, :] for the rows of a mask: how the re-evaluated f0 of the rows that jumped
//                            is taken, and nothing of any other row.
//   row_impulse_kernel       y[r, :] += dy[k, row, :] for the rows of the same mask (`jump_dy`): the state impulse of the jump
//                            point the row's step ended on, k looked up from the position the controller reported.
//
// IMPULSE (a solve with `jump_dy`) is a compile-time flag of the controller, as ROWTOL is of the row reductions: false is the
// kernel without it.  true tests the jump table with `t0 < p <= t0 + dt` — a step that lands on a point exactly is a step
// onto it, or the row's index would stick there and the dose and every later one be lost; such a step keeps its dt (it ends
// on the point's bits already) — and an accepted step onto a jump point writes jump_hit[r], the position of the point in the
// row's sorted column.
//
// Modes 1, 2 and 3 run `row_control` for their norms and heuristics; what depends on the bounds, the points or the end of
// an accepted step — mode 0 and the prepared step — is restated here on the `ctl_*` helpers, with the row's own bounds.
// (`base.c` carries the bounds (-inf, inf), so that the scalar clamp inside `row_control` leaves every dt as it is.)
#pragma once

#include "tdeq_kernels_rowwise.hpp"

namespace tdeq {

struct RowCtrlPointsArgs {
    RowCtrlArgs base;                 // status: [3] = {active rows, first row in error, rows that jumped in this launch}
    double lo, hi;                    // the scalar bounds, for a null vector
    const double* step_t;             // [n_step, n_rows] sorted per row, padded with +inf; null: none
    const double* jump_t;             // [n_jump, n_rows]
    const int32_t* step_count;        // [n_rows] points of the row (null with a null table)
    const int32_t* jump_count;
    int32_t* next_step;               // [n_rows] index of the row's next point (-1 for a row without points)
    int32_t* next_jump;
    double* clip_t;                   // [n_rows] the point the prepared step ends on (written when on_point != 0)
    int32_t* on_point;                // [n_rows] the prepared step: 0 not cut, 1 cut at a step point, 2 at a jump point
    const double* min_step;           // [n_rows]; null: lo
    const double* max_step;           // [n_rows]; null: hi
    int32_t* jumped;                  // [n_rows] mode 0, every row: the accepted step ended on a jump point
    void* jump_times;                 // [n_rows] of T, mode 0: sign * next_T(T(t0_r)) (ctl_next) where jumped, else sign * T(t0_r)
    int32_t* jump_hit;                // [n_rows] IMPULSE, mode 0, rows that jumped: next_jump[r] before it moved on
};

// the next step size of the I-controller (misc.py:85-95) in host doubles, before the clamp: the expressions of row_control
__device__ __forceinline__ double row_next_dt(const tdeq_step_ctrl& c, double step_dt, double ratio) {
    if (ratio == 0.0) return step_dt * c.ifactor;
    const double dfactor = ratio < 1.0 ? 1.0 : c.dfactor;
    const double scaled = c.safety / pow(ratio, c.exponent);
    return step_dt * ctl_nan_min(c.ifactor, ctl_nan_max(scaled, dfactor));
}

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

// row_prepare with the row's bounds [lo, hi] (rk_common.py:266-287), then the prepared step cut short at the row's next
// step point and at its next jump point, which wins (rk_common.py:289-309); returns code != 0
template <typename T, bool IMPULSE>
__device__ __forceinline__ bool row_prepare_points(const RowCtrlPointsArgs& a, int64_t r, double lo, double hi) {
    const RowCtrlArgs& b = a.base;
    const tdeq_step_ctrl& c = b.c;
    double dt = b.dt[r];
    if (!__builtin_isfinite(dt)) dt = lo;
    dt = ctl_clamp(dt, lo, hi);
    b.dt[r] = dt;
    const double t0 = b.t0[r];
    static_cast<T*>(b.dts_out)[r] = (T)dt * (T)c.time_sign;
    for (int i = 0; i < c.n_times; ++i) static_cast<T*>(b.times)[i * b.n_rows + r] = ctl_stage_time<T>(c, t0, dt, i);
    int code = 0;
    if (b.bad_y[r]) code = 3;
    if (!(t0 + dt > t0)) code = 1;
    if (b.since[r] >= b.max_num_steps) code = 2;
    b.code[r] = code;
    double t1 = 0.0, p;
    int on = 0;
    if (row_point_inside(a.step_t, a.step_count, a.next_step, r, b.n_rows, t0, dt, p)) {
        on = 1;
        t1 = p;
        dt = p - t0;
    }
    if (row_point_inside<IMPULSE>(a.jump_t, a.jump_count, a.next_jump, r, b.n_rows, t0, dt, p)) {
        on = 2;
        t1 = p;
        // (a step that lands on the point keeps its size: p - t0 may round above dt, hence above max_step, and a step above
        //  the ceiling is never accepted)
        if (!IMPULSE || p < t0 + dt) dt = p - t0;
    }
    a.on_point[r] = on;
    if (on) {
        a.clip_t[r] = t1;
        b.dt[r] = dt;
        static_cast<T*>(b.dts_out)[r] = (T)dt * (T)c.time_sign;
        for (int i = 0; i < c.n_times; ++i)
            static_cast<T*>(b.times)[i * b.n_rows + r] = row_stage_time_to<T>(c, t0, dt, t1, i);
    }
    return code != 0;
}

// row_control with the row's bounds and points; `jump`: the row's accepted step ended on a jump point
template <typename T, bool IMPULSE>
__device__ __forceinline__ void row_control_points(const RowCtrlPointsArgs& a, int64_t r, double s0, double s1, double sb,
                                                   bool& live, bool& err, bool& jump) {
    const RowCtrlArgs& b = a.base;
    const tdeq_step_ctrl& c = b.c;
    const double lo = a.min_step ? a.min_step[r] : a.lo, hi = a.max_step ? a.max_step[r] : a.hi;
    jump = false;
    if (b.mode != 0) {
        row_control<T>(b, r, s0, s1, sb, live, err);      // (modes 2, 3: its prepared step is replaced below)
        if (b.mode != 1) {
            if (live) err = row_prepare_points<T, IMPULSE>(a, r, lo, hi);
            else a.on_point[r] = 0;
        }
        return;
    }
    live = b.active[r] != 0;
    err = false;
    T tj = (T)b.t0[r];
    if (!live) {
        b.accepted[r] = 0;
        row_freeze<T>(b, r);
    } else {
        const double ratio = row_norm(s0, b.row_len, b.tkind);
        const double step_t0 = b.t0[r], step_dt = b.dt[r];
        bool accept = ratio <= 1.0;
        if (step_dt > hi) accept = false;
        if (step_dt <= lo) accept = true;
        const double dt_next = ctl_clamp(row_next_dt(c, step_dt, ratio), lo, hi);
        b.ratio_out[r] = ratio;
        b.since[r] += 1;
        b.accepted[r] = accept ? 1 : 0;
        if (accept) {
            const int on = a.on_point[r];
            const double t1 = on ? a.clip_t[r] : step_t0 + step_dt;      // a cut step ends on the point's own bits
            b.tprev[r] = step_t0;
            b.t0[r] = t1;
            b.n_acc[r] += 1;
            const int lo = b.next_out[r];
            int hi = lo;
            while (hi < b.n_out && b.tgrid[(int64_t)hi * b.n_rows + r] <= t1) ++hi;
            b.out_lo[r] = lo;
            b.out_hi[r] = hi;
            b.next_out[r] = hi;
            if (hi > lo) b.since[r] = 0;
            b.bad_y[r] = sb != 0.0 ? 1 : 0;
            if (on == 1 && a.next_step[r] != a.step_count[r] - 1) a.next_step[r] += 1;
            if (on == 2) {
                if (IMPULSE) a.jump_hit[r] = a.next_jump[r];
                if (a.next_jump[r] != a.jump_count[r] - 1) a.next_jump[r] += 1;
                jump = true;
            }
            tj = jump ? ctl_next((T)t1) : (T)t1;
            if (hi >= b.n_out) {
                live = false;
                b.active[r] = 0;
            }
        } else {
            b.n_rej[r] += 1;
        }
        b.dt[r] = dt_next;
        if (live) {
            err = row_prepare_points<T, IMPULSE>(a, r, lo, hi);
        } else {
            row_freeze<T>(b, r);
            a.on_point[r] = 0;
        }
    }
    a.jumped[r] = jump ? 1 : 0;
    static_cast<T*>(a.jump_times)[r] = (T)c.time_sign * tj;
}

// The lane-per-row and wave-per-row forms, the sums and the status protocol of row_ctrl_kernel, plus status[2].
template <typename T, bool WAVE, bool IMPULSE>
__global__ __launch_bounds__(kBlock) void row_ctrl_points_kernel(const RowCtrlPointsArgs a) {
    const RowCtrlArgs& b = a.base;
    const int lane = threadIdx.x & (kWave - 1);
    int64_t r;
    double s0 = 0.0, s1 = 0.0, sb = 0.0;
    const int64_t np = b.n_rows * b.nch;
    if (WAVE) {
        r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;
        if (r < b.n_rows) {
            for (int64_t q = lane; q < b.nch; q += kWave) {
                s0 += b.part[r * b.nch + q];
                s1 += b.part[np + r * b.nch + q];
                sb += b.part[2 * np + r * b.nch + q];
            }
        }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        sb = wave_sum(sb);
    } else {
        r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        if (r < b.n_rows) {
            s0 = b.part[r];
            s1 = b.part[np + r];
            sb = b.part[2 * np + r];
        }
    }
    bool live = false, err = false, jump = false;
    if (r < b.n_rows && (!WAVE || lane == 0)) {
        row_control_points<T, IMPULSE>(a, r, s0, s1, sb, live, err, jump);
        if (b.mode == 1) b.dt[r] = (double)(T)row_norm(s1, b.row_len, b.tkind);     // d1 for mode 2
        if (err) atomicMin(b.status + 1, (int32_t)r);
    }
    // the two counts: one atomic per wave each
    const uint64_t m = __ballot(live ? 1 : 0);
    if (lane == 0 && m) atomicAdd(b.status, (int32_t)__popcll(m));
    const uint64_t mj = __ballot(jump ? 1 : 0);
    if (lane == 0 && mj) atomicAdd(b.status + 2, (int32_t)__popcll(mj));
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

}  // namespace tdeq
