// tdeq_abi_rowwise.hpp — extern "C" entry points of the per-row step control (tdeq_kernels_rowwise.hpp, declared in
// include/tdeq_hip.h).  Included by tdeq_abi.hip after its anonymous namespace, whose dispatch helpers it shares: host-side
// validation, launch geometry, template dispatch.  No allocation, no synchronisation.
#pragma once

#include "tdeq_kernels_rowwise.hpp"
#include "tdeq_kernels_rowwise_event.hpp"
#include "tdeq_kernels_rowwise_dense.hpp"

namespace {
using namespace tdeq;

// (the run-time choices of a launch — real_dtype, flag, terms, real_dtype_terms — and all_aligned / Ptrs are those of
//  tdeq_abi.hip: every helper calls f with a tag and returns its status)

// ---- the 16-byte decision ---------------------------------------------------------------------------------------------
// 16-byte elements when a row is a whole number of them (an element then never straddles two rows)
template <typename T>
int row_lanes(int64_t row_len) {
    return row_len % VecOf<T>::L == 0 ? VecOf<T>::L : 1;
}

// A launch takes 16-byte elements when the row is a whole number of them and every pointer is `aligned`: row_len_e
// becomes the row length in the launch's elements, and f(std::bool_constant<VEC>{}) launches.
template <typename T, typename F>
int row_vec(int64_t row_len, bool aligned, int64_t& row_len_e, F f) {
    const int lv = row_lanes<T>(row_len);
    const bool vec = lv > 1 && aligned;
    row_len_e = vec ? row_len / lv : row_len;
    return flag(vec, f);
}

// The same decision for the copy-style kernels, which are templated on the element alone: f(E{}, row_len_e) with
// E = T or VecOf<T>::type.
template <typename F>
int row_elem(int dtype, int64_t row_len, bool aligned, F f) {
    return real_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        const int lv = row_lanes<T>(row_len);
        return lv > 1 && aligned ? f(typename VecOf<T>::type{}, row_len / lv) : f(t, row_len);
    });
}

// Reduction geometry of a row: a function of (L, dtype) only, so that a row's sums never depend on B.
struct RowGeom {
    int lv;           // T elements per E element
    int64_t nv;       // E elements per row
    int group;        // short rows: lanes per row; 0 = long row (one workgroup per chunk, also when nch == 1)
    int64_t chunk;    // long rows: E elements per workgroup
    int64_t nch;      // partials per row
};

template <typename T>
RowGeom row_geom(int64_t row_len) {
    RowGeom g;
    g.lv = row_lanes<T>(row_len);
    g.nv = row_len / g.lv;
    if (g.nv <= kRowWaveMax) {
        const int64_t want = (g.nv + 3) / 4;
        int grp = 1;
        while (grp < want && grp < kWave) grp <<= 1;
        g.group = grp;
        g.chunk = g.nv;
        g.nch = 1;
    } else {
        g.group = 0;
        g.chunk = 8 * kBlock;
        g.nch = (g.nv + g.chunk - 1) / g.chunk;
    }
    return g;
}

inline RowGeom row_geom(int64_t row_len, int dtype) {
    return dtype == TDEQ_F32 ? row_geom<float>(row_len) : row_geom<double>(row_len);
}

template <typename T, int NT>
int row_combine_n(const tdeq_multi_out* outs, int n_out, const void* y0, const void* acc_in, const void* const* k,
                  const void* dts, const int32_t* active, int64_t n_rows, int64_t row_len, hipStream_t s) {
    RowMultiArgs<T, NT> a;
    a.y0 = static_cast<const T*>(y0);
    a.acc_in = static_cast<const T*>(acc_in);
    for (int j = 0; j < NT; ++j) a.k[j] = static_cast<const T*>(k[j]);
    a.add_y0 = 0;
    bool aligned = all_aligned(y0, acc_in, Ptrs{k, NT});
    for (int o = 0; o < kMaxMultiOut; ++o) {
        const bool live = o < n_out;
        a.out[o] = live ? static_cast<T*>(outs[o].out) : nullptr;
        a.mask[o] = live ? outs[o].mask : 0u;
        if (live && outs[o].add_y0) a.add_y0 |= 1u << o;
        for (int j = 0; j < NT; ++j) a.c[o][j] = live ? (T)outs[o].coef[j] : (T)0;
        aligned = aligned && aligned16(a.out[o]);
    }
    a.n_out = n_out;
    a.dts = static_cast<const T*>(dts);
    a.active = active;
    a.n = n_rows * row_len;
    return row_vec<T>(row_len, aligned, a.row_len, [&](auto vec) {
        hipLaunchKernelGGL((row_combine_kernel<T, NT, decltype(vec)::value>), dim3(stream_grid(n_rows * a.row_len, kBlock)),
                           dim3(kBlock), 0, s, a);
        return check_launch();
    });
}

template <typename T, int NT, int MODE, bool PARTIAL, bool ROWTOL>
int row_reduce_launch(RowRedArgsOf<T, NT, ROWTOL>& a, const RowGeom& g, bool vec, hipStream_t s) {
    return flag(vec, [&](auto v) {
        constexpr bool VEC = decltype(v)::value;
        if (g.group > 0) {            // short row; a long row of one chunk (1024 < nv <= 2048) takes the chunk kernel,
            const int64_t threads = a.n_rows * g.group;  // whose part[q * B + r] is what the lane-per-row controller reads
            const dim3 grid((unsigned)((threads + kBlock - 1) / kBlock));
            a.group = g.group;
            a.nch = 1;
            hipLaunchKernelGGL((row_reduce_wave_kernel<T, NT, MODE, PARTIAL, VEC, ROWTOL>), grid, dim3(kBlock), 0, s, a);
        } else {
            a.chunk = g.chunk;
            a.nch = (int)g.nch;
            const dim3 grid((unsigned)(a.n_rows * g.nch));
            hipLaunchKernelGGL((row_reduce_chunk_kernel<T, NT, MODE, PARTIAL, VEC, ROWTOL>), grid, dim3(kBlock), 0, s, a);
        }
        return check_launch();
    });
}

// The tolerances of one reduce launch: the two scalars of tdeq_row_reduce, or the two [n_rows] device vectors of
// tdeq_row_reduce_tol.
struct RowTols {
    double rtol, atol;
    const void* rtol_rows;
    const void* atol_rows;
};

template <typename T, int NT, bool ROWTOL>
int row_reduce_n(int mode, const void* y0, const void* y1, const void* partial, const void* const* k,
                 const double* coef, const void* dts, const int32_t* active, const RowTols& tol, int64_t n_rows,
                 int64_t row_len, double* part, hipStream_t s) {
    const RowGeom g = row_geom<T>(row_len);
    RowRedArgsOf<T, NT, ROWTOL> a;
    a.y0 = static_cast<const T*>(y0);
    a.y1 = static_cast<const T*>(y1);
    a.partial = static_cast<const T*>(partial);
    for (int j = 0; j < (NT > 0 ? NT : 1); ++j) {
        a.k[j] = j < NT ? static_cast<const T*>(k[j]) : nullptr;
        a.c[j] = j < NT ? (T)coef[j] : (T)0;
    }
    a.dts = static_cast<const T*>(dts);
    a.active = active;
    if constexpr (ROWTOL) {
        a.rtol = (T)0;                // (not read)
        a.atol = (T)0;
        a.rtol_rows = static_cast<const T*>(tol.rtol_rows);
        a.atol_rows = static_cast<const T*>(tol.atol_rows);
    } else {
        a.rtol = (T)tol.rtol;
        a.atol = (T)tol.atol;
    }
    a.row_len = g.nv;
    a.n_rows = n_rows;
    a.chunk = g.chunk;
    a.nch = (int)g.nch;
    a.group = g.group;
    a.part = part;
    const bool vec = g.lv > 1 && all_aligned(y0, y1, partial, Ptrs{k, NT});
    if (g.lv > 1 && !vec) return TDEQ_EINVAL;      // (the geometry, hence the sums, must not depend on alignment)
    if constexpr (NT == 0) {
        if (mode == 1) return row_reduce_launch<T, NT, 1, false, ROWTOL>(a, g, vec, s);
        if (mode == 2) return row_reduce_launch<T, NT, 2, false, ROWTOL>(a, g, vec, s);
        return TDEQ_EINVAL;
    } else {
        if (mode != 0) return TDEQ_EINVAL;
        return partial ? row_reduce_launch<T, NT, 0, true, ROWTOL>(a, g, vec, s)
                       : row_reduce_launch<T, NT, 0, false, ROWTOL>(a, g, vec, s);
    }
}

// what the two reduce entry points share: the argument checks (> 0: nothing to do, no row), then the launch
template <bool ROWTOL>
int row_reduce_entry(int mode, const void* y0, const void* y1, const void* partial, const void* const* k,
                     const double* coef, int n_terms, const void* dts, const int32_t* active, const RowTols& tol,
                     int64_t n_rows, int64_t row_len, double* part, size_t part_bytes, int dtype, void* stream) {
    if (!y0 || !y1 || !part || n_rows < 0 || row_len < 1 || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (mode < 0 || mode > 2 || n_terms < 0 || n_terms > TDEQ_MAX_TERMS) return TDEQ_EINVAL;
    if (mode == 0 && (n_terms < 1 || !k || !coef || !dts || !active)) return TDEQ_EINVAL;
    if (mode != 0 && (n_terms != 0 || !partial)) return TDEQ_EINVAL;
    for (int j = 0; j < n_terms; ++j) if (!k[j]) return TDEQ_EINVAL;
    const int64_t nch = row_geom(row_len, dtype).nch;
    if (part_bytes < (size_t)(3 * n_rows * nch) * sizeof(double)) return TDEQ_EWORKSPACE;
    if (n_rows == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype_terms<0>(dtype, n_terms, [&](auto t, auto n) {
        return row_reduce_n<decltype(t), decltype(n)::value, ROWTOL>(mode, y0, y1, partial, k, coef, dts, active, tol,
                                                                     n_rows, row_len, part, s);
    });
}

// one wave per row when a row has several partials to add, one lane per row otherwise
template <typename T, bool POINTS, bool IMPULSE>
int row_control_launch(const RowCtrlArgsOf<POINTS>& a, hipStream_t s) {
    if (a.nch > 1) {
        const dim3 grid((unsigned)((a.st.n_rows * kWave + kBlock - 1) / kBlock));
        hipLaunchKernelGGL((row_ctrl_kernel<T, true, POINTS, IMPULSE>), grid, dim3(kBlock), 0, s, a);
    } else {
        const dim3 grid((unsigned)((a.st.n_rows + kBlock - 1) / kBlock));
        hipLaunchKernelGGL((row_ctrl_kernel<T, false, POINTS, IMPULSE>), grid, dim3(kBlock), 0, s, a);
    }
    return check_launch();
}

// The inputs of a step's quartic, which the dense-commit and event-fit argument blocks name alike (P = void where the
// kernel also writes y0 and f0, const void where it only reads them); their 16-byte decision includes the output.
template <typename T, int NT, typename A, typename P>
bool row_quartic_args(A& a, const void* out, P* y0, const void* y1, P* f0, const void* f1, const void* const* k,
                      const double* coef, const void* dts) {
    a.y0 = static_cast<decltype(a.y0)>(y0);
    a.y1 = static_cast<const T*>(y1);
    a.f0 = static_cast<decltype(a.f0)>(f0);
    a.f1 = static_cast<const T*>(f1);
    for (int j = 0; j < NT; ++j) {
        a.k[j] = static_cast<const T*>(k[j]);
        a.c[j] = (T)coef[j];
    }
    a.dts = static_cast<const T*>(dts);
    return all_aligned(out, y0, y1, f0, f1, Ptrs{k, NT});
}

// tdeq_row_dense_commit and (MAPPED: row_map, sol_rows) tdeq_row_dense_commit_mapped
template <typename T, int NT, bool MAPPED>
int row_dense_n(void* sol, const int32_t* row_map, int64_t sol_rows, void* y0, const void* y1, void* f0, const void* f1,
                const void* const* k, const double* coef, const void* dts, const tdeq_row_state* st, hipStream_t s) {
    typename std::conditional<MAPPED, RowDenseMappedArgs<T, NT>, RowDenseArgs<T, NT>>::type a;
    a.sol = static_cast<T*>(sol);
    const bool aligned = row_quartic_args<T, NT>(a, sol, y0, y1, f0, f1, k, coef, dts);
    a.tgrid = st->tgrid;
    a.tprev = st->tprev;
    a.t1 = st->t0;
    a.accepted = st->accepted;
    a.out_lo = st->out_lo;
    a.out_hi = st->out_hi;
    a.n_rows = st->n_rows;
    a.n = st->n_rows * st->row_len;
    if constexpr (MAPPED) {
        a.row_map = row_map;
        a.sol_rows = sol_rows;
    }
    return row_vec<T>(st->row_len, aligned, a.row_len, [&](auto vec) {
        constexpr bool VEC = decltype(vec)::value;
        const dim3 grid(stream_grid(a.n_rows * a.row_len, kBlock));
        if constexpr (MAPPED) hipLaunchKernelGGL((row_dense_commit_mapped_kernel<T, NT, VEC>), grid, dim3(kBlock), 0, s, a);
        else hipLaunchKernelGGL((row_dense_commit_kernel<T, NT, VEC>), grid, dim3(kBlock), 0, s, a);
        return check_launch();
    });
}

template <typename E, int NS>
int row_gather_n(void* const* dst, const void* const* src, const int32_t* idx, int64_t n_idx, int64_t row_len_e,
                 hipStream_t s) {
    RowGatherArgs<NS> a;
    for (int m = 0; m < NS; ++m) {
        a.dst[m] = dst[m];
        a.src[m] = src[m];
    }
    a.idx = idx;
    a.row_len = row_len_e;
    a.ne = n_idx * row_len_e;
    hipLaunchKernelGGL((row_gather_kernel<E, NS>), dim3(stream_grid(a.ne, kBlock)), dim3(kBlock), 0, s, a);
    return check_launch();
}

template <typename E>
int row_gather_dispatch(void* const* dst, const void* const* src, int n_src, const int32_t* idx, int64_t n_idx,
                        int64_t row_len_e, hipStream_t s) {
    switch (n_src) {
        case 1: return row_gather_n<E, 1>(dst, src, idx, n_idx, row_len_e, s);
        case 2: return row_gather_n<E, 2>(dst, src, idx, n_idx, row_len_e, s);
        case 3: return row_gather_n<E, 3>(dst, src, idx, n_idx, row_len_e, s);
        case 4: return row_gather_n<E, 4>(dst, src, idx, n_idx, row_len_e, s);
    }
    return TDEQ_EINVAL;
}

}  // namespace

int64_t tdeq_row_partials(int64_t row_len, int dtype) {
    if (row_len < 1 || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    return row_geom(row_len, dtype).nch;
}

int tdeq_row_combine(const tdeq_multi_out* outs, int n_out, const void* y0, const void* acc_in, const void* const* k,
                     int n_terms, const void* dts, const int32_t* active, int64_t n_rows, int64_t row_len, int dtype,
                     void* stream) {
    if (!outs || !y0 || !k || !dts || !active || n_rows < 0 || row_len < 1 || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (n_terms < 1 || n_terms > TDEQ_MAX_TERMS || n_out < 1 || n_out > TDEQ_MAX_MULTI_OUT) return TDEQ_EINVAL;
    for (int j = 0; j < n_terms; ++j) if (!k[j]) return TDEQ_EINVAL;
    for (int o = 0; o < n_out; ++o) {
        if (!outs[o].out || outs[o].mask == 0u || (n_terms < 32 && (outs[o].mask >> n_terms) != 0u)) return TDEQ_EINVAL;
    }
    if (n_rows == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype_terms<1>(dtype, n_terms, [&](auto t, auto n) {
        return row_combine_n<decltype(t), decltype(n)::value>(outs, n_out, y0, acc_in, k, dts, active, n_rows, row_len, s);
    });
}

int tdeq_row_reduce(int mode, const void* y0, const void* y1, const void* partial, const void* const* k,
                    const double* coef, int n_terms, const void* dts, const int32_t* active, double rtol, double atol,
                    int64_t n_rows, int64_t row_len, double* part, size_t part_bytes, int dtype, void* stream) {
    return row_reduce_entry<false>(mode, y0, y1, partial, k, coef, n_terms, dts, active, {rtol, atol, nullptr, nullptr},
                                   n_rows, row_len, part, part_bytes, dtype, stream);
}

int tdeq_row_reduce_tol(int mode, const void* y0, const void* y1, const void* partial, const void* const* k,
                        const double* coef, int n_terms, const void* dts, const int32_t* active, const void* rtol_rows,
                        const void* atol_rows, int64_t n_rows, int64_t row_len, double* part, size_t part_bytes, int dtype,
                        void* stream) {
    if (!rtol_rows || !atol_rows) return TDEQ_EINVAL;
    return row_reduce_entry<true>(mode, y0, y1, partial, k, coef, n_terms, dts, active, {0.0, 0.0, rtol_rows, atol_rows},
                                  n_rows, row_len, part, part_bytes, dtype, stream);
}

namespace {
// what tdeq_row_control and tdeq_row_control_points check and fill alike: the status words are reset, and with at least
// one row (`launch`) the argument block is filled
int row_control_args(RowCtrlArgs& a, int mode, const double* part, const tdeq_step_ctrl* ctrl, const tdeq_row_state* st,
                     void* dts_out, void* times_out, int dtype, int n_status, hipStream_t s, bool& launch) {
    launch = false;
    if (!part || !ctrl || !st || !real_dtype_ok(dtype) || mode < 0 || mode > 3) return TDEQ_EINVAL;
    if (st->n_rows < 0 || st->row_len < 1 || st->n_out < 1 || !st->status) return TDEQ_EINVAL;
    if (ctrl->n_times < 1 || ctrl->n_times > TDEQ_MAX_STAGE_TIMES) return TDEQ_EINVAL;
    if (!dts_out || !times_out) return TDEQ_EINVAL;
    // status = {0 active rows, no row in error[, 0 rows that jumped]}
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(st->status), 0, 1, s);
    if (e == hipSuccess)
        e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(st->status + 1), 0x7fffffff, 1, s);
    if (e == hipSuccess && n_status > 2)
        e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(st->status + 2), 0, 1, s);
    if (e != hipSuccess) return (int)e;
    if (st->n_rows == 0) return 0;
    launch = true;
    a.part = part;
    a.nch = (int)row_geom(st->row_len, dtype).nch;
    a.tkind = dtype == TDEQ_F32 ? 1 : 0;
    a.mode = mode;
    a.c = *ctrl;
    a.st = *st;
    a.dts_out = dts_out;
    a.times = times_out;
    return 0;
}
}  // namespace

int tdeq_row_control(int mode, const double* part, const tdeq_step_ctrl* ctrl, const tdeq_row_state* st,
                     void* dts_out, void* times_out, int dtype, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    RowCtrlArgs a;
    bool launch;
    const int e = row_control_args(a, mode, part, ctrl, st, dts_out, times_out, dtype, 2, s, launch);
    if (e || !launch) return e;
    return real_dtype(dtype, [&](auto t) { return row_control_launch<decltype(t), false, false>(a, s); });
}

// ---- per-row step options: tdeq_row_control_points / tdeq_row_select / tdeq_row_impulse -------------------------------
int tdeq_row_control_points(int mode, const double* part, const tdeq_step_ctrl* ctrl, const tdeq_row_state* st,
                            const tdeq_row_points* pts, void* dts_out, void* times_out, int dtype, void* stream) {
    if (!pts || !pts->clip_t || !pts->on_point || !pts->jumped || !pts->jump_times) return TDEQ_EINVAL;
    if (pts->step_t && (pts->n_step < 1 || !pts->step_count || !pts->next_step)) return TDEQ_EINVAL;
    if (pts->jump_t && (pts->n_jump < 1 || !pts->jump_count || !pts->next_jump)) return TDEQ_EINVAL;
    if ((pts->jump_hit != nullptr) != (pts->jump_closed != 0) || (pts->jump_hit && !pts->jump_t)) return TDEQ_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    RowCtrlPointsArgs a;
    bool launch;
    const int e = row_control_args(a, mode, part, ctrl, st, dts_out, times_out, dtype, 3, s, launch);
    if (e || !launch) return e;
    a.pts = *pts;
    return real_dtype(dtype, [&](auto t) {                // a solve with impulses: the closed rule for the jump table
        return pts->jump_hit ? row_control_launch<decltype(t), true, true>(a, s)
                             : row_control_launch<decltype(t), true, false>(a, s);
    });
}

int tdeq_row_select(void* dst, const void* src, const int32_t* mask, int64_t n_rows, int64_t row_len, int dtype,
                    void* stream) {
    if (!dst || !src || !mask || n_rows < 0 || row_len < 1 || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (n_rows == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    RowSelectArgs a;
    a.dst = dst;
    a.src = src;
    a.mask = mask;
    return row_elem(dtype, row_len, all_aligned(dst, src), [&](auto e, int64_t row_len_e) {
        a.row_len = row_len_e;
        a.ne = n_rows * row_len_e;
        hipLaunchKernelGGL((row_select_kernel<decltype(e)>), dim3(stream_grid(a.ne, kBlock)), dim3(kBlock), 0, s, a);
        return check_launch();
    });
}

int tdeq_row_impulse(void* y, const void* dy, int64_t dy_rows, const int32_t* dy_index, int64_t n_orig,
                     const int32_t* jump_hit, const int32_t* jumped, const int32_t* row_map, int64_t n_rows, int64_t row_len,
                     int dtype, void* stream) {
    if (!y || !dy || !dy_index || !jump_hit || !jumped || n_rows < 0 || row_len < 1 || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (n_orig < 1 || (dy_rows != 1 && dy_rows != n_orig)) return TDEQ_EINVAL;
    if (n_rows == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    RowImpulseArgs a;
    a.y = y;
    a.dy = dy;
    a.dy_index = dy_index;
    a.jump_hit = jump_hit;
    a.jumped = jumped;
    a.row_map = row_map;
    a.dy_rows = dy_rows;
    a.n_orig = n_orig;
    return row_elem(dtype, row_len, all_aligned(y, dy), [&](auto e, int64_t row_len_e) {
        a.row_len = row_len_e;
        a.ne = n_rows * row_len_e;
        hipLaunchKernelGGL((row_impulse_kernel<decltype(e)>), dim3(stream_grid(a.ne, kBlock)), dim3(kBlock), 0, s, a);
        return check_launch();
    });
}

int tdeq_row_dense_commit(void* sol, void* y0, const void* y1, void* f0, const void* f1, const void* const* k,
                          const double* coef, int n_terms, const void* dts, const tdeq_row_state* st, int dtype,
                          void* stream) {
    if (!sol || !y0 || !y1 || !f0 || !f1 || !k || !coef || !dts || !st || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (n_terms < 1 || n_terms > TDEQ_MAX_TERMS || st->n_rows < 0 || st->row_len < 1) return TDEQ_EINVAL;
    for (int j = 0; j < n_terms; ++j) if (!k[j]) return TDEQ_EINVAL;
    if (st->n_rows == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype_terms<1>(dtype, n_terms, [&](auto t, auto n) {
        return row_dense_n<decltype(t), decltype(n)::value, false>(sol, nullptr, 0, y0, y1, f0, f1, k, coef, dts, st, s);
    });
}

// ---- compaction of a rowwise batch: tdeq_row_gather / tdeq_row_dense_commit_mapped ------------------------------------
int tdeq_row_gather(void* const* dst, const void* const* src, int n_src, const int32_t* idx, int64_t n_idx,
                    int64_t row_len, int dtype, void* stream) {
    if (!dst || !src || !idx || n_src < 1 || n_src > kMaxGather || n_idx < 0 || row_len < 1 || !real_dtype_ok(dtype))
        return TDEQ_EINVAL;
    for (int m = 0; m < n_src; ++m) if (!dst[m] || !src[m]) return TDEQ_EINVAL;
    if (n_idx == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool aligned = all_aligned(Ptrs{dst, n_src}, Ptrs{src, n_src});
    return row_elem(dtype, row_len, aligned, [&](auto e, int64_t row_len_e) {
        return row_gather_dispatch<decltype(e)>(dst, src, n_src, idx, n_idx, row_len_e, s);
    });
}

int tdeq_row_dense_commit_mapped(void* sol, const int32_t* row_map, int64_t sol_rows, void* y0, const void* y1, void* f0,
                                 const void* f1, const void* const* k, const double* coef, int n_terms, const void* dts,
                                 const tdeq_row_state* st, int dtype, void* stream) {
    if (!sol || !row_map || !y0 || !y1 || !f0 || !f1 || !k || !coef || !dts || !st || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (n_terms < 1 || n_terms > TDEQ_MAX_TERMS || st->n_rows < 0 || st->row_len < 1) return TDEQ_EINVAL;
    if (sol_rows < 1 || sol_rows < st->n_rows) return TDEQ_EINVAL;
    for (int j = 0; j < n_terms; ++j) if (!k[j]) return TDEQ_EINVAL;
    if (st->n_rows == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype_terms<1>(dtype, n_terms, [&](auto t, auto n) {
        return row_dense_n<decltype(t), decltype(n)::value, true>(sol, row_map, sol_rows, y0, y1, f0, f1, k, coef, dts, st,
                                                                   s);
    });
}

// ---- backward of the row-linear operations: tdeq_row_scale_many / tdeq_row_multi_dot ---------------------------------
namespace {

template <typename T, int NT>
int row_scale_n(void* const* outs, const void* g, const void* w, int64_t n_rows, int64_t row_len, hipStream_t s) {
    RowScaleArgs<T, NT> a;
    a.g = static_cast<const T*>(g);
    a.w = static_cast<const T*>(w);
    a.n_rows = n_rows;
    a.n = n_rows * row_len;
    for (int j = 0; j < NT; ++j) a.out[j] = static_cast<T*>(outs[j]);
    return row_vec<T>(row_len, all_aligned(g, Ptrs{outs, NT}), a.row_len, [&](auto vec) {
        hipLaunchKernelGGL((row_scale_many_kernel<T, NT, decltype(vec)::value>),
                           dim3(stream_grid(n_rows * a.row_len, kBlock)), dim3(kBlock), 0, s, a);
        return check_launch();
    });
}

template <typename T, int NT>
int row_dot_n(const void* g, const void* const* x, int64_t n_rows, int64_t row_len, double* out, double* ws,
              hipStream_t s) {
    const RowGeom geo = row_geom<T>(row_len);
    RowDotArgs<T, NT> a;
    a.g = static_cast<const T*>(g);
    for (int j = 0; j < NT; ++j) a.x[j] = static_cast<const T*>(x[j]);
    const bool vec = geo.lv > 1 && all_aligned(g, Ptrs{x, NT});
    if (geo.lv > 1 && !vec) return TDEQ_EINVAL;      // (the geometry, hence the sums, must not depend on alignment)
    a.row_len = geo.nv;
    a.n_rows = n_rows;
    a.chunk = geo.chunk;
    a.nch = (int)geo.nch;
    a.group = geo.group;
    a.out = geo.nch == 1 ? out : ws;                 // one chunk per row: the chunk sums are the results, [NT, B]
    const int e = flag(vec, [&](auto v) {
        constexpr bool VEC = decltype(v)::value;
        if (geo.group > 0) {
            const dim3 grid((unsigned)((n_rows * geo.group + kBlock - 1) / kBlock));
            hipLaunchKernelGGL((row_dot_wave_kernel<T, NT, VEC>), grid, dim3(kBlock), 0, s, a);
        } else {
            hipLaunchKernelGGL((row_dot_chunk_kernel<T, NT, VEC>), dim3((unsigned)(n_rows * geo.nch)), dim3(kBlock), 0, s, a);
        }
        return check_launch();
    });
    if (e || geo.nch == 1) return e;
    RowDotFinalizeArgs f;
    f.part = ws;
    f.nch = (int)geo.nch;
    f.n_x = NT;
    f.n_rows = n_rows;
    f.out = out;
    hipLaunchKernelGGL(row_dot_finalize_kernel, dim3((unsigned)((n_rows * kWave + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       s, f);
    return check_launch();
}

}  // namespace

int tdeq_row_scale_many(void* const* outs, int n_out, const void* g, const void* w, int64_t n_rows, int64_t row_len,
                        int dtype, void* stream) {
    if (!outs || !g || !w || n_rows < 0 || row_len < 0 || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (n_out < 1 || n_out > TDEQ_MAX_TERMS) return TDEQ_EINVAL;
    for (int j = 0; j < n_out; ++j) if (!outs[j]) return TDEQ_EINVAL;
    if (n_rows == 0 || row_len == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype_terms<1>(dtype, n_out, [&](auto t, auto n) {
        return row_scale_n<decltype(t), decltype(n)::value>(outs, g, w, n_rows, row_len, s);
    });
}

size_t tdeq_row_dots_workspace_bytes(int64_t n_rows, int64_t row_len, int n_x, int dtype) {
    if (n_rows < 1 || row_len < 1 || n_x < 1 || !real_dtype_ok(dtype)) return 0;
    const int64_t nch = row_geom(row_len, dtype).nch;
    return nch == 1 ? 0 : (size_t)n_x * (size_t)n_rows * (size_t)nch * sizeof(double);
}

int tdeq_row_multi_dot(const void* g, const void* const* x, int n_x, int64_t n_rows, int64_t row_len, double* out,
                       void* workspace, size_t workspace_bytes, int dtype, void* stream) {
    if (!g || !x || !out || n_rows < 0 || row_len < 0 || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (n_x < 1 || n_x > TDEQ_MAX_TERMS) return TDEQ_EINVAL;
    for (int j = 0; j < n_x; ++j) if (!x[j]) return TDEQ_EINVAL;
    if (n_rows == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (row_len == 0) return (int)hipMemsetAsync(out, 0, (size_t)n_x * (size_t)n_rows * sizeof(double), s);
    const size_t need = tdeq_row_dots_workspace_bytes(n_rows, row_len, n_x, dtype);
    if (need > 0 && (!workspace || workspace_bytes < need)) return TDEQ_EWORKSPACE;
    if (n_rows * row_geom(row_len, dtype).nch > 0x7fffffffLL) return TDEQ_EINVAL;
    double* ws = static_cast<double*>(workspace);
    return real_dtype_terms<1>(dtype, n_x, [&](auto t, auto n) {
        return row_dot_n<decltype(t), decltype(n)::value>(g, x, n_rows, row_len, out, ws, s);
    });
}

// ---- per-row terminal events: tdeq_row_event_detect / tdeq_row_event_fit / tdeq_row_event_eval, and the two of a
// ---- compacted event solve: tdeq_row_event_fit_mapped / tdeq_row_event_eval_mapped -----------------------------------
namespace {

// tdeq_row_event_fit and (MAPPED: row_map, q_rows) tdeq_row_event_fit_mapped
template <typename T, int NT, bool MAPPED>
int row_event_fit_n(void* q, const int32_t* row_map, int64_t q_rows, const int32_t* fired_now, const void* y0,
                    const void* y1, const void* f0, const void* f1, const void* const* k, const double* coef,
                    const void* dts, int64_t n_rows, int64_t row_len, hipStream_t s) {
    typename std::conditional<MAPPED, RowEventFitMappedArgs<T, NT>, RowEventFitArgs<T, NT>>::type a;
    a.q = static_cast<T*>(q);
    const bool aligned = row_quartic_args<T, NT>(a, q, y0, y1, f0, f1, k, coef, dts);
    a.fired_now = fired_now;
    a.n = n_rows * row_len;
    if constexpr (MAPPED) {
        a.row_map = row_map;
        a.q_plane = q_rows * row_len;
    }
    // (16-byte elements: row_len is a whole number of them, so every row start and every plane of q is aligned as q is)
    return row_vec<T>(row_len, aligned, a.row_len, [&](auto vec) {
        constexpr bool VEC = decltype(vec)::value;
        const dim3 grid(stream_grid(n_rows * a.row_len, kBlock));
        if constexpr (MAPPED) hipLaunchKernelGGL((row_event_fit_mapped_kernel<T, NT, VEC>), grid, dim3(kBlock), 0, s, a);
        else hipLaunchKernelGGL((row_event_fit_kernel<T, NT, VEC>), grid, dim3(kBlock), 0, s, a);
        return check_launch();
    });
}

template <typename T>
int row_event_eval_launch(void* out, const void* q, const void* x, const int32_t* mask, int64_t n_rows, int64_t row_len,
                          hipStream_t s) {
    RowEventEvalArgs<T> a;
    a.out = static_cast<T*>(out);
    a.q = static_cast<const T*>(q);
    a.x = static_cast<const T*>(x);
    a.mask = mask;
    a.n = n_rows * row_len;
    return row_vec<T>(row_len, all_aligned(out, q), a.row_len, [&](auto vec) {
        hipLaunchKernelGGL((row_event_eval_kernel<T, decltype(vec)::value>), dim3(stream_grid(n_rows * a.row_len, kBlock)),
                           dim3(kBlock), 0, s, a);
        return check_launch();
    });
}

template <typename T>
int row_event_eval_mapped_launch(void* out, const int32_t* dst_map, const void* q, const int32_t* src_map, int64_t q_rows,
                                 const void* x, int64_t n_idx, int64_t row_len, hipStream_t s) {
    RowEventEvalMappedArgs<T> a;
    a.out = static_cast<T*>(out);
    a.q = static_cast<const T*>(q);
    a.x = static_cast<const T*>(x);
    a.src_map = src_map;
    a.dst_map = dst_map;
    a.q_plane = q_rows * row_len;
    return row_vec<T>(row_len, all_aligned(out, q), a.row_len, [&](auto vec) {
        a.ne = n_idx * a.row_len;
        return flag(dst_map != nullptr, [&](auto dst) {
            hipLaunchKernelGGL((row_event_eval_mapped_kernel<T, decltype(vec)::value, decltype(dst)::value>),
                               dim3(stream_grid(a.ne, kBlock)), dim3(kBlock), 0, s, a);
            return check_launch();
        });
    });
}

}  // namespace

int tdeq_row_event_detect(const void* g1, const int32_t* sign0, const tdeq_step_ctrl* ctrl, const tdeq_row_state* st,
                          void* dts, void* times, int32_t* fired, int32_t* fired_now, double* lo, double* hi, int dtype,
                          void* stream) {
    if (!g1 || !sign0 || !ctrl || !st || !dts || !times || !fired || !fired_now || !lo || !hi || !real_dtype_ok(dtype))
        return TDEQ_EINVAL;
    if (st->n_rows < 0 || !st->accepted || !st->tprev || !st->t0 || !st->active || !st->status) return TDEQ_EINVAL;
    if (ctrl->n_times < 1 || ctrl->n_times > TDEQ_MAX_STAGE_TIMES) return TDEQ_EINVAL;
    if (st->n_rows == 0) return 0;
    RowEventDetectArgs a;
    a.g1 = g1;
    a.sign0 = sign0;
    a.accepted = st->accepted;
    a.tprev = st->tprev;
    a.t0 = st->t0;
    a.active = st->active;
    a.status = st->status;
    a.dts = dts;
    a.times = times;
    a.n_times = ctrl->n_times;
    a.time_sign = ctrl->time_sign;
    a.n_rows = st->n_rows;
    a.fired = fired;
    a.fired_now = fired_now;
    a.lo = lo;
    a.hi = hi;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((a.n_rows + kBlock - 1) / kBlock));
    return real_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL((row_event_detect_kernel<decltype(t)>), grid, dim3(kBlock), 0, s, a);
        return check_launch();
    });
}

int tdeq_row_event_fit(void* q, const int32_t* fired_now, const void* y0, const void* y1, const void* f0, const void* f1,
                       const void* const* k, const double* coef, int n_terms, const void* dts, int64_t n_rows,
                       int64_t row_len, int dtype, void* stream) {
    if (!q || !fired_now || !y0 || !y1 || !f0 || !f1 || !k || !coef || !dts || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (n_terms < 1 || n_terms > TDEQ_MAX_TERMS || n_rows < 0 || row_len < 1) return TDEQ_EINVAL;
    for (int j = 0; j < n_terms; ++j) if (!k[j]) return TDEQ_EINVAL;
    if (n_rows == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype_terms<1>(dtype, n_terms, [&](auto t, auto n) {
        return row_event_fit_n<decltype(t), decltype(n)::value, false>(q, nullptr, 0, fired_now, y0, y1, f0, f1, k, coef,
                                                                        dts, n_rows, row_len, s);
    });
}

int tdeq_row_event_eval(void* out, const void* q, const void* x, const int32_t* mask, int64_t n_rows, int64_t row_len,
                        int dtype, void* stream) {
    if (!out || !q || !x || !mask || n_rows < 0 || row_len < 1 || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (n_rows == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype(dtype, [&](auto t) {
        return row_event_eval_launch<decltype(t)>(out, q, x, mask, n_rows, row_len, s);
    });
}

int tdeq_row_event_fit_mapped(void* q, const int32_t* row_map, int64_t q_rows, const int32_t* fired_now, const void* y0,
                              const void* y1, const void* f0, const void* f1, const void* const* k, const double* coef,
                              int n_terms, const void* dts, int64_t n_rows, int64_t row_len, int dtype, void* stream) {
    if (!q || !row_map || !fired_now || !y0 || !y1 || !f0 || !f1 || !k || !coef || !dts || !real_dtype_ok(dtype))
        return TDEQ_EINVAL;
    if (n_terms < 1 || n_terms > TDEQ_MAX_TERMS || n_rows < 0 || q_rows < 0 || row_len < 1) return TDEQ_EINVAL;
    for (int j = 0; j < n_terms; ++j) if (!k[j]) return TDEQ_EINVAL;
    if (n_rows == 0) return 0;
    if (q_rows < n_rows) return TDEQ_EINVAL;          // (row_map names n_rows different rows of q)
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype_terms<1>(dtype, n_terms, [&](auto t, auto n) {
        return row_event_fit_n<decltype(t), decltype(n)::value, true>(q, row_map, q_rows, fired_now, y0, y1, f0, f1, k, coef,
                                                                       dts, n_rows, row_len, s);
    });
}

int tdeq_row_event_eval_mapped(void* out, const int32_t* dst_map, int64_t out_rows, const void* q, const int32_t* src_map,
                               int64_t q_rows, const void* x, int64_t n_idx, int64_t row_len, int dtype, void* stream) {
    if (!out || !q || !src_map || !x || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (n_idx < 0 || out_rows < 0 || q_rows < 0 || row_len < 1) return TDEQ_EINVAL;
    if (n_idx == 0) return 0;
    if (q_rows < 1 || out_rows < 1 || (!dst_map && out_rows < n_idx)) return TDEQ_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype(dtype, [&](auto t) {
        return row_event_eval_mapped_launch<decltype(t)>(out, dst_map, q, src_map, q_rows, x, n_idx, row_len, s);
    });
}

// ---- per-row dense output: tdeq_row_dense_slots / tdeq_row_dense_pack / tdeq_row_dense_search -------------------------
int tdeq_row_dense_slots(const tdeq_row_state* st, const int32_t* row_map, int64_t cap, int32_t* counter, int32_t* slot_row,
                         int32_t* slot_ord, double* slot_ta, double* slot_tb, int32_t* slot, int32_t* mask, void* stream) {
    if (!st || !counter || !slot_row || !slot_ord || !slot_ta || !slot_tb || !slot || !mask) return TDEQ_EINVAL;
    if (st->n_rows < 0 || !st->accepted || !st->tprev || !st->t0 || !st->n_acc) return TDEQ_EINVAL;
    // (a slot is an int32, and the counter may run n_rows past cap before the host looks at it)
    if (cap < 0 || st->n_rows > 0x7fffffffLL || cap > 0x7fffffffLL - st->n_rows) return TDEQ_EINVAL;
    if (st->n_rows == 0) return 0;
    RowDenseSlotsArgs a;
    a.accepted = st->accepted;
    a.tprev = st->tprev;
    a.t0 = st->t0;
    a.n_acc = st->n_acc;
    a.row_map = row_map;
    a.n_rows = st->n_rows;
    a.cap = (int32_t)cap;
    a.counter = counter;
    a.slot_row = slot_row;
    a.slot_ord = slot_ord;
    a.slot_ta = slot_ta;
    a.slot_tb = slot_tb;
    a.slot = slot;
    a.mask = mask;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((a.n_rows + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(row_dense_slots_kernel, grid, dim3(kBlock), 0, s, a);
    return check_launch();
}

int tdeq_row_dense_pack(void* dst, int64_t dst_rows, const void* src, int64_t src_rows, const int64_t* dest, int64_t n_used,
                        int64_t row_len, int dtype, void* stream) {
    if (!dst || !src || !dest || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (dst_rows < 0 || src_rows < 0 || n_used < 0 || row_len < 1 || n_used > src_rows) return TDEQ_EINVAL;
    if (n_used == 0) return 0;
    if (dst_rows < 1) return TDEQ_EINVAL;
    RowDensePackArgs a;
    a.dst = dst;
    a.src = src;
    a.dest = dest;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (16-byte elements: row_len is a whole number of them, so every row start and every plane is aligned as its base is)
    return row_elem(dtype, row_len, all_aligned(dst, src), [&](auto e, int64_t row_len_e) {
        a.row_len = row_len_e;
        a.ne = n_used * row_len_e;
        a.dst_plane = dst_rows * row_len_e;
        a.src_plane = src_rows * row_len_e;
        hipLaunchKernelGGL((row_dense_pack_kernel<decltype(e)>), dim3(stream_grid(a.ne, kBlock)), dim3(kBlock), 0, s, a);
        return check_launch();
    });
}

int tdeq_row_dense_search(const double* tq, int64_t n_q, const int64_t* offsets, const double* seg_ta, const double* seg_tb,
                          int64_t n_seg, const double* t0, const double* t1, int64_t n_rows, int32_t* seg, void* x,
                          int32_t* status, int dtype, void* stream) {
    if (!tq || !offsets || !seg_ta || !seg_tb || !t0 || !t1 || !seg || !x || !status || !real_dtype_ok(dtype))
        return TDEQ_EINVAL;
    if (n_q < 0 || n_rows < 0 || n_seg < 0) return TDEQ_EINVAL;
    if (n_q == 0 || n_rows == 0) return 0;
    // (a segment and a query index are int32 words; INT32_MAX itself is the status word's "none")
    if (n_seg < 1 || n_seg > 0x7fffffffLL || n_q > 0x7ffffffeLL / n_rows) return TDEQ_EINVAL;
    RowDenseSearchArgs a;
    a.tq = tq;
    a.offsets = offsets;
    a.seg_ta = seg_ta;
    a.seg_tb = seg_tb;
    a.t0 = t0;
    a.t1 = t1;
    a.n_rows = n_rows;
    a.n_seg = n_seg;
    a.n = n_q * n_rows;
    a.seg = seg;
    a.x = x;
    a.status = status;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((a.n + kBlock - 1) / kBlock));
    return real_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL((row_dense_search_kernel<decltype(t)>), grid, dim3(kBlock), 0, s, a);
        return check_launch();
    });
}

// ---- calculus on the record: tdeq_row_dense_prefix / tdeq_row_dense_calc ----------------------------------------------
namespace {

template <typename T>
int row_dense_prefix_launch(double* prefix, const void* coeffs, const int64_t* offsets, const double* seg_ta,
                            const double* seg_tb, int64_t n_seg, int64_t n_rows, int64_t row_len, hipStream_t s) {
    RowDensePrefixArgs<T> a;
    a.prefix = prefix;
    a.q = static_cast<const T*>(coeffs);
    a.offsets = offsets;
    a.seg_ta = seg_ta;
    a.seg_tb = seg_tb;
    a.n_seg = n_seg;
    a.q_plane = n_seg * row_len;
    return row_vec<T>(row_len, all_aligned(prefix, coeffs), a.row_len, [&](auto vec) {
        a.ne = n_rows * a.row_len;
        hipLaunchKernelGGL((row_dense_prefix_kernel<T, decltype(vec)::value>), dim3(stream_grid(a.ne, kBlock)), dim3(kBlock),
                           0, s, a);
        return check_launch();
    });
}

template <typename T>
int row_dense_calc_launch(void* out, int mode, const void* coeffs, int64_t n_seg, const double* seg_ta, const double* seg_tb,
                          const double* prefix, double time_sign, const int32_t* seg, const void* x, const double* tq,
                          const int32_t* seg2, const void* x2, const double* tq2, int64_t n_idx, int64_t row_len,
                          hipStream_t s) {
    RowDenseCalcArgs<T> a;
    a.out = static_cast<T*>(out);
    a.q = static_cast<const T*>(coeffs);
    a.seg_ta = seg_ta;
    a.seg_tb = seg_tb;
    a.prefix = prefix;
    a.sign = time_sign;
    a.seg = seg;
    a.x = static_cast<const T*>(x);
    a.tq = tq;
    a.seg2 = seg2;
    a.x2 = static_cast<const T*>(x2);
    a.tq2 = tq2;
    a.q_plane = n_seg * row_len;
    return row_vec<T>(row_len, all_aligned(out, coeffs, prefix), a.row_len, [&](auto vec) {
        constexpr bool VEC = decltype(vec)::value;
        a.ne = n_idx * a.row_len;
        const dim3 grid(stream_grid(a.ne, kBlock)), block(kBlock);
        if (mode == kDenseDerivative) hipLaunchKernelGGL((row_dense_calc_kernel<T, VEC, kDenseDerivative>), grid, block, 0, s, a);
        else if (mode == kDenseAntiderivative)
            hipLaunchKernelGGL((row_dense_calc_kernel<T, VEC, kDenseAntiderivative>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((row_dense_calc_kernel<T, VEC, kDenseIntegral>), grid, block, 0, s, a);
        return check_launch();
    });
}

}  // namespace

int tdeq_row_dense_prefix(double* prefix, const void* coeffs, const int64_t* offsets, const double* seg_ta,
                          const double* seg_tb, int64_t n_seg, int64_t n_rows, int64_t row_len, int dtype, void* stream) {
    if (!prefix || !coeffs || !offsets || !seg_ta || !seg_tb || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (n_seg < 0 || n_rows < 0 || row_len < 1) return TDEQ_EINVAL;
    if (n_rows == 0 || n_seg == 0) return 0;
    if (n_seg > 0x7fffffffLL) return TDEQ_EINVAL;      // (a segment index is an int32 word everywhere else)
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype(dtype, [&](auto t) {
        return row_dense_prefix_launch<decltype(t)>(prefix, coeffs, offsets, seg_ta, seg_tb, n_seg, n_rows, row_len, s);
    });
}

int tdeq_row_dense_calc(void* out, int mode, const void* coeffs, int64_t n_seg, const double* seg_ta, const double* seg_tb,
                        const double* prefix, double time_sign, const int32_t* seg, const void* x, const double* tq,
                        const int32_t* seg2, const void* x2, const double* tq2, int64_t n_idx, int64_t row_len, int dtype,
                        void* stream) {
    if (!out || !coeffs || !seg_ta || !seg_tb || !seg || !x || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (mode != TDEQ_DENSE_DERIVATIVE && mode != TDEQ_DENSE_ANTIDERIVATIVE && mode != TDEQ_DENSE_INTEGRAL) return TDEQ_EINVAL;
    if (mode != TDEQ_DENSE_DERIVATIVE && (!prefix || !tq)) return TDEQ_EINVAL;
    if (mode == TDEQ_DENSE_INTEGRAL && (!seg2 || !x2 || !tq2)) return TDEQ_EINVAL;
    if (!(time_sign == 1.0 || time_sign == -1.0)) return TDEQ_EINVAL;
    if (n_idx < 0 || n_seg < 0 || row_len < 1) return TDEQ_EINVAL;
    if (n_idx == 0) return 0;
    if (n_seg < 1 || n_seg > 0x7fffffffLL) return TDEQ_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype(dtype, [&](auto t) {
        return row_dense_calc_launch<decltype(t)>(out, mode, coeffs, n_seg, seg_ta, seg_tb, prefix, time_sign, seg, x, tq,
                                                  seg2, x2, tq2, n_idx, row_len, s);
    });
}

// ---- queries over a time window: tdeq_row_dense_extremum / _level / _level_times / _exposure ------------------------------
namespace {

// what the four entry points share, as it arrives (`level`, `n_rows`: the level family; NULL and 0 for the extrema)
struct RowDenseWindowIn {
    const void* level;
    int64_t n_rows;
    const void* coeffs;
    int64_t n_seg;
    const double* seg_ta;
    const double* seg_tb;
    double time_sign;
    const int32_t* seg;
    const void* x;
    const double* tq;
    const int32_t* seg2;
    const void* x2;
    const double* tq2;
    int64_t n_idx;
    int64_t row_len;
};

// The shared checks, after those of an entry point's own arguments (`outputs`: none of its outputs is NULL) ->
// TDEQ_EINVAL, 0 (nothing to do) or 1 (launch).
int row_dense_window_check(bool outputs, bool leveled, const RowDenseWindowIn& w, int dtype) {
    if (!outputs || (leveled && !w.level) || !w.coeffs || !w.seg_ta || !w.seg_tb || !w.seg || !w.x || !w.tq || !w.seg2 ||
        !w.x2 || !w.tq2 || !real_dtype_ok(dtype))
        return TDEQ_EINVAL;
    if (!(w.time_sign == 1.0 || w.time_sign == -1.0)) return TDEQ_EINVAL;
    if (w.n_idx < 0 || w.n_seg < 0 || w.row_len < 0 || w.n_rows < 0) return TDEQ_EINVAL;
    if (leveled && w.n_idx > 0 && (w.n_rows == 0 || w.n_idx % w.n_rows != 0)) return TDEQ_EINVAL;
    if (w.n_idx == 0 || w.row_len == 0) return 0;
    if (w.n_seg < 1 || w.n_seg > 0x7fffffffLL) return TDEQ_EINVAL;
    return 1;
}

// (row_len and ne follow the 16-byte decision of the launch)
template <typename T>
void row_dense_window_fill(RowDenseWindowArgs<T>& a, const RowDenseWindowIn& w) {
    a.q = static_cast<const T*>(w.coeffs);
    a.seg_ta = w.seg_ta;
    a.seg_tb = w.seg_tb;
    a.sign = w.time_sign;
    a.seg = w.seg;
    a.x = static_cast<const T*>(w.x);
    a.tq = w.tq;
    a.seg2 = w.seg2;
    a.x2 = static_cast<const T*>(w.x2);
    a.tq2 = w.tq2;
    a.n_rows = w.n_rows;
    a.n_seg = w.n_seg;
    a.q_plane = w.n_seg * w.row_len;
}

// int32 outputs are stored as one word of 16 / sizeof(T) int32: 16 bytes for float, 8 for double
template <typename T>
bool int_word_aligned(const int32_t* p) {
    return reinterpret_cast<uintptr_t>(p) % (sizeof(int32_t) * (16 / sizeof(T))) == 0;
}

template <typename T>
int row_dense_extremum_launch(void* values, double* times, int which, const RowDenseWindowIn& w, hipStream_t s) {
    RowDenseExtremumArgs<T> a;
    row_dense_window_fill<T>(a, w);
    a.values = static_cast<T*>(values);
    a.times = times;
    return row_vec<T>(w.row_len, all_aligned(values, times, w.coeffs), a.row_len, [&](auto vec) {
        constexpr bool VEC = decltype(vec)::value;
        a.ne = w.n_idx * a.row_len;
        const dim3 grid(stream_grid(a.ne, kBlock)), block(kBlock);
        if (which == kDenseMaximum) hipLaunchKernelGGL((row_dense_extremum_kernel<T, VEC, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((row_dense_extremum_kernel<T, VEC, false>), grid, block, 0, s, a);
        return check_launch();
    });
}

template <typename T>
int row_dense_level_launch(int32_t* count, double* first, double* last, double* time_above, const RowDenseWindowIn& w,
                           hipStream_t s) {
    RowDenseLevelArgs<T> a;
    row_dense_window_fill<T>(a, w);
    a.count = count;
    a.first = first;
    a.last = last;
    a.total = time_above;
    a.level = static_cast<const T*>(w.level);
    const bool aligned = int_word_aligned<T>(count) && all_aligned(first, last, time_above, w.level, w.coeffs);
    return row_vec<T>(w.row_len, aligned, a.row_len, [&](auto vec) {
        constexpr bool VEC = decltype(vec)::value;
        a.ne = w.n_idx * a.row_len;
        hipLaunchKernelGGL((row_dense_level_kernel<T, VEC>), dim3(stream_grid(a.ne, kBlock)), dim3(kBlock), 0, s, a);
        return check_launch();
    });
}

template <typename T>
int row_dense_level_times_launch(int32_t* n_rising, int32_t* n_falling, double* rising, double* falling, int64_t max_count,
                                 const RowDenseWindowIn& w, hipStream_t s) {
    RowDenseLevelTimesArgs<T> a;
    row_dense_window_fill<T>(a, w);
    // rising is meant in true time: rising = (the state becomes above) == (time_sign > 0)
    const bool up_rises = w.time_sign > 0.0;
    a.n_up = up_rises ? n_rising : n_falling;
    a.n_dn = up_rises ? n_falling : n_rising;
    a.ups = up_rises ? rising : falling;
    a.dns = up_rises ? falling : rising;
    a.k = static_cast<int32_t>(max_count);
    a.level = static_cast<const T*>(w.level);
    a.t_plane = w.n_idx * w.row_len;
    // (the lists take 8-byte stores in either form)
    const bool aligned = int_word_aligned<T>(n_rising) && int_word_aligned<T>(n_falling) && all_aligned(w.level, w.coeffs);
    return row_vec<T>(w.row_len, aligned, a.row_len, [&](auto vec) {
        constexpr bool VEC = decltype(vec)::value;
        a.ne = w.n_idx * a.row_len;
        hipLaunchKernelGGL((row_dense_level_times_kernel<T, VEC>), dim3(stream_grid(a.ne, kBlock)), dim3(kBlock), 0, s, a);
        return check_launch();
    });
}

template <typename T>
int row_dense_exposure_launch(void* area_above, void* area_below, double* time_above, const RowDenseWindowIn& w,
                              hipStream_t s) {
    RowDenseExposureArgs<T> a;
    row_dense_window_fill<T>(a, w);
    a.area_above = static_cast<T*>(area_above);
    a.area_below = static_cast<T*>(area_below);
    a.total = time_above;
    a.level = static_cast<const T*>(w.level);
    const bool aligned = all_aligned(area_above, area_below, time_above, w.level, w.coeffs);
    return row_vec<T>(w.row_len, aligned, a.row_len, [&](auto vec) {
        constexpr bool VEC = decltype(vec)::value;
        a.ne = w.n_idx * a.row_len;
        hipLaunchKernelGGL((row_dense_exposure_kernel<T, VEC>), dim3(stream_grid(a.ne, kBlock)), dim3(kBlock), 0, s, a);
        return check_launch();
    });
}

}  // namespace

int tdeq_row_dense_extremum(void* values, double* times, int which, const void* coeffs, int64_t n_seg, const double* seg_ta,
                            const double* seg_tb, double time_sign, const int32_t* seg, const void* x, const double* tq,
                            const int32_t* seg2, const void* x2, const double* tq2, int64_t n_idx, int64_t row_len, int dtype,
                            void* stream) {
    const RowDenseWindowIn w{nullptr, 0, coeffs, n_seg, seg_ta, seg_tb, time_sign, seg, x, tq, seg2, x2, tq2, n_idx, row_len};
    if (which != TDEQ_DENSE_MAXIMUM && which != TDEQ_DENSE_MINIMUM) return TDEQ_EINVAL;
    const int go = row_dense_window_check(values && times, false, w, dtype);
    if (go != 1) return go;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype(dtype, [&](auto t) { return row_dense_extremum_launch<decltype(t)>(values, times, which, w, s); });
}

int tdeq_row_dense_level(int32_t* count, double* first, double* last, double* time_above, const void* level, int64_t n_rows,
                         const void* coeffs, int64_t n_seg, const double* seg_ta, const double* seg_tb, double time_sign,
                         const int32_t* seg, const void* x, const double* tq, const int32_t* seg2, const void* x2,
                         const double* tq2, int64_t n_idx, int64_t row_len, int dtype, void* stream) {
    const RowDenseWindowIn w{level, n_rows, coeffs, n_seg, seg_ta, seg_tb, time_sign, seg, x, tq, seg2, x2, tq2, n_idx, row_len};
    const int go = row_dense_window_check(count && first && last && time_above, true, w, dtype);
    if (go != 1) return go;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype(dtype, [&](auto t) {
        return row_dense_level_launch<decltype(t)>(count, first, last, time_above, w, s);
    });
}

int tdeq_row_dense_level_times(int32_t* n_rising, int32_t* n_falling, double* rising, double* falling, int64_t max_count,
                               const void* level, int64_t n_rows, const void* coeffs, int64_t n_seg, const double* seg_ta,
                               const double* seg_tb, double time_sign, const int32_t* seg, const void* x, const double* tq,
                               const int32_t* seg2, const void* x2, const double* tq2, int64_t n_idx, int64_t row_len,
                               int dtype, void* stream) {
    const RowDenseWindowIn w{level, n_rows, coeffs, n_seg, seg_ta, seg_tb, time_sign, seg, x, tq, seg2, x2, tq2, n_idx, row_len};
    if (max_count < 1 || max_count > 65535) return TDEQ_EINVAL;
    const int go = row_dense_window_check(n_rising && n_falling && rising && falling, true, w, dtype);
    if (go != 1) return go;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype(dtype, [&](auto t) {
        return row_dense_level_times_launch<decltype(t)>(n_rising, n_falling, rising, falling, max_count, w, s);
    });
}

// (the areas and the time above are durations: `time_sign` is checked and not used)
int tdeq_row_dense_exposure(void* area_above, void* area_below, double* time_above, const void* level, int64_t n_rows,
                            const void* coeffs, int64_t n_seg, const double* seg_ta, const double* seg_tb, double time_sign,
                            const int32_t* seg, const void* x, const double* tq, const int32_t* seg2, const void* x2,
                            const double* tq2, int64_t n_idx, int64_t row_len, int dtype, void* stream) {
    const RowDenseWindowIn w{level, n_rows, coeffs, n_seg, seg_ta, seg_tb, time_sign, seg, x, tq, seg2, x2, tq2, n_idx, row_len};
    const int go = row_dense_window_check(area_above && area_below && time_above, true, w, dtype);
    if (go != 1) return go;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype(dtype, [&](auto t) {
        return row_dense_exposure_launch<decltype(t)>(area_above, area_below, time_above, w, s);
    });
}
