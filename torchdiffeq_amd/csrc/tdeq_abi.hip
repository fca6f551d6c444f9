// tdeq_abi.hip — extern "C" entry points of libtdeq_hip.so (declared in include/tdeq_hip.h).
// Host-side validation + template dispatch + launch; no allocation, no synchronisation, no globals.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdlib>
#include <type_traits>

#include "tdeq_kernels.hpp"
#include "tdeq_kernels_complex.hpp"
#include "tdeq_kernels_lp.hpp"

namespace {
using namespace tdeq;

// Launch geometry for the streaming (elementwise) kernels: one 16-byte element per lane, i.e. enough
// workgroups to cover the tensor exactly once (tools/sweep_combine.hip on the MI355X: 8192 workgroups
// of one float4 per lane beat a 2048-workgroup grid-stride loop by 6-8 %, cold and warm); only beyond
// kMaxGrid workgroups does the kernel grid-stride.
constexpr int64_t kMaxGrid = 1 << 16;

inline unsigned stream_grid(int64_t n_items, int items_per_block) {
    int64_t g = (n_items + items_per_block - 1) / items_per_block;
    const int64_t cap = kMaxGrid;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int check_launch() {
    const hipError_t e = hipGetLastError();
    return (int)e;
}

// ---- the run-time choices of a launch, each written once: every helper calls f with a tag and returns its status -----
// (shared by the three host files: this one, tdeq_abi_lp.hpp, tdeq_abi_rowwise.hpp)
inline bool real_dtype_ok(int dtype) { return dtype == TDEQ_F32 || dtype == TDEQ_F64; }
// bfloat16 / float16 states: the entry points of the host-driven step (tdeq_kernels_lp.hpp; include/tdeq_hip.h lists them)
inline bool lp_dtype(int dtype) { return dtype == TDEQ_BF16 || dtype == TDEQ_F16; }
inline bool state_dtype_ok(int dtype) { return real_dtype_ok(dtype) || lp_dtype(dtype); }
// the norm entry points also take interleaved complex states (TDEQ_C64 / TDEQ_C128: tdeq_kernels_complex.hpp)
inline bool cplx_dtype(int dtype) { return dtype == TDEQ_C64 || dtype == TDEQ_C128; }

template <typename T>
constexpr bool is_lp = std::is_same_v<T, lp::BF16> || std::is_same_v<T, lp::F16>;

// f(T{}), T = float or double
template <typename F>
int real_dtype(int dtype, F f) {
    return dtype == TDEQ_F32 ? f(float{}) : f(double{});
}

// f(T{}) or, for a 16-bit state, f(S{}) with S = lp::BF16 or lp::F16 (is_lp<S>)
template <typename F>
int state_dtype(int dtype, F f) {
    if (dtype == TDEQ_BF16) return f(lp::BF16{});
    if (dtype == TDEQ_F16) return f(lp::F16{});
    return real_dtype(dtype, f);
}

// the norm entry points: f(tag, std::bool_constant<CPLX>{}) — a complex state comes as its real type with CPLX set
template <typename F>
int norm_dtype(int dtype, F f) {
    if (dtype == TDEQ_C64) return f(float{}, std::true_type{});
    if (dtype == TDEQ_C128) return f(double{}, std::true_type{});
    return state_dtype(dtype, [&](auto t) { return f(t, std::false_type{}); });
}

// f(std::true_type{}) or f(std::false_type{}): one bool template argument of a kernel; flags: two of them
template <typename F>
int flag(bool b, F f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

template <typename F>
int flags(bool b0, bool b1, F f) {
    return flag(b0, [&](auto t0) { return flag(b1, [&](auto t1) { return f(t0, t1); }); });
}

// f(std::integral_constant<int, N>{}) for LO <= N = nt <= HI: the only switch over a term (or stage) count
template <int LO, int HI = TDEQ_MAX_TERMS, typename F>
int terms(int nt, F f) {
    static_assert(LO >= 0 && HI <= TDEQ_MAX_TERMS);
    switch (nt) {
#define TDEQ_CASE(N) case N: if constexpr (N >= LO && N <= HI) return f(std::integral_constant<int, N>{}); break;
        TDEQ_CASE(0) TDEQ_CASE(1) TDEQ_CASE(2) TDEQ_CASE(3) TDEQ_CASE(4) TDEQ_CASE(5) TDEQ_CASE(6) TDEQ_CASE(7)
        TDEQ_CASE(8) TDEQ_CASE(9) TDEQ_CASE(10) TDEQ_CASE(11) TDEQ_CASE(12) TDEQ_CASE(13) TDEQ_CASE(14)
#undef TDEQ_CASE
    }
    return TDEQ_EINVAL;
}

// f(T{}, std::integral_constant<int, N>{}): what a term-templated entry point launches through
template <int LO, int HI = TDEQ_MAX_TERMS, typename F>
int real_dtype_terms(int dtype, int nt, F f) {
    return real_dtype(dtype, [&](auto t) { return terms<LO, HI>(nt, [&](auto n) { return f(t, n); }); });
}

template <int LO, int HI = TDEQ_MAX_TERMS, typename F>
int state_dtype_terms(int dtype, int nt, F f) {
    return state_dtype(dtype, [&](auto t) { return terms<LO, HI>(nt, [&](auto n) { return f(t, n); }); });
}

struct Ptrs {                         // an array of n pointers: k[], outs[], x[]
    const void* const* p;
    int n;
};

inline bool aligned16(Ptrs a) {
    for (int j = 0; j < a.n; ++j) if (!aligned16(a.p[j])) return false;
    return true;
}

// are all of these pointers (and every pointer of these arrays) 16-byte aligned; so is a null pointer: an absent input
template <typename... P>
bool all_aligned(P... p) {
    return (aligned16(p) && ...);
}

// A streaming launch over n elements of T: 16-byte elements when `vec`; f(std::bool_constant<VEC>{}, grid) launches.
template <typename T, typename F>
int stream_launch(bool vec, int64_t n, F f) {
    const dim3 g(stream_grid(vec ? n / VecOf<T>::L : n, kBlock));
    return flag(vec, [&](auto v) {
        f(v, g);
        return check_launch();
    });
}

// The terms of a launch: a.k[j] and the coefficients as the reference rounds them, c_j = fl_T(fl_T(coef_j) * fl_T(dt)) —
// rk_common.py:79,201-205 (a stage row), :89 (dt * c_error, the second row `e` of the fused error), :365-366 (dt * c_mid).
// With dt in device memory (`dev_dt`: captured steps) c_j = fl_T(coef_j) and the kernel multiplies.  The zero-term forms
// keep one unused slot.  Returns whether every k[j] is 16-byte aligned.
template <typename T, int NT, int M>
bool fill_terms(const T* (&ak)[M], T (&ac)[M], const void* const* k, const double* coef, double dt, bool dev_dt,
                T (*ae)[M] = nullptr, const double* err_coef = nullptr) {
    static_assert(NT <= M);
    const T dtT = (T)dt;
    if (NT == 0) {
        ak[0] = nullptr;
        ac[0] = (T)0;
    }
    for (int j = 0; j < NT; ++j) {
        ak[j] = static_cast<const T*>(k[j]);
        ac[j] = dev_dt ? (T)coef[j] : (T)coef[j] * dtT;
        if (ae) (*ae)[j] = dev_dt ? (T)err_coef[j] : (T)err_coef[j] * dtT;
    }
    return all_aligned(Ptrs{k, NT});
}

// out = y0 + sum_j c_j k_j: the argument block of every stage combine; returns the 16-byte decision of its pointers
template <typename T, int NT>
bool fill_combine(CombineArgs<T, NT>& a, void* out, const void* y0, const void* const* k, const double* coef, double dt,
                  int64_t n, bool dev_dt = false, T (*e)[NT] = nullptr, const double* err_coef = nullptr) {
    a.out = static_cast<T*>(out);
    a.y0 = static_cast<const T*>(y0);
    a.n = n;
    const bool k_aligned = fill_terms<T, NT>(a.k, a.c, k, coef, dt, dev_dt, e, err_coef);
    return all_aligned(out, y0) && k_aligned;
}

// Cache policy of a streaming launch (bit 0: non-temporal loads, bit 1: non-temporal stores), chosen from the bytes
// its streams touch.  Measured on the MI355X (tools/stream_count.hip, profiles/r05_stream_count.json): with every byte
// coming from DRAM, 5 read + 2 write streams run at 5.4 TB/s with the default policy and at 6.0 TB/s with both hints
// (10 R + 4 W fp64: 5.6 -> 5.9-6.3) — the hints keep single-use lines from churning through L2 / the Infinity Cache.
// A launch whose streams fit the 256 MiB Infinity Cache is better off WITHOUT them (its inputs were just written by
// func and are still resident; its outputs are read by func next).  TDEQ_COMBINE_POLICY = 0..3 forces one policy for
// every launch (tuning runs); TDEQ_NT_THRESHOLD_MB moves the switch point.
constexpr int64_t kNtDefaultThreshold = (int64_t)TDEQ_NT_THRESHOLD_DEFAULT_MB << 20;
constexpr int kNtPolicy = 3;

inline int stream_policy(int64_t stream_bytes) {
    static const int forced = [] {
        const char* e = getenv("TDEQ_COMBINE_POLICY");
        if (!e || !*e || *e == 'a') return -1;      // unset / "auto"
        const int v = atoi(e);
        return (v >= 0 && v <= 3) ? v : -1;
    }();
    if (forced >= 0) return forced;
    static const int64_t threshold = [] {
        const char* e = getenv("TDEQ_NT_THRESHOLD_MB");
        return (e && *e) ? ((int64_t)atoll(e) << 20) : kNtDefaultThreshold;
    }();
    return stream_bytes > threshold ? kNtPolicy : 0;
}

// f(std::integral_constant<int, POLICY>{}) with the policy of a launch that touches stream_bytes
template <typename F>
int with_policy(int64_t stream_bytes, F f) {
    switch (stream_policy(stream_bytes)) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
    }
    return f(std::integral_constant<int, 0>{});
}

// ---- stage_combine --------------------------------------------------------------------------------
template <typename T, int NT>
int launch_combine(void* out, const void* y0, const void* const* k, const double* coef, double dt,
                   int64_t n, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr) {
    CombineArgs<T, NT> a;
    const bool vec = fill_combine(a, out, y0, k, coef, dt, n);
    constexpr int L = VecOf<T>::L;
    constexpr int U = 1;
    const dim3 b(kBlock);
    if (!vec) {
        hipLaunchKernelGGL((stage_combine_kernel<T, NT, U, false>), dim3(stream_grid(n, kBlock * U)), b, 0, s, a);
        return check_launch();
    }
    const dim3 g(stream_grid(n / L, kBlock * U));
    if (ev_start && ev_stop) {
        // measurement hook (tdeq_stage_combine_timed): the events carry the dispatch's own begin / end timestamps
        hipExtLaunchKernelGGL((stage_combine_kernel<T, NT, U, true, 0>), g, b, 0, s, ev_start, ev_stop, 0, a);
        return check_launch();
    }
    return with_policy((int64_t)(NT + 2) * n * (int64_t)sizeof(T), [&](auto p) {      // see stream_policy()
        constexpr int P = decltype(p)::value;
        if (P == 0 && (int64_t)g.x * kBlock * U >= n / L)      // the default policy in one pass
            hipLaunchKernelGGL((stage_combine_kernel<T, NT, U, true, 0, true>), g, b, 0, s, a);
        else hipLaunchKernelGGL((stage_combine_kernel<T, NT, U, true, P>), g, b, 0, s, a);
        return check_launch();
    });
}

template <typename T, int NT>
int launch_combine_fill(void* out, const void* y0, const void* const* k, const double* coef, double dt, int64_t n,
                        void* fill_dst, const double* fill_vals, int n_fill, hipStream_t s) {
    CombineArgs<T, NT> a;
    const bool vec = fill_combine(a, out, y0, k, coef, dt, n);
    SideFill<T> f;
    f.dst = static_cast<T*>(fill_dst);
    for (int i = 0; i < 16; ++i) f.v[i] = i < n_fill ? (T)fill_vals[i] : (T)0;
    f.n = n_fill;
    return stream_launch<T>(vec, n, [&](auto v, dim3 g) {
        hipLaunchKernelGGL((stage_combine_fill_kernel<T, NT, decltype(v)::value>), g, dim3(kBlock), 0, s, a, f);
    });
}

template <typename T, int NT>
int launch_combine_err(void* out, void* err_out, const void* y0, const void* const* k, const double* coef,
                       const double* err_coef, double dt, int64_t n, hipStream_t s) {
    CombineErrArgs<T, NT> a;
    a.err_out = static_cast<T*>(err_out);
    const bool vec = fill_combine(a.c, out, y0, k, coef, dt, n, false, &a.e, err_coef) && aligned16(err_out);
    constexpr int L = VecOf<T>::L;
    const dim3 b(kBlock);
    if (!vec) {
        hipLaunchKernelGGL((stage_combine_err_kernel<T, NT, false>), dim3(stream_grid(n, kBlock)), b, 0, s, a);
        return check_launch();
    }
    const dim3 g(stream_grid(n / L, kBlock));
    // (r05, tried: non-temporal loads for the k streams of THIS launch only — their last use in a dopri5 step — with the
    //  default policy elsewhere: 0.3357 vs 0.3336 ms per cfg2 step, loads + stores 0.3323: noise; not kept)
    return with_policy((int64_t)(NT + 3) * n * (int64_t)sizeof(T), [&](auto p) {
        constexpr int P = decltype(p)::value;
        if (P == 0 && (int64_t)g.x * kBlock >= n / L)
            hipLaunchKernelGGL((stage_combine_err_kernel<T, NT, true, 0, true>), g, b, 0, s, a);
        else hipLaunchKernelGGL((stage_combine_err_kernel<T, NT, true, P>), g, b, 0, s, a);
        return check_launch();
    });
}

// ---- stage_combine_multi (carried partial sums) ---------------------------------------------------------
template <typename T, int NT>
int launch_combine_multi(const tdeq_multi_out* outs, int n_out, const void* y0, const void* acc_in,
                         const void* const* k, double dt, int64_t n, hipStream_t s, hipEvent_t ev_start = nullptr,
                         hipEvent_t ev_stop = nullptr, const double* dt_dev = nullptr) {
    MultiArgs<T, NT> a;
    a.dt_dev = dt_dev;
    a.y0 = static_cast<const T*>(y0);
    a.acc_in = static_cast<const T*>(acc_in);
    for (int j = 0; j < NT; ++j) a.k[j] = static_cast<const T*>(k[j]);
    bool vec = all_aligned(y0, acc_in, Ptrs{k, NT});
    const T dtT = (T)dt;
    a.add_y0 = 0;
    for (int o = 0; o < kMaxMultiOut; ++o) {
        const bool live = o < n_out;
        a.out[o] = live ? static_cast<T*>(outs[o].out) : nullptr;
        a.mask[o] = live ? outs[o].mask : 0u;
        if (live && outs[o].add_y0) a.add_y0 |= 1u << o;
        for (int j = 0; j < NT; ++j)      // the rounding of fill_terms, one row per output; a dead output's row is zero
            a.c[o][j] = !live ? (T)0 : (dt_dev ? (T)outs[o].coef[j] : (T)outs[o].coef[j] * dtT);
        if (live) vec = vec && aligned16(outs[o].out);
    }
    a.n_out = n_out;
    a.n = n;
    constexpr int L = VecOf<T>::L;
    const dim3 b(kBlock);
    if (!vec) {
        hipLaunchKernelGGL((stage_combine_multi_kernel<T, NT, false>), dim3(stream_grid(n, kBlock)), b, 0, s, a);
        return check_launch();
    }
    const dim3 g(stream_grid(n / L, kBlock));
    const bool timed = ev_start && ev_stop;      // measurement hook (tdeq_stage_combine_multi_timed)
    auto launch = [&](void (*kernel)(const MultiArgs<T, NT>)) {
        if (timed) hipExtLaunchKernelGGL(kernel, g, b, 0, s, ev_start, ev_stop, 0, a);
        else hipLaunchKernelGGL(kernel, g, b, 0, s, a);
        return check_launch();
    };
    const bool one_pass = (int64_t)g.x * kBlock >= n / L;      // exact cover (always, up to 2^24 16-byte elements)
    const int64_t streams = NT + 1 + (acc_in ? 1 : 0) + n_out;
    return with_policy(streams * n * (int64_t)sizeof(T), [&](auto p) {
        constexpr int P = decltype(p)::value;
        if (P != 0 || n_out > 2) return launch(stage_combine_multi_kernel<T, NT, true, P>);
        // the in-cache regime (every dopri5 launch at cfg2): output count and prefix continuation as compile-time
        // constants for the one- and two-output launches (tdeq_kernels.hpp multi_elem), then dt from device memory —
        // captured steps — and one pass
        return flags(n_out == 2, acc_in != nullptr, [&](auto two, auto acc) {
            constexpr int NO = decltype(two)::value ? 2 : 1, AC = decltype(acc)::value ? 1 : 0;
            if (!one_pass) return launch(stage_combine_multi_kernel<T, NT, true, 0, NO, AC>);
            if (dt_dev) return launch(stage_combine_multi_kernel<T, NT, true, 0, NO, AC, true, true>);
            return launch(stage_combine_multi_kernel<T, NT, true, 0, NO, AC, false, true>);
        });
    });
}

// ---- segment table / workspace ---------------------------------------------------------------------
int fill_segtable(SegTable& st, const tdeq_segment* segs, const void* segs_dev, int n_seg,
                  int64_t chunk, int64_t n_chunks) {
    if (!segs || n_seg < 1 || n_seg > TDEQ_MAX_SEGMENTS) return TDEQ_EINVAL;
    if (chunk < TDEQ_CHUNK_QUANTUM || chunk % TDEQ_CHUNK_QUANTUM != 0 || n_chunks < 1) return TDEQ_EINVAL;
    if (n_chunks > 0x7fffffffLL) return TDEQ_EINVAL;
    if (n_seg > TDEQ_INLINE_SEGMENTS && !segs_dev) return TDEQ_EINVAL;
    for (int q = 0; q < TDEQ_INLINE_SEGMENTS; ++q) {
        if (q < n_seg && n_seg <= TDEQ_INLINE_SEGMENTS) st.inl[q] = segs[q];
        else st.inl[q] = tdeq_segment{0, 0, 0.0, 0.0};
    }
    if (n_seg > TDEQ_INLINE_SEGMENTS) st.inl[0] = segs[0];
    st.dev = static_cast<const tdeq_segment*>(segs_dev);
    st.n_seg = n_seg;
    st.chunk = chunk;
    st.n_chunks = n_chunks;
    return 0;
}

// What a norm launch works on: the segment table, the partial-sum workspace [3][n_chunks] and the stream.
struct NormSetup {
    SegTable st;
    double* ws;
    hipStream_t s;
};

// The prologue of the norm entry points: the segment table first, then the size of the workspace.
int norm_setup(NormSetup& ns, const tdeq_segment* segs, const void* segs_dev, int n_seg, int64_t chunk, int64_t n_chunks,
               void* workspace, size_t workspace_bytes, void* stream) {
    const int e = fill_segtable(ns.st, segs, segs_dev, n_seg, chunk, n_chunks);
    if (e) return e;
    if (workspace_bytes < tdeq_workspace_bytes(n_chunks)) return TDEQ_EWORKSPACE;
    ns.ws = static_cast<double*>(workspace);
    ns.s = static_cast<hipStream_t>(stream);
    return 0;
}

int launch_finalize(const SegTable& st, double* ws, int n_sum, double* out_sumsq, double* out_bad,
                    hipStream_t s) {
    FinalizeArgs f;
    for (int q = 0; q < 3; ++q) f.part[q] = ws + (int64_t)q * st.n_chunks;
    // the non-finite counters always live in the third array; remap so part[n_sum] is that array
    f.part[n_sum] = ws + 2 * st.n_chunks;
    f.st = st;
    f.n_sum = n_sum;
    f.out_sumsq = out_sumsq;
    f.out_bad = out_bad;
    hipLaunchKernelGGL(norm_finalize_kernel, dim3(st.n_seg, n_sum + 1), dim3(kBlock), 0, s, f);
    return check_launch();
}

// Optional controller bundle of the *_ctrl entry points (null => plain finalize).
struct CtrlBundle {
    const tdeq_step_ctrl* ctrl;
    double* out_ctrl;
    double* ctrl_dev;
    void* next_times;
    int state_in_dev;     // hipGraph mode: (t0, dt) of the trial step and the kernels' dt live in ctrl_dev
};

// The prologue of the *_ctrl entry points: every pointer of the bundle, then the counts of the controller's constants.
int make_ctrl(CtrlBundle& cb, const tdeq_step_ctrl* ctrl, double* out_ctrl, double* ctrl_dev, void* next_times,
              int state_in_dev, int n_seg) {
    if (!ctrl || !out_ctrl || !ctrl_dev || !next_times) return TDEQ_EINVAL;
    if (ctrl->n_times < 1 || ctrl->n_times > TDEQ_MAX_STAGE_TIMES || ctrl->n_norm_seg < 0 || ctrl->n_norm_seg > n_seg)
        return TDEQ_EINVAL;
    cb = CtrlBundle{ctrl, out_ctrl, ctrl_dev, next_times, state_in_dev ? 1 : 0};
    return 0;
}

// the state's real type as the controller kernel names it: 0 fp64, 1 fp32, 2 bfloat16, 3 float16
template <typename T>
constexpr int kTkind = std::is_same_v<T, lp::BF16> ? 2 : std::is_same_v<T, lp::F16> ? 3 : sizeof(T) == 4 ? 1 : 0;

int launch_finalize_ctrl(const SegTable& st, double* ws, double* out_sumsq, double* out_bad, const CtrlBundle& cb,
                         int tkind, hipStream_t s, int ratio_kind) {
    CtrlArgs a;
    a.part_sumsq = ws;
    a.part_bad = ws + 2 * st.n_chunks;
    a.st = st;
    a.c = *cb.ctrl;
    a.is_f32 = tkind;
    a.ratio_kind = ratio_kind < 0 ? tkind : ratio_kind;
    a.out_sumsq = out_sumsq;
    a.out_bad = out_bad;
    a.out_ctrl = cb.out_ctrl;
    a.ctrl_dev = cb.ctrl_dev;
    a.next_times = cb.next_times;
    a.state_in_dev = cb.state_in_dev;
    a.presummed = 0;
    a.in_sumsq = nullptr;
    a.in_bad = nullptr;
    if (st.n_seg > kCtrlInlineSegments) {
        // more segments than the one-workgroup form handles well: the per-segment sums by the parallel finalize (one
        // workgroup per segment; segment table inline, or from device memory beyond TDEQ_INLINE_SEGMENTS), then the
        // one-workgroup controller on those sums
        const int e = launch_finalize(st, ws, 1, out_sumsq, out_bad, s);
        if (e) return e;
        a.presummed = 1;
    }
    // one instantiation per segment-count bucket (the per-lane accumulators are a static array of 2·NS doubles)
    if (a.presummed || st.n_seg == 1) hipLaunchKernelGGL(norm_finalize_ctrl_kernel<1>, dim3(1), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL(norm_finalize_ctrl_kernel<kCtrlInlineSegments>, dim3(1), dim3(kBlock), 0, s, a);
    return check_launch();
}

// The tail of every norm launch: the status of the launch just made, then the per-segment sums — with a controller
// bundle the step controller too (ratio_kind -1: the ratio in the state's type; 0: in fp64, the promoted type).
int finish_norm(const NormSetup& ns, int n_sum, double* out_sumsq, double* out_bad, const CtrlBundle* cb = nullptr,
                int tkind = 0, int ratio_kind = -1) {
    const int e = check_launch();
    if (e) return e;
    if (cb) return launch_finalize_ctrl(ns.st, ns.ws, out_sumsq, out_bad, *cb, tkind, ns.s, ratio_kind);
    return launch_finalize(ns.st, ns.ws, n_sum, out_sumsq, out_bad, ns.s);
}

// ---- error_norm ------------------------------------------------------------------------------------
template <typename T, int NT>
int launch_error(void* scaled, const void* y0, const void* y1, const void* const* k, const double* coef,
                 double dt, const NormSetup& ns, double* out_sumsq, double* out_bad) {
    ErrArgs<T, NT> a;
    a.scaled = static_cast<T*>(scaled);
    a.y0 = static_cast<const T*>(y0);
    a.y1 = static_cast<const T*>(y1);
    const bool vec = fill_terms<T, NT>(a.k, a.c, k, coef, dt, false) && all_aligned(y0, y1, scaled);
    a.st = ns.st;
    a.part_sumsq = ns.ws;
    a.part_bad = ns.ws + 2 * ns.st.n_chunks;
    const dim3 g((unsigned)ns.st.n_chunks), b(kBlock);
    flags(vec, scaled != nullptr, [&](auto v, auto sc) {
        hipLaunchKernelGGL((error_norm_kernel<T, NT, decltype(v)::value, decltype(sc)::value>), g, b, 0, ns.s, a);
        return 0;
    });
    return finish_norm(ns, 1, out_sumsq, out_bad);
}

template <typename T, int NT>
int launch_error_vec(const void* partial, const void* y0, const void* y1, const void* const* k, const double* coef, double dt,
                     const double* rtol_v, double rtol_s, const double* atol_v, double atol_s, const NormSetup& ns,
                     double* out_sumsq, double* out_bad, const CtrlBundle* cb = nullptr) {
    if (NT == 0 && !partial) return TDEQ_EINVAL;
    ErrVecArgs<T, NT> a;
    a.y0 = static_cast<const T*>(y0);
    a.y1 = static_cast<const T*>(y1);
    a.partial = static_cast<const T*>(partial);
    const bool dev_dt = cb && cb->state_in_dev;      // hipGraph mode: dt = ctrl_dev[1] on the device
    fill_terms<T, NT>(a.k, a.c, k, coef, dt, dev_dt);
    a.dt_dev = dev_dt ? cb->ctrl_dev + 1 : nullptr;
    a.rtol_v = rtol_v;
    a.atol_v = atol_v;
    a.rtol_s = rtol_s;
    a.atol_s = atol_s;
    a.st = ns.st;
    a.part_sumsq = ns.ws;
    a.part_bad = ns.ws + 2 * ns.st.n_chunks;
    const dim3 g((unsigned)ns.st.n_chunks), b(kBlock);
    flags(partial != nullptr, dev_dt, [&](auto pt, auto dd) {
        constexpr bool PARTIAL = decltype(pt)::value, DEVDT = decltype(dd)::value;
        if constexpr (PARTIAL || NT > 0) {
            if constexpr (DEVDT) hipLaunchKernelGGL((error_norm_vec_kernel<T, NT, PARTIAL, true>), g, b, 0, ns.s, a);
            else hipLaunchKernelGGL((error_norm_vec_kernel<T, NT, PARTIAL>), g, b, 0, ns.s, a);
        }
        return 0;
    });
    // with a controller bundle: the ratio in fp64 (the promoted type), the step size and the stage times in T
    return finish_norm(ns, 1, out_sumsq, out_bad, cb, kTkind<T>, 0);
}

template <typename T, int NT>
int launch_error_partial(const void* partial, const void* y0, const void* y1, const void* const* k,
                         const double* coef, double dt, const NormSetup& ns, double* out_sumsq, double* out_bad,
                         const CtrlBundle* cb, void* copy_last = nullptr) {
    ErrPartialArgs<T, NT> a;
    a.copy_out = static_cast<T*>(copy_last);
    if (copy_last && NT == 0) return TDEQ_EINVAL;        // nothing to copy: the error row ended with the last combine
    a.partial = static_cast<const T*>(partial);
    a.y0 = static_cast<const T*>(y0);
    a.y1 = static_cast<const T*>(y1);
    const bool dev_dt = cb && cb->state_in_dev;      // hipGraph mode: dt = ctrl_dev[1] on the device
    const bool vec = fill_terms<T, NT>(a.k, a.c, k, coef, dt, dev_dt) && all_aligned(partial, y0, y1);
    a.dt_dev = dev_dt ? cb->ctrl_dev + 1 : nullptr;
    const SegTable& st = ns.st;
    hipStream_t s = ns.s;
    a.st = st;
    a.part_sumsq = ns.ws;
    a.part_bad = ns.ws + 2 * st.n_chunks;
    const dim3 g((unsigned)st.n_chunks), b(kBlock);
    // the common shape — one segment whose chunk_start is 0, dt folded by the host — has its own lean instantiation
    const bool single = st.n_seg == 1 && st.inl[0].chunk_start == 0, lean = single && !dev_dt;
    if (copy_last) {
        // (captured steps only: states of at most 2^22 elements, always the default cache policy)
        if constexpr (NT > 0) {
            const bool v = vec && aligned16(copy_last);
            if (v && single) hipLaunchKernelGGL((error_norm_partial_kernel<T, NT, true, 0, true, true, true>), g, b, 0, s, a);
            else if (v) hipLaunchKernelGGL((error_norm_partial_kernel<T, NT, true, 0, false, true, true>), g, b, 0, s, a);
            else hipLaunchKernelGGL((error_norm_partial_kernel<T, NT, false, 0, false, true, true>), g, b, 0, s, a);
        }
    } else if (vec && (stream_policy((int64_t)(NT + 3) * st.n_chunks * st.chunk * (int64_t)sizeof(T)) & 1))
        hipLaunchKernelGGL((error_norm_partial_kernel<T, NT, true, 1>), g, b, 0, s, a);
    else if (vec && lean) hipLaunchKernelGGL((error_norm_partial_kernel<T, NT, true, 0, true, false>), g, b, 0, s, a);
    else if (vec && single) hipLaunchKernelGGL((error_norm_partial_kernel<T, NT, true, 0, true, true>), g, b, 0, s, a);
    else if (vec) hipLaunchKernelGGL((error_norm_partial_kernel<T, NT, true, 0>), g, b, 0, s, a);
    else hipLaunchKernelGGL((error_norm_partial_kernel<T, NT, false>), g, b, 0, s, a);
    return finish_norm(ns, 1, out_sumsq, out_bad, cb, kTkind<T>);
}

template <typename T, int NT>
int launch_combine_devdt(void* out, void* err_out, const void* y0, const void* const* k, const double* coef,
                         const double* err_coef, const double* dt_dev, int64_t n, hipStream_t s) {
    CombineDevTArgs<T, NT> a;
    a.err_out = static_cast<T*>(err_out);
    const bool vec = fill_combine(a.c, out, y0, k, coef, 0.0, n, true, err_out ? &a.e : nullptr, err_coef) && aligned16(err_out);
    if (!err_out) for (int j = 0; j < NT; ++j) a.e[j] = (T)0;
    a.dt_dev = dt_dev;
    return stream_launch<T>(vec, n, [&](auto v, dim3 g) {
        flag(err_out != nullptr, [&](auto err) {
            hipLaunchKernelGGL((combine_devdt_kernel<T, NT, decltype(v)::value, decltype(err)::value>), g, dim3(kBlock), 0, s, a);
            return 0;
        });
    });
}

// States below this size are launch-latency-bound: the run-time-term-count kernel (one instantiation, smallest code)
// is as fast there; above it the unrolled 16-byte-per-lane form wins (profiles/r02_shard_regime.json).
constexpr int64_t kDevCombineTunedFrom = 1 << 17;

template <typename T>
int launch_combine_dev(void* out, void* err_out, const void* y0, const void* const* k, const double* coef,
                       const double* err_coef, int nt, const double* dt_dev, int64_t n, hipStream_t s) {
    if (n >= kDevCombineTunedFrom)
        return terms<1>(nt, [&](auto t) {
            return launch_combine_devdt<T, decltype(t)::value>(out, err_out, y0, k, coef, err_coef, dt_dev, n, s);
        });
    CombineDevArgs<T> a;
    a.out = static_cast<T*>(out);
    a.err_out = static_cast<T*>(err_out);
    a.y0 = static_cast<const T*>(y0);
    for (int j = 0; j < TDEQ_MAX_TERMS; ++j) {
        a.k[j] = j < nt ? static_cast<const T*>(k[j]) : nullptr;
        a.c[j] = j < nt ? (T)coef[j] : (T)0;
        a.e[j] = (j < nt && err_coef) ? (T)err_coef[j] : (T)0;
    }
    a.nt = nt;
    a.dt_dev = dt_dev;
    a.n = n;
    hipLaunchKernelGGL((combine_dev_kernel<T>), dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, s, a);
    return check_launch();
}

template <typename T>
int launch_commit(void* y_prev, void* f_prev, void* y_cur, void* f_cur, const void* y1, const void* f1,
                  const double* ctrl_dev, int64_t n, hipStream_t s) {
    CommitArgs<T> a;
    a.y_prev = static_cast<T*>(y_prev);
    a.f_prev = static_cast<T*>(f_prev);
    a.y_cur = static_cast<T*>(y_cur);
    a.f_cur = static_cast<T*>(f_cur);
    a.y1 = static_cast<const T*>(y1);
    a.f1 = static_cast<const T*>(f1);
    a.ctrl_dev = ctrl_dev;
    a.n = n;
    return stream_launch<T>(all_aligned(y_prev, f_prev, y_cur, f_cur, y1, f1), n, [&](auto v, dim3 g) {
        hipLaunchKernelGGL((step_commit_kernel<T, decltype(v)::value>), g, dim3(kBlock), 0, s, a);
    });
}

template <typename T>
int launch_combine_sel(void* out, const void* y_acc, const void* f_acc, const void* y_rej, const void* f_rej,
                       double coef, const double* ctrl_dev, int64_t n, hipStream_t s) {
    SelArgs<T> a;
    a.out = static_cast<T*>(out);
    a.y_acc = static_cast<const T*>(y_acc);
    a.f_acc = static_cast<const T*>(f_acc);
    a.y_rej = static_cast<const T*>(y_rej);
    a.f_rej = static_cast<const T*>(f_rej);
    a.coef = (T)coef;
    a.ctrl_dev = ctrl_dev;
    a.n = n;
    const dim3 b(kBlock);
    if (!all_aligned(out, y_acc, f_acc, y_rej, f_rej)) {
        hipLaunchKernelGGL((stage_combine_sel_kernel<T, false>), dim3(stream_grid(n, kBlock)), b, 0, s, a);
        return check_launch();
    }
    const dim3 g(stream_grid(n / VecOf<T>::L, kBlock));
    // (reads 2 of the 4 inputs; the k tensors of the step just finished are the cache's other tenants)
    return with_policy((int64_t)3 * n * (int64_t)sizeof(T), [&](auto p) {
        hipLaunchKernelGGL((stage_combine_sel_kernel<T, true, decltype(p)::value>), g, b, 0, s, a);
        return check_launch();
    });
}

// ---- init norms ------------------------------------------------------------------------------------
template <typename T>
int launch_init(int mode, const void* a_, const void* b_, const void* y_, const NormSetup& ns, double* out_sumsq,
                double* out_bad) {
    InitArgs<T> a;
    a.a = static_cast<const T*>(a_);
    a.b = static_cast<const T*>(b_);
    a.y = static_cast<const T*>(y_);
    a.st = ns.st;
    a.part0 = ns.ws;
    a.part1 = ns.ws + ns.st.n_chunks;
    a.part_bad = ns.ws + 2 * ns.st.n_chunks;
    const dim3 g((unsigned)ns.st.n_chunks), b(kBlock);
    flags(mode != 0, all_aligned(a_, b_, y_), [&](auto m, auto v) {
        hipLaunchKernelGGL((init_norms_kernel<T, decltype(m)::value ? 1 : 0, decltype(v)::value>), g, b, 0, ns.s, a);
        return 0;
    });
    return finish_norm(ns, mode == 0 ? 2 : 1, out_sumsq, out_bad);
}

template <typename T>
int launch_init_vec(int mode, const void* a_, const void* b_, const void* y_, const double* rtol_v, double rtol_s,
                    const double* atol_v, double atol_s, const NormSetup& ns, double* out_sumsq, double* out_bad) {
    InitVecArgs<T> a;
    a.a = static_cast<const T*>(a_);
    a.b = static_cast<const T*>(b_);
    a.y = static_cast<const T*>(y_);
    a.rtol_v = rtol_v;
    a.atol_v = atol_v;
    a.rtol_s = rtol_s;
    a.atol_s = atol_s;
    a.st = ns.st;
    a.part0 = ns.ws;
    a.part1 = ns.ws + ns.st.n_chunks;
    a.part_bad = ns.ws + 2 * ns.st.n_chunks;
    const dim3 g((unsigned)ns.st.n_chunks), b(kBlock);
    flag(mode != 0, [&](auto m) {
        hipLaunchKernelGGL((init_norms_vec_kernel<T, decltype(m)::value ? 1 : 0>), g, b, 0, ns.s, a);
        return 0;
    });
    return finish_norm(ns, mode == 0 ? 2 : 1, out_sumsq, out_bad);
}

// ---- complex states: the norm launches (tdeq_kernels_complex.hpp); T = the real type -------------------------------
template <typename T, int NT, bool PARTIAL>
int launch_cplx_error(const void* partial, void* scaled, const void* y0, const void* y1, const void* const* k,
                      const double* coef, double dt, const NormSetup& ns, double* out_sumsq, double* out_bad,
                      const CtrlBundle* cb) {
    CplxErrArgs<T, NT> a;
    a.partial = static_cast<const T*>(partial);
    a.scaled = static_cast<T*>(scaled);
    a.y0 = static_cast<const T*>(y0);
    a.y1 = static_cast<const T*>(y1);
    const bool dev_dt = cb && cb->state_in_dev;
    const bool vec = fill_terms<T, NT>(a.k, a.c, k, coef, dt, dev_dt) && all_aligned(y0, y1, scaled) &&
                     (!PARTIAL || aligned16(partial));
    a.dt_dev = dev_dt ? cb->ctrl_dev + 1 : nullptr;
    a.st = ns.st;
    a.part_sumsq = ns.ws;
    a.part_bad = ns.ws + 2 * ns.st.n_chunks;
    const dim3 g((unsigned)ns.st.n_chunks), b(kBlock);
    flags(vec, scaled != nullptr, [&](auto v, auto sc) {
        hipLaunchKernelGGL((cplx_error_norm_kernel<T, NT, decltype(v)::value, PARTIAL, decltype(sc)::value>), g, b, 0, ns.s, a);
        return 0;
    });
    return finish_norm(ns, 1, out_sumsq, out_bad, cb, kTkind<T>);
}

// mode 0 / 1; out0 given: the quotients are stored (tdeq_init_scaled: no workspace, no sums), else their sums
// (tdeq_init_norms)
template <typename T>
int launch_cplx_init(int mode, const void* a_, const void* b_, const void* y_, const NormSetup& ns, double* out_sumsq,
                     double* out_bad, void* out0, void* out1) {
    CplxInitArgs<T> a;
    a.a = static_cast<const T*>(a_);
    a.b = static_cast<const T*>(b_);
    a.y = static_cast<const T*>(y_);
    a.st = ns.st;
    a.part0 = ns.ws;
    a.part1 = ns.ws ? ns.ws + ns.st.n_chunks : nullptr;
    a.part_bad = ns.ws ? ns.ws + 2 * ns.st.n_chunks : nullptr;
    a.out0 = static_cast<T*>(out0);
    a.out1 = static_cast<T*>(out1);
    const dim3 g((unsigned)ns.st.n_chunks), b(kBlock);
    flags(mode != 0, out0 != nullptr, [&](auto m, auto o) {
        hipLaunchKernelGGL((cplx_init_norms_kernel<T, decltype(m)::value ? 1 : 0, decltype(o)::value>), g, b, 0, ns.s, a);
        return 0;
    });
    if (out0) return check_launch();
    return finish_norm(ns, mode == 0 ? 2 : 1, out_sumsq, out_bad);
}

// ---- dense output ----------------------------------------------------------------------------------
// the argument block of the dense-output kernels (c_j = dt * c_mid_j); returns the 16-byte decision of its pointers
template <typename T, int NT>
bool fill_dense(DenseArgs<T, NT>& a, void* out, const void* y0, const void* y1, const void* f0, const void* f1,
                const void* const* k, const double* coef, double dt, double x, int64_t n) {
    a.out = static_cast<T*>(out);
    a.y0 = static_cast<const T*>(y0);
    a.y1 = static_cast<const T*>(y1);
    a.f0 = static_cast<const T*>(f0);
    a.f1 = static_cast<const T*>(f1);
    a.dt = (T)dt;
    a.x = (T)x;
    a.n = n;
    return fill_terms<T, NT>(a.k, a.c, k, coef, dt, false) && all_aligned(out, y0, y1, f0, f1);
}

template <typename T, int NT, bool FIT_ONLY>
int launch_dense(void* out, const void* y0, const void* y1, const void* f0, const void* f1,
                 const void* const* k, const double* coef, double dt, double x, int64_t n, hipStream_t s) {
    DenseArgs<T, NT> a;
    bool vec = fill_dense(a, out, y0, y1, f0, f1, k, coef, dt, x, n);
    if (FIT_ONLY) vec = vec && (n % VecOf<T>::L == 0);   // the 5 coefficient planes must stay 16-byte aligned
    return stream_launch<T>(vec, n, [&](auto v, dim3 g) {
        hipLaunchKernelGGL((dense_kernel<T, NT, FIT_ONLY, decltype(v)::value>), g, dim3(kBlock), 0, s, a);
    });
}

template <typename T, int NT>
int launch_dense_multi(void* out, int64_t out_stride, const void* y0, const void* y1, const void* f0, const void* f1,
                       const void* const* k, const double* coef, double dt, const double* x, int n_x, int64_t n,
                       hipStream_t s) {
    DenseMultiArgs<T, NT> a;
    bool vec = fill_dense(a.d, out, y0, y1, f0, f1, k, coef, dt, 0.0, n);
    for (int r = 0; r < kMaxDenseOutputs; ++r) a.xs[r] = r < n_x ? (T)x[r] : (T)0;
    a.m = n_x;
    a.out_stride = out_stride;
    vec = vec && (n_x == 1 || (out_stride * (int64_t)sizeof(T)) % 16 == 0);   // every output row 16-byte aligned
    return stream_launch<T>(vec, n, [&](auto v, dim3 g) {
        hipLaunchKernelGGL((dense_multi_kernel<T, NT, decltype(v)::value>), g, dim3(kBlock), 0, s, a);
    });
}

// ---- rk4 / lerp ------------------------------------------------------------------------------------
// (a stage reads k1..k<STAGE>: the entry points have checked those)
template <typename T, int STAGE>
int launch_rk4(void* out, const void* y0, const void* const (&ks)[4], double dt, int64_t n, hipStream_t s,
               const double* dt_dev = nullptr) {
    Rk4Args<T> a;
    a.dt_dev = dt_dev;
    a.out = static_cast<T*>(out);
    a.y0 = static_cast<const T*>(y0);
    a.k1 = static_cast<const T*>(ks[0]);
    a.k2 = static_cast<const T*>(ks[1]);
    a.k3 = static_cast<const T*>(ks[2]);
    a.k4 = static_cast<const T*>(ks[3]);
    a.dt = (T)dt;
    a.third = (T)(1.0 / 3.0);   // `_one_third` rounded to T — rk_common.py:94,114-115
    a.n = n;
    return stream_launch<T>(all_aligned(out, y0, Ptrs{ks, STAGE}), n, [&](auto v, dim3 g) {
        hipLaunchKernelGGL((rk4_kernel<T, STAGE, decltype(v)::value>), g, dim3(kBlock), 0, s, a);
    });
}

template <typename T>
int launch_grid_commit(void* solution, int64_t row_stride, void* y_cur, const void* y_new, const int64_t* counter,
                       int64_t n, hipStream_t s) {
    GridCommitArgs<T> a;
    a.solution = static_cast<T*>(solution);
    a.row_stride = row_stride;
    a.y_cur = static_cast<T*>(y_cur);
    a.y_new = static_cast<const T*>(y_new);
    a.counter = counter;
    a.n = n;
    hipLaunchKernelGGL((grid_commit_kernel<T>), dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, s, a);
    return check_launch();
}

template <typename T>
int launch_lerp(void* out, const void* y0, const void* y1, double slope, int64_t n, hipStream_t s) {
    LerpArgs<T> a;
    a.out = static_cast<T*>(out);
    a.y0 = static_cast<const T*>(y0);
    a.y1 = static_cast<const T*>(y1);
    a.slope = (T)slope;
    a.n = n;
    return stream_launch<T>(all_aligned(out, y0, y1), n, [&](auto v, dim3 g) {
        hipLaunchKernelGGL((lerp_kernel<T, decltype(v)::value>), g, dim3(kBlock), 0, s, a);
    });
}

// ---- low-order fixed-grid stages / weighted sums -----------------------------------------------------
template <typename T, int NT, int MODE>
int launch_fixed(void* out, const void* y0, const void* const* k, const double* w, double dt, int64_t n,
                 hipStream_t s, const double* dt_dev = nullptr) {
    FixedArgs<T, NT> a;
    a.dt_dev = dt_dev;
    a.out = static_cast<T*>(out);
    a.y0 = static_cast<const T*>(y0);
    for (int j = 0; j < NT; ++j) {
        a.k[j] = static_cast<const T*>(k[j]);
        a.w[j] = (T)w[j];   // Python-float weights meet a T tensor: rounded to T (rk_common.py:139-157)
    }
    a.dt = (T)dt;
    a.n = n;
    const bool vec = all_aligned(out, Ptrs{k, NT}) && (MODE == 2 || aligned16(y0));
    return stream_launch<T>(vec, n, [&](auto v, dim3 g) {
        hipLaunchKernelGGL((fixed_stage_kernel<T, NT, MODE, decltype(v)::value>), g, dim3(kBlock), 0, s, a);
    });
}

// ---- backward helpers: scale_many / multi_dot ------------------------------------------------------------
template <typename T, int NT>
int launch_scale(void* const* outs, const void* g, const double* w, int64_t n, hipStream_t s) {
    ScaleArgs<T, NT> a;
    a.g = static_cast<const T*>(g);
    for (int j = 0; j < NT; ++j) {
        a.out[j] = static_cast<T*>(outs[j]);
        a.w[j] = (T)w[j];
    }
    a.n = n;
    return stream_launch<T>(all_aligned(g, Ptrs{outs, NT}), n, [&](auto v, dim3 grid) {
        hipLaunchKernelGGL((scale_many_kernel<T, NT, decltype(v)::value>), grid, dim3(kBlock), 0, s, a);
    });
}

constexpr int64_t kDotChunk = 4096;

template <typename T, int NT>
int launch_dots(const void* g, const void* const* x, int64_t n, double* out, double* ws, hipStream_t s) {
    DotArgs<T, NT> a;
    a.g = static_cast<const T*>(g);
    for (int j = 0; j < NT; ++j) a.x[j] = static_cast<const T*>(x[j]);
    a.n = n;
    a.chunk = kDotChunk;
    a.n_chunks = (n + kDotChunk - 1) / kDotChunk;
    if (a.n_chunks < 1) a.n_chunks = 1;
    a.part = ws;
    const dim3 grid((unsigned)a.n_chunks), blk(kBlock);
    const int e = flag(all_aligned(g, Ptrs{x, NT}), [&](auto v) {
        hipLaunchKernelGGL((multi_dot_kernel<T, NT, decltype(v)::value>), grid, blk, 0, s, a);
        return check_launch();
    });
    if (e) return e;
    DotFinalizeArgs f;
    f.part = ws;
    f.n_chunks = a.n_chunks;
    f.out = out;
    hipLaunchKernelGGL(dot_finalize_kernel, dim3(NT), dim3(kBlock), 0, s, f);
    return check_launch();
}

template <typename T>
int launch_pack(void* out, const void* const* src, const int64_t* chunk_start, const int64_t* numel,
                const double* scale, int n_seg, int64_t chunk, int64_t n_chunks, hipStream_t s) {
    PackArgs<T> a;
    a.out = static_cast<T*>(out);
    for (int q = 0; q < TDEQ_INLINE_SEGMENTS; ++q) {
        if (q < n_seg) a.seg[q] = PackSeg{src[q], chunk_start[q], numel[q], scale[q], aligned16(src[q]) ? 1 : 0};
        else a.seg[q] = PackSeg{nullptr, 0, 0, 0.0, 0};
    }
    a.n_seg = n_seg;
    a.chunk = chunk;
    hipLaunchKernelGGL((pack_segments_kernel<T>), dim3((unsigned)n_chunks), dim3(kBlock), 0, s, a);
    return check_launch();
}

// ---- Adams–Bashforth(–Moulton) -----------------------------------------------------------------------
template <typename T, int NT>
int launch_adams_predict(void* y_out, void* dy_out, void* delta_out, const void* y0, const void* const* f,
                         const double* cb, const double* cm, double dt, int64_t n, hipStream_t s) {
    AdamsPredictArgs<T, NT> a;
    const bool implicit = dy_out != nullptr;
    a.y_out = static_cast<T*>(y_out);
    a.dy_out = static_cast<T*>(dy_out);
    a.delta_out = static_cast<T*>(delta_out);
    a.y0 = static_cast<const T*>(y0);
    for (int j = 0; j < NT; ++j) {
        a.f[j] = static_cast<const T*>(f[j]);
        a.cb[j] = (T)cb[j];
        a.cm[j] = implicit ? (T)cm[j] : (T)0;
    }
    a.dt = (T)dt;
    a.n = n;
    return stream_launch<T>(all_aligned(y_out, y0, dy_out, delta_out, Ptrs{f, NT}), n, [&](auto v, dim3 g) {
        flag(implicit, [&](auto im) {
            hipLaunchKernelGGL((adams_predict_kernel<T, NT, decltype(im)::value, decltype(v)::value>), g, dim3(kBlock), 0, s, a);
            return 0;
        });
    });
}

template <typename T>
int launch_adams_correct(void* y_out, void* dy_out, const void* f, const void* delta, const void* dy_old,
                         const void* y0, double c, bool compute, const NormSetup& ns, int64_t n, double* out_count,
                         double* out_bad) {
    AdamsCorrectArgs<T> a;
    a.y_out = static_cast<T*>(y_out);
    a.dy_out = static_cast<T*>(dy_out);
    a.f = static_cast<const T*>(f);
    a.delta = static_cast<const T*>(delta);
    a.dy_old = static_cast<const T*>(dy_old);
    a.y0 = static_cast<const T*>(y0);
    a.c = (T)c;
    a.n = n;
    a.st = ns.st;
    a.part_count = ns.ws;
    a.part_bad = ns.ws + 2 * ns.st.n_chunks;
    const dim3 g((unsigned)ns.st.n_chunks), b(kBlock);
    flags(compute, all_aligned(y_out, dy_out, f, delta, dy_old, y0), [&](auto cp, auto v) {
        hipLaunchKernelGGL((adams_correct_kernel<T, decltype(cp)::value, decltype(v)::value>), g, b, 0, ns.s, a);
        return 0;
    });
    return finish_norm(ns, 1, out_count, out_bad);
}

#include "tdeq_abi_lp.hpp"

// ---- what the entry points check before anything else -----------------------------------------------------------------
// n_terms in [lo, hi] and every pointer of the array non-null
inline int check_terms(const void* const* k, int n_terms, int lo, int hi = TDEQ_MAX_TERMS) {
    if (n_terms < lo || n_terms > hi || (n_terms > 0 && !k)) return TDEQ_EINVAL;
    for (int j = 0; j < n_terms; ++j) if (!k[j]) return TDEQ_EINVAL;
    return 0;
}

}  // namespace

extern "C" {

int tdeq_abi_version(void) { return TDEQ_ABI_VERSION; }

size_t tdeq_workspace_bytes(int64_t n_chunks) {
    if (n_chunks < 1) n_chunks = 1;
    return (size_t)n_chunks * 3 * sizeof(double);
}

int tdeq_stage_combine(void* out, const void* y0, const void* const* k, const double* coef, int n_terms,
                       double dt, int64_t n, int dtype, void* stream) {
    if (!out || !y0 || !k || !coef || n < 0 || !state_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (const int e = check_terms(k, n_terms, 1)) return e;
    if (n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return state_dtype_terms<1>(dtype, n_terms, [&](auto t, auto nt) {
        using T = decltype(t);
        constexpr int NT = decltype(nt)::value;
        if constexpr (is_lp<T>) return lp_launch_combine<T, NT, 1>(out, nullptr, y0, k, coef, nullptr, dt, n, s);
        else return launch_combine<T, NT>(out, y0, k, coef, dt, n, s);
    });
}

int tdeq_stage_combine_timed(void* out, const void* y0, const void* const* k, const double* coef, int n_terms,
                             double dt, int64_t n, int dtype, void* stream, void* start_event, void* stop_event) {
    if (!out || !y0 || !k || !coef || n < 1 || !real_dtype_ok(dtype) || !start_event || !stop_event) return TDEQ_EINVAL;
    if (const int e = check_terms(k, n_terms, 1)) return e;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipEvent_t e0 = static_cast<hipEvent_t>(start_event), e1 = static_cast<hipEvent_t>(stop_event);
    return real_dtype_terms<1>(dtype, n_terms, [&](auto t, auto nt) {
        return launch_combine<decltype(t), decltype(nt)::value>(out, y0, k, coef, dt, n, s, e0, e1);
    });
}

int tdeq_stage_combine_fill(void* out, const void* y0, const void* const* k, const double* coef, int n_terms,
                            double dt, int64_t n, int dtype, void* fill_dst, const double* fill_vals, int n_fill,
                            void* stream) {
    if (!out || !y0 || !k || !coef || n < 1 || !state_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (const int e = check_terms(k, n_terms, 1, 2)) return e;
    if (!fill_dst || !fill_vals || n_fill < 1 || n_fill > 16) return TDEQ_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return state_dtype_terms<1, 2>(dtype, n_terms, [&](auto t, auto nt) {
        using T = decltype(t);
        constexpr int NT = decltype(nt)::value;
        if constexpr (is_lp<T>)
            return lp_launch_combine<T, NT, 1>(out, nullptr, y0, k, coef, nullptr, dt, n, s, nullptr, fill_dst, fill_vals, n_fill);
        else return launch_combine_fill<T, NT>(out, y0, k, coef, dt, n, fill_dst, fill_vals, n_fill, s);
    });
}

int tdeq_error_norm(void* scaled_out, const void* y0, const void* y1, const void* const* k,
                    const double* coef, int n_terms, double dt, const tdeq_segment* segs,
                    const void* segs_dev, int n_seg, int64_t chunk, int64_t n_chunks, double* out_sumsq,
                    double* out_nonfinite, void* workspace, size_t workspace_bytes, int dtype,
                    void* stream) {
    if (!y0 || !y1 || !k || !coef || !out_sumsq || !out_nonfinite || !workspace || !(state_dtype_ok(dtype) || cplx_dtype(dtype)))
        return TDEQ_EINVAL;
    if (const int e = check_terms(k, n_terms, 1)) return e;
    NormSetup ns;
    if (const int e = norm_setup(ns, segs, segs_dev, n_seg, chunk, n_chunks, workspace, workspace_bytes, stream)) return e;
    // bf16 / fp16: out_sumsq[s] = sum of fl(|r|^2) — |r| itself for a one-element segment (tdeq_kernels_lp.hpp norm_term)
    return norm_dtype(dtype, [&](auto t, auto cplx) {
        return terms<1>(n_terms, [&](auto nt) {
            using T = decltype(t);
            constexpr int NT = decltype(nt)::value;
            if constexpr (is_lp<T>) return lp_launch_error<T, NT>(scaled_out, y0, y1, k, coef, dt, ns, out_sumsq, out_nonfinite);
            else if constexpr (decltype(cplx)::value)
                return launch_cplx_error<T, NT, false>(nullptr, scaled_out, y0, y1, k, coef, dt, ns, out_sumsq, out_nonfinite, nullptr);
            else return launch_error<T, NT>(scaled_out, y0, y1, k, coef, dt, ns, out_sumsq, out_nonfinite);
        });
    });
}

// tdeq_error_norm_vec with an optional controller bundle (ctrl == nullptr: none)
static int error_norm_vec_checked(const void* err_partial, const void* y0, const void* y1, const void* const* k,
                                  const double* coef, int n_terms, double dt, const double* rtol_vec, double rtol_scalar,
                                  const double* atol_vec, double atol_scalar, const tdeq_segment* segs, const void* segs_dev,
                                  int n_seg, int64_t chunk, int64_t n_chunks, double* out_sumsq, double* out_nonfinite,
                                  const CtrlBundle* cb, void* workspace, size_t workspace_bytes, int dtype, void* stream) {
    if (!y0 || !y1 || !out_sumsq || !out_nonfinite || !workspace || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (!rtol_vec && !atol_vec) return TDEQ_EINVAL;      // two 0-dim tolerances: tdeq_error_norm (a different promotion)
    if ((n_terms > 0 && !coef) || check_terms(k, n_terms, err_partial ? 0 : 1)) return TDEQ_EINVAL;
    NormSetup ns;
    if (const int e = norm_setup(ns, segs, segs_dev, n_seg, chunk, n_chunks, workspace, workspace_bytes, stream)) return e;
    return real_dtype_terms<0>(dtype, n_terms, [&](auto t, auto nt) {
        return launch_error_vec<decltype(t), decltype(nt)::value>(err_partial, y0, y1, k, coef, dt, rtol_vec, rtol_scalar,
                                                                  atol_vec, atol_scalar, ns, out_sumsq, out_nonfinite, cb);
    });
}

int tdeq_error_norm_vec(const void* err_partial, const void* y0, const void* y1, const void* const* k, const double* coef,
                        int n_terms, double dt, const double* rtol_vec, double rtol_scalar, const double* atol_vec, double atol_scalar,
                        const tdeq_segment* segs, const void* segs_dev, int n_seg, int64_t chunk, int64_t n_chunks,
                        double* out_sumsq, double* out_nonfinite, void* workspace, size_t workspace_bytes, int dtype,
                        void* stream) {
    return error_norm_vec_checked(err_partial, y0, y1, k, coef, n_terms, dt, rtol_vec, rtol_scalar, atol_vec, atol_scalar, segs,
                                  segs_dev, n_seg, chunk, n_chunks, out_sumsq, out_nonfinite, nullptr, workspace,
                                  workspace_bytes, dtype, stream);
}

int tdeq_error_norm_vec_ctrl(const void* err_partial, const void* y0, const void* y1, const void* const* k,
                             const double* coef, int n_terms, double dt, const double* rtol_vec, double rtol_scalar, const double* atol_vec, double atol_scalar,
                             const tdeq_segment* segs, const void* segs_dev, int n_seg, int64_t chunk, int64_t n_chunks,
                             double* out_sumsq, double* out_nonfinite, const tdeq_step_ctrl* ctrl, double* out_ctrl,
                             double* ctrl_dev, void* next_times, int state_in_dev, void* workspace, size_t workspace_bytes,
                             int dtype, void* stream) {
    CtrlBundle cb;
    if (const int e = make_ctrl(cb, ctrl, out_ctrl, ctrl_dev, next_times, state_in_dev, n_seg)) return e;
    return error_norm_vec_checked(err_partial, y0, y1, k, coef, n_terms, dt, rtol_vec, rtol_scalar, atol_vec, atol_scalar, segs,
                                  segs_dev, n_seg, chunk, n_chunks, out_sumsq, out_nonfinite, &cb, workspace, workspace_bytes,
                                  dtype, stream);
}

int tdeq_stage_combine_err(void* out, void* err_out, const void* y0, const void* const* k, const double* coef,
                           const double* err_coef, int n_terms, double dt, int64_t n, int dtype, void* stream) {
    if (!out || !err_out || !y0 || !k || !coef || !err_coef || n < 0 || !state_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (const int e = check_terms(k, n_terms, 1)) return e;
    if (n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (bf16 / fp16: err_out is the row sum over THESE stages rounded once — a caller that continues it rounds twice)
    return state_dtype_terms<1>(dtype, n_terms, [&](auto t, auto nt) {
        using T = decltype(t);
        constexpr int NT = decltype(nt)::value;
        if constexpr (is_lp<T>) return lp_launch_combine<T, NT, 2>(out, err_out, y0, k, coef, err_coef, dt, n, s);
        else return launch_combine_err<T, NT>(out, err_out, y0, k, coef, err_coef, dt, n, s);
    });
}

static int combine_multi_checked(const tdeq_multi_out* outs, int n_out, const void* y0, const void* acc_in,
                                 const void* const* k, int n_terms, double dt, int64_t n, int dtype, void* stream,
                                 void* e0, void* e1, const double* dt_dev = nullptr) {
    if (!outs || !y0 || !k || n < 0 || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (check_terms(k, n_terms, 1) || n_out < 1 || n_out > TDEQ_MAX_MULTI_OUT) return TDEQ_EINVAL;
    for (int o = 0; o < n_out; ++o) {
        if (!outs[o].out || outs[o].mask == 0u) return TDEQ_EINVAL;
        if (n_terms < 32 && (outs[o].mask >> n_terms) != 0u) return TDEQ_EINVAL;
    }
    if (n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype_terms<1>(dtype, n_terms, [&](auto t, auto nt) {
        return launch_combine_multi<decltype(t), decltype(nt)::value>(outs, n_out, y0, acc_in, k, dt, n, s, static_cast<hipEvent_t>(e0),
                                                                      static_cast<hipEvent_t>(e1), dt_dev);
    });
}

int tdeq_stage_combine_multi(const tdeq_multi_out* outs, int n_out, const void* y0, const void* acc_in,
                             const void* const* k, int n_terms, double dt, int64_t n, int dtype, void* stream) {
    return combine_multi_checked(outs, n_out, y0, acc_in, k, n_terms, dt, n, dtype, stream, nullptr, nullptr);
}

int tdeq_stage_combine_multi_dev(const tdeq_multi_out* outs, int n_out, const void* y0, const void* acc_in,
                                 const void* const* k, int n_terms, const double* ctrl_dev, int64_t n, int dtype,
                                 void* stream) {
    if (!ctrl_dev) return TDEQ_EINVAL;
    return combine_multi_checked(outs, n_out, y0, acc_in, k, n_terms, 0.0, n, dtype, stream, nullptr, nullptr, ctrl_dev);
}

int tdeq_stage_combine_multi_timed(const tdeq_multi_out* outs, int n_out, const void* y0, const void* acc_in,
                                   const void* const* k, int n_terms, double dt, int64_t n, int dtype, void* stream,
                                   void* start_event, void* stop_event) {
    if (!start_event || !stop_event) return TDEQ_EINVAL;
    return combine_multi_checked(outs, n_out, y0, acc_in, k, n_terms, dt, n, dtype, stream, start_event, stop_event);
}

// tdeq_error_norm_partial with an optional controller bundle.  fp32 / fp64 / complex continue err_partial with 0..2
// terms.  bf16 / fp16 (with a bundle only): the WHOLE error row in one launch — a row is rounded once, so there is no
// partial sum to continue: err_partial must be NULL and there is at least one term — then finalize + controller in the
// state's type.
static int error_norm_partial_checked(const void* err_partial, const void* y0, const void* y1, const void* const* k,
                                      const double* coef, int n_terms, double dt, const tdeq_segment* segs,
                                      const void* segs_dev, int n_seg, int64_t chunk, int64_t n_chunks, double* out_sumsq,
                                      double* out_nonfinite, const CtrlBundle* cb, void* copy_last_k, void* workspace,
                                      size_t workspace_bytes, int dtype, void* stream) {
    const bool low = cb && lp_dtype(dtype);
    if (copy_last_k && (low || cplx_dtype(dtype) || n_terms < 1)) return TDEQ_EINVAL;
    if (!y0 || !y1 || !out_sumsq || !out_nonfinite || !workspace || !(low || real_dtype_ok(dtype) || cplx_dtype(dtype)))
        return TDEQ_EINVAL;
    if (low ? err_partial != nullptr : !err_partial) return TDEQ_EINVAL;
    if ((n_terms > 0 && !coef) || check_terms(k, n_terms, low ? 1 : 0, low ? TDEQ_MAX_TERMS : 2)) return TDEQ_EINVAL;
    NormSetup ns;
    if (const int e = norm_setup(ns, segs, segs_dev, n_seg, chunk, n_chunks, workspace, workspace_bytes, stream)) return e;
    return norm_dtype(dtype, [&](auto t, auto cplx) {
        using T = decltype(t);
        if constexpr (is_lp<T>)
            return terms<1>(n_terms, [&](auto nt) {
                return lp_launch_error<T, decltype(nt)::value>(nullptr, y0, y1, k, coef, dt, ns, out_sumsq, out_nonfinite, cb);
            });
        else
            return terms<0, 2>(n_terms, [&](auto nt) {
                constexpr int NT = decltype(nt)::value;
                if constexpr (decltype(cplx)::value)
                    return launch_cplx_error<T, NT, true>(err_partial, nullptr, y0, y1, k, coef, dt, ns, out_sumsq, out_nonfinite, cb);
                else return launch_error_partial<T, NT>(err_partial, y0, y1, k, coef, dt, ns, out_sumsq, out_nonfinite, cb, copy_last_k);
            });
    });
}

int tdeq_error_norm_partial(const void* err_partial, const void* y0, const void* y1, const void* const* k,
                            const double* coef, int n_terms, double dt, const tdeq_segment* segs,
                            const void* segs_dev, int n_seg, int64_t chunk, int64_t n_chunks, double* out_sumsq,
                            double* out_nonfinite, void* workspace, size_t workspace_bytes, int dtype,
                            void* stream) {
    return error_norm_partial_checked(err_partial, y0, y1, k, coef, n_terms, dt, segs, segs_dev, n_seg, chunk, n_chunks,
                                      out_sumsq, out_nonfinite, nullptr, nullptr, workspace, workspace_bytes, dtype, stream);
}

int tdeq_error_norm_partial_ctrl(const void* err_partial, const void* y0, const void* y1, const void* const* k,
                                 const double* coef, int n_terms, double dt, const tdeq_segment* segs,
                                 const void* segs_dev, int n_seg, int64_t chunk, int64_t n_chunks, double* out_sumsq,
                                 double* out_nonfinite, const tdeq_step_ctrl* ctrl, double* out_ctrl, double* ctrl_dev,
                                 void* next_times, int state_in_dev, void* copy_last_k, void* workspace,
                                 size_t workspace_bytes, int dtype, void* stream) {
    CtrlBundle cb;
    if (const int e = make_ctrl(cb, ctrl, out_ctrl, ctrl_dev, next_times, state_in_dev, n_seg)) return e;
    return error_norm_partial_checked(err_partial, y0, y1, k, coef, n_terms, dt, segs, segs_dev, n_seg, chunk, n_chunks,
                                      out_sumsq, out_nonfinite, &cb, copy_last_k, workspace, workspace_bytes, dtype, stream);
}

int tdeq_step_controller(const double* sums, const double* nonfinite, const tdeq_segment* segs, const void* segs_dev,
                         int n_seg, double* out_sumsq, double* out_nonfinite, const tdeq_step_ctrl* ctrl,
                         double* out_ctrl, double* ctrl_dev, void* next_times, int state_in_dev, int dtype,
                         void* stream) {
    if (!sums || !nonfinite || !segs || !out_sumsq || !out_nonfinite || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    CtrlBundle cb;
    if (const int e = make_ctrl(cb, ctrl, out_ctrl, ctrl_dev, next_times, state_in_dev, n_seg)) return e;
    SegTable st;
    const int e = fill_segtable(st, segs, segs_dev, n_seg, TDEQ_CHUNK_QUANTUM, 1);   // only numel is read
    if (e) return e;
    CtrlArgs a;
    a.part_sumsq = nullptr;
    a.part_bad = nullptr;
    a.st = st;
    a.c = *ctrl;
    a.is_f32 = dtype == TDEQ_F32 ? 1 : 0;
    a.ratio_kind = a.is_f32;
    a.out_sumsq = out_sumsq;
    a.out_bad = out_nonfinite;
    a.out_ctrl = out_ctrl;
    a.ctrl_dev = ctrl_dev;
    a.next_times = next_times;
    a.state_in_dev = cb.state_in_dev;
    a.presummed = 1;
    a.in_sumsq = sums;
    a.in_bad = nonfinite;
    hipLaunchKernelGGL(norm_finalize_ctrl_kernel<1>, dim3(1), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    return check_launch();
}

int tdeq_stage_combine_dev(void* out, void* err_out, const void* y0, const void* const* k, const double* coef,
                           const double* err_coef, int n_terms, const double* ctrl_dev, int64_t n, int dtype,
                           void* stream) {
    if (!out || !y0 || !k || !coef || !ctrl_dev || n < 0 || !state_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (check_terms(k, n_terms, 1) || (err_out && !err_coef)) return TDEQ_EINVAL;
    if (lp_dtype(dtype) && err_out) return TDEQ_EINVAL;      // a 16-bit row is rounded once: no partial error to continue
    if (n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return state_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if constexpr (is_lp<T>)
            return terms<1>(n_terms, [&](auto nt) {
                return lp_launch_combine<T, decltype(nt)::value, 1>(out, nullptr, y0, k, coef, nullptr, 0.0, n, s, ctrl_dev);
            });
        else return launch_combine_dev<T>(out, err_out, y0, k, coef, err_coef, n_terms, ctrl_dev + 1, n, s);
    });
}

int tdeq_step_commit(void* y_prev, void* f_prev, void* y_cur, void* f_cur, const void* y1, const void* f1,
                     const double* ctrl_dev, int64_t n, int dtype, void* stream) {
    if (!y_prev || !f_prev || !y_cur || !f_cur || !y1 || !f1 || !ctrl_dev || n < 0 || !real_dtype_ok(dtype))
        return TDEQ_EINVAL;
    if (n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype(dtype, [&](auto t) {
        return launch_commit<decltype(t)>(y_prev, f_prev, y_cur, f_cur, y1, f1, ctrl_dev, n, s);
    });
}

int tdeq_stage_combine_sel(void* out, const void* y_acc, const void* f_acc, const void* y_rej, const void* f_rej,
                           double coef, const double* ctrl_dev, int64_t n, int dtype, void* stream) {
    if (!out || !y_acc || !f_acc || !y_rej || !f_rej || !ctrl_dev || n < 0 || !state_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return state_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if constexpr (is_lp<T>) return lp_launch_sel<T>(out, y_acc, f_acc, y_rej, f_rej, coef, ctrl_dev, n, s);
        else return launch_combine_sel<T>(out, y_acc, f_acc, y_rej, f_rej, coef, ctrl_dev, n, s);
    });
}

int tdeq_init_norms(int mode, const void* a, const void* b, const void* yscale, const tdeq_segment* segs,
                    const void* segs_dev, int n_seg, int64_t chunk, int64_t n_chunks, double* out_sumsq,
                    double* out_nonfinite, void* workspace, size_t workspace_bytes, int dtype,
                    void* stream) {
    if ((mode != 0 && mode != 1) || !a || !b || !yscale || !out_sumsq || !out_nonfinite || !workspace ||
        !(state_dtype_ok(dtype) || cplx_dtype(dtype)))
        return TDEQ_EINVAL;
    NormSetup ns;
    if (const int e = norm_setup(ns, segs, segs_dev, n_seg, chunk, n_chunks, workspace, workspace_bytes, stream)) return e;
    return norm_dtype(dtype, [&](auto t, auto cplx) {
        using T = decltype(t);
        if constexpr (is_lp<T>) return lp_launch_init<T>(mode, a, b, yscale, ns, out_sumsq, out_nonfinite, nullptr, nullptr);
        else if constexpr (decltype(cplx)::value)
            return launch_cplx_init<T>(mode, a, b, yscale, ns, out_sumsq, out_nonfinite, nullptr, nullptr);
        else return launch_init<T>(mode, a, b, yscale, ns, out_sumsq, out_nonfinite);
    });
}

int tdeq_init_norms_vec(int mode, const void* a, const void* b, const void* yscale, const double* rtol_vec,
                        double rtol_scalar, const double* atol_vec, double atol_scalar, const tdeq_segment* segs,
                        const void* segs_dev, int n_seg, int64_t chunk, int64_t n_chunks, double* out_sumsq,
                        double* out_nonfinite, void* workspace, size_t workspace_bytes, int dtype, void* stream) {
    if ((mode != 0 && mode != 1) || !a || !b || !yscale || !out_sumsq || !out_nonfinite || !workspace || !real_dtype_ok(dtype))
        return TDEQ_EINVAL;
    if (!rtol_vec && !atol_vec) return TDEQ_EINVAL;      // two 0-dim tolerances: tdeq_init_norms (a different promotion)
    NormSetup ns;
    if (const int e = norm_setup(ns, segs, segs_dev, n_seg, chunk, n_chunks, workspace, workspace_bytes, stream)) return e;
    return real_dtype(dtype, [&](auto t) {
        return launch_init_vec<decltype(t)>(mode, a, b, yscale, rtol_vec, rtol_scalar, atol_vec, atol_scalar, ns, out_sumsq,
                                            out_nonfinite);
    });
}

int tdeq_init_scaled(int mode, const void* a, const void* b, const void* yscale, const tdeq_segment* segs,
                     const void* segs_dev, int n_seg, int64_t chunk, int64_t n_chunks, void* out0, void* out1,
                     int dtype, void* stream) {
    if ((mode != 0 && mode != 1) || !a || !b || !yscale || !out0 || (mode == 0 && !out1) ||
        !(state_dtype_ok(dtype) || cplx_dtype(dtype)))
        return TDEQ_EINVAL;
    NormSetup ns{{}, nullptr, static_cast<hipStream_t>(stream)};      // no sums: no workspace
    const int e = fill_segtable(ns.st, segs, segs_dev, n_seg, chunk, n_chunks);
    if (e) return e;
    return norm_dtype(dtype, [&](auto t, auto cplx) {
        using T = decltype(t);
        if constexpr (is_lp<T>) return lp_launch_init<T>(mode, a, b, yscale, ns, nullptr, nullptr, out0, out1);
        else if constexpr (decltype(cplx)::value) return launch_cplx_init<T>(mode, a, b, yscale, ns, nullptr, nullptr, out0, out1);
        else {
            InitScaledArgs<T> x{static_cast<const T*>(a), static_cast<const T*>(b), static_cast<const T*>(yscale), ns.st,
                                static_cast<T*>(out0), static_cast<T*>(out1)};
            return flag(mode != 0, [&](auto m) {
                hipLaunchKernelGGL((init_scaled_kernel<T, decltype(m)::value ? 1 : 0>), dim3((unsigned)ns.st.n_chunks), dim3(kBlock),
                                   0, ns.s, x);
                return check_launch();
            });
        }
    });
}

int tdeq_dense_eval(void* out, const void* y0, const void* y1, const void* f0, const void* f1,
                    const void* const* k, const double* coef, int n_terms, double dt, double x, int64_t n,
                    int dtype, void* stream) {
    if (!out || !y0 || !y1 || !f0 || !f1 || !k || !coef || n < 0 || !state_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (const int e = check_terms(k, n_terms, 1)) return e;
    if (n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return state_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if constexpr (is_lp<T>) return lp_dense_eval<T>(out, n, y0, y1, f0, f1, k, coef, n_terms, dt, &x, 1, n, s);
        else
            return terms<1>(n_terms, [&](auto nt) {
                return launch_dense<T, decltype(nt)::value, false>(out, y0, y1, f0, f1, k, coef, dt, x, n, s);
            });
    });
}

int tdeq_dense_eval_multi(void* out, int64_t out_stride, const void* y0, const void* y1, const void* f0,
                          const void* f1, const void* const* k, const double* coef, int n_terms, double dt,
                          const double* x, int n_x, int64_t n, int dtype, void* stream) {
    if (!out || !y0 || !y1 || !f0 || !f1 || !k || !coef || !x || n < 0 || !state_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (check_terms(k, n_terms, 1) || n_x < 1 || n_x > TDEQ_MAX_DENSE_OUTPUTS) return TDEQ_EINVAL;
    if (n_x > 1 && out_stride < n) return TDEQ_EINVAL;
    if (n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return state_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if constexpr (is_lp<T>) return lp_dense_eval<T>(out, out_stride, y0, y1, f0, f1, k, coef, n_terms, dt, x, n_x, n, s);
        else
            return terms<1>(n_terms, [&](auto nt) {
                return launch_dense_multi<T, decltype(nt)::value>(out, out_stride, y0, y1, f0, f1, k, coef, dt, x, n_x, n, s);
            });
    });
}

int tdeq_interp_fit(void* coeffs, const void* y0, const void* y1, const void* f0, const void* f1,
                    const void* const* k, const double* coef, int n_terms, double dt, int64_t n, int dtype,
                    void* stream) {
    if (!coeffs || !y0 || !y1 || !f0 || !f1 || !k || !coef || n < 0 || !state_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (const int e = check_terms(k, n_terms, 1)) return e;
    if (n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return state_dtype_terms<1>(dtype, n_terms, [&](auto t, auto nt) {
        using T = decltype(t);
        constexpr int NT = decltype(nt)::value;
        if constexpr (is_lp<T>) return lp_launch_fit<T, NT>(coeffs, y0, y1, f0, f1, k, coef, dt, n, s);
        else return launch_dense<T, NT, true>(coeffs, y0, y1, f0, f1, k, coef, dt, 0.0, n, s);
    });
}

// tdeq_rk4_38_stage with the step size from the host (dt) or from device memory (dt_dev: fp32 / fp64 only)
static int rk4_stage_checked(int stage, void* out, const void* y0, const void* const (&ks)[4], double dt,
                             const double* dt_dev, int64_t n, int dtype, void* stream) {
    if (!out || !y0 || n < 0 || !(dt_dev ? real_dtype_ok(dtype) : state_dtype_ok(dtype))) return TDEQ_EINVAL;
    if (n == 0) return (stage >= 1 && stage <= 4) ? 0 : TDEQ_EINVAL;
    if (const int e = check_terms(ks, stage, 1, 4)) return e;      // stage 1..4 with its k1..k<stage>
    hipStream_t s = static_cast<hipStream_t>(stream);
    return state_dtype(dtype, [&](auto t) {
        return terms<1, 4>(stage, [&](auto st) {
            using T = decltype(t);
            if constexpr (is_lp<T>) return lp_launch_rk4<T, decltype(st)::value>(out, y0, ks, dt, n, s);
            else return launch_rk4<T, decltype(st)::value>(out, y0, ks, dt, n, s, dt_dev);
        });
    });
}

int tdeq_rk4_38_stage(int stage, void* out, const void* y0, const void* k1, const void* k2, const void* k3,
                      const void* k4, double dt, int64_t n, int dtype, void* stream) {
    return rk4_stage_checked(stage, out, y0, {k1, k2, k3, k4}, dt, nullptr, n, dtype, stream);
}

int tdeq_rk4_38_stage_dev(int stage, void* out, const void* y0, const void* k1, const void* k2, const void* k3,
                          const void* k4, const double* dt_dev, int64_t n, int dtype, void* stream) {
    if (!dt_dev) return TDEQ_EINVAL;
    return rk4_stage_checked(stage, out, y0, {k1, k2, k3, k4}, 0.0, dt_dev, n, dtype, stream);
}

int tdeq_grid_advance(const void* grid, int grid_dtype, int64_t n_grid, int64_t* counter, int perturb, double sign,
                      void* times_out, double* dt_out, int state_dtype, void* stream) {
    if (!grid || !counter || !times_out || !dt_out || n_grid < 2 || !real_dtype_ok(grid_dtype) || !real_dtype_ok(state_dtype))
        return TDEQ_EINVAL;
    GridAdvanceArgs a;
    a.grid = grid;
    a.grid_is_f32 = grid_dtype == TDEQ_F32;
    a.n_grid = n_grid;
    a.counter = counter;
    a.perturb = perturb ? 1 : 0;
    a.sign = sign;
    a.times_out = times_out;
    a.state_is_f32 = state_dtype == TDEQ_F32;
    a.dt_out = dt_out;
    hipLaunchKernelGGL(grid_advance_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    return check_launch();
}

int tdeq_grid_advance_stages(const void* grid, int grid_dtype, int64_t n_grid, int64_t* counter, int perturb, double sign,
                             const double* frac, const int* mode, int n_times, void* times_out, double* dt_out,
                             int state_dtype, void* stream) {
    if (!grid || !counter || !times_out || !dt_out || !frac || !mode || n_grid < 2 || !real_dtype_ok(grid_dtype) ||
        !real_dtype_ok(state_dtype) || n_times < 1 || n_times > kMaxGridStages)
        return TDEQ_EINVAL;
    GridStagesArgs a;
    a.base.grid = grid;
    a.base.grid_is_f32 = grid_dtype == TDEQ_F32;
    a.base.n_grid = n_grid;
    a.base.counter = counter;
    a.base.perturb = perturb ? 1 : 0;
    a.base.sign = sign;
    a.base.times_out = times_out;
    a.base.state_is_f32 = state_dtype == TDEQ_F32;
    a.base.dt_out = dt_out;
    a.n_times = n_times;
    for (int i = 0; i < kMaxGridStages; ++i) {
        a.frac[i] = i < n_times ? frac[i] : 0.0;
        a.mode[i] = i < n_times ? mode[i] : 0;
    }
    hipLaunchKernelGGL(grid_advance_stages_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    return check_launch();
}

int tdeq_grid_commit(void* solution, int64_t row_stride, void* y_cur, const void* y_new, const int64_t* counter,
                     int64_t n, int dtype, void* stream) {
    if (!solution || !y_cur || !y_new || !counter || n < 0 || row_stride < n || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype(dtype, [&](auto t) {
        return launch_grid_commit<decltype(t)>(solution, row_stride, y_cur, y_new, counter, n, s);
    });
}

int tdeq_lerp(void* out, const void* y0, const void* y1, double slope, int64_t n, int dtype, void* stream) {
    if (!out || !y0 || !y1 || n < 0 || !state_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return state_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if constexpr (is_lp<T>) return lp_launch_lerp<T>(out, y0, y1, slope, n, s);
        else return launch_lerp<T>(out, y0, y1, slope, n, s);
    });
}

// tdeq_fixed_stage with the step size from the host (dt) or from device memory (dt_dev: fp32 / fp64 only)
static int fixed_stage_checked(int mode, void* out, const void* y0, const void* const* k, const double* w, int n_terms,
                               double dt, const double* dt_dev, int64_t n, int dtype, void* stream) {
    if (!out || !y0 || !k || !w || n < 0 || !(dt_dev ? real_dtype_ok(dtype) : state_dtype_ok(dtype))) return TDEQ_EINVAL;
    if ((mode != 0 && mode != 1) || (mode == 1 && n_terms != 1)) return TDEQ_EINVAL;
    if (const int e = check_terms(k, n_terms, 1, 4)) return e;
    if (n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return state_dtype(dtype, [&](auto t) {
        auto launch = [&](auto nt, auto m) {
            using T = decltype(t);
            constexpr int NT = decltype(nt)::value, MODE = decltype(m)::value;
            if constexpr (is_lp<T>) return lp_launch_fixed<T, NT, MODE>(out, y0, k, w, dt, n, s);
            else return launch_fixed<T, NT, MODE>(out, y0, k, w, dt, n, s, dt_dev);
        };
        if (mode == 1) return launch(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{});
        return terms<1, 4>(n_terms, [&](auto nt) { return launch(nt, std::integral_constant<int, 0>{}); });
    });
}

int tdeq_fixed_stage(int mode, void* out, const void* y0, const void* const* k, const double* w, int n_terms,
                     double dt, int64_t n, int dtype, void* stream) {
    return fixed_stage_checked(mode, out, y0, k, w, n_terms, dt, nullptr, n, dtype, stream);
}

int tdeq_fixed_stage_dev(int mode, void* out, const void* y0, const void* const* k, const double* w, int n_terms,
                         const double* dt_dev, int64_t n, int dtype, void* stream) {
    if (!dt_dev) return TDEQ_EINVAL;
    return fixed_stage_checked(mode, out, y0, k, w, n_terms, 0.0, dt_dev, n, dtype, stream);
}

int tdeq_weighted_sum(void* out, const void* const* x, const double* w, int n_terms, int64_t n, int dtype,
                      void* stream) {
    if (!out || !x || !w || n < 0 || !state_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (const int e = check_terms(x, n_terms, 1, TDEQ_MAX_SUM_TERMS)) return e;
    if (n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return state_dtype_terms<1, TDEQ_MAX_SUM_TERMS>(dtype, n_terms, [&](auto t, auto nt) {
        using T = decltype(t);
        constexpr int NT = decltype(nt)::value;
        if constexpr (is_lp<T>) return lp_launch_weighted<T, NT>(out, x, w, n, s);
        else return launch_fixed<T, NT, 2>(out, nullptr, x, w, 0.0, n, s);
    });
}

int tdeq_scale_many(void* const* outs, const void* g, const double* w, int n_out, int64_t n, int dtype,
                    void* stream) {
    if (!outs || !g || !w || n < 0 || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (const int e = check_terms(outs, n_out, 1)) return e;
    if (n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype_terms<1>(dtype, n_out, [&](auto t, auto nt) {
        return launch_scale<decltype(t), decltype(nt)::value>(outs, g, w, n, s);
    });
}

size_t tdeq_dots_workspace_bytes(int64_t n, int n_x) {
    int64_t n_chunks = (n + kDotChunk - 1) / kDotChunk;
    if (n_chunks < 1) n_chunks = 1;
    if (n_x < 1) n_x = 1;
    return (size_t)n_chunks * (size_t)n_x * sizeof(double);
}

int tdeq_multi_dot(const void* g, const void* const* x, int n_x, int64_t n, double* out, void* workspace,
                   size_t workspace_bytes, int dtype, void* stream) {
    if (!g || !x || !out || !workspace || n < 0 || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (const int e = check_terms(x, n_x, 1)) return e;
    if (workspace_bytes < tdeq_dots_workspace_bytes(n, n_x)) return TDEQ_EWORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* ws = static_cast<double*>(workspace);
    return real_dtype_terms<1>(dtype, n_x, [&](auto t, auto nt) {
        return launch_dots<decltype(t), decltype(nt)::value>(g, x, n, out, ws, s);
    });
}

int tdeq_pack_segments(void* out, const void* const* src, const int64_t* chunk_start, const int64_t* numel,
                       const double* scale, int n_seg, int64_t chunk, int64_t n_chunks, int dtype, void* stream) {
    if (!out || !src || !chunk_start || !numel || !scale || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if (n_seg < 1 || n_seg > TDEQ_INLINE_SEGMENTS) return TDEQ_EINVAL;
    if (chunk < TDEQ_CHUNK_QUANTUM || chunk % TDEQ_CHUNK_QUANTUM != 0 || n_chunks < 1 || n_chunks > 0x7fffffffLL)
        return TDEQ_EINVAL;
    if (chunk_start[0] != 0) return TDEQ_EINVAL;
    for (int q = 0; q < n_seg; ++q) {
        if (numel[q] < 0 || (q > 0 && chunk_start[q] <= chunk_start[q - 1]) || chunk_start[q] >= n_chunks) return TDEQ_EINVAL;
        const int64_t end = (q + 1 < n_seg) ? chunk_start[q + 1] : n_chunks;
        if (q + 1 < n_seg && chunk_start[q + 1] <= chunk_start[q]) return TDEQ_EINVAL;
        if (numel[q] > (end - chunk_start[q]) * chunk) return TDEQ_EINVAL;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype(dtype, [&](auto t) {
        return launch_pack<decltype(t)>(out, src, chunk_start, numel, scale, n_seg, chunk, n_chunks, s);
    });
}

int tdeq_fill_scalars(void* dst, const double* vals, int n_vals, int dtype, void* stream) {
    if (!dst || !vals || n_vals < 1 || n_vals > 16 || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    FillArgs a;
    a.dst = dst;
    for (int i = 0; i < 16; ++i) a.v[i] = i < n_vals ? vals[i] : 0.0;
    a.n = n_vals;
    a.dtype = dtype;
    hipLaunchKernelGGL(fill_scalars_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    return check_launch();
}

int tdeq_adams_predict(void* y_out, void* dy_out, void* delta_out, const void* y0, const void* const* f_hist,
                       const double* cb, const double* cm, int n_terms, double dt, int64_t n, int dtype,
                       void* stream) {
    if (!y_out || !y0 || !f_hist || !cb || n < 0 || !real_dtype_ok(dtype)) return TDEQ_EINVAL;
    if ((dy_out == nullptr) != (delta_out == nullptr)) return TDEQ_EINVAL;
    if (dy_out && !cm) return TDEQ_EINVAL;
    if (const int e = check_terms(f_hist, n_terms, 1)) return e;
    if (n == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return real_dtype_terms<1>(dtype, n_terms, [&](auto t, auto nt) {
        return launch_adams_predict<decltype(t), decltype(nt)::value>(y_out, dy_out, delta_out, y0, f_hist, cb, cm, dt, n, s);
    });
}

int tdeq_adams_correct(void* y_out, void* dy_out, const void* f, const void* delta, const void* dy_old,
                       const void* y0, double c, int compute, const tdeq_segment* segs, const void* segs_dev,
                       int n_seg, int64_t chunk, int64_t n_chunks, int64_t n, double* out_count,
                       double* out_nonfinite, void* workspace, size_t workspace_bytes, int dtype, void* stream) {
    if (!dy_out || !dy_old || !out_count || !out_nonfinite || !workspace || n < 0 || !real_dtype_ok(dtype))
        return TDEQ_EINVAL;
    if (compute && (!y_out || !f || !delta || !y0)) return TDEQ_EINVAL;
    NormSetup ns;
    if (const int e = norm_setup(ns, segs, segs_dev, n_seg, chunk, n_chunks, workspace, workspace_bytes, stream)) return e;
    return real_dtype(dtype, [&](auto t) {
        return launch_adams_correct<decltype(t)>(y_out, dy_out, f, delta, dy_old, y0, c, compute != 0, ns, n, out_count,
                                                 out_nonfinite);
    });
}

}  // extern "C"

#include "tdeq_abi_rowwise.hpp"
