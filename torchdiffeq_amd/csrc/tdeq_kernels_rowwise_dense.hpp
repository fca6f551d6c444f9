// tdeq_kernels_rowwise_dense.hpp — gfx950 device code of `odeint_rowwise_dense` (torchdiffeq_amd/rowwise_dense.py): the
// piecewise quartic of a whole rowwise solve, one segment per accepted step of each row.
//
// Rows accept very different numbers of steps, so the quartics are kept ragged: during the solve every accepted step takes
// a slot of the current CHUNK ([5, cap, L] coefficients plus per-slot metadata), after it the chunks are packed into
// [5, n_seg, L] with row r's segments contiguous and in step order.  A trial step of a dense solve is the trial step of
// `odeint_rowwise` plus two launches between the controller and the dense-output commit:
//   row_dense_slots    one lane per carried row: every accepted row takes a unique slot of the chunk (a ballot prefix inside
//                      the wave, one atomicAdd per wave on the chunk's counter) and writes the slot's metadata
//   row_event_fit_mapped   (tdeq_kernels_rowwise_event.hpp) with q = the chunk, row_map = the slots, fired_now = the slot mask
// after the solve, per chunk:
//   row_dense_pack     dst[p, dest[s], :] = src[p, s, :] for the used slots s and the 5 planes: a copy of bits
// and per evaluation of the dense object:
//   row_dense_search   one lane per query: the segment of the row that holds the query time (bisection over the row's
//                      segment ends) and the fraction x of that step, in the arithmetic of row_dense_commit
// followed by row_event_eval_mapped on (coeffs, seg, x).  No LDS; plain vector loads and stores; 64-bit element offsets.
// The derivative, antiderivative and integral of the record (row_dense_prefix, row_dense_calc) follow, and at the end of the
// file the queries over a time window: one walk over the window's segments (row_dense_walk) and one level machine on it
// (row_dense_level_walk) carry the extrema (row_dense_extremum), the crossings of a level (row_dense_level), the area above
// and below a level (row_dense_exposure) and the times of all crossings of a level (row_dense_level_times).
#pragma once

#include "tdeq_kernels_rowwise.hpp"

namespace tdeq {

struct RowDenseSlotsArgs {
    const int32_t* accepted;          // [n_rows] the controller accepted this trial step
    const double* tprev;              // [n_rows] start of the accepted step (solver time)
    const double* t0;                 // [n_rows] its end
    const int64_t* n_acc;             // [n_rows] accepted steps so far, this one counted
    const int32_t* row_map;           // [n_rows] original row of each carried row, or NULL: identity
    int64_t n_rows;
    int32_t cap;                      // slots of the chunk
    int32_t* counter;                 // [2] = {slots taken (may run past cap), a row found no slot}
    int32_t* slot_row;                // [cap] original row
    int32_t* slot_ord;                // [cap] index of the step within its row
    double* slot_ta;                  // [cap]
    double* slot_tb;                  // [cap]
    int32_t* slot;                    // [n_rows] the row's slot, -1 without one
    int32_t* mask;                    // [n_rows] the row has a slot
};

__global__ __launch_bounds__(kBlock) void row_dense_slots_kernel(const RowDenseSlotsArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool want = r < a.n_rows && a.accepted[r] != 0;
    const uint64_t m = __ballot(want ? 1 : 0);
    int32_t base = 0;
    if (lane == 0 && m) base = atomicAdd(a.counter, (int32_t)__popcll(m));      // one atomic per wave
    base = __shfl(base, 0, kWave);
    if (r >= a.n_rows) return;
    // (64-bit: the counter keeps counting after an overflow, base + rank is compared before it is narrowed)
    const int64_t s = (int64_t)base + (int64_t)__popcll(m & (((uint64_t)1 << lane) - 1));
    const bool placed = want && s < (int64_t)a.cap;
    if (placed) {
        a.slot_row[s] = a.row_map ? a.row_map[r] : (int32_t)r;
        a.slot_ord[s] = (int32_t)(a.n_acc[r] - 1);
        a.slot_ta[s] = a.tprev[r];
        a.slot_tb[s] = a.t0[r];
    } else if (want) {
        // the chunk is full: nothing written at or beyond cap.  Several lanes and waves may store here at once, next to
        // the atomicAdds of other waves on counter[0]: every store writes the same value to a word no atomic touches
        a.counter[1] = 1;
    }
    a.slot[r] = placed ? (int32_t)s : -1;
    a.mask[r] = placed ? 1 : 0;
}

struct RowDensePackArgs {
    void* dst;                        // [5, dst_rows, L]
    const void* src;                  // [5, src_rows, L]
    const int64_t* dest;              // [n_used] row of dst of each used slot
    int64_t row_len;                  // E units
    int64_t ne;                       // n_used * row_len
    int64_t dst_plane;                // dst_rows * row_len, E units
    int64_t src_plane;                // src_rows * row_len
};

template <typename E>
__global__ __launch_bounds__(kBlock) void row_dense_pack_kernel(const RowDensePackArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.ne; i += stride) {
        const int64_t s = i / a.row_len;
        const int64_t to = a.dest[s] * a.row_len + (i - s * a.row_len);
#pragma unroll
        for (int p = 0; p < 5; ++p)
            static_cast<E*>(a.dst)[p * a.dst_plane + to] = static_cast<const E*>(a.src)[p * a.src_plane + i];
    }
}

struct RowDenseSearchArgs {
    const double* tq;                 // [n_q, n_rows] query times (solver time)
    const int64_t* offsets;           // [n_rows + 1] row r's segments are offsets[r] .. offsets[r + 1] - 1
    const double* seg_ta;             // [n_seg] start of each segment (solver time)
    const double* seg_tb;             // [n_seg] its end, ascending inside a row
    const double* t0;                 // [n_rows] the row's interval [t0, t1] in solver time
    const double* t1;
    int64_t n_rows;
    int64_t n_seg;                    // >= 1
    int64_t n;                        // n_q * n_rows queries
    int32_t* seg;                     // [n]
    void* x;                          // [n] of T
    int32_t* status;                  // [1] lowered to the smallest out-of-range query index
};

template <typename T>
__global__ __launch_bounds__(kBlock) void row_dense_search_kernel(const RowDenseSearchArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool bad = false;
    if (i < a.n) {
        const int64_t r = i % a.n_rows;
        const double tq = a.tq[i];
        const int64_t first = a.offsets[r], end = a.offsets[r + 1];
        int64_t s = first;
        T x = (T)__builtin_nan("");
        if (tq >= a.t0[r] && tq <= a.t1[r] && end > first) {          // (a NaN fails both comparisons)
            int64_t lo = first, hi = end - 1;                         // the first s with tq <= seg_tb[s]; the last segment
            while (lo < hi) {                                         // ends at or beyond t1, so it is the answer if none
                const int64_t mid = lo + ((hi - lo) >> 1);            // before it is
                if (tq <= a.seg_tb[mid]) hi = mid;
                else lo = mid + 1;
            }
            s = lo;
            const double ta = a.seg_ta[s], tb = a.seg_tb[s];
            x = (T)((tq - ta) / (tb - ta));                           // interp.py:39-40 in fp64, then T, as row_dense_commit
        } else {
            bad = true;
        }
        a.seg[i] = (int32_t)(s < a.n_seg ? s : a.n_seg - 1);          // (an empty last row: still a segment that exists)
        static_cast<T*>(a.x)[i] = x;
    }
    // the wave's smallest offending index is that of its lowest lane: one atomic per wave that has one
    const uint64_t m = __ballot(bad ? 1 : 0);
    if (m && lane == __ffsll((unsigned long long)m) - 1) atomicMin(a.status, (int32_t)i);
}

// ---- calculus on the record (ABI 31): derivative, antiderivative and integral of the piecewise quartic -----------------
//   row_dense_prefix   one lane per (row, element): walks the row's segments in step order and writes the EXCLUSIVE prefix
//                      of the whole-segment integrals, P[s] = sum of I over the row's segments before s, added left to
//                      right in fp64 (that order is the contract: a row's bits depend neither on B nor on the backend)
//   row_dense_calc     the shape of row_event_eval_mapped with three modes: the derivative in T, the antiderivative
//                      T(sign * (P[s] + J_s(x64))) in fp64, and the integral T(F64(b) - F64(a)) of two query lists
// No LDS, no atomics; 64-bit element offsets.  Nothing is contracted (the library is built with -ffp-contract=off).

// J_s(x) of a segment with coefficients e, d, c, b, a (as doubles), fp64 throughout; I_s = J_s(1.0), the same expression
__device__ __forceinline__ double quartic_integral_one(double e, double d, double c, double b, double a, double x, double h) {
    return (((((a * 0.2) * x + b * 0.25) * x + c * (1.0 / 3.0)) * x + d * 0.5) * x + e) * x * h;
}

// LV consecutive elements of T, moved as one E (E = T: LV = 1)
template <typename T, typename E, int LV>
__device__ __forceinline__ void load_lanes(const T* base, int64_t at, T (&v)[LV]) {
    const E w = reinterpret_cast<const E*>(base)[at];
    __builtin_memcpy(v, &w, sizeof(E));
}

// the five planes e, d, c, b, a of a record `q` at element offset `at`
template <typename T, typename E, int LV>
__device__ __forceinline__ void load_planes(const T* q, int64_t q_plane, int64_t at, T (&qe)[LV], T (&qd)[LV], T (&qc)[LV],
                                            T (&qb)[LV], T (&qa)[LV]) {
    load_lanes<T, E, LV>(q, at, qe);
    load_lanes<T, E, LV>(q + q_plane, at, qd);
    load_lanes<T, E, LV>(q + 2 * q_plane, at, qc);
    load_lanes<T, E, LV>(q + 3 * q_plane, at, qb);
    load_lanes<T, E, LV>(q + 4 * q_plane, at, qa);
}

template <int LV>
__device__ __forceinline__ void store_doubles(double* p, const double (&v)[LV]) {
    if constexpr (LV == 1) {
        p[0] = v[0];
    } else {
#pragma unroll
        for (int c = 0; c < LV; c += 2) {
            f64x2 w;
            w[0] = v[c];
            w[1] = v[c + 1];
            reinterpret_cast<f64x2*>(p)[c / 2] = w;
        }
    }
}

template <int LV>
__device__ __forceinline__ void load_doubles(const double* p, double (&v)[LV]) {
    if constexpr (LV == 1) {
        v[0] = p[0];
    } else {
#pragma unroll
        for (int c = 0; c < LV; c += 2) {
            const f64x2 w = reinterpret_cast<const f64x2*>(p)[c / 2];
            v[c] = w[0];
            v[c + 1] = w[1];
        }
    }
}

template <typename T>
struct RowDensePrefixArgs {
    double* prefix;                   // [n_seg, L]
    const T* q;                       // [5, n_seg, L] planes e, d, c, b, a
    const int64_t* offsets;           // [n_rows + 1]
    const double* seg_ta;             // [n_seg]
    const double* seg_tb;             // [n_seg]
    int64_t n_seg;
    int64_t row_len;                  // E units
    int64_t ne;                       // n_rows * row_len
    int64_t q_plane;                  // n_seg * L elements of T
};

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void row_dense_prefix_kernel(const RowDensePrefixArgs<T> a) {
    using E = typename std::conditional<VEC, typename VecOf<T>::type, T>::type;
    constexpr int LV = VEC ? VecOf<T>::L : 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.ne; i += stride) {
        const int64_t r = i / a.row_len;
        const int64_t el = i - r * a.row_len;
        int64_t s = a.offsets[r], end = a.offsets[r + 1];
        if (s < 0) s = 0;                                             // (nothing is read or written outside the record)
        if (end > a.n_seg) end = a.n_seg;
        double acc[LV];
#pragma unroll
        for (int c = 0; c < LV; ++c) acc[c] = 0.0;
        for (; s < end; ++s) {                                        // serial by construction: the order is the contract
            const int64_t at = s * a.row_len + el;
            T qe[LV], qd[LV], qc[LV], qb[LV], qa[LV];
            load_planes<T, E, LV>(a.q, a.q_plane, at, qe, qd, qc, qb, qa);
            const double h = a.seg_tb[s] - a.seg_ta[s];
            store_doubles<LV>(a.prefix + at * LV, acc);
#pragma unroll
            for (int c = 0; c < LV; ++c)
                acc[c] = acc[c] + quartic_integral_one((double)qe[c], (double)qd[c], (double)qc[c], (double)qb[c],
                                                       (double)qa[c], 1.0, h);
        }
    }
}

// modes of row_dense_calc (== TDEQ_DENSE_DERIVATIVE / _ANTIDERIVATIVE / _INTEGRAL of include/tdeq_hip.h)
constexpr int kDenseDerivative = 0;
constexpr int kDenseAntiderivative = 1;
constexpr int kDenseIntegral = 2;

template <typename T>
struct RowDenseCalcArgs {
    T* out;                           // [n_idx, L]
    const T* q;                       // [5, n_seg, L]
    const double* seg_ta;             // [n_seg]
    const double* seg_tb;             // [n_seg]
    const double* prefix;             // [n_seg, L] (not read by the derivative)
    double sign;                      // +1 ascending, -1 descending solve
    const int32_t* seg;               // [n_idx] segment of each query (row_dense_search)
    const T* x;                       // [n_idx] its fraction in T; NaN marks an out-of-range query
    const double* tq;                 // [n_idx] the query in solver time (not read by the derivative)
    const int32_t* seg2;              // the integral's upper ends; not read otherwise
    const T* x2;
    const double* tq2;
    int64_t row_len;                  // E units
    int64_t ne;                       // n_idx * row_len
    int64_t q_plane;                  // n_seg * L elements of T
};

// sign * (P[s] + J_s(x64)) of LV elements, x64 = (tq - ta) / (tb - ta) in fp64 and NOT rounded to T
template <typename T, typename E, int LV>
__device__ __forceinline__ void row_dense_antiderivative_one(const RowDenseCalcArgs<T>& a, int64_t s, int64_t el, T xT,
                                                             double tq, double (&f)[LV]) {
    const double ta = a.seg_ta[s], tb = a.seg_tb[s];
    const double h = tb - ta;
    const double x64 = xT != xT ? __builtin_nan("") : (tq - ta) / h;
    const int64_t at = s * a.row_len + el;
    T qe[LV], qd[LV], qc[LV], qb[LV], qa[LV];
    load_planes<T, E, LV>(a.q, a.q_plane, at, qe, qd, qc, qb, qa);
    double p[LV];
    load_doubles<LV>(a.prefix + at * LV, p);
#pragma unroll
    for (int c = 0; c < LV; ++c)
        f[c] = a.sign * (p[c] + quartic_integral_one((double)qe[c], (double)qd[c], (double)qc[c], (double)qb[c],
                                                     (double)qa[c], x64, h));
}

template <typename T, bool VEC, int MODE>
__global__ __launch_bounds__(kBlock) void row_dense_calc_kernel(const RowDenseCalcArgs<T> a) {
    using E = typename std::conditional<VEC, typename VecOf<T>::type, T>::type;
    constexpr int LV = VEC ? VecOf<T>::L : 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.ne; i += stride) {
        const int64_t r = i / a.row_len;
        const int64_t el = i - r * a.row_len;
        const int64_t s = a.seg[r];
        if constexpr (MODE == kDenseDerivative) {
            const int64_t from = s * a.row_len + el;
            const E d = reinterpret_cast<const E*>(a.q + a.q_plane)[from];
            const E c = reinterpret_cast<const E*>(a.q + 2 * a.q_plane)[from];
            const E b = reinterpret_cast<const E*>(a.q + 3 * a.q_plane)[from];
            const E qa = reinterpret_cast<const E*>(a.q + 4 * a.q_plane)[from];
            const T x = a.x[r];
            const T w = (T)(a.sign * (a.seg_tb[s] - a.seg_ta[s]));
            E tot = d + (c + c) * x;
            T xp = x * x;
            tot = tot + (b * (T)3) * xp;
            xp = xp * x;
            tot = tot + (qa * (T)4) * xp;
            reinterpret_cast<E*>(a.out)[i] = tot / w;
        } else {
            double f[LV];
            row_dense_antiderivative_one<T, E, LV>(a, s, el, a.x[r], a.tq[r], f);
            T o[LV];
            if constexpr (MODE == kDenseIntegral) {
                double g[LV];
                row_dense_antiderivative_one<T, E, LV>(a, a.seg2[r], el, a.x2[r], a.tq2[r], g);
#pragma unroll
                for (int c = 0; c < LV; ++c) o[c] = (T)(g[c] - f[c]);
            } else {
#pragma unroll
                for (int c = 0; c < LV; ++c) o[c] = (T)f[c];
            }
            E w;
            __builtin_memcpy(&w, o, sizeof(E));
            reinterpret_cast<E*>(a.out)[i] = w;
        }
    }
}

// ---- queries over a time window (ABI 32 to 35): extrema, level crossings, exposure, crossing times -----------------------
// Four kernels in the shape of row_dense_calc, one lane per (query, 16-byte element), on ONE walk and ONE level machine:
//   row_dense_walk         the window's prologue (both ends, in solver-time order, clamped to the record), the serial loop over
//                          its segments segA .. segB, the five planes of each, and per element a WindowQuartic: the
//                          coefficients as doubles, y' and y'', the segment clipped to the window, the candidates of the
//                          isolation in increasing x and the time of a candidate
//   row_dense_level_walk   the walk with a state machine over the candidates of phi = y - level: between two neighbouring
//                          candidates the quartic is monotone, so phi has at most one root there, found by one more bisection.
//                          It keeps above / nan per element and tells its caller of the window's opening, of every crossing
//                          (tz, above after it) and, for the exposure alone, of every piece K(v) - K(u)
// and what each kernel keeps:
//   row_dense_extremum     (RowDenseOutput.maximum / .minimum) the best candidate value and its time
//   row_dense_level        (.crossings / .time_above) count / first / last and the time above
//   row_dense_exposure     (.exposure / .area_above / .area_below) the time above and the two areas: K is J_s of
//                          row_dense_prefix with e - level in place of e; a piece adds to the area above or takes from the
//                          area below by the state, and a crossing at z splits its piece there
//   row_dense_level_times  (.crossing_times) one int32 counter per direction; a crossing located at tz goes straight to global
//                          memory: slot n of its direction's list while n < K, as one 8-byte store; the counter runs on.
//                          Rising is defined in true time: the state becomes above and time_sign > 0, or it becomes not above
//                          and time_sign < 0; the launcher hands the two directions over as `ups` and `dns` accordingly.  After
//                          the walk the free slots are filled with NaN, so every slot of the four outputs is written.  The list
//                          index is an offset in global memory, never an index into a per-lane array
// The arithmetic — fp64, + - * /, comparisons and fabs only — is stated in include/tdeq_hip.h and is the contract; the host
// model (rowwise.py: _window_walk, _level_walk and quartic_extrema / _levels / _exposure / _crossing_times) has its bits.
// On a segment where the element is monotone the lane evaluates g1 twice (three times with x1 inside), g twice and p twice
// and takes no loop; the level machine adds at most 7 evaluations of phi, the exposure as many of K.  A bisection is at most 64
// dependent rounds of one Horner form (4 to 6 fp64 operations and a compare); lanes of a wave that need none wait for those
// that do.  Per-lane state is named scalars and arrays indexed by the unrolled element only.  No LDS, no atomics, no workspace.

// modes of row_dense_extremum (== TDEQ_DENSE_MAXIMUM / _MINIMUM)
constexpr int kDenseMaximum = 0;
constexpr int kDenseMinimum = 1;

// what the four kernels share: the record and the two query lists of row_dense_search
template <typename T>
struct RowDenseWindowArgs {
    const T* q;                       // [5, n_seg, L]
    const double* seg_ta;             // [n_seg]
    const double* seg_tb;             // [n_seg]
    double sign;                      // (the exposure keeps durations only and does not read it)
    const int32_t* seg;               // [n_idx] one end of each window
    const T* x;                       // [n_idx] NaN marks an out-of-range end
    const double* tq;                 // [n_idx] solver time
    const int32_t* seg2;              // the other end
    const T* x2;
    const double* tq2;
    int64_t n_rows;                   // query i belongs to row i % n_rows (read with a level only)
    int64_t n_seg;
    int64_t row_len;                  // E units
    int64_t ne;                       // n_idx * row_len
    int64_t q_plane;                  // n_seg * L elements of T
};

// c0 + x*(c1 + x*(c2 + x*c3)): g with (d, c+c, 3b, 4a); g1 with (c+c, 6b, 12a, 0) skips the last term
struct QuarticSlope {
    double c0, c1, c2, c3;
    __device__ __forceinline__ double operator()(double x) const { return c0 + x * (c1 + x * (c2 + x * c3)); }
};
struct QuarticCurvature {
    double c0, c1, c2;
    __device__ __forceinline__ double operator()(double x) const { return c0 + x * (c1 + x * c2); }
};

// bisect(phi, lo, hi) of the header -> a root was found (in `root`)
template <typename F>
__device__ __forceinline__ bool quartic_bisect(const F& phi, double lo, double hi, double& root) {
    double flo = phi(lo), fhi = phi(hi);
    const bool nlo = flo < 0.0;
    if (flo == 0.0 || fhi == 0.0 || nlo == (fhi < 0.0)) return false;
    for (int k = 0; k < 64; ++k) {
        const double mid = 0.5 * (lo + hi);
        if (mid == lo || mid == hi) break;
        const double fm = phi(mid);
        if (fm == 0.0) {
            root = mid;
            return true;
        }
        if ((fm < 0.0) == nlo) {
            lo = mid;
            flo = fm;
        } else {
            hi = mid;
            fhi = fm;
        }
    }
    root = __builtin_fabs(flo) <= __builtin_fabs(fhi) ? lo : hi;
    return true;
}

// the candidates of one element on one segment (Isolation of the header), visited in increasing x; repeats are not skipped
template <typename V>
__device__ __forceinline__ void quartic_candidates(const QuarticSlope& g, const QuarticCurvature& g1, double b, double aa,
                                                   double a4, double xlo, double xhi, V&& visit) {
    // the roots of g1 bound the pieces of g; a piece without a root passes its lower bound on
    double xm = xlo;
    if (aa != 0.0) {
        const double x1 = (-b) / a4;
        if (xlo < x1 && x1 < xhi) xm = x1;
    }
    double r0 = xlo, r1, z;
    if (xm > xlo) quartic_bisect(g1, xlo, xm, r0);
    r1 = r0;
    quartic_bisect(g1, xm, xhi, r1);
    visit(xlo);
    if (r0 > xlo) {
        if (quartic_bisect(g, xlo, r0, z)) visit(z);
        visit(r0);
    }
    if (r1 > r0) {
        if (quartic_bisect(g, r0, r1, z)) visit(z);
        visit(r1);
    }
    if (quartic_bisect(g, r1, xhi, z)) visit(z);
    visit(xhi);
}

// one element on one segment of its window, as the walk hands it over; operator() is p of the header
struct WindowQuartic {
    double e, d, c, b, a;             // the element's coefficients
    QuarticSlope g;                   // y'
    QuarticCurvature g1;              // y''
    double ta, tb, h;                 // the segment
    double tqa, tqb;                  // the window's ends, tqa <= tqb
    bool atA, atB;                    // this is the window's first / last segment
    double xlo, xhi;                  // the segment clipped to the window
    __device__ __forceinline__ double operator()(double x) const { return e + x * (d + x * (c + x * (b + x * a))); }
    template <typename V>
    __device__ __forceinline__ void candidates(V&& visit) const {
        quartic_candidates(g, g1, b, a, g.c3, xlo, xhi, visit);
    }
    // the time of a candidate: a window's end and a breakpoint are the stored words, not ta + x * h
    __device__ __forceinline__ double time_of(double z) const {
        return (atA && z == xlo) ? tqa : (atB && z == xhi) ? tqb : z == 0.0 ? ta : z == 1.0 ? tb : ta + z * h;
    }
};

struct RowDenseWindow {
    double tqb;                       // the window's later end
    bool bad;                         // an end is out of range: no segment was walked
};

// The walk of window r for the LV elements at `el`: each(c, WindowQuartic) for every segment in order and, inside it, every
// element c.  Serial by construction.
template <typename T, typename E, int LV, typename F>
__device__ __forceinline__ RowDenseWindow row_dense_walk(const RowDenseWindowArgs<T>& a, int64_t r, int64_t el, F&& each) {
    int64_t sA = a.seg[r], sB = a.seg2[r];
    double tqa = a.tq[r], tqb = a.tq2[r];
    const T xa = a.x[r], xb = a.x2[r];
    if (tqb < tqa) {
        const int64_t s = sA;
        sA = sB;
        sB = s;
        const double t = tqa;
        tqa = tqb;
        tqb = t;
    }
    if (sA < 0) sA = 0;                                               // (nothing is read outside the record)
    if (sB > a.n_seg - 1) sB = a.n_seg - 1;
    const bool bad = xa != xa || xb != xb || sA > sB;                 // (sA > sB: only from ends the search did not write)
    for (int64_t s = bad ? sB + 1 : sA; s <= sB; ++s) {               // serial: segments in order
        T qe[LV], qd[LV], qc[LV], qb[LV], qa[LV];
        load_planes<T, E, LV>(a.q, a.q_plane, s * a.row_len + el, qe, qd, qc, qb, qa);
        const double ta = a.seg_ta[s], tb = a.seg_tb[s];
        const double h = tb - ta;
        const bool atA = s == sA, atB = s == sB;
        const double xlo = atA ? (tqa - ta) / h : 0.0;
        const double xhi = atB ? (tqb - ta) / h : 1.0;
#pragma unroll
        for (int c = 0; c < LV; ++c) {
            const double e = (double)qe[c], d = (double)qd[c], cc = (double)qc[c], b = (double)qb[c], aa = (double)qa[c];
            const double c2 = cc + cc, a4 = 4.0 * aa;
            each(c, WindowQuartic{e, d, cc, b, aa, {d, c2, 3.0 * b, a4}, {c2, 6.0 * b, 12.0 * aa}, ta, tb, h, tqa, tqb, atA, atB,
                                  xlo, xhi});
        }
    }
    return {tqb, bad};
}

template <int LV>
struct RowDenseLevelWalk {
    double tqb;                       // the window's later end
    bool above[LV];                   // the state at the window's end
    bool nan[LV];                     // the element's answer is NaN: a bad window, or phi was NaN at a candidate
};

struct NoPieces {
    __device__ __forceinline__ void operator()(int, double, bool) const {}
};

// The level machine on the walk, for `level` [n_rows, L].  Its caller hears open(c, tqa) at the window's first candidate,
// cross(c, tz, ab) at every crossing (tz in solver time; ab: above after it) and, with AREA, piece(c, q, over) for every
// piece between two candidates of a segment, split at a crossing: q = K(v) - K(u), over: the state on it.  K is evaluated
// with AREA only.
template <typename T, typename E, int LV, bool AREA, typename Open, typename Cross, typename Piece>
__device__ __forceinline__ RowDenseLevelWalk<LV> row_dense_level_walk(const RowDenseWindowArgs<T>& a, const T* level, int64_t r,
                                                                      int64_t el, Open&& open, Cross&& cross, Piece&& piece) {
    T lev[LV];
    load_lanes<T, E, LV>(level, (r % a.n_rows) * a.row_len + el, lev);
    RowDenseLevelWalk<LV> m;
#pragma unroll
    for (int c = 0; c < LV; ++c) m.above[c] = m.nan[c] = false;
    const RowDenseWindow w = row_dense_walk<T, E, LV>(a, r, el, [&](int c, const WindowQuartic& s) {
        const double lv = (double)lev[c], el0 = s.e - lv;
        auto phi = [&](double x) { return s(x) - lv; };               // phi of the header: p, then one subtraction
        auto K = [&](double x) { return quartic_integral_one(el0, s.d, s.c, s.b, s.a, x, s.h); };
        bool st = m.above[c], entry = true;                           // entry: the segment's first candidate comes next
        double u = s.xlo, fu = 0.0, ku = 0.0;
        s.candidates([&](double x) {
            const double v = phi(x);
            if (v != v) m.nan[c] = true;
            const bool ab = v > 0.0;
            double kx = 0.0;
            if constexpr (AREA) kx = K(x);
            if (entry && s.atA) {                                     // the window's first candidate sets the state
                st = ab;
                open(c, s.tqa);
            } else {
                double kz = ku;                                       // (no crossing: one piece, K(x) - K(u))
                if (ab != st) {
                    double z = x;                                     // (a later segment's first candidate: the breakpoint)
                    if (!entry) {
                        if (fu == 0.0) z = u;
                        else if (v != 0.0) quartic_bisect(phi, u, x, z);
                        if constexpr (AREA) {
                            kz = K(z);
                            piece(c, kz - ku, st);
                        }
                    }
                    cross(c, s.time_of(z), ab);
                    st = ab;
                }
                if constexpr (AREA) {
                    if (!entry) piece(c, kx - kz, st);
                }
            }
            entry = false;
            u = x;
            fu = v;
            ku = kx;
        });
        m.above[c] = st;
    });
    m.tqb = w.tqb;
#pragma unroll
    for (int c = 0; c < LV; ++c) m.nan[c] = m.nan[c] || w.bad;
    return m;
}

// the time above the level, as row_dense_level and row_dense_exposure keep it: the start of the current stay and the sum of
// the finished ones, left to right
struct TimeAbove {
    double up = 0.0, sum = 0.0;
    __device__ __forceinline__ void open(double tqa) { up = tqa; }
    __device__ __forceinline__ void cross(double tz, bool ab) {
        if (ab) up = tz;
        else sum = sum + (tz - up);
    }
    __device__ __forceinline__ double close(bool above, double tqb) const { return above ? sum + (tqb - up) : sum; }
};

template <int LV>
__device__ __forceinline__ void store_ints(int32_t* p, const int32_t (&v)[LV]) {
    if constexpr (LV == 1) {
        p[0] = v[0];
    } else {
        typedef int32_t W __attribute__((ext_vector_type(LV)));
        W w;
#pragma unroll
        for (int c = 0; c < LV; ++c) w[c] = v[c];
        *reinterpret_cast<W*>(p) = w;
    }
}

template <typename T, typename E, int LV>
__device__ __forceinline__ void store_lanes(T* base, int64_t at, const T (&v)[LV]) {
    E w;
    __builtin_memcpy(&w, v, sizeof(E));
    reinterpret_cast<E*>(base)[at] = w;
}

template <typename T>
struct RowDenseExtremumArgs : RowDenseWindowArgs<T> {
    T* values;                        // [n_idx, L]
    double* times;                    // [n_idx, L] true time
};

template <typename T, bool VEC, bool MAX>
__global__ __launch_bounds__(kBlock) void row_dense_extremum_kernel(const RowDenseExtremumArgs<T> a) {
    using E = typename std::conditional<VEC, typename VecOf<T>::type, T>::type;
    constexpr int LV = VEC ? VecOf<T>::L : 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.ne; i += stride) {
        const int64_t r = i / a.row_len;
        double best[LV], when[LV];
        bool nanv[LV];
#pragma unroll
        for (int c = 0; c < LV; ++c) {
            best[c] = when[c] = 0.0;
            nanv[c] = false;
        }
        const RowDenseWindow w = row_dense_walk<T, E, LV>(a, r, i - r * a.row_len, [&](int c, const WindowQuartic& s) {
            double bst = best[c], whn = when[c];
            bool have = !s.atA;                                       // (the window's first candidate is taken as it is)
            s.candidates([&](double x) {
                const double v = s(x);
                if (v != v) nanv[c] = true;
                if (!have || (MAX ? v > bst : v < bst)) {
                    have = true;
                    bst = v;
                    whn = s.time_of(x);
                }
            });
            best[c] = bst;
            when[c] = whn;
        });
        T o[LV];
#pragma unroll
        for (int c = 0; c < LV; ++c) {
            const bool nan = w.bad || nanv[c];
            o[c] = nan ? (T)__builtin_nan("") : (T)best[c];
            when[c] = nan ? __builtin_nan("") : a.sign * when[c];
        }
        store_lanes<T, E, LV>(a.values, i, o);
        store_doubles<LV>(a.times + i * LV, when);
    }
}

template <typename T>
struct RowDenseLevelArgs : RowDenseWindowArgs<T> {
    int32_t* count;                   // [n_idx, L]
    double* first;                    // [n_idx, L] true time
    double* last;                     // [n_idx, L] true time
    double* total;                    // [n_idx, L] duration
    const T* level;                   // [n_rows, L]
};

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void row_dense_level_kernel(const RowDenseLevelArgs<T> a) {
    using E = typename std::conditional<VEC, typename VecOf<T>::type, T>::type;
    constexpr int LV = VEC ? VecOf<T>::L : 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.ne; i += stride) {
        const int64_t r = i / a.row_len;
        TimeAbove dur[LV];
        double tfirst[LV], tlast[LV], total[LV];
        int32_t count[LV];
#pragma unroll
        for (int c = 0; c < LV; ++c) {
            tfirst[c] = tlast[c] = 0.0;
            count[c] = 0;
        }
        const RowDenseLevelWalk<LV> m = row_dense_level_walk<T, E, LV, false>(
            a, a.level, r, i - r * a.row_len, [&](int c, double tqa) { dur[c].open(tqa); },
            [&](int c, double tz, bool ab) {
                if (count[c] == 0) tfirst[c] = tz;
                tlast[c] = tz;
                ++count[c];
                dur[c].cross(tz, ab);
            },
            NoPieces{});
#pragma unroll
        for (int c = 0; c < LV; ++c) {
            total[c] = dur[c].close(m.above[c], m.tqb);
            const bool none = count[c] == 0;
            tfirst[c] = (m.nan[c] || none) ? __builtin_nan("") : a.sign * tfirst[c];
            tlast[c] = (m.nan[c] || none) ? __builtin_nan("") : a.sign * tlast[c];
            if (m.nan[c]) {
                total[c] = __builtin_nan("");
                count[c] = -1;
            }
        }
        store_ints<LV>(a.count + i * LV, count);
        store_doubles<LV>(a.first + i * LV, tfirst);
        store_doubles<LV>(a.last + i * LV, tlast);
        store_doubles<LV>(a.total + i * LV, total);
    }
}

template <typename T>
struct RowDenseExposureArgs : RowDenseWindowArgs<T> {
    T* area_above;                    // [n_idx, L]
    T* area_below;                    // [n_idx, L]
    double* total;                    // [n_idx, L] duration above
    const T* level;                   // [n_rows, L]
};

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void row_dense_exposure_kernel(const RowDenseExposureArgs<T> a) {
    using E = typename std::conditional<VEC, typename VecOf<T>::type, T>::type;
    constexpr int LV = VEC ? VecOf<T>::L : 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.ne; i += stride) {
        const int64_t r = i / a.row_len;
        TimeAbove dur[LV];
        double a_up[LV], a_dn[LV], total[LV];
#pragma unroll
        for (int c = 0; c < LV; ++c) a_up[c] = a_dn[c] = 0.0;
        const RowDenseLevelWalk<LV> m = row_dense_level_walk<T, E, LV, true>(
            a, a.level, r, i - r * a.row_len, [&](int c, double tqa) { dur[c].open(tqa); },
            [&](int c, double tz, bool ab) { dur[c].cross(tz, ab); },
            [&](int c, double q, bool over) {
                if (over) a_up[c] = a_up[c] + q;
                else a_dn[c] = a_dn[c] - q;
            });
        T oa[LV], ob[LV];
#pragma unroll
        for (int c = 0; c < LV; ++c) {
            total[c] = m.nan[c] ? __builtin_nan("") : dur[c].close(m.above[c], m.tqb);
            oa[c] = m.nan[c] ? (T)__builtin_nan("") : (T)(a_up[c] < 0.0 ? 0.0 : a_up[c]);
            ob[c] = m.nan[c] ? (T)__builtin_nan("") : (T)(a_dn[c] < 0.0 ? 0.0 : a_dn[c]);
        }
        store_lanes<T, E, LV>(a.area_above, i, oa);
        store_lanes<T, E, LV>(a.area_below, i, ob);
        store_doubles<LV>(a.total + i * LV, total);
    }
}

template <typename T>
struct RowDenseLevelTimesArgs : RowDenseWindowArgs<T> {
    int32_t* n_up;                    // [n_idx, L] crossings after which the state is above: n_rising if sign > 0, else
    int32_t* n_dn;                    // n_falling; and those after which it is not (the launcher maps the directions)
    double* ups;                      // [K, n_idx, L] true time: rising if sign > 0, else falling
    double* dns;                      // [K, n_idx, L]
    int32_t k;                        // K: slots per list
    const T* level;                   // [n_rows, L]
    int64_t t_plane;                  // n_idx * L doubles: one slot of a list
};

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void row_dense_level_times_kernel(const RowDenseLevelTimesArgs<T> a) {
    using E = typename std::conditional<VEC, typename VecOf<T>::type, T>::type;
    constexpr int LV = VEC ? VecOf<T>::L : 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int32_t K = a.k;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.ne; i += stride) {
        const int64_t r = i / a.row_len;
        int32_t n_up[LV], n_dn[LV];                                   // crossings of the walk: to above, to not above
#pragma unroll
        for (int c = 0; c < LV; ++c) n_up[c] = n_dn[c] = 0;
        double* const ups = a.ups + i * LV;                           // slot 0 of this lane's elements
        double* const dns = a.dns + i * LV;
        const RowDenseLevelWalk<LV> m = row_dense_level_walk<T, E, LV, false>(
            a, a.level, r, i - r * a.row_len, [](int, double) {},
            [&](int c, double tz, bool ab) {
                const int32_t n = ab ? n_up[c] : n_dn[c];
                if (n < K) (ab ? ups : dns)[(int64_t)n * a.t_plane + c] = a.sign * tz;
                n_up[c] += ab ? 1 : 0;                                // (both counters by value: no pointer to either)
                n_dn[c] += ab ? 0 : 1;
            },
            NoPieces{});
        const double nan = __builtin_nan("");
#pragma unroll
        for (int c = 0; c < LV; ++c) {
            for (int32_t n = m.nan[c] ? 0 : n_up[c]; n < K; ++n) ups[(int64_t)n * a.t_plane + c] = nan;
            for (int32_t n = m.nan[c] ? 0 : n_dn[c]; n < K; ++n) dns[(int64_t)n * a.t_plane + c] = nan;
            if (m.nan[c]) n_up[c] = n_dn[c] = -1;
        }
        store_ints<LV>(a.n_up + i * LV, n_up);
        store_ints<LV>(a.n_dn + i * LV, n_dn);
    }
}

}  // namespace tdeq
