// tdeq_kernels_rowwise_event.hpp — gfx950 device code of `odeint_rowwise_event` (torchdiffeq_amd/rowwise_event.py): a
// terminal event per row of a rowwise batch.
//
// A trial step of an event solve is the trial step of `odeint_rowwise` plus two launches between the controller and the
// dense-output commit:
//   row_event_detect   one lane per row: a row whose step was accepted and whose event value changed sign against the
//                      row's starting sign FIRES — its bracket [tprev_r, t0_r] is kept, it leaves the active rows and is
//                      frozen like a row that reached its last output time
//   row_event_fit      the quartic of the step of every row that fired in THIS trial step (interp.py:1-22 with the row's
//                      own step size), kept in a [5, n_rows, L] buffer: the commit that follows overwrites y0 and f0
// and, once every row has stopped, one bisection over the kept quartics:
//   row_event_eval     out[r, :] = the row's quartic at x[r] (interp.py:42-47), for the rows of a mask
// With `compact=` the stopped rows leave the batch, and the quartics stay in a buffer indexed by ORIGINAL row:
//   row_event_fit_mapped    row_event_fit of a compacted batch: the quartic of compact row r goes to q[:, row_map[r], :]
//   row_event_eval_mapped   the quartics of an index list: out[dst_map[i] or i, :] = q[:, src_map[i], :] at x[i]
// The arithmetic of an element is that of row_dense_commit_kernel (fit_one / eval_one of tdeq_kernels.hpp).
#pragma once

#include "tdeq_kernels_rowwise.hpp"

namespace tdeq {

struct RowEventDetectArgs {
    const void* g1;                   // [n_rows] of T: event_fn at the end of each row's trial step
    const int32_t* sign0;             // [n_rows] sign of the event value at the row's start (-1, 0, 1)
    const int32_t* accepted;          // [n_rows] the controller accepted this trial step
    const double* tprev;              // [n_rows] start of the accepted step
    const double* t0;                 // [n_rows] its end
    int32_t* active;
    int32_t* status;                  // status[0] = active rows (the controller's count, lowered by the rows that fire)
    void* dts;                        // [n_rows] of T: the NEXT trial step's sign * T(dt), zeroed for a row that fires
    void* times;                      // [n_times, n_rows] of T: the next stage times, frozen at the row's t0
    int n_times;
    double time_sign;
    int64_t n_rows;
    int32_t* fired;                   // [n_rows] sticky
    int32_t* fired_now;               // [n_rows] written for every row
    double* lo;                       // [n_rows] bracket of a row that fires
    double* hi;
};

// sign(g) = (g > 0) - (g < 0): 0 for a zero and for a NaN
template <typename T>
__device__ __forceinline__ int32_t row_event_sign(T g) {
    return (g > (T)0 ? 1 : 0) - (g < (T)0 ? 1 : 0);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void row_event_detect_kernel(const RowEventDetectArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool left = false;
    if (r < a.n_rows) {
        int32_t now = 0;
        if (a.accepted[r] && !a.fired[r] && row_event_sign<T>(static_cast<const T*>(a.g1)[r]) != a.sign0[r]) {
            now = 1;
            a.fired[r] = 1;
            a.lo[r] = a.tprev[r];
            a.hi[r] = a.t0[r];
            if (a.active[r]) {        // (a row whose step also reached its last output time has left already)
                a.active[r] = 0;
                left = true;
                row_freeze<T>(a.dts, a.times, a.n_times, a.n_rows, a.time_sign, a.t0[r], r);
            }
        }
        a.fired_now[r] = now;
    }
    // one atomic per wave, as the controller counts the active rows
    const uint64_t m = __ballot(left ? 1 : 0);
    if (lane == 0 && m) atomicSub(a.status, (int32_t)__popcll(m));
}

template <typename T, int NT>
struct RowEventFitArgs {
    T* q;                             // [5, n_rows, L]: e, d, c, b, a
    const T* y0;
    const T* y1;
    const T* f0;
    const T* f1;
    const T* k[NT];
    T c[NT];                          // fl_T(c_mid)
    const T* dts;                     // sign * T(dt) of the step just taken
    const int32_t* fired_now;
    int64_t row_len;                  // E units
    int64_t n;                        // n_rows * L elements of T
};

// fit_one (tdeq_kernels.hpp) on the row's own step: the same expressions in the same order, with the mid-point weights
// c_mid[j] * T(dt) formed where they are used, so that no DenseArgs block has to be built per element.
template <typename T, int NT, typename E>
__device__ __forceinline__ Quartic<T, E> row_event_fit_one(const T (&c)[NT], T dt, const E& y0, const E& y1, const E& f0,
                                                           const E& f1, const E (&kk)[NT]) {
    E acc = kk[0] * (c[0] * dt);                                     // fl_T(fl_T(mid_j) * T(dt)), as row_dense_commit
#pragma unroll
    for (int j = 1; j < NT; ++j) acc = acc + kk[j] * (c[j] * dt);
    const E ymid = y0 + acc;
    const T two_dt = (T)2 * dt;
    Quartic<T, E> q;
    q.a = ((f1 - f0) * two_dt - (y1 + y0) * (T)8) + ymid * (T)16;
    q.b = (((f0 * (T)5 - f1 * (T)3) * dt + y0 * (T)18) + y1 * (T)14) - ymid * (T)32;
    q.c = (((f1 - f0 * (T)4) * dt - y0 * (T)11) - y1 * (T)5) + ymid * (T)16;
    q.d = f0 * dt;
    q.e = y0;
    return q;
}

template <typename T, int NT, bool VEC>
__global__ __launch_bounds__(kBlock) void row_event_fit_kernel(const RowEventFitArgs<T, NT> a) {
    using E = typename std::conditional<VEC, typename VecOf<T>::type, T>::type;
    constexpr int LV = VEC ? VecOf<T>::L : 1;
    const int64_t ne = a.n / LV;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < ne; i += stride) {
        const int64_t r = i / a.row_len;
        if (!a.fired_now[r]) continue;
        const T dtT = a.dts[r];
        E kk[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) kk[j] = reinterpret_cast<const E*>(a.k[j])[i];
        const Quartic<T, E> q = row_event_fit_one<T, NT, E>(
            a.c, dtT, reinterpret_cast<const E*>(a.y0)[i], reinterpret_cast<const E*>(a.y1)[i],
            reinterpret_cast<const E*>(a.f0)[i], reinterpret_cast<const E*>(a.f1)[i], kk);
        reinterpret_cast<E*>(a.q)[i] = q.e;
        reinterpret_cast<E*>(a.q + a.n)[i] = q.d;
        reinterpret_cast<E*>(a.q + 2 * a.n)[i] = q.c;
        reinterpret_cast<E*>(a.q + 3 * a.n)[i] = q.b;
        reinterpret_cast<E*>(a.q + 4 * a.n)[i] = q.a;
    }
}

// The mapped form serves a compacted batch (`odeint_rowwise_event(compact=...)`): the state tensors, `dts` and
// `fired_now` hold the compact rows, `q` keeps all q_rows original ones (a row's quartic is read by the bisection after
// the row has left), and the quartic of compact row r goes to q[j, row_map[r], :].  A second kernel on the shared
// arithmetic (`row_event_fit_one`), not a flag on the first: a body shared through a reference to the argument block
// changes the register allocation of the plain instantiations, whose figures are to stay what they were.
template <typename T, int NT>
struct RowEventFitMappedArgs : RowEventFitArgs<T, NT> {
    const int32_t* row_map;           // [n_rows] row of q of each compact row
    int64_t q_plane;                  // q_rows * L elements of T: the stride of q's leading dimension
};

template <typename T, int NT, bool VEC>
__global__ __launch_bounds__(kBlock) void row_event_fit_mapped_kernel(const RowEventFitMappedArgs<T, NT> a) {
    using E = typename std::conditional<VEC, typename VecOf<T>::type, T>::type;
    constexpr int LV = VEC ? VecOf<T>::L : 1;
    const int64_t ne = a.n / LV;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < ne; i += stride) {
        const int64_t r = i / a.row_len;
        if (!a.fired_now[r]) continue;
        const T dtT = a.dts[r];
        E kk[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) kk[j] = reinterpret_cast<const E*>(a.k[j])[i];
        const Quartic<T, E> q = row_event_fit_one<T, NT, E>(
            a.c, dtT, reinterpret_cast<const E*>(a.y0)[i], reinterpret_cast<const E*>(a.y1)[i],
            reinterpret_cast<const E*>(a.f0)[i], reinterpret_cast<const E*>(a.f1)[i], kk);
        const int64_t at = (int64_t)a.row_map[r] * a.row_len + (i - r * a.row_len);
        reinterpret_cast<E*>(a.q)[at] = q.e;
        reinterpret_cast<E*>(a.q + a.q_plane)[at] = q.d;
        reinterpret_cast<E*>(a.q + 2 * a.q_plane)[at] = q.c;
        reinterpret_cast<E*>(a.q + 3 * a.q_plane)[at] = q.b;
        reinterpret_cast<E*>(a.q + 4 * a.q_plane)[at] = q.a;
    }
}

template <typename T>
struct RowEventEvalArgs {
    T* out;                           // [n_rows, L]
    const T* q;                       // [5, n_rows, L]
    const T* x;                       // [n_rows] the fraction of each row's step
    const int32_t* mask;              // [n_rows]
    int64_t row_len;                  // E units
    int64_t n;
};

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void row_event_eval_kernel(const RowEventEvalArgs<T> a) {
    using E = typename std::conditional<VEC, typename VecOf<T>::type, T>::type;
    constexpr int LV = VEC ? VecOf<T>::L : 1;
    const int64_t ne = a.n / LV;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < ne; i += stride) {
        const int64_t r = i / a.row_len;
        if (!a.mask[r]) continue;
        Quartic<T, E> q;
        q.e = reinterpret_cast<const E*>(a.q)[i];
        q.d = reinterpret_cast<const E*>(a.q + a.n)[i];
        q.c = reinterpret_cast<const E*>(a.q + 2 * a.n)[i];
        q.b = reinterpret_cast<const E*>(a.q + 3 * a.n)[i];
        q.a = reinterpret_cast<const E*>(a.q + 4 * a.n)[i];
        reinterpret_cast<E*>(a.out)[i] = eval_one<T, E>(q, a.x[r]);
    }
}

// The quartics of an index list (the bisection of a compacted event solve): for i < n_idx,
// out[DST ? dst_map[i] : i, :] = the quartic q[:, src_map[i], :] at x[i].  No mask: the list is the mask.
template <typename T>
struct RowEventEvalMappedArgs {
    T* out;                           // [out_rows, L]
    const T* q;                       // [5, q_rows, L]
    const T* x;                       // [n_idx] the fraction of each listed row's step
    const int32_t* src_map;           // [n_idx] row of q
    const int32_t* dst_map;           // [n_idx] row of out (DST), else not read
    int64_t row_len;                  // E units
    int64_t ne;                       // n_idx * row_len
    int64_t q_plane;                  // q_rows * L elements of T
};

template <typename T, bool VEC, bool DST>
__global__ __launch_bounds__(kBlock) void row_event_eval_mapped_kernel(const RowEventEvalMappedArgs<T> a) {
    using E = typename std::conditional<VEC, typename VecOf<T>::type, T>::type;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.ne; i += stride) {
        const int64_t r = i / a.row_len;
        const int64_t e = i - r * a.row_len;
        const int64_t from = (int64_t)a.src_map[r] * a.row_len + e;
        Quartic<T, E> q;
        q.e = reinterpret_cast<const E*>(a.q)[from];
        q.d = reinterpret_cast<const E*>(a.q + a.q_plane)[from];
        q.c = reinterpret_cast<const E*>(a.q + 2 * a.q_plane)[from];
        q.b = reinterpret_cast<const E*>(a.q + 3 * a.q_plane)[from];
        q.a = reinterpret_cast<const E*>(a.q + 4 * a.q_plane)[from];
        const int64_t to = DST ? (int64_t)a.dst_map[r] * a.row_len + e : i;
        reinterpret_cast<E*>(a.out)[to] = eval_one<T, E>(q, a.x[r]);
    }
}

}  // namespace tdeq
