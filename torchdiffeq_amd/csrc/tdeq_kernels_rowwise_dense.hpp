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

}  // namespace tdeq
