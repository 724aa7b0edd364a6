// Kernels of the data selection (datatype/selectdata.py): out = the selected rows of a tensor, of every row the selected
// elements, moved as raw bits.  One family, memory-bound: the lane (4, 8 or 16 bytes) and the addressing mode are template
// parameters, so that a whole-row copy carries none of the index arithmetic of an axis selection.
//
// Addressing.  The output rows of one launch follow each other; trial k of the launch owns the output rows
// [desc[3k], desc[3k] + desc[3k + 2]) and reads the source from row desc[3k + 1] on.  An output row has `wo` elements, a
// source row `ws`.  FLAT: wo = ws and an element keeps its column.  AXES: the column splits into up to three indices
// (i0, i1, i2) of the collapsed axes (select_route.h), each mapped to a source index by its start or through its index
// list, which the workgroup reads from LDS (AXES_LDS) or from global memory.  A lane moves 1 << vshift elements that are
// contiguous in both tensors (the route saw to that).  A workgroup takes a contiguous range of the launch's lanes and its
// threads walk it side by side; a thread looks its trial up by binary search only when it leaves the trial it was in.
// All index arithmetic is int64.
#pragma once
#include <cstdint>

#include "select_route.h"

namespace spysel {

constexpr int THREADS = 256;

struct Lane4 { unsigned v; };
struct Lane8 { unsigned long long v; };
struct alignas(8) Lane16e { unsigned long long v[2]; };     // a 16-byte element on an 8-byte boundary
struct alignas(16) Lane16 { unsigned long long v[2]; };

struct Args {
    const void* src;
    void* out;
    const long long* desc;      // (ntrials, 3): output row, source row, rows
    const int* idx;             // the index lists, one after the other
    long long ntrials, row0, nrows, wo, ws;
    long long n[3], s[3], start[3], loff[3];
    int nidx, vshift;
};

// a / b for 0 <= a, 0 < b: the 32-bit division where both fit
__device__ __forceinline__ long long idiv(long long a, long long b) {
    if ((((unsigned long long)a | (unsigned long long)b) >> 32) == 0) return (long long)((unsigned)a / (unsigned)b);
    return a / b;
}

// the last trial whose first output row is <= row (trials without rows share their row with the one that follows)
__device__ __forceinline__ long long find_trial(const long long* desc, long long n, long long row) {
    long long lo = 0, hi = n - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (desc[3 * mid] <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <class L, int MODE>
__global__ __launch_bounds__(THREADS) void select_kernel(const Args g) {
    const L* __restrict__ src = reinterpret_cast<const L*>(g.src);
    L* __restrict__ out = reinterpret_cast<L*>(g.out);
    const int* list = g.idx;
    if constexpr (MODE == AXES_LDS) {
        __shared__ int lds_idx[LDS_CAP];
        for (int i = threadIdx.x; i < g.nidx; i += THREADS) lds_idx[i] = g.idx[i];
        __syncthreads();
        list = lds_idx;
    }
    const long long nitem = (g.nrows * g.wo) >> g.vshift;
    long long per = (nitem + gridDim.x - 1) / gridDim.x;
    per = (per + THREADS - 1) / THREADS * THREADS;
    const long long lo = (long long)blockIdx.x * per;
    const long long hi = lo + per < nitem ? lo + per : nitem;
    long long t_out = 0, t_rows = 0, t_src = 0;                  // the trial this thread is in: none yet
    for (long long it = lo + threadIdx.x; it < hi; it += THREADS) {
        const long long e = it << g.vshift;
        const long long rrow = idiv(e, g.wo), col = e - rrow * g.wo, row = g.row0 + rrow;
        if (row < t_out || row >= t_out + t_rows) {
            const long long k = find_trial(g.desc, g.ntrials, row);
            t_out = g.desc[3 * k]; t_src = g.desc[3 * k + 1]; t_rows = g.desc[3 * k + 2];
        }
        long long scol = col;
        if constexpr (MODE != FLAT) {
            const long long q = idiv(col, g.n[2]), i2 = col - q * g.n[2];
            const long long i0 = idiv(q, g.n[1]), i1 = q - i0 * g.n[1];
            const long long m0 = g.loff[0] >= 0 ? list[g.loff[0] + i0] : g.start[0] + i0;
            const long long m1 = g.loff[1] >= 0 ? list[g.loff[1] + i1] : g.start[1] + i1;
            const long long m2 = g.loff[2] >= 0 ? list[g.loff[2] + i2] : g.start[2] + i2;
            scol = m0 * g.s[0] + m1 * g.s[1] + m2;
        }
        const long long si = (t_src + (row - t_out)) * g.ws + scol, oi = row * g.wo + col;
        out[oi >> g.vshift] = src[si >> g.vshift];
    }
}

}  // namespace spysel
