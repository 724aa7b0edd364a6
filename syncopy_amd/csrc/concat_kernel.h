// Kernel of the channel concatenation (datatype/concat.py): out = the rows of up to eight tensors side by side, moved as raw
// bits.  Memory-bound: every byte is read once and written once.  The lane (4, 8 or 16 bytes) is the template parameter.
//
// Addressing.  The output rows of one launch follow each other, so the launch's output is one contiguous range of lanes
// and lane `it` of the launch is lane `it` of that range.  A workgroup takes a contiguous part of it and its threads walk
// that part side by side, 256 lanes a pass: consecutive threads store to consecutive addresses, and a thread stays inside
// one trial for many passes (with the passes of ALL workgroups interleaved instead, 4096 x 256 lanes apart, every pass of
// a thread lands in another trial and pays for the search: 1.8 TB/s measured).  A lane is (line, column) =
// (it / w, it % w), kept up from pass to pass by adding the step without a division.  The column
// names the source (the one whose run [cum[s], cum[s + 1]) holds it) by a chain of at most seven compares against
// values that sit in scalar registers.  Trial k of the launch owns the output rows [desc[k][0], desc[k][0] + desc[k][1])
// and reads source s from row desc[k][2 + s] on, so the source's lane is
//     ((desc[k][2 + s] - desc[k][0] + row0) * pre * run[s] - cum[s])  +  line * run[s] + column,
// the first term fixed per trial and source: a thread folds it into one address per source when it enters a trial (found
// by binary search) and does one multiply-add per lane.  Runs, offsets and the line are in LANES (the route saw to it
// that they divide).  All index arithmetic is int64.
#pragma once
#include <cstdint>

#include "concat_route.h"

namespace spycat {

constexpr int THREADS = 256;

struct Lane4 { unsigned v; };
struct Lane8 { unsigned long long v; };
struct alignas(8) Lane16e { unsigned long long v[2]; };     // a 16-byte element on an 8-byte boundary
struct alignas(16) Lane16 { unsigned long long v[2]; };

struct Args {
    const void* src[MAX_SRC];   // unused slots repeat the last source
    void* out;
    const long long* desc;      // (ntrials, 2 + nsrc): output row, rows, the first row in each source
    long long cum[MAX_SRC + 1]; // lanes: first lane of each source's run in a line; unused slots hold w (an empty run)
    long long ntrials, row0, nrows, pre, w;     // w: lanes of an output line
    int nsrc;
};

// a / b for 0 <= a, 0 < b: the 32-bit division where both fit
__device__ __forceinline__ long long idiv(long long a, long long b) {
    if ((((unsigned long long)a | (unsigned long long)b) >> 32) == 0) return (long long)((unsigned)a / (unsigned)b);
    return a / b;
}

// the last trial whose first output row is <= row (trials without rows share their row with the one that follows)
__device__ __forceinline__ long long find_trial(const long long* desc, long long stride, long long n, long long row) {
    long long lo = 0, hi = n - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (desc[stride * mid] <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <class L>
__global__ __launch_bounds__(THREADS) void concat_kernel(const Args g) {
    L* __restrict__ out = reinterpret_cast<L*>(g.out) + g.row0 * g.pre * g.w;
    const long long nitem = g.nrows * g.pre * g.w, stride = 2 + g.nsrc;
    long long per = (nitem + gridDim.x - 1) / gridDim.x;            // a workgroup's contiguous range of lanes
    per = (per + THREADS - 1) / THREADS * THREADS;
    const long long lo = (long long)blockIdx.x * per, hi = lo + per < nitem ? lo + per : nitem;
    const long long step_line = THREADS / g.w, step_col = THREADS - step_line * g.w;
    long long it = lo + threadIdx.x;
    long long line = idiv(it, g.w), col = it - line * g.w;
    long long t_lo = 0, t_hi = 0;                       // the lines of the trial this thread is in: none yet
    const char* addr[MAX_SRC] = {};                     // per source the address that lane (line 0, column 0) would have
    for (; it < hi; it += THREADS) {
        if (line < t_lo || line >= t_hi) {
            const long long row = g.row0 + idiv(line, g.pre);
            const long long* d = g.desc + stride * find_trial(g.desc, stride, g.ntrials, row);
            t_lo = (d[0] - g.row0) * g.pre; t_hi = t_lo + d[1] * g.pre;
#pragma unroll
            for (int s = 0; s < MAX_SRC; ++s)
                if (s < g.nsrc)
                    addr[s] = reinterpret_cast<const char*>(g.src[s]) +
                              ((d[2 + s] - d[0] + g.row0) * g.pre * (g.cum[s + 1] - g.cum[s]) - g.cum[s]) * (long long)sizeof(L);
        }
        // the source of this column: constant indices only, so the tables stay in registers
        const char* a = addr[0];
        long long run = g.cum[1];
        if (col >= g.cum[1]) { a = addr[1]; run = g.cum[2] - g.cum[1]; }
        if (g.nsrc > 2) {                               // (the same for every thread: two sources skip the rest)
#pragma unroll
            for (int s = 2; s < MAX_SRC; ++s)
                if (s < g.nsrc && col >= g.cum[s]) { a = addr[s]; run = g.cum[s + 1] - g.cum[s]; }
        }
        out[it] = *reinterpret_cast<const L*>(a + (line * run + col) * (long long)sizeof(L));
        line += step_line; col += step_col;
        if (col >= g.w) { col -= g.w; ++line; }
    }
}

}  // namespace spycat
