// K13: the phase slope index (Nolte et al. 2008; FieldTrip's `psi`).  Not in the reference; the definition (DESIGN.md
// section 8).  With c_ij(f) the complex64 coherency exactly as K5 forms it (csd_kernel.h: scaled values, the diagonal's
// imaginary part zeroed, v / sqrtf(d_i d_j) in float32) but 0, not NaN, where d_i d_j is not positive, edge e joins the
// bins e and e + 1:
//     p_ij(e) = Im(conj(c_ij(e)) c_ij(e + 1)) = c.x(e) c.y(e + 1) - c.y(e) c.x(e + 1)
// (both products float64 of float32 values, so exact), and for the half width h >= 1
//     psi[k, i, j] = sum_{e = k - h}^{k + h - 1} p_ij(e),   h <= k <= F - 1 - h,   whole planes NaN elsewhere;
// h = 0: one plane, psi[0, i, j] = sum_{e = 0}^{F - 2} p_ij(e).  Every sum is float64, rounded to float32 once.
//
// One workgroup owns one lower-triangle 32 x 32 tile and one RUN of output bins, and walks down the frequencies of the
// run and its halo of 2h bins: the float64 window sum of each of its four elements per thread stays in registers, the
// newest edge is added and the oldest, re-read 2h bins behind (it is in the L2 or the Infinity Cache), subtracted.  The
// diagonal values of the tile's rows and columns are staged in LDS for NB bins at a time; the loads of the next bin are
// issued before the barrier of this one.  The upper triangle is the negated mirror and goes through an LDS transpose,
// so that both triangles are written row-wise (see coh_from_acc_kernel).  No atomics.  h = 0 has one output plane: the
// runs leave float64 partial sums, which phaseslope_reduce_kernel adds in run order.
#pragma once
#include <algorithm>
#include "spy_intrinsics.h"
#include "../../include/spyhip.h"

namespace spyphaseslope {

constexpr int NB = 16;          // bins whose diagonal values are staged at once
constexpr int MIN_RUN = 16;     // output bins of a run at the least (h >= 1; 2h where that is more)
constexpr int MIN_RUN0 = 32;    // edges of a run at the least (h = 0)

struct PhaseSlopeArgs {
    const float2* in;   // (F, C, C) complex64: the Hermitian CSD, or the raw lower-triangle accumulator (RAW)
    int F, C;
    float scale;        // RAW only
    int half;           // h
    int run, nruns;     // output bins (h = 0: edges) per run, number of runs
    float* out;         // (F, C, C), h = 0: (1, C, C)
    double* part;       // h = 0 with nruns > 1: (nruns, C, C) partial sums on the lower triangle
};

// runs of `count` output bins (edges) such that a single tile still gives every CU close to four workgroups - but not
// more than four, which is what a CU holds at once at the kernel's 4 waves per SIMD: a few workgroups more than that run
// alone in a second round - and no run shorter than `min_run`: the halo of 2h bins is read again by every run
inline int plan_runs(int count, int min_run, long long ntiles, int num_cu, int& run) {
    const long long want = std::max(1LL, 4LL * num_cu / ntiles);
    long long r = (count + want - 1) / want;
    if (r < min_run) r = min_run;
    if (r > count) r = count;
    run = (int)r;
    return (count + run - 1) / run;
}

__device__ __forceinline__ void tile_of(int tt, int& ti, int& tj) {
    // inverse of tt = ti*(ti+1)/2 + tj, tj <= ti
    int i = (int)((sqrtf(8.0f * (float)tt + 1.0f) - 1.0f) * 0.5f);
    while ((i + 1) * (i + 2) / 2 <= tt) ++i;
    while (i * (i + 1) / 2 > tt) --i;
    ti = i;
    tj = tt - i * (i + 1) / 2;
}

// K5's coherency of one element; 0 where the product of the diagonal values is not positive
__device__ __forceinline__ float2 coherency(float2 v, float di, float dj) {
    const float q = di * dj;
    const float s = sqrtf(q);
    return q > 0.f ? make_float2(v.x / s, v.y / s) : make_float2(0.f, 0.f);
}

__device__ __forceinline__ double edge(float2 a, float2 b) {
    return (double)a.x * (double)b.y - (double)a.y * (double)b.x;
}

// one plane of a tile: the lower part row-wise, the negated mirror row-wise through `tile`.  One barrier; the caller
// alternates between two tiles, so that no second one is needed.
__device__ __forceinline__ void store_tile(float* O, int C, int ti, int tj, int tx, int ty, const float (&val)[4],
                                           float (*tile)[33]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = ty + 8 * k, i = ti * 32 + r, j = tj * 32 + tx;
        float up = 0.f;
        if (i < C && j < C && j <= i) {
            const float lo = i == j ? 0.f : val[k];
            O[(size_t)i * C + j] = lo;
            up = -lo;
        }
        tile[tx][r] = up;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = ty + 8 * k;                                // element (r, tx) of the mirrored tile (tj, ti)
        const int i = tj * 32 + r, j = ti * 32 + tx;
        if (i < C && j < C && j > i) O[(size_t)i * C + j] = tile[r][tx];
    }
}

template <bool RAW>
__global__ void __launch_bounds__(256) phaseslope_kernel(PhaseSlopeArgs a) {
    __shared__ float tile[2][32][33];
    __shared__ float dlead[NB][64], dtrail[NB][64];              // [bin][32 row channels, 32 column channels]
    const int C = a.C, F = a.F, h = a.half, W = 2 * a.half;
    const int nt = (C + 31) / 32, ntiles = nt * (nt + 1) / 2;
    const int q = (int)(blockIdx.x / ntiles);
    int ti, tj;
    tile_of((int)(blockIdx.x % ntiles), ti, tj);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const size_t plane = (size_t)C * C;
    // bins bstart ... bend of this run: its output bins k0 ... k1 - 1 and h bins on either side, or (h = 0) its edges
    const int first = h + q * a.run;                             // h = 0: the first edge
    const int left = (h ? F - h : F - 1) - first;
    const int count = a.run < left ? a.run : left;
    const int bstart = first - h, bend = first + count - 1 + (h ? h : 1);
    const int j = tj * 32 + tx;
    bool ok[4];
    unsigned off[4];                                             // (the launcher refuses C * C >= 2^32)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = ti * 32 + ty + 8 * k;
        ok[k] = i < C && j < C && j <= i;
        off[k] = (unsigned)i * (unsigned)C + (unsigned)j;
    }
    auto load = [&](int bin, float2 (&v)[4]) {
        const float2* A = a.in + (size_t)bin * plane;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float2 x = make_float2(0.f, 0.f);
            if (ok[k]) {
                x = A[off[k]];
                if (RAW) { x.x *= a.scale; x.y *= a.scale; }
                if (ti * 32 + ty + 8 * k == j) x.y = 0.f;
            }
            v[k] = x;
        }
    };
    auto diagonal = [&](int bin, int ch) {
        const float d = a.in[(size_t)bin * plane + (size_t)ch * C + ch].x;
        return RAW ? d * a.scale : d;
    };
    float2 nl[4], nl2[4], ntr[4], cl[4], ct[4];                  // leading values one and two bins ahead, trailing ones
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    load(bstart, nl);
    load(bstart + 1, nl2);                                       // (a run has two bins at the least)
#pragma unroll
    for (int k = 0; k < 4; ++k) ntr[k] = cl[k] = ct[k] = make_float2(0.f, 0.f);
    int buf = 0;
    for (int b = bstart; b <= bend; ++b) {
        const int s = (b - bstart) % NB;
        if (s == 0) {
            __syncthreads();
            for (int n = threadIdx.x; n < NB * 64; n += 256) {
                const int bb = n >> 6, w = n & 63;
                const int ch = w < 32 ? ti * 32 + w : tj * 32 + w - 32;
                const int lb = b + bb, tb = b + bb - W + 1;      // the trailing bin is consumed from bstart + 1 on
                dlead[bb][w] = (ch < C && lb <= bend) ? diagonal(lb, ch) : 1.f;
                dtrail[bb][w] = (W > 0 && ch < C && tb > bstart && tb <= bend) ? diagonal(tb, ch) : 1.f;
            }
            __syncthreads();
        }
        const bool emit = W > 0 && b - bstart >= W;              // the window that ends with edge b - 1 is full
        float2 v[4], vt[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = nl[k]; vt[k] = ntr[k]; nl[k] = nl2[k]; }
        // the values of the steps to come, issued before this step's barrier
        if (b + 2 <= bend) load(b + 2, nl2);
        if (b < bend && W > 0 && b + 1 - bstart >= W) load(b + 2 - W, ntr);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float2 c = coherency(v[k], dlead[s][ty + 8 * k], dlead[s][32 + tx]);
            if (b > bstart) sum[k] += edge(cl[k], c);
            else ct[k] = c;                                      // the oldest edge starts at bstart
            cl[k] = c;
        }
        if (emit) {
            float val[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) val[k] = (float)sum[k];
            store_tile(a.out + (size_t)(b - h) * plane, C, ti, tj, tx, ty, val, tile[buf]);
            buf ^= 1;
            if (b < bend) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float2 c = coherency(vt[k], dtrail[s][ty + 8 * k], dtrail[s][32 + tx]);
                    sum[k] -= edge(ct[k], c);
                    ct[k] = c;
                }
            }
        }
    }
    if (h == 0) {
        if (a.part == nullptr) {
            float val[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) val[k] = (float)sum[k];
            store_tile(a.out, C, ti, tj, tx, ty, val, tile[0]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ok[k]) a.part[(size_t)q * plane + off[k]] = sum[k];
        }
        return;
    }
    // the 2h planes in which the band does not fit, dealt out over the runs
    const float nan = __int_as_float(0x7fc00000);
    for (int n = q; n < W; n += a.nruns) {
        float* O = a.out + (size_t)(n < h ? n : F - W + n) * plane;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = ty + 8 * k;
            if (ok[k]) O[off[k]] = nan;
            const int i = tj * 32 + r, jj = ti * 32 + tx;
            if (i < C && jj < C && jj > i) O[(size_t)i * C + jj] = nan;
        }
    }
}

// h = 0 with more than one run: the partial sums of a tile in run order, rounded once, both triangles
__global__ void __launch_bounds__(256) phaseslope_reduce_kernel(const double* part, int nparts, int C, float* out) {
    __shared__ float tile[32][33];
    int ti, tj;
    tile_of((int)blockIdx.x, ti, tj);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const size_t plane = (size_t)C * C;
    float val[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = ti * 32 + ty + 8 * k, j = tj * 32 + tx;
        double s = 0.0;
        if (i < C && j < C && j <= i)
            for (int p = 0; p < nparts; ++p) s += part[(size_t)p * plane + (size_t)i * C + j];
        val[k] = (float)s;
    }
    store_tile(out, C, ti, tj, tx, ty, val, tile);
}

}  // namespace spyphaseslope
