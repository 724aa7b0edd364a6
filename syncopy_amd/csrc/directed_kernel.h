// K11: row- or column-normalised, transposed float32 magnitudes of a stack of complex128 matrices - the directed transfer
// function (axis 0, M = H) and partial directed coherence (axis 1, M = H^-1) with their noise-weighted forms:
//   axis 0: out[f,s,r] = w_s |M[f,r,s]| / sqrt(sum_k w_k^2 |M[f,r,k]|^2)
//   axis 1: out[f,s,r] = w_r |M[f,r,s]| / sqrt(sum_k w_k^2 |M[f,k,s]|^2)
// In both the weight of an entry is the weight of its index ALONG the norm, so with "line" = the row (axis 0) or the
// column (axis 1) the norm runs along and k = the position on it, an entry contributes p = w_k^2 |M|^2 to its line's sum
// and becomes sqrt(p / sum) - or p / sum for the squared form; a zero sum gives 0.  float64 throughout, one rounding.
//
// The output is the transpose of the input's index order: axis 0 reads along k (16-byte loads, a wave per line) and
// writes along the line; axis 1 reads along the line (DL x 16 bytes per row of M) and writes along k.  The strip of DL
// lines passes through an LDS tile of doubles with an odd row stride (directed_route.h): the side that walks the lines
// with its lanes meets DL different bank pairs, the other side consecutive addresses.  Which strip a workgroup takes:
// ids are dealt round-robin to the 8 XCDs, so id % 8 picks the XCD and the strips of one matrix get consecutive slots
// of one XCD (as zgemm_mfma_kernel numbers its tiles): neighbouring strips share the cache lines at their seams, and the
// second sweep of a strip that does not fit LDS finds it in that XCD's L2.
#pragma once
#include "spy_common.h"
#include "directed_route.h"

namespace spydir {

typedef double2 cd;

// the entry at position k of line `line`
template <int AXIS>
__device__ __forceinline__ double entry_power(const cd* Mf, const double* w, int n, int line, int k) {
    const cd v = AXIS == 0 ? Mf[(size_t)line * n + k] : Mf[(size_t)k * n + line];
    const double wk = w ? w[k] : 1.0;
    return wk * wk * (v.x * v.x + v.y * v.y);
}

__device__ __forceinline__ float normalised(double p, double sum, int squared) {
    const double r = sum > 0.0 ? p / sum : 0.0;
    return (float)(squared ? r : sqrt(r));
}

template <int AXIS>
__global__ void __launch_bounds__(DT) directed_norm_kernel(const cd* M, const double* w, int F, int n, int kc, int cached,
                                                           int squared, float* out) {
    SPY_DYN_SMEM(char, raw);
    const int ld = norm_ld(kc);
    double* P = reinterpret_cast<double*>(raw);      // DL x ld: w_k^2 |M|^2 of the strip (or of one chunk of it)
    double* den = P + (size_t)DL * ld;               // DL sums
    double* red = den + DL;                          // DW x DL partial sums (axis 1)
    const int strips = norm_strips(n);
    const int lin = blockIdx.x, slot = lin >> 3;
    const int f = (slot / strips) * 8 + (lin & 7), strip = slot % strips;
    if (f >= F) return;
    const cd* Mf = M + (size_t)f * n * n;
    float* of = out + (size_t)f * n * n;
    const int l0 = strip * DL, nl = n - l0 < DL ? n - l0 : DL;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tl = tid & (DL - 1), tq = tid / DL;    // the mapping that walks the lines: line tl, positions tq, tq + DT / DL, ...
    constexpr int QS = DT / DL, LW = DL / DW;        // positions per step of that mapping; lines per wave of the other

    // ---- sweep 1: the sums (and, when the strip fits, the tile)
    if (AXIS == 0) {
        double sum[LW];
#pragma unroll
        for (int i = 0; i < LW; ++i) sum[i] = 0.0;
        for (int c0 = 0; c0 < n; c0 += kc) {
            const int kend = n - c0 < kc ? n - c0 : kc;
#pragma unroll
            for (int i = 0; i < LW; ++i) {
                const int line = wave + DW * i;
                if (line >= nl) continue;
#pragma unroll 4
                for (int kk = lane; kk < kend; kk += 64) {
                    const double p = entry_power<0>(Mf, w, n, l0 + line, c0 + kk);
                    sum[i] += p;
                    if (cached) P[(size_t)line * ld + kk] = p;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < LW; ++i) {
            double s = sum[i];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
            if (lane == 0) den[wave + DW * i] = s;
        }
    } else {
        double s = 0.0;
        for (int c0 = 0; c0 < n; c0 += kc) {
            const int kend = n - c0 < kc ? n - c0 : kc;
            if (tl < nl) {
#pragma unroll 8
                for (int kk = tq; kk < kend; kk += QS) {
                    const double p = entry_power<1>(Mf, w, n, l0 + tl, c0 + kk);
                    s += p;
                    if (cached) P[(size_t)tl * ld + kk] = p;
                }
            }
        }
        s += __shfl_xor(s, 32);                      // lanes l and l + 32 of a wave hold the same line (DL = 32)
        if (lane < DL) red[wave * DL + lane] = s;
        __syncthreads();
        if (tid < DL) {
            double t = 0.0;
#pragma unroll
            for (int v = 0; v < DW; ++v) t += red[v * DL + tid];
            den[tid] = t;
        }
    }
    __syncthreads();

    // ---- sweep 2: out = sqrt(p / sum), transposed
    for (int c0 = 0; c0 < n; c0 += kc) {
        const int kend = n - c0 < kc ? n - c0 : kc;
        if (!cached) {
            __syncthreads();                         // the tile of the chunk before has been written out
            if (AXIS == 0) {
#pragma unroll
                for (int i = 0; i < LW; ++i) {
                    const int line = wave + DW * i;
                    if (line >= nl) continue;
                    for (int kk = lane; kk < kend; kk += 64) P[(size_t)line * ld + kk] = entry_power<0>(Mf, w, n, l0 + line, c0 + kk);
                }
            } else if (tl < nl) {
                for (int kk = tq; kk < kend; kk += QS) P[(size_t)tl * ld + kk] = entry_power<1>(Mf, w, n, l0 + tl, c0 + kk);
            }
            __syncthreads();
        }
        if (AXIS == 0) {                             // out[f, s = k, r = line]: the lanes walk the lines
            if (tl < nl) {
                const double d = den[tl];
                for (int kk = tq; kk < kend; kk += QS)
                    of[(size_t)(c0 + kk) * n + l0 + tl] = normalised(P[(size_t)tl * ld + kk], d, squared);
            }
        } else {                                     // out[f, s = line, r = k]: the lanes walk k
#pragma unroll
            for (int i = 0; i < LW; ++i) {
                const int line = wave + DW * i;
                if (line >= nl) continue;
                const double d = den[line];
                for (int kk = lane; kk < kend; kk += 64)
                    of[(size_t)(l0 + line) * n + c0 + kk] = normalised(P[(size_t)line * ld + kk], d, squared);
            }
        }
    }
}

}  // namespace spydir
