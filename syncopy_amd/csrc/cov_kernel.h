// Per-trial channel covariance of spy.timelockanalysis (statistics/compRoutines.py: cov_cF = np.cov(trial, ddof=ddof,
// rowvar=False)) on the fp64 matrix cores.  Kept in a header so that the CPU emulation of the tests compiles the same
// kernels; the launcher lives in cov.hip.
//
// x (ntrials, n, nchan) float32, channel fastest -> out (ntrials, nchan, nchan) float32.  Per trial, as NumPy does it:
//
//     m[c]      = sum_k (double)x[k][c] / n                                  cov_mean_kernel
//     out[i][j] = (float)(sum_k (x[k][i] - m[i]) * (x[k][j] - m[j]) * (1.0 / (n - ddof)))      cov_kernel
//
// everything up to the one rounding at the end in float64.  The centred two-pass form is on purpose: the one-pass form
// sum xy - n mx my loses the digits a DC offset takes.  No sum has an order that depends on the launch: the
// mean adds the rows NW apart per wave and the waves' parts in wave order, a covariance element is one fma chain over k
// inside v_mfma_f64_16x16x4_f64.  Two runs give the same bits.
//
// Mapping of cov_kernel.  The matrix is cut into blocks of 64 x 64 channels; a workgroup of 4 waves takes one block
// (bi, bj) with bi >= bj of one trial, wave w the 32 x 32 quadrant (w >> 1, w & 1) as 2 x 2 tiles of 16 x 16.  Only
// tiles on or below the diagonal that reach into the matrix are computed; a tile below the diagonal is also stored
// transposed above it.  A diagonal tile holds both halves, which are the same fma chains with the factors swapped, so
// the result is symmetric to the bit.  Time is walked in chunks of KC rows: the 64 channels of block row bi and of block
// column bj are centred, converted and staged in LDS as doubles ([k][channel], row stride LD = 80 doubles, so that the
// two rows k a 32-lane group of ds_read_b64 touches lie 32 banks apart); a diagonal block stages one slab and reads it
// as both operands.  The floats of the next chunk are requested before the matrix instructions of the current one.
// Operand layout (cdna_hip_programming.md 3): A one double per lane at [row = lane & 15][k = lane >> 4], B at
// [k = lane >> 4][col = lane & 15], D four doubles per lane at row = (lane >> 4) + 4 * reg, col = lane & 15.
// Rows past the trial and channels past nchan are staged as exact zeros (not 0 - mean), so a NaN in channel c - which
// makes m[c] and with it the whole centred column c NaN - reaches row and column c of the result and nothing else.
// All sample and element indices are 64-bit.  out must not be x.
#pragma once

namespace spycov {

constexpr int CB = 64;           // channels per block side
constexpr int LD = CB + 16;      // doubles per staged row

// lower-triangle blocks of an nchan x nchan matrix
__host__ __device__ inline long long cov_blocks(long long nchan) {
    const long long nb = (nchan + CB - 1) / CB;
    return nb * (nb + 1) / 2;
}

// grid = (ceil(nchan / 64), trials), 64 * NW threads: lane = channel, wave w adds rows w, w + NW, ...
template <int NW>
__global__ void __launch_bounds__(64 * NW)
cov_mean_kernel(const float* __restrict__ x, double* __restrict__ mean, long long n, long long nchan) {
    __shared__ double part[NW * 64];
    const int lane = threadIdx.x & 63;
    const int w = spy_wave_index(threadIdx.x);
    const long long c = (long long)blockIdx.x * 64 + lane;
    const long long trial = blockIdx.y;
    const bool ok = c < nchan;
    const float* p = x + trial * n * nchan + (ok ? c : 0);
    double s = 0.0;
#pragma unroll 4
    for (long long k = w; k < n; k += NW) s += (double)p[k * nchan];
    part[w * 64 + lane] = s;
    __syncthreads();
    if (w == 0 && ok) {
        double t = 0.0;
        for (int i = 0; i < NW; ++i) t += part[i * 64 + lane];
        mean[trial * nchan + c] = t / (double)n;
    }
}

template <int KC>
struct CovTile {
    static constexpr int THREADS = 256;
    static constexpr int Q = KC / 4;                                        // staged rows per thread and slab
    static_assert(KC % 4 == 0, "four waves stage a chunk row by row, and a matrix instruction takes four rows");
    static constexpr long long lds_bytes() { return 2LL * KC * LD * 8; }
};

// grid = (cov_blocks(nchan), trials), 256 threads, CovTile<KC>::lds_bytes() of dynamic LDS; scale = 1.0 / (n - ddof)
template <int KC>
__global__ void __launch_bounds__(256)
cov_kernel(const float* __restrict__ x, const double* __restrict__ mean, float* __restrict__ out, long long n,
           long long nchan, double scale) {
    using Tile = CovTile<KC>;
    SPY_DYN_SMEM(double, As);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = spy_wave_index(tid);
    const int l15 = lane & 15, l4 = lane >> 4;
    // block (bi, bj), bi >= bj, from its index in the row-wise walk of the lower triangle
    const long long p = blockIdx.x;
    long long bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= p) ++bi;
    const long long bj = p - bi * (bi + 1) / 2;
    const bool diag = bi == bj;
    double* Bs = diag ? As : As + KC * LD;
    const long long ci0 = bi * CB, cj0 = bj * CB;
    const int wr = (w >> 1) * 32, wc = (w & 1) * 32;
    // tiles of this wave: on or below the diagonal and inside the matrix (uniform over the wave)
    bool on[2][2];
    bool any = false;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const long long ti = ci0 + wr + 16 * u, tj = cj0 + wc + 16 * v;
            on[u][v] = ti >= tj && ti < nchan;
            any = any || on[u][v];
        }
    const long long trial = blockIdx.y;
    const float* xt = x + trial * n * nchan;
    const long long ca = ci0 + lane, cb = cj0 + lane;
    const bool okA = ca < nchan, okB = !diag && cb < nchan;
    const double ma = okA ? mean[trial * nchan + ca] : 0.0;
    const double mb = okB ? mean[trial * nchan + cb] : 0.0;
    const float* xa = xt + (okA ? ca : 0);
    const float* xb = xt + (okB ? cb : 0);

    f64x4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[u][v][r] = 0.0;

    // thread (wave w, lane) stages rows w, w + 4, ... of the chunk for channel `lane` of either slab
    float pa[Tile::Q], pb[Tile::Q];
    auto fetch = [&](long long k0) {
#pragma unroll
        for (int q = 0; q < Tile::Q; ++q) {
            const long long k = k0 + w + 4 * q;
            pa[q] = (okA && k < n) ? xa[k * nchan] : 0.f;
            pb[q] = (okB && k < n) ? xb[k * nchan] : 0.f;
        }
    };
    fetch(0);
    for (long long k0 = 0; k0 < n; k0 += KC) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < Tile::Q; ++q) {
            const int row = w + 4 * q;
            const bool in = k0 + row < n;
            As[row * LD + lane] = (okA && in) ? (double)pa[q] - ma : 0.0;
            if (!diag) Bs[row * LD + lane] = (okB && in) ? (double)pb[q] - mb : 0.0;
        }
        if (k0 + KC < n) fetch(k0 + KC);
        __syncthreads();
        if (any) {
#pragma unroll
            for (int ks = 0; ks < KC; ks += 4) {
                double a[2], b[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) a[u] = As[(ks + l4) * LD + wr + 16 * u + l15];
#pragma unroll
                for (int v = 0; v < 2; ++v) b[v] = Bs[(ks + l4) * LD + wc + 16 * v + l15];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int v = 0; v < 2; ++v)
                        if (on[u][v]) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[v], acc[u][v], 0, 0, 0);
            }
        }
    }

    float* o = out + trial * nchan * nchan;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            if (!on[u][v]) continue;
            const long long ti = ci0 + wr + 16 * u, tj = cj0 + wc + 16 * v;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long gi = ti + l4 + 4 * r, gj = tj + l15;
                if (gi < nchan && gj < nchan) {
                    const float val = (float)(acc[u][v][r] * scale);
                    o[gi * nchan + gj] = val;
                    if (ti > tj) o[gj * nchan + gi] = val;
                }
            }
        }
}

}  // namespace spycov
