// Kernels of the synthetic-data generators (synthdata.py): the deterministic part of a trial, assembled on the device
// from random numbers that the host drew.  Every tensor is (ntrials, nsamples, nchan), C-order, so the threads of a
// workgroup, one per channel, load and store consecutive addresses.
//
// AR(2) network (syncopy/synthdata/analog.py: ar2_network), sample i >= 2 of channel c, in the reference's arithmetic:
//     acc  = sum_j M[c][j] * (double)s[i-1][j]       float64, over ascending j, by fma(); M = diag(alpha1) + AdjMat.T
//     lag2 = (float)alpha2 * s[i-2][c]               float32
//     v    = (float)(acc + (double)lag2)
//     s[i][c] = (float)((double)v + noise[i][c])
// and s[0], s[1] are noise[0], noise[1] rounded to float32.  M is never formed: the coupling travels as the CSR table of
// the non-zeros of AdjMat.T (per receiver c its senders j ascending, float32 weights), and alpha1 joins the sum at j = c,
// on top of the table's weight where the table has a diagonal entry.  Every fused product is an explicit fma() and every
// other operation a plain operator under `fp contract(off)` (hipcc contracts a * b + c by default, through HIP's
// __fmul_rn / __fadd_rn too: stats_kernel.h), so the CPU emulation of tests/emu gives the same bits as the device.
//
// ar2_coupled_kernel: one workgroup per trial, one thread per channel.  s[i-1] of all channels is what a thread reads of
// the others: it lies in LDS twice, written by step i into the half that step i-1 read from, so one barrier per step
// orders both the write before the next step's reads and this step's reads before the next step's write.  s[i-2][c] and
// s[i-1][c] of the thread's own channel stay in registers.  The noise does not depend on the state: a thread keeps the
// loads of the next PF steps in flight while it walks the current PF, so no step waits for HBM.  The coupling table is
// copied to LDS behind the state where the route found room (CSR_LDS), else read from global memory (it is the same for
// every step and every workgroup, so it comes from the caches).
//
// ar2_series_kernel: no entry off the diagonal (red_noise, uncoupled networks): one thread per (trial, channel), no LDS,
// no barrier, the same arithmetic with the one term of its row.
//
// phase_kernel (phase_diffusion): one thread per (trial, channel); the running float32 sum of (float)rel_eps * wn[i] in
// sample order is np.cumsum's, the phase (lin[i] + ps0[t][c]) + sum, the output the phase or its cosine.
//
// tile_kernel (harmonic, linear_trend): out[t][i][c] = col[i].
#pragma once
#include <cmath>
#include <cstdint>

#include "synth_route.h"

#pragma clang fp contract(off)

namespace spysyn {

// Plain operators, not HIP's __fmul_rn / __fadd_rn: the names only mark the operations that must round once, and it is
// the pragma above that keeps the compiler from fusing them.
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

constexpr int PF = 8;           // loads a thread keeps in flight ahead of the steps it walks

struct Ar2Args {
    const double* noise;        // (ntrials, nsamples, nchan)
    const int* rowptr;          // (nchan + 1)
    const int* col;             // (nnz) senders
    const float* w;             // (nnz) weights
    float* out;                 // (ntrials, nsamples, nchan)
    double alpha1;
    float alpha2;
    long long nsamples;
    int nchan, nnz;
};

// what follows the sum over the senders
__device__ __forceinline__ float ar2_finish(double acc, float alpha2, float s2, double noise) {
    const float lag2 = mul_rn(alpha2, s2);
    const float v = (float)(acc + (double)lag2);
    return (float)((double)v + noise);
}

template <bool CSR_LDS>
__global__ __launch_bounds__(MAX_CHAN) void ar2_coupled_kernel(const Ar2Args g) {
    SPY_DYN_SMEM(float, state);                                 // [2][nchan], then the table where CSR_LDS
    const int c = threadIdx.x, nchan = g.nchan;
    const bool live = c < nchan;
    const long long n = g.nsamples;
    const int* rowptr = g.rowptr;
    const int* col = g.col;
    const float* w = g.w;
    if (CSR_LDS) {
        int* lr = reinterpret_cast<int*>(state + 2 * nchan);
        int* lc = lr + nchan + 1;
        float* lw = reinterpret_cast<float*>(lc + g.nnz);
        for (int k = threadIdx.x; k <= nchan; k += blockDim.x) lr[k] = g.rowptr[k];
        for (int k = threadIdx.x; k < g.nnz; k += blockDim.x) { lc[k] = g.col[k]; lw[k] = g.w[k]; }
        rowptr = lr; col = lc; w = lw;
    }
    const long long base = (long long)blockIdx.x * n * nchan + c;
    const double* nz = g.noise + base;
    float* out = g.out + base;
    float s1 = 0.0f, s2 = 0.0f;
    if (live) {
        s2 = (float)nz[0];
        s1 = (float)nz[nchan];
        out[0] = s2;
        out[nchan] = s1;
        state[nchan + c] = s1;                                  // s[1] lies in half 1
    }
    __syncthreads();
    const int r0 = live ? rowptr[c] : 0, r1 = live ? rowptr[c + 1] : 0;

    double nxt[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) nxt[u] = (live && 2 + u < n) ? nz[(2 + u) * (long long)nchan] : 0.0;
    for (long long b = 2; b < n; b += PF) {
        double cur[PF];
#pragma unroll
        for (int u = 0; u < PF; ++u) cur[u] = nxt[u];
#pragma unroll
        for (int u = 0; u < PF; ++u) nxt[u] = (live && b + PF + u < n) ? nz[(b + PF + u) * nchan] : 0.0;
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const long long i = b + u;
            if (i < n) {                                        // (the same for every thread)
                if (live) {
                    const float* prev = state + ((i - 1) & 1) * nchan;
                    double acc = 0.0;
                    bool diag = false;
                    for (int k = r0; k < r1; ++k) {
                        const int j = col[k];
                        double m = (double)w[k];
                        if (!diag && j >= c) {
                            diag = true;
                            if (j == c) m = g.alpha1 + m;
                            else acc = fma(g.alpha1, (double)s1, acc);
                        }
                        acc = fma(m, (double)prev[j], acc);
                    }
                    if (!diag) acc = fma(g.alpha1, (double)s1, acc);
                    const float o = ar2_finish(acc, g.alpha2, s2, cur[u]);
                    out[i * nchan] = o;
                    state[(i & 1) * nchan + c] = o;
                    s2 = s1;
                    s1 = o;
                }
                __syncthreads();
            }
        }
    }
}

__global__ __launch_bounds__(SERIES_THREADS) void ar2_series_kernel(const Ar2Args g, long long nseries) {
    const long long s = (long long)blockIdx.x * SERIES_THREADS + threadIdx.x;
    if (s >= nseries) return;
    const int nchan = g.nchan;
    const long long n = g.nsamples, t = s / nchan;
    const int c = (int)(s - t * nchan);
    const int r0 = g.rowptr[c];
    const double m = g.rowptr[c + 1] > r0 ? g.alpha1 + (double)g.w[r0] : g.alpha1;
    const long long base = t * n * nchan + c;
    const double* nz = g.noise + base;
    float* out = g.out + base;
    float s2 = (float)nz[0], s1 = (float)nz[nchan];
    out[0] = s2;
    out[nchan] = s1;
    double nxt[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) nxt[u] = 2 + u < n ? nz[(2 + u) * (long long)nchan] : 0.0;
    for (long long b = 2; b < n; b += PF) {
        double cur[PF];
#pragma unroll
        for (int u = 0; u < PF; ++u) cur[u] = nxt[u];
#pragma unroll
        for (int u = 0; u < PF; ++u) nxt[u] = b + PF + u < n ? nz[(b + PF + u) * nchan] : 0.0;
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const long long i = b + u;
            if (i < n) {
                const float o = ar2_finish(fma(m, (double)s1, 0.0), g.alpha2, s2, cur[u]);
                out[i * nchan] = o;
                s2 = s1;
                s1 = o;
            }
        }
    }
}

struct PhaseArgs {
    const float* wn;            // (ntrials, nsamples, nchan) white noise
    const float* lin;           // (nsamples) omega0 * tvec
    const float* ps0;           // (ntrials, nchan) initial phases
    float* out;
    float rel_eps;
    long long nsamples, nseries;
    int nchan, want_cos;
};

__global__ __launch_bounds__(SERIES_THREADS) void phase_kernel(const PhaseArgs g) {
    const long long s = (long long)blockIdx.x * SERIES_THREADS + threadIdx.x;
    if (s >= g.nseries) return;
    const int nchan = g.nchan;
    const long long n = g.nsamples, t = s / nchan;
    const int c = (int)(s - t * nchan);
    const long long base = t * n * nchan + c;
    const float* wn = g.wn + base;
    float* out = g.out + base;
    const float p0 = g.ps0[s];
    float sum = 0.0f;
    float nxt[PF], lnx[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        nxt[u] = u < n ? wn[u * (long long)nchan] : 0.0f;
        lnx[u] = u < n ? g.lin[u] : 0.0f;
    }
    for (long long b = 0; b < n; b += PF) {
        float cur[PF], lcu[PF];
#pragma unroll
        for (int u = 0; u < PF; ++u) { cur[u] = nxt[u]; lcu[u] = lnx[u]; }
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const long long i = b + PF + u;
            nxt[u] = i < n ? wn[i * nchan] : 0.0f;
            lnx[u] = i < n ? g.lin[i] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const long long i = b + u;
            if (i < n) {
                const float incr = mul_rn(g.rel_eps, cur[u]);
                sum = i == 0 ? incr : add_rn(sum, incr);
                const float phase = add_rn(add_rn(lcu[u], p0), sum);
                out[i * nchan] = g.want_cos ? cosf(phase) : phase;
            }
        }
    }
}

struct Lane4 { float v; };
struct alignas(16) Lane16 { float v[4]; };

__device__ __forceinline__ Lane4 spread(float v, Lane4*) { return Lane4{v}; }
__device__ __forceinline__ Lane16 spread(float v, Lane16*) { return Lane16{{v, v, v, v}}; }

// a / b for 0 <= a, 0 < b: the 32-bit division where both fit
__device__ __forceinline__ long long idiv(long long a, long long b) {
    if ((((unsigned long long)a | (unsigned long long)b) >> 32) == 0) return (long long)((unsigned)a / (unsigned)b);
    return a / b;
}

// wl: lanes of a row of channels; lanes: ntrials * nsamples * wl
template <class L>
__global__ __launch_bounds__(TILE_THREADS) void tile_kernel(const float* __restrict__ col, long long nsamples, long long wl,
                                                            long long lanes, L* __restrict__ out) {
    const long long step = (long long)gridDim.x * TILE_THREADS;
    for (long long it = (long long)blockIdx.x * TILE_THREADS + threadIdx.x; it < lanes; it += step) {
        const long long row = idiv(it, wl);
        const long long i = row - idiv(row, nsamples) * nsamples;
        out[it] = spread(col[i], (L*)nullptr);
    }
}

}  // namespace spysyn
