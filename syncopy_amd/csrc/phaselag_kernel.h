// K10: the phase-lag family - phase-lag index (Stam 2007), weighted phase-lag index and its debiased square (Vinck 2011) -
// and the phase-locking value.  Not in the reference; the definitions:
//     S_t = sum_k x_ik conj(x_jk) of trial t,  s_t = Im S_t  (a positive scale such as 1 / K changes no result),
//     A = sum_t s_t,  B = sum_t |s_t|,  Q = sum_t s_t^2,  N = sum_t sign(s_t)  with sign(0) = 0,
//     pli = |N| / T,   wpli = |A| / B  (0 where B = 0),   wpli_debiased = (A^2 - Q) / (B^2 - Q)  (0 where B^2 - Q <= 0),
//     plv = |U| / T  with K7's phasor sum U (ppc_kernel.h).
// All are non-linear in the single-trial cross spectrum, so like K7 the accumulation streams the tapered spectra of
// every trial once and never stores an S_t.  One accumulator of float4 {A, B, Q, N} serves the three measures.
#pragma once
#include "spy_intrinsics.h"
#include "../../include/spyhip.h"

namespace spyphaselag {

struct PhaselagArgs {
    const float2* spec;   // (ntrials * ntaper, F, C) complex64: tapered spectra, rows of a trial adjacent
    int ntrials, ntaper, F, C;
    float4* acc;          // (F, C, C) x {A, B, Q, N}: the lower triangle (32 x 32 tile granularity)
};

// sign(s) with sign(0) = 0 (and 0 for a NaN)
__device__ __forceinline__ float sign0(float s) { return (s > 0.f ? 1.f : 0.f) - (s < 0.f ? 1.f : 0.f); }

__device__ __forceinline__ void add_trial(float4& v, float s) {
    v.x += s;
    v.y += fabsf(s);
    v.z = fmaf(s, s, v.z);
    v.w += sign0(s);
}

// Tiling and streaming of ppc_accum_kernel (K7): workgroup = (frequency, 32 x 32 tile of the lower triangle), 256 threads,
// thread (ti, tq) owns the pairs (i = ti, j = 4 tq .. 4 tq + 3); per trial the ntaper x 64 spectra of the tile's channels
// go through LDS, double-buffered.  Only the imaginary part of the taper sum is formed - two FMAs per pair and taper - and
// the four sums of the 4 pairs stay in registers; one read-modify-write of the accumulator per launch.
__global__ void __launch_bounds__(256) phaselag_accum_kernel(PhaselagArgs a) {
    SPY_DYN_SMEM(float2, pl_lds);
    const int tid = threadIdx.x, ti = tid & 31, tq = tid >> 5;
    const int nt = (a.C + 31) / 32, ntl = nt * (nt + 1) / 2;
    // all tiles of a frequency run on ONE XCD (ids congruent mod 8), as in K7
    const int fchunk = (a.F + 7) >> 3;
    const unsigned yid = blockIdx.x >> 3;
    const int f = (int)(blockIdx.x & 7u) * fchunk + (int)(yid / ntl);
    if ((int)(yid / ntl) >= fchunk || f >= a.F) return;
    int rem = (int)(yid % ntl), bi = 0;
    while (rem >= bi + 1) { rem -= bi + 1; ++bi; }
    const int bj = rem;
    const int K = a.ntaper, per = 2 * K * 32;

    // staging offsets inside a trial are the same for every trial: computed once for up to 4 elements per thread
    // (16 tapers); the generic walk below serves anything larger
    constexpr int NST = 4;
    unsigned soff[NST];
    bool sok[NST];
#pragma unroll
    for (int n = 0; n < NST; ++n) {
        const int e = tid + 256 * n;
        const int side = e / (K * 32), k = (e - side * K * 32) >> 5, c = e & 31;
        const int ch = (side ? bj : bi) * 32 + c;
        sok[n] = e < per && ch < a.C;
        soff[n] = sok[n] ? (unsigned)(((size_t)k * a.F + f) * a.C + ch) : 0u;
    }
    const size_t tstride = (size_t)K * a.F * a.C;
    const bool small = per <= 256 * NST && tstride < (1ull << 31);
    auto stage = [&](int t, float2* dst) {
        if (small) {
            const float2* base = a.spec + (size_t)t * tstride;
#pragma unroll
            for (int n = 0; n < NST; ++n) {
                const int e = tid + 256 * n;
                if (256 * n < per && e < per) dst[e] = sok[n] ? base[soff[n]] : make_float2(0.f, 0.f);
            }
            return;
        }
        for (int e = tid; e < per; e += 256) {
            const int side = e / (K * 32), k = (e - side * K * 32) >> 5, c = e & 31;
            const int ch = (side ? bj : bi) * 32 + c;
            float2 v = make_float2(0.f, 0.f);
            if (ch < a.C) v = a.spec[((size_t)((size_t)t * K + k) * a.F + f) * a.C + ch];
            dst[e] = v;
        }
    };

    float4 sum[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) sum[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    stage(0, pl_lds);
    __syncthreads();
    for (int t = 0; t < a.ntrials; ++t) {
        const float2* b = pl_lds + (t & 1) * per;
        if (t + 1 < a.ntrials) stage(t + 1, pl_lds + ((t + 1) & 1) * per);
        // Im(xi conj(xj)) = xi.im xj.re - xi.re xj.im
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int k = 0; k < K; ++k) {
            const float2 xi = b[k * 32 + ti];
            const float4* pj = reinterpret_cast<const float4*>(b + (K + k) * 32 + tq * 4);
            const float4 j01 = pj[0], j23 = pj[1];
            const float nre = -xi.x;
            s0 = fmaf(xi.y, j01.x, s0);
            s1 = fmaf(xi.y, j01.z, s1);
            s2 = fmaf(xi.y, j23.x, s2);
            s3 = fmaf(xi.y, j23.z, s3);
            s0 = fmaf(nre, j01.y, s0);
            s1 = fmaf(nre, j01.w, s1);
            s2 = fmaf(nre, j23.y, s2);
            s3 = fmaf(nre, j23.w, s3);
        }
        add_trial(sum[0], s0);
        add_trial(sum[1], s1);
        add_trial(sum[2], s2);
        add_trial(sum[3], s3);
        __syncthreads();
    }
    const int i = bi * 32 + ti;
    if (i >= a.C) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = bj * 32 + tq * 4 + q;
        if (j >= a.C) continue;
        float4* o = a.acc + ((size_t)f * a.C + i) * a.C + j;
        float4 v = *o;
        v.x += sum[q].x;
        v.y += sum[q].y;
        v.z += sum[q].z;
        v.w += sum[q].w;
        *o = v;
    }
}

// the same accumulation from single-trial cross spectra that exist already: csd (ntrials, n) -> acc (n) += {A, B, Q, N}
__global__ void __launch_bounds__(256) phaselag_accum_csd_kernel(const float2* csd, long long n, int ntrials, float4* acc) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    float4 v = acc[idx];
    for (int t = 0; t < ntrials; ++t) add_trial(v, csd[(size_t)t * n + idx].y);
    acc[idx] = v;
}

// lower_only: element (i, j) with i < j is read from its mirror (j, i) - A and N change sign there, which no measure sees -
// and the diagonal is exactly 0 (Im(x conj x) is a rounding residue in fused arithmetic: it must not reach 0 / 0).
// float64 throughout, one rounding at the end: A^2 - Q cancels.
__global__ void __launch_bounds__(256) phaselag_finalize_kernel(const float4* acc, int F, int ni, int nj, int lower_only,
                                                                double T, int measure, float* out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n = (long long)F * ni * nj;
    if (idx >= n) return;
    const int j = (int)(idx % nj), i = (int)((idx / nj) % ni);
    const long long f = idx / ((long long)ni * nj);
    if (lower_only && i == j) { out[idx] = 0.f; return; }
    const bool mirror = lower_only && j > i;
    const float4 v = mirror ? acc[(f * ni + j) * nj + i] : acc[idx];
    const double A = v.x, B = v.y, Q = v.z, N = v.w;
    double r;
    if (measure == SPYHIP_PHASELAG_PLI) {
        r = fabs(N) / T;
    } else if (measure == SPYHIP_PHASELAG_WPLI) {
        r = B > 0.0 ? fabs(A) / B : 0.0;
    } else {
        const double den = B * B - Q;
        r = den > 0.0 ? (A * A - Q) / den : 0.0;
    }
    out[idx] = (float)r;
}

// plv[f,i,j] = |U| / T from K7's accumulator (ppc_kernel.h), mirrored as ppc_finalize_kernel mirrors
__global__ void __launch_bounds__(256) plv_finalize_kernel(const float2* acc, int F, int ni, int nj, int lower_only, double T,
                                                           float* out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n = (long long)F * ni * nj;
    if (idx >= n) return;
    const int j = (int)(idx % nj), i = (int)((idx / nj) % ni);
    const long long f = idx / ((long long)ni * nj);
    const bool mirror = lower_only && j > i;
    const float2 u = mirror ? acc[(f * ni + j) * nj + i] : acc[idx];
    out[idx] = (float)(sqrt((double)u.x * u.x + (double)u.y * u.y) / T);
}

}  // namespace spyphaselag
