// K12: the envelope correlations - amplitude correlation, power correlation and the orthogonalised power correlation of
// Hipp et al. 2012.  Not in the reference; the definitions.  Over the R = T K repetitions
// r = (trial, taper) of the tapered spectra x_i(r) of one frequency - every taper is a repetition, nothing is summed
// over tapers first - and with
//     corr(X; E1a, E2a, E1b, E2b) = (X - E1a E1b / R) / sqrt(va vb),   va = E2a - E1a^2 / R,  vb = E2b - E1b^2 / R,
//     0 where a variance is zero: v <= 2^-40 E2,
//   amplcorr  (e = |x|)  and  powcorr  (e = |x|^2):   corr(sum e_i e_j; sum e_i, sum e_i^2, sum e_j, sum e_j^2),
//   powcorr_ortho:  p = |x|^2,  s = Im(x_i conj(x_j)),  q_j|i = s^2 / p_i (0 where p_i = 0) the power of j orthogonal to i;
//       p_i q_j|i = s^2, so Z = sum s^2 is the cross moment of both directions,
//       c_j|i = corr(Z; sum p_i, sum p_i^2, sum q_j|i, sum q_j|i^2),   result (c_j|i + c_i|j) / 2, 0 unless both exist.
// The float32 values are |x|, p, 1 / p, s, s^2 and q; every product of two of them and every sum over repetitions is
// float64, so the products are exact and no sum's error grows with R.  A positive scale per channel changes no result.
#pragma once
#include "spy_intrinsics.h"
#include "../../include/spyhip.h"

namespace spyenvcorr {

struct EnvcorrArgs {
    const float2* spec;   // (ntrials * ntaper, F, C) complex64: tapered spectra, rows of a trial adjacent
    int ntrials, ntaper, F, C;
    double* pair;         // (NP, F, C, C) planar: the lower triangle (32 x 32 tile granularity); at [i, j] the one plane
                          // {sum e_i e_j}, or the five {Z, sum q_j|i, sum q_j|i^2, sum q_i|j, sum q_i|j^2}
    double* chan;         // (F, C, 2): {sum e, sum e^2} (amplcorr, powcorr) or {sum p, sum p^2} (powcorr_ortho)
};

// What staging leaves in LDS per channel and repetition, computed once so that no pair recomputes it: the float32 envelope
// as a double (amplcorr, powcorr), or {Re x, Im x, p, 1 / p} with 1 / p = 0 for p = 0 (powcorr_ortho).
template <int M> struct Staged { typedef double type; };
template <> struct Staged<SPYHIP_ENVCORR_POW_ORTHO> { typedef float4 type; };

__device__ __forceinline__ float power(float2 v) { return fmaf(v.x, v.x, v.y * v.y); }

template <int M> __device__ __forceinline__ typename Staged<M>::type staged(float2 v);
template <> __device__ __forceinline__ double staged<SPYHIP_ENVCORR_AMPL>(float2 v) { return (double)sqrtf(power(v)); }
template <> __device__ __forceinline__ double staged<SPYHIP_ENVCORR_POW>(float2 v) { return (double)power(v); }
template <> __device__ __forceinline__ float4 staged<SPYHIP_ENVCORR_POW_ORTHO>(float2 v) {
    const float p = power(v);
    return make_float4(v.x, v.y, p, p > 0.f ? 1.0f / p : 0.f);
}

// the sums of one pair, in registers for the whole launch
template <int M> struct PairSums {
    double x = 0.0;
    __device__ __forceinline__ void add(double ei, double ej) { x = fma(ei, ej, x); }
    __device__ __forceinline__ void flush(double* o, size_t plane) const { *o += x; }
};
template <> struct PairSums<SPYHIP_ENVCORR_POW_ORTHO> {
    double z = 0.0, g1ji = 0.0, g2ji = 0.0, g1ij = 0.0, g2ij = 0.0;
    // xi of the row channel i, (re, im, 1 / p) of the column channel j
    __device__ __forceinline__ void add(float4 xi, float re, float im, float invp) {
        const float s = fmaf(-xi.x, im, xi.y * re);          // Im(xi conj(xj)) = xi.im xj.re - xi.re xj.im
        const float s2 = s * s;
        const double qji = (double)(s2 * xi.w), qij = (double)(s2 * invp);
        z += (double)s2;
        g1ji += qji;
        g2ji = fma(qji, qji, g2ji);
        g1ij += qij;
        g2ij = fma(qij, qij, g2ij);
    }
    __device__ __forceinline__ void flush(double* o, size_t plane) const {
        o[0] += z;
        o[plane] += g1ji;
        o[2 * plane] += g2ji;
        o[3 * plane] += g1ij;
        o[4 * plane] += g2ij;
    }
};

// Tiling and streaming of ppc_accum_kernel (K7) and phaselag_accum_kernel (K10): workgroup = (frequency, 32 x 32 tile of
// the lower triangle), 256 threads, thread (ti, tq) owns the pairs (i = ti, j = 4 tq .. 4 tq + 3); per trial the
// ntaper x 64 staged values of the tile's channels go through LDS, double-buffered.  The loop over tapers does not reduce
// over them: every taper adds to the sums of the 4 pairs, which stay in registers (at most 4 x 5 doubles); one
// read-modify-write of the accumulator per launch.  The diagonal tiles form the per-channel sums.
template <int M>
__global__ void __launch_bounds__(256) envcorr_accum_kernel(EnvcorrArgs a) {
    typedef typename Staged<M>::type elem;
    SPY_DYN_SMEM(elem, ec_lds);
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
    auto stage = [&](int t, elem* dst) {
        if (small) {
            const float2* base = a.spec + (size_t)t * tstride;
#pragma unroll
            for (int n = 0; n < NST; ++n) {
                const int e = tid + 256 * n;
                if (256 * n < per && e < per) dst[e] = staged<M>(sok[n] ? base[soff[n]] : make_float2(0.f, 0.f));
            }
            return;
        }
        for (int e = tid; e < per; e += 256) {
            const int side = e / (K * 32), k = (e - side * K * 32) >> 5, c = e & 31;
            const int ch = (side ? bj : bi) * 32 + c;
            float2 v = make_float2(0.f, 0.f);
            if (ch < a.C) v = a.spec[((size_t)((size_t)t * K + k) * a.F + f) * a.C + ch];
            dst[e] = staged<M>(v);
        }
    };

    PairSums<M> sum[4];
    double c1 = 0.0, c2 = 0.0;                            // the channel sums of i, in the threads tq = 0 of a diagonal tile
    const bool chan_sums = bi == bj && tq == 0;
    stage(0, ec_lds);
    __syncthreads();
    for (int t = 0; t < a.ntrials; ++t) {
        const elem* b = ec_lds + (t & 1) * per;
        if (t + 1 < a.ntrials) stage(t + 1, ec_lds + ((t + 1) & 1) * per);
        for (int k = 0; k < K; ++k) {
            const elem xi = b[k * 32 + ti];
            const elem* pj = b + (K + k) * 32 + tq * 4;
            if constexpr (M == SPYHIP_ENVCORR_POW_ORTHO) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 xj = pj[q];
                    sum[q].add(xi, xj.x, xj.y, xj.w);
                }
                if (chan_sums) {
                    const double p = (double)xi.z;
                    c1 += p;
                    c2 = fma(p, p, c2);
                }
            } else {
                const double2* p2 = reinterpret_cast<const double2*>(pj);
                const double2 j01 = p2[0], j23 = p2[1];
                sum[0].add(xi, j01.x);
                sum[1].add(xi, j01.y);
                sum[2].add(xi, j23.x);
                sum[3].add(xi, j23.y);
                if (chan_sums) {
                    c1 += xi;
                    c2 = fma(xi, xi, c2);
                }
            }
        }
        __syncthreads();
    }
    const int i = bi * 32 + ti;
    if (i >= a.C) return;
    if (chan_sums) {
        double* o = a.chan + ((size_t)f * a.C + i) * 2;
        o[0] += c1;
        o[1] += c2;
    }
    const size_t plane = (size_t)a.F * a.C * a.C;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = bj * 32 + tq * 4 + q;
        if (j >= a.C) continue;
        sum[q].flush(a.pair + ((size_t)f * a.C + i) * a.C + j, plane);
    }
}

// corr of the header, in float64; a variance v of second moment E2 is zero when v <= 2^-40 E2: a channel whose envelope is
// the same float32 value in every repetition leaves a rounding residue of either sign there, not 0
__device__ __forceinline__ bool corr(double X, double E1a, double E2a, double E1b, double E2b, double R, double* r) {
    const double va = E2a - E1a * E1a / R, vb = E2b - E1b * E1b / R;
    if (!(va > 0x1p-40 * E2a) || !(vb > 0x1p-40 * E2b)) { *r = 0.0; return false; }
    *r = (X - E1a * E1b / R) / sqrt(va * vb);
    return true;
}

// out[f, i, j] float32 from the accumulators of R repetitions: element (i, j) with i < j is evaluated from its mirror
// (j, i), so the result is exactly symmetric; the diagonal is exact (amplcorr, powcorr: 1 where the channel's variance is
// not zero, else 0; powcorr_ortho: 0 - Im(x conj x) is a rounding residue at best); clamped to [-1, 1], one rounding.
__global__ void __launch_bounds__(256) envcorr_finalize_kernel(const double* pair, const double* chan, int F, int C, double R,
                                                               int measure, float* out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n = (long long)F * C * C;
    if (idx >= n) return;
    const int c1 = (int)(idx % C), c0 = (int)((idx / C) % C);
    const long long f = idx / ((long long)C * C);
    const int i = c0 > c1 ? c0 : c1, j = c0 > c1 ? c1 : c0;           // the maintained element: i >= j
    const double* ci = chan + (f * C + i) * 2;
    const double* cj = chan + (f * C + j) * 2;
    const double* p = pair + (f * C + i) * C + j;
    double r;
    if (measure != SPYHIP_ENVCORR_POW_ORTHO) {
        const bool ok = corr(p[0], ci[0], ci[1], cj[0], cj[1], R, &r);
        if (i == j) r = ok ? 1.0 : 0.0;
    } else if (i == j) {
        r = 0.0;
    } else {
        double rji, rij;
        const bool ok_ji = corr(p[0], ci[0], ci[1], p[n], p[2 * n], R, &rji);
        const bool ok_ij = corr(p[0], cj[0], cj[1], p[3 * n], p[4 * n], R, &rij);
        r = ok_ji && ok_ij ? 0.5 * (rji + rij) : 0.0;
    }
    out[idx] = (float)fmin(1.0, fmax(-1.0, r));
}

}  // namespace spyenvcorr
