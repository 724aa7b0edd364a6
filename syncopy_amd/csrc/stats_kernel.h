// Summary statistics of spy.var / spy.std / spy.median / spy.itc (statistics/summary_stats.py:156-205, 321-486;
// statistics/compRoutines.py:22-141).  Kept in a header so that the CPU emulation of the tests compiles the same
// kernels; the launchers live in stats.hip.
//
// Every step that claims the reference's rounding is a single IEEE operation: no float atomics, and no FMA.  hipcc
// contracts a*b+c into an FMA by default, and HIP's __fmul_rn / __fadd_rn come from device-library code that allows it
// too (a __fmul_rn followed by a __fadd_rn compiles to v_fmac_f32), so products that feed sums here are plain operators
// under `fp contract(off)`: mul_rn / add_rn / sub_rn.  Every result is reproducible bit for bit from run to run.
#pragma once
#include "np_sum.h"

#pragma clang fp contract(off)

namespace spystat {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
// correctly rounded float32 sqrt (np.sqrt): through float64, exact enough that the one rounding to float32 is the right
// one (53 >= 2 * 24 + 2); __fsqrt_rn may lower to the hardware's approximate v_sqrt_f32
__device__ __forceinline__ float sqrt_rn(float a) { return (float)__dsqrt_rn((double)a); }

constexpr int TRIAL_UNROLL = 4;           // trials whose loads are issued ahead of the (sequential) dependent adds
constexpr int MED_THREADS = 256;          // workgroup of the median kernel
constexpr int MED_STAGE_BYTES = 32768;    // LDS that holds one slice's keys: 8192 float32 / 4096 complex64 elements
constexpr long long MED_SHORT = 600;      // np.nanmedian takes its masked-array branch below this axis length

// |z| correctly rounded (glibc's hypotf): both products are exact in float64, so a contracted FMA rounds the same sum
__device__ __forceinline__ float cabs_rn(float re, float im) {
    return (float)__dsqrt_rn((double)re * (double)re + (double)im * (double)im);
}

// ---- trial moments: dim="trials" (summary_stats.py:321-456) -------------------------------------------------------
// acc[i] += in[0, i] + in[1, i] + ... in trial order (the `out += trl` loop of _trial_average); n floats (complex64:
// the interleaved components).  acc is float32 between calls, so streaming the trials in chunks gives the same bits.
__global__ void trial_sum_kernel(const float* __restrict__ in, float* __restrict__ acc, long long ntrials, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float s = acc[i];
        long long t = 0;
        for (; t + TRIAL_UNROLL <= ntrials; t += TRIAL_UNROLL) {
            float v[TRIAL_UNROLL];
            for (int u = 0; u < TRIAL_UNROLL; ++u) v[u] = in[(t + u) * n + i];
            for (int u = 0; u < TRIAL_UNROLL; ++u) s = add_rn(s, v[u]);
        }
        for (; t < ntrials; ++t) s = add_rn(s, in[t * n + i]);
        acc[i] = s;
    }
}

// out = acc / T: float32 divides by the count; complex64 multiplies by the float32 reciprocal (NumPy's Smith division
// by a real divisor, as trial_mean_kernel in api.hip).  out may alias acc.
template <bool RECIP>
__global__ void trial_scale_kernel(const float* acc, float* out, long long ntotal, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const float scl = __fdiv_rn(1.0f, (float)ntotal);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = RECIP ? mul_rn(acc[i], scl) : __fdiv_rn(acc[i], (float)ntotal);
}

// fl(|x - mean|)^2 of one element (_trial_var: np.abs(trl - average) ** 2 in the data's dtype)
template <bool CPLX>
__device__ __forceinline__ float sqdev(const float* x, const float* mean, long long i) {
    if (CPLX) {
        const float a = cabs_rn(sub_rn(x[2 * i], mean[2 * i]), sub_rn(x[2 * i + 1], mean[2 * i + 1]));
        return mul_rn(a, a);
    }
    const float a = fabsf(sub_rn(x[i], mean[i]));
    return mul_rn(a, a);
}

// acc[i] += sum over the chunk's trials of fl(|x - mean|)^2, in trial order; n elements, acc is real
template <bool CPLX>
__global__ void trial_sqdev_kernel(const float* __restrict__ in, const float* __restrict__ mean, float* __restrict__ acc,
                                   long long ntrials, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long tstep = CPLX ? 2 * n : n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float s = acc[i];
        long long t = 0;
        for (; t + TRIAL_UNROLL <= ntrials; t += TRIAL_UNROLL) {
            float v[TRIAL_UNROLL];
            for (int u = 0; u < TRIAL_UNROLL; ++u) v[u] = sqdev<CPLX>(in + (t + u) * tstep, mean, i);
            for (int u = 0; u < TRIAL_UNROLL; ++u) s = add_rn(s, v[u]);
        }
        for (; t < ntrials; ++t) s = add_rn(s, sqdev<CPLX>(in + t * tstep, mean, i));
        acc[i] = s;
    }
}

// out = acc / T (complex64: times fl(1/T), imaginary part 0), then np.sqrt for std.  np.sqrt of the complex (v, +0) is
// (sqrt(v), +0) except for a NaN v, where C99's csqrt gives (NaN, NaN).
template <bool CPLX, bool SQRT>
__global__ void trial_var_finalize_kernel(const float* __restrict__ acc, float* __restrict__ out, long long ntotal,
                                          long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const float scl = __fdiv_rn(1.0f, (float)ntotal);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (CPLX) {
            float v = mul_rn(acc[i], scl);
            float im = 0.f;
            if (SQRT) {
                im = (v != v) ? v : 0.f;
                v = sqrt_rn(v);
            }
            out[2 * i] = v;
            out[2 * i + 1] = im;
        } else {
            const float v = __fdiv_rn(acc[i], (float)ntotal);
            out[i] = SQRT ? sqrt_rn(v) : v;
        }
    }
}

// ---- inter-trial coherence (summary_stats.py:364-377, 459-486) ----------------------------------------------------
// trl / np.abs(trl): NumPy's Smith division by the real divisor (r, 0) - rat = 0, scl = fl(1/r), out = ((re + im*0)*scl,
// (im - re*0)*scl).  Kept literally so that z = 0 (0 * inf) and non-finite z (inf * 0, NaN) give NaN in both parts.
__device__ __forceinline__ float2 unit_phasor(float re, float im) {
    const float scl = __fdiv_rn(1.0f, cabs_rn(re, im));
    return make_float2(mul_rn(add_rn(re, mul_rn(im, 0.f)), scl),
                       mul_rn(sub_rn(im, mul_rn(re, 0.f)), scl));
}

// acc[i] += sum over the chunk's trials of z / |z|, in trial order (complex64, n elements)
__global__ void itc_accum_kernel(const float2* __restrict__ in, float2* __restrict__ acc, long long ntrials, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float2 s = acc[i];
        long long t = 0;
        for (; t + TRIAL_UNROLL <= ntrials; t += TRIAL_UNROLL) {
            float2 v[TRIAL_UNROLL];
            for (int u = 0; u < TRIAL_UNROLL; ++u) v[u] = in[(t + u) * n + i];
            for (int u = 0; u < TRIAL_UNROLL; ++u) {
                const float2 p = unit_phasor(v[u].x, v[u].y);
                s.x = add_rn(s.x, p.x);
                s.y = add_rn(s.y, p.y);
            }
        }
        for (; t < ntrials; ++t) {
            const float2 z = in[t * n + i];
            const float2 p = unit_phasor(z.x, z.y);
            s.x = add_rn(s.x, p.x);
            s.y = add_rn(s.y, p.y);
        }
        acc[i] = s;
    }
}

// acc (outer, ntaper, inner) complex64 -> out (outer, inner) float32: `/= T` (times fl(1/T)), np.mean over the tapers
// (sequential sum, then the division by NumPy's intp count - a complex128 Smith division: times 1.0/K in float64),
// np.abs correctly rounded
__global__ void itc_finalize_kernel(const float2* __restrict__ acc, float* __restrict__ out, long long ntotal,
                                    long long outer, long long ntaper, long long inner) {
    const long long tot = outer * inner, stride = (long long)gridDim.x * blockDim.x;
    const float scl = __fdiv_rn(1.0f, (float)ntotal);
    const double rk = 1.0 / (double)ntaper;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += stride) {
        const long long o = e / inner, i = e - o * inner;
        float sr = 0.f, si = 0.f;
        for (long long k = 0; k < ntaper; ++k) {
            const float2 a = acc[(o * ntaper + k) * inner + i];
            const float ar = mul_rn(a.x, scl), ai = mul_rn(a.y, scl);
            sr = k ? add_rn(sr, ar) : ar;
            si = k ? add_rn(si, ai) : ai;
        }
        out[e] = cabs_rn((float)((double)sr * rk), (float)((double)si * rk));
    }
}

// ---- np.nanvar / np.nanstd along one axis (compRoutines.py:22-57 with operation "var" / "std", ddof 0) -------------
// NumPy's pairwise_sum_FLOAT over get(0) ... get(n-1): the order of np_pairwise_sum for values that are computed
template <class F>
__device__ float np_pairwise_sum_of(const F& get, long long lo, long long n) {
    if (n < 8) {
        float res = 0.f;
        for (long long i = 0; i < n; ++i) res = add_rn(res, get(lo + i));
        return res;
    }
    if (n <= 128) {
        float r[8];
        for (int j = 0; j < 8; ++j) r[j] = get(lo + j);
        long long i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] = add_rn(r[j], get(lo + i + j));
        float res = add_rn(add_rn(add_rn(r[0], r[1]), add_rn(r[2], r[3])),
                              add_rn(add_rn(r[4], r[5]), add_rn(r[6], r[7])));
        for (; i < n; ++i) res = add_rn(res, get(lo + i));
        return res;
    }
    long long n2 = n / 2;
    n2 -= n2 % 8;
    return add_rn(np_pairwise_sum_of(get, lo, n2), np_pairwise_sum_of(get, lo + n2, n - n2));
}

// x (outer, n, inner) float32 / complex64 -> out (outer, inner) float32 / complex64 (imaginary part 0: the reference
// writes the real result into an array of the input's dtype).  np.nanvar: count, NaN-free sum in the order of
// axis_nanmean_kernel (rows in order / pairwise along the last axis), mean by the count in float64 (complex: a
// complex128 Smith division, times 1.0/cnt), then the sum of d*d (complex: re*re + im*im, the real part of
// arr * arr.conj()) in the same order - pairwise along the last axis, over the stride-2 real view for complex - divided
// by the count in float64; np.nanstd takes the float32 sqrt.  An all-NaN slice gives NaN.
template <bool CPLX, bool SQRT>
__global__ void axis_nanvar_kernel(const float* __restrict__ x, long long outer, long long n, long long inner,
                                   float* __restrict__ out) {
    const long long tot = outer * inner, stride = (long long)gridDim.x * blockDim.x;
    const long long es = CPLX ? 2 : 1;              // floats per element
    const long long st = inner * es;                // floats between consecutive elements of a slice
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += stride) {
        const long long o = e / inner, i = e - o * inner;
        const float* p = x + (o * n * inner + i) * es;
        auto bad = [&](long long k) {
            const float v = p[k * st];
            return CPLX ? ((v != v) || (p[k * st + 1] != p[k * st + 1])) : (v != v);
        };
        long long cnt = 0;
        for (long long k = 0; k < n; ++k) cnt += bad(k) ? 0 : 1;
        float sr = 0.f, si = 0.f;
        if (inner == 1) {
            if (CPLX) {
                sr = np_pairwise_sum_c(p, n, 1);
                si = np_pairwise_sum_c(p + 1, n, -1);
            } else {
                sr = np_pairwise_sum(p, n);
            }
        } else {
            for (long long k = 0; k < n; ++k) {
                const bool b = bad(k);
                sr = add_rn(sr, b ? 0.f : p[k * st]);
                if (CPLX) si = add_rn(si, b ? 0.f : p[k * st + 1]);
            }
        }
        float mr, mi = 0.f;
        if (CPLX) {
            const double rc = 1.0 / (double)cnt;
            mr = (float)((double)sr * rc);
            mi = (float)((double)si * rc);
        } else {
            mr = (float)((double)sr / (double)cnt);
        }
        auto sq = [&](long long k) {
            if (bad(k)) return 0.f;
            const float dr = sub_rn(p[k * st], mr);
            if (!CPLX) return mul_rn(dr, dr);
            const float di = sub_rn(p[k * st + 1], mi);
            return add_rn(mul_rn(dr, dr), mul_rn(di, di));
        };
        float ss;
        if (inner == 1) {
            ss = np_pairwise_sum_of(sq, 0, n);
        } else {
            ss = 0.f;
            for (long long k = 0; k < n; ++k) ss = add_rn(ss, sq(k));
        }
        float v = (float)((double)ss / (double)cnt);
        if (SQRT) v = sqrt_rn(v);
        if (CPLX) {
            out[2 * e] = v;
            out[2 * e + 1] = 0.f;
        } else {
            out[e] = v;
        }
    }
}

// ---- np.nanmedian along one axis ----------------------------------------------------------------------------------
// (outer, n, inner) -> (outer, inner, n), 32 x 32 tiles through LDS, so that every slice of the median is contiguous.
// E = float (float32) or float2 (complex64); 256 threads.
template <typename E>
__global__ void axis_transpose_kernel(const E* __restrict__ in, E* __restrict__ out, long long outer, long long n,
                                      long long inner) {
    __shared__ E tile[32][33];
    const long long tn = (n + 31) / 32, ti = (inner + 31) / 32, ntile = outer * tn * ti;
    const int tx = (int)(threadIdx.x & 31), ty = (int)(threadIdx.x >> 5), rows = (int)(blockDim.x >> 5);
    for (long long b = blockIdx.x; b < ntile; b += gridDim.x) {
        const long long o = b / (tn * ti), rem = b - o * tn * ti, bn = rem / ti, bi = rem - bn * ti;
        for (int r = ty; r < 32; r += rows) {
            const long long k = bn * 32 + r, i = bi * 32 + tx;
            if (k < n && i < inner) tile[r][tx] = in[(o * n + k) * inner + i];
        }
        __syncthreads();
        for (int r = ty; r < 32; r += rows) {
            const long long i = bi * 32 + r, k = bn * 32 + tx;
            if (k < n && i < inner) out[(o * inner + i) * n + k] = tile[tx][r];
        }
        __syncthreads();
    }
}

// order-preserving keys: float32 -> uint32 (negatives: all bits flipped; others: sign bit set); complex64 -> uint64
// (real part's key, then the imaginary part's: NumPy's lexicographic order).  NaN elements get the all-ones key, above
// every other key, so that ranks below the NaN-free count never see them.  -0 takes the key of +0: NumPy's comparisons
// see them as equal, so a complex tie in the real part between them is decided by the imaginary part.
__device__ __forceinline__ unsigned f32_key(float f) {
    const unsigned u = (f == 0.f) ? 0u : __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

template <bool CPLX>
struct MedKey;
template <>
struct MedKey<false> {
    typedef unsigned T;
    static __device__ __forceinline__ T of(const float* s, long long k) {
        const float v = s[k];
        return (v != v) ? ~0u : f32_key(v);
    }
};
template <>
struct MedKey<true> {
    typedef unsigned long long T;
    static __device__ __forceinline__ T of(const float* s, long long k) {
        const float re = s[2 * k], im = s[2 * k + 1];
        if ((re != re) || (im != im)) return ~0ull;
        return ((T)f32_key(re) << 32) | (T)f32_key(im);
    }
};

// slices (nslice, n) contiguous -> out (nslice) elements.  One workgroup per slice (power-of-two blockDim <= 256):
// count the NaNs, then an MSB-first radix select with 8-bit digits of rank (m-1)/2 among the m NaN-free keys
// (histograms in LDS, integer LDS atomics); for even m the upper middle is the same key when enough equal keys remain,
// otherwise the smallest key above it.  The result is fl(a + b) / 2 per component (exact halving; an odd count has
// b = a) as np.nanmedian forms it, down to its infinities and all-NaN slices.  The keys sit in LDS when the slice fits.
template <bool CPLX>
__global__ void axis_nanmedian_kernel(const float* __restrict__ x, long long nslice, long long n,
                                      float* __restrict__ out) {
    typedef typename MedKey<CPLX>::T K;
    constexpr long long STAGE = MED_STAGE_BYTES / (long long)sizeof(K);
    constexpr int DIGITS = (int)sizeof(K);
    const K NANKEY = ~(K)0;
    __shared__ K stage[STAGE];
    __shared__ unsigned hist[256];
    __shared__ K red[MED_THREADS];
    __shared__ long long s_below;
    __shared__ unsigned s_digit, s_count;
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const bool staged = n <= STAGE;
    for (long long sl = blockIdx.x; sl < nslice; sl += gridDim.x) {
        const float* s = x + sl * n * (CPLX ? 2 : 1);
        // NaN count (the staged keys are written on the way)
        K nn = 0;
        for (long long k = tid; k < n; k += nt) {
            const K kk = MedKey<CPLX>::of(s, k);
            if (staged) stage[k] = kk;
            nn += (kk == NANKEY) ? 1 : 0;
        }
        red[tid] = nn;
        __syncthreads();
        for (int h = nt / 2; h > 0; h >>= 1) {
            if (tid < h) red[tid] += red[tid + h];
            __syncthreads();
        }
        const long long m = n - (long long)red[0];
        __syncthreads();
        float* o = out + sl * (CPLX ? 2 : 1);
        if (m == 0) {                                   // all-NaN slice: the masked branch gives NaN (complex: (NaN, 0)),
            if (tid == 0) {                             // the long branch the slice's last element
                o[0] = (n < MED_SHORT) ? __uint_as_float(0x7fc00000u) : s[CPLX ? 2 * n - 2 : n - 1];
                if (CPLX) o[1] = (n < MED_SHORT) ? 0.f : s[2 * n - 1];
            }
            continue;
        }
        long long r = (m - 1) / 2;                      // rank of the lower middle among the keys
        K prefix = 0, pmask = 0;
        unsigned cnt = 0;
        for (int d = DIGITS - 1; d >= 0; --d) {
            const int sh = 8 * d;
            for (int j = tid; j < 256; j += nt) hist[j] = 0;
            __syncthreads();
            for (long long k = tid; k < n; k += nt) {
                const K kk = staged ? stage[k] : MedKey<CPLX>::of(s, k);
                if ((kk & pmask) == prefix) atomicAdd(&hist[(unsigned)(kk >> sh) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                long long below = 0;
                unsigned b = 0;
                for (; b < 255u; ++b) {
                    if (below + (long long)hist[b] > r) break;
                    below += hist[b];
                }
                s_digit = b;
                s_below = below;
                s_count = hist[b];
            }
            __syncthreads();
            prefix |= (K)s_digit << sh;
            pmask |= (K)255 << sh;
            r -= s_below;
            cnt = s_count;
            __syncthreads();
        }
        const K a = prefix;
        K b = a;
        if ((m & 1) == 0 && (unsigned long long)(r + 1) >= (unsigned long long)cnt) {
            K mn = NANKEY;                              // the smallest key above a (NaN-free: rank m/2 < m exists)
            for (long long k = tid; k < n; k += nt) {
                const K kk = staged ? stage[k] : MedKey<CPLX>::of(s, k);
                if (kk > a && kk < mn) mn = kk;
            }
            red[tid] = mn;
            __syncthreads();
            for (int h = nt / 2; h > 0; h >>= 1) {
                if (tid < h && red[tid + h] < red[tid]) red[tid] = red[tid + h];
                __syncthreads();
            }
            b = red[0];
            __syncthreads();
        }
        if (tid == 0) {
            // NumPy's (low + high) / 2: the masked branch doubles the middle element of an odd count and halves it; the
            // long branch divides the single middle element by 1.  Complex: a Smith division by the real divisor
            // ((re + im*0) * h, (im - re*0) * h), so an infinite component turns the other one into NaN.
            const bool one = (m & 1) && n >= MED_SHORT;
            const float h = one ? 1.0f : 0.5f;
            if (CPLX) {
                const float ar = f32_unkey((unsigned)(a >> 32)), ai = f32_unkey((unsigned)a);
                const float br = f32_unkey((unsigned)(b >> 32)), bi = f32_unkey((unsigned)b);
                const float sr = one ? ar : add_rn(ar, br), si = one ? ai : add_rn(ai, bi);
                o[0] = mul_rn(add_rn(sr, mul_rn(si, 0.f)), h);
                o[1] = mul_rn(sub_rn(si, mul_rn(sr, 0.f)), h);
            } else {
                const float fa = f32_unkey((unsigned)a), fb = f32_unkey((unsigned)b);
                o[0] = one ? fa : mul_rn(add_rn(fa, fb), 0.5f);
            }
        }
        __syncthreads();                                // stage[] and red[] are reused by the next slice
    }
}

}  // namespace spystat
