// The Hilbert option of spy.preprocessing: analytic signal of every channel of a batch of equal-length trials,
// scipy.signal.hilbert(trial, axis=0) followed by spectralConversions[output] (preproc/compRoutines.py:365-417 of the
// reference), circular over the trial length N with no padding.  Families and lengths: hilbert_route.h.
//
// Two real channels travel as one complex sequence z = x_a + i x_b.  The Hilbert transform H is linear, so
//     ifft(h fft(z)) = (x_a - H[x_b]) + i (H[x_a] + x_b):
// one forward and one inverse transform serve two channels and no k <-> N - k exchange separates them; the real part of
// a channel's analytic signal is its input, bit for bit, and H[x_a] = Im(...) - x_b, H[x_b] = x_a - Re(...).  The
// float32 families remove each channel's mean first (H[const] = 0: exact, and it takes the DC term out of the error).
// The inverse transform is conj -> forward -> conj, and the weight h[k] / N is applied between the two.
//
// NaN contract: a non-finite sample (NaN or +-inf) is replaced by zero where it is loaded, so that the channels packed
// with it see an ordinary sequence; its own channel is overwritten with NaN at the store and the trial's flag is raised.
#pragma once
#include "../../include/spyhip.h"
#include "spy_intrinsics.h"
#include "fft2_device.h"
#include "cd_math.h"
#include "f64_stockham.h"
#include "hilbert_route.h"

namespace spyhil {

using spyfft::C2;
using spyfft::Cfg2;
using spyfft::v2f;

struct HilArgs {
    const float* in;        // (ntrials, nsamp, nchan)
    void* out;              // the same shape, float32 or complex64
    int* nan;               // one flag per trial
    int ntrials, nsamp, nchan;
    int kind;               // SPYHIP_OUT_* of the real outputs
    int npg, S, ncl;        // PackedGrid
    const float2* tw;       // exp(-2 pi i m / M)
    const float2* chirp;    // BLUE: exp(-i pi n^2 / N), n < N
    const float2* bhat;     // BLUE: FFT_M of the wrapped conjugate chirp, / M
    float inv_n;            // 1 / N
};

struct HilArgs64 {
    const float* in;
    void* out;
    int* nan;
    int ntrials, nsamp, nchan, kind;
    long long wg0;          // first (trial, channel pair) of this launch
    int blue;               // Bluestein's form: plan.L = M >= 2 N - 1
    spywil::PlusPlan plan;
    const double2* tw;      // exp(-2 pi i m / plan.L)
    const double2* chirp;
    const double2* bhat;
    double2* work;          // two arrays of plan.L per workgroup of the launch
};

__device__ __forceinline__ bool nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ float quiet_nan() { return __int_as_float(0x7fc00000); }

// spectralConversions of the reference (shared/const_def.py:25-37); `kind` is wave-uniform
__device__ __forceinline__ float convert(float re, float im, int kind) {
    switch (kind) {
        case SPYHIP_OUT_REAL: return re;
        case SPYHIP_OUT_IMAG: return im;
        case SPYHIP_OUT_ANGLE: return atan2f(im, re);
        case SPYHIP_OUT_ABSREAL: return fabsf(re);
        case SPYHIP_OUT_ABSIMAG: return fabsf(im);
        default: return sqrtf(re * re + im * im);
    }
}

// h[k] / N as a float
__device__ __forceinline__ float weight(int k, int N, float inv_n) {
    const float one = (k == 0 || 2 * k == N) ? inv_n : 0.f;
    return (k > 0 && 2 * k < N) ? 2.f * inv_n : one;
}

// PACKED (BLUE = false): N = 2^LOG2N.  BLUE: N < M = 2^LOG2N, chirp-z in both directions; with c[n] = exp(-i pi n^2 / N),
// conv(u) = IFFT_M(FFT_M(u) Bhat) and w = h / N:
//     Z = c conv(x c),   y = conj(c conv(conj(Z w) c)) = conj(c) conj(conv(conj(conv(x c)) w))
// (|c| = 1 cancels the two chirp products around the weight), four forward transforms of the engine in all.
// A thread slot carries the channel quad (c0 .. c3) as r = (c0, c1), i = (c2, c3), as in the tapered-FFT kernels.
template <int LOG2N, int G, bool BLUE, bool CPLX>
__global__ void __launch_bounds__((Cfg2<LOG2N, G>::NTHREADS)) hilbert_packed_kernel(HilArgs a) {
    using C = Cfg2<LOG2N, G>;
    static_assert(C::LDS_BYTES == route_detail::packed_lds(LOG2N, G), "hilbert_route.h sizes the LDS of this engine");
    constexpr int T = C::T;
    SPY_DYN_SMEM(v2f, lds);

    const int tid = threadIdx.x;
    const int h = tid % G, j0 = tid / G;
    const int N = a.nsamp;

    // XCD-aware block -> (trial, quad group): the S workgroups that share 128-byte lines of the (time x channel) rows get
    // ids congruent mod 8 (same XCD / L2) and adjacent in dispatch order; each XCD walks a contiguous run of clusters
    const long long id = blockIdx.x;
    const int xcd = (int)(id & 7);
    const long long y = id >> 3;
    const long long nclt = (long long)a.ntrials * a.ncl, chunk = (nclt + 7) >> 3;
    const long long cidx = (long long)xcd * chunk + y / a.S;
    const int q = (int)(y % a.S);
    if (cidx >= nclt) return;
    const int b = (int)(cidx / a.ncl);
    const int pg = (int)(cidx % a.ncl) * a.S + q;
    if (pg >= a.npg) return;

    const int c0 = 4 * (pg * G + h);
    bool has[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) has[i] = c0 + i < a.nchan;
    const bool full = has[3];
    const unsigned rowb = (unsigned)a.nchan * 4u;                      // bytes per input row
    const size_t trial = (size_t)b * (size_t)N * (size_t)a.nchan;      // elements ahead of this trial
    const float* seg = a.in + trial;                                   // wave-uniform
    const bool quad_rows = full && (a.nchan & 3) == 0;

    // ---- load the trial: v[e] = sample n = j + T*e (rows beyond N: zero); non-finite samples are counted and zeroed
    C2 v[16];
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const bool vec4 = quad_rows && ((reinterpret_cast<size_t>(a.in) & 15) == 0);
    auto load_row = [&](int n, float (&u)[4]) {      // the four channels of row n < N, non-finite or absent ones as zero
        if (vec4) {
            const float4 t = spyfft::ldg<float4>(seg, (unsigned)n * rowb + (unsigned)c0 * 4u);
            u[0] = t.x; u[1] = t.y; u[2] = t.z; u[3] = t.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                u[i] = spyfft::ldg<float>(seg, (unsigned)n * rowb + (unsigned)(has[i] ? c0 + i : 0) * 4u);
        }
    };
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int n = j0 + T * e;
        const bool in = !BLUE || n < N;
        float u[4];
        load_row(in ? n : N - 1, u);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool use = in && has[i];
            const bool bad = use && nonfinite(u[i]);
            u[i] = (use && !bad) ? u[i] : 0.f;
            s[i] += (double)u[i];
            s[4 + i] += bad ? 1.0 : 0.0;
        }
        v[e].r = v2f{u[0], u[1]};
        v[e].i = v2f{u[2], u[3]};
    }
    // ---- channel means and non-finite counts over the T threads of the quad (float64 sums)
    spyfft::block_sum<C::NTHREADS, G, 8>(s, reinterpret_cast<double*>(lds), tid, h);
    const v2f mr = v2f{(float)(s[0] / N), (float)(s[1] / N)};
    const v2f mi = v2f{(float)(s[2] / N), (float)(s[3] / N)};
    bool bad[4];
    bool any_bad = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bad[i] = has[i] && s[4 + i] > 0.0;
        any_bad = any_bad || bad[i];
    }

    const int j = spyfft::opaque(j0);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const bool in = !BLUE || j + T * e < N;
        v[e].r = in ? v[e].r - mr : spyfft::splat(0.f);
        v[e].i = in ? v[e].i - mi : spyfft::splat(0.f);
    }

    if (!BLUE) {
        spyfft::fft2_forward<LOG2N, G>(v, lds, j, h, a.tw);
        const int j2 = spyfft::opaque(j);           // (the second transform redoes its index arithmetic: fewer live registers)
#pragma unroll
        for (int e = 0; e < 16; ++e) {                  // conj(Z h / N): the inverse transform's input
            const float w = weight(j2 + T * e, N, a.inv_n);
            v[e].r = v[e].r * w;
            v[e].i = v[e].i * -w;
        }
        spyfft::fft2_forward<LOG2N, G>(v, lds, j2, h, a.tw);
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e].i = -v[e].i;
    } else {
        const unsigned n_m1 = (unsigned)(N - 1);
#pragma unroll 1
        for (int half = 0; half < 2; ++half) {
            const int jl = spyfft::opaque(j);       // (index arithmetic redone per round instead of 32 live offsets)
            if (half == 0) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {          // x c (rows beyond N are zero already)
                    const unsigned n = (unsigned)(jl + T * e);
                    v[e] = spyfft::cmul_s(v[e], spyfft::ldg<float2>(a.chirp, (n < n_m1 ? n : n_m1) * 8u));
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) {          // conj(conv) h / N for k < N, zero beyond
                    const int k = jl + T * e;
                    const float w = k < N ? weight(k, N, a.inv_n) : 0.f;
                    v[e].r = v[e].r * w;
                    v[e].i = v[e].i * w;
                }
            }
            spyfft::fft2_forward<LOG2N, G>(v, lds, jl, h, a.tw);
#pragma unroll
            for (int e = 0; e < 16; ++e) {              // conj(V Bhat): the unnormalised inverse transform's input
                v[e] = spyfft::cmul_s(v[e], spyfft::ldg<float2>(a.bhat, (unsigned)(jl + T * e) * 8u));
                v[e].i = -v[e].i;
            }
            spyfft::fft2_forward<LOG2N, G>(v, lds, jl, h, a.tw);
        }
        const int jy = spyfft::opaque(j);
#pragma unroll
        for (int e = 0; e < 16; ++e) {                  // y = conj(c) conj(conv)
            const unsigned n = (unsigned)(jy + T * e);
            float2 c = spyfft::ldg<float2>(a.chirp, (n < n_m1 ? n : n_m1) * 8u);
            c.y = -c.y;
            v[e] = spyfft::cmul_s(v[e], c);
        }
    }

    // ---- store: analytic signal of c0, c1 = (x.r, Im y - x.i), of c2, c3 = (x.i, x.r - Re y), on the de-meaned input.
    // The input rows are read a second time here (they sit in L2 / the last-level cache: this workgroup read them a few
    // microseconds ago) instead of holding 64 registers across the transforms.
    if (any_bad && j0 == 0) a.nan[b] = 1;
    const float qn = quiet_nan();
    constexpr unsigned OSZ = CPLX ? 8u : 4u;
    char* const slab = reinterpret_cast<char*>(a.out) + trial * OSZ;
    const bool vec_out = quad_rows && ((reinterpret_cast<size_t>(a.out) & 15) == 0);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int n = j0 + T * e;
        if (BLUE && n >= N) continue;
        float re[4];
        load_row(n, re);
#pragma unroll
        for (int i = 0; i < 4; ++i) re[i] = (has[i] && !nonfinite(re[i])) ? re[i] : 0.f;
        const v2f h01 = v[e].i - (v2f{re[2], re[3]} - mi);
        const v2f h23 = (v2f{re[0], re[1]} - mr) - v[e].r;
        float im[4] = {h01[0], h01[1], h23[0], h23[1]};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            re[i] = bad[i] ? qn : re[i];
            im[i] = bad[i] ? qn : im[i];
        }
        const unsigned o = ((unsigned)n * (unsigned)a.nchan + (unsigned)c0) * OSZ;
        if (CPLX) {
            if (vec_out) {
                spyfft::stg<float4>(slab, o, make_float4(re[0], im[0], re[1], im[1]));
                spyfft::stg<float4>(slab, o + 16u, make_float4(re[2], im[2], re[3], im[3]));
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (has[i]) spyfft::stg<float2>(slab, o + i * OSZ, make_float2(re[i], im[i]));
            }
        } else {
            float r[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = convert(re[i], im[i], a.kind);
            if (vec_out) {
                spyfft::stg<float4>(slab, o, make_float4(r[0], r[1], r[2], r[3]));
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (has[i]) spyfft::stg<float>(slab, o + i * OSZ, r[i]);
            }
        }
    }
}

// ANY64: one workgroup of 256 threads per (trial, channel pair), the complex128 sequence in two work arrays of length L in
// global memory (L2-resident while the workgroup owns them), Stockham passes of any radix (f64_stockham.h).  Slow and
// exact: it keeps long and awkward trial lengths from being refused.
__device__ __forceinline__ spywil::cd* any64_passes(spywil::cd* src, spywil::cd* dst, const spywil::PlusPlan& plan,
                                                    const spywil::cd* tw, int sign, int tid) {
    int Ns = 1;
    for (int q = 0; q < plan.nfac; ++q) {
        spywil::po_pass_any(src, dst, plan.L, plan.radix[q], Ns, tw, sign, tid);
        __syncthreads();
        Ns *= plan.radix[q];
        spywil::cd* t = src; src = dst; dst = t;
    }
    return src;             // where the result is; the other array is free
}

template <bool CPLX>
__global__ void __launch_bounds__(256) hilbert_any64_kernel(HilArgs64 a) {
    using spywil::cd;
    __shared__ int bad[2];
    const int tid = threadIdx.x;
    const int L = a.plan.L, N = a.nsamp;
    const long long wg = a.wg0 + blockIdx.x;
    const int npair = (a.nchan + 1) / 2;
    const long long b = wg / npair;
    const int c0 = 2 * (int)(wg % npair);
    const bool has1 = c0 + 1 < a.nchan;
    const float* seg = a.in + (size_t)b * (size_t)N * (size_t)a.nchan + c0;
    cd* A = a.work + (size_t)blockIdx.x * 2 * (size_t)L;
    cd* B = A + L;
    const cd* tw = a.tw;
    const double inv_n = 1.0 / (double)N;

    if (tid < 2) bad[tid] = 0;
    __syncthreads();
    for (int n = tid; n < L; n += 256) {
        cd z = make_double2(0.0, 0.0);
        if (n < N) {
            float x0 = seg[(size_t)n * a.nchan];
            float x1 = has1 ? seg[(size_t)n * a.nchan + 1] : 0.f;
            if (nonfinite(x0)) { bad[0] = 1; x0 = 0.f; }
            if (nonfinite(x1)) { bad[1] = 1; x1 = 0.f; }
            z = make_double2((double)x0, (double)x1);
            if (a.blue) z = spywil::cmul(z, a.chirp[n]);
        }
        A[n] = z;
    }
    __syncthreads();
    cd* src = any64_passes(A, B, a.plan, tw, -1, tid);
    cd* dst = src == A ? B : A;
    if (!a.blue) {
        for (int k = tid; k < N; k += 256) {
            const double w = hilbert_weight(k, N) * inv_n;
            src[k] = make_double2(src[k].x * w, src[k].y * w);
        }
        __syncthreads();
        src = any64_passes(src, dst, a.plan, tw, +1, tid);
    } else {
        for (int k = tid; k < L; k += 256) src[k] = spywil::cmul(src[k], a.bhat[k]);
        __syncthreads();
        src = any64_passes(src, dst, a.plan, tw, +1, tid);
        dst = src == A ? B : A;
        for (int k = tid; k < L; k += 256) {            // conj(conv) h / N, zero beyond N
            const double w = k < N ? hilbert_weight(k, N) * inv_n : 0.0;
            src[k] = make_double2(src[k].x * w, -src[k].y * w);
        }
        __syncthreads();
        src = any64_passes(src, dst, a.plan, tw, -1, tid);
        dst = src == A ? B : A;
        for (int k = tid; k < L; k += 256) src[k] = spywil::cmul(src[k], a.bhat[k]);
        __syncthreads();
        src = any64_passes(src, dst, a.plan, tw, +1, tid);
        for (int n = tid; n < N; n += 256) {            // y = conj(c conv)
            const cd t = spywil::cmul(src[n], a.chirp[n]);
            src[n] = make_double2(t.x, -t.y);
        }
        __syncthreads();
    }
    const bool bad0 = bad[0] != 0, bad1 = has1 && bad[1] != 0;
    if (tid == 0 && (bad0 || bad1)) a.nan[b] = 1;
    const float qn = quiet_nan();
    const size_t obase = (size_t)b * (size_t)N * (size_t)a.nchan + c0;
    for (int n = tid; n < N; n += 256) {
        float x0 = seg[(size_t)n * a.nchan];
        float x1 = has1 ? seg[(size_t)n * a.nchan + 1] : 0.f;
        x0 = nonfinite(x0) ? 0.f : x0;
        x1 = nonfinite(x1) ? 0.f : x1;
        const cd yv = src[n];
        float re0 = x0, im0 = (float)(yv.y - (double)x1);
        float re1 = x1, im1 = (float)((double)x0 - yv.x);
        if (bad0) re0 = im0 = qn;
        if (bad1) re1 = im1 = qn;
        const size_t o = obase + (size_t)n * a.nchan;
        if (CPLX) {
            float2* out = reinterpret_cast<float2*>(a.out);
            out[o] = make_float2(re0, im0);
            if (has1) out[o + 1] = make_float2(re1, im1);
        } else {
            float* out = reinterpret_cast<float*>(a.out);
            out[o] = convert(re0, im0, a.kind);
            if (has1) out[o + 1] = convert(re1, im1, a.kind);
        }
    }
}

// COPY: N = 1, the analytic signal of a single sample is x + 0j
template <bool CPLX>
__global__ void __launch_bounds__(256) hilbert_copy_kernel(HilArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)a.ntrials * a.nchan) return;
    const float x = a.in[i];
    const bool bad = nonfinite(x);
    if (bad) a.nan[i / a.nchan] = 1;
    const float re = bad ? quiet_nan() : x, im = bad ? quiet_nan() : 0.f;
    if (CPLX) reinterpret_cast<float2*>(a.out)[i] = make_float2(re, im);
    else reinterpret_cast<float*>(a.out)[i] = convert(re, im, a.kind);
}

}  // namespace spyhil
