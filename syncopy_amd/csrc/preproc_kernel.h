// Time-domain preprocessing of spy.preprocessing (preproc/compRoutines.py: detrending_cF, standardize_cF,
// but_filtering_cF, sinc_filtering_cF, rectify_cF; preproc/firws.py: apply_fir).  Kept in a header so that the CPU
// emulation of the tests compiles the same kernels; the launchers live in preproc.hip.
//
// Data layout everywhere: a batch of equal-length trials (ntrials, nsamp, nchan) float32, channel fastest - the
// reference's (time, channel) trial.  One SERIES is one channel of one trial.  The pointwise kernels and the recursive
// filter give one thread to a series (thread index = trial * nchan + channel, so neighbouring lanes read neighbouring
// channels of one row); the FIR kernel gives a wave to 64 channels of a time tile.
//
// Sums whose order is the reference's (the float32 mean and variance of detrend / z-score, SciPy's filter recursion)
// are plain operators under `fp contract(off)`; the FIR sum, which is compared with a float64 model and has no order to
// keep, uses explicit fma().  Each kernel raises flag[trial] (an int store from every thread that saw a NaN; all write
// the same 1) - the reference's has_nan per trial.
#pragma once
#include "np_sum.h"

#pragma clang fp contract(off)

namespace spypre {

constexpr int SERIES_THREADS = 64;      // workgroup of the one-thread-per-series kernels
constexpr int LOAD_AHEAD = 8;           // samples whose loads are issued ahead of the dependent arithmetic
constexpr int MAX_SECTIONS = 12;        // second-order sections of one filter (butter order 24 lp/hp, 12 bp/bs)

__device__ __forceinline__ float sqrt_f32(float a) { return (float)sqrt((double)a); }     // correctly rounded, as np.sqrt

struct Series {
    long long base;     // offset of sample 0
    int trial;
    int chan;
    bool valid;
};

__device__ __forceinline__ Series my_series(int ntrials, int nsamp, int nchan) {
    const long long sid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    Series s;
    s.valid = sid < (long long)ntrials * nchan;
    s.trial = (int)(sid / nchan);
    s.chan = (int)(sid - (long long)s.trial * nchan);
    s.base = (long long)s.trial * nsamp * nchan + s.chan;
    return s;
}

// float32 sum of the series as np.mean / np.sum(axis=0) forms it on a C-ordered (time, channel) float32 array: rows added
// in time order.  `nan` reports a NaN among the samples.
__device__ __forceinline__ float seq_sum(const float* x, int nsamp, int nchan, bool& nan) {
    float s = 0.f;
    int i = 0;
    for (; i + LOAD_AHEAD <= nsamp; i += LOAD_AHEAD) {
        float v[LOAD_AHEAD];
        for (int u = 0; u < LOAD_AHEAD; ++u) v[u] = x[(i + u) * nchan];
        for (int u = 0; u < LOAD_AHEAD; ++u) {
            nan |= v[u] != v[u];
            s = s + v[u];
        }
    }
    for (; i < nsamp; ++i) {
        const float v = x[i * nchan];
        nan |= v != v;
        s = s + v;
    }
    return s;
}

// the mean NumPy takes over axis 0: one channel makes the reduction contiguous, where NumPy sums pairwise (np_sum.h;
// that routine reads NaN as 0, so a NaN is put back here)
__device__ __forceinline__ float np_mean(const float* x, int nsamp, int nchan, bool& nan) {
    float s = seq_sum(x, nsamp, nchan, nan);
    if (nchan == 1) s = nan ? __int_as_float(0x7fc00000) : np_pairwise_sum(x, nsamp);
    return __fdiv_rn(s, (float)nsamp);
}

// ---- detrending (scipy.signal.detrend on the float32 trial) --------------------------------------------------------
// ORDER 0: out = x - np.mean(x, axis=0) in float32.  ORDER 1: out = x - least-squares line, sums and fit in float64
// about the centre of the time axis (SciPy solves the same problem in float32; compared with a float64 model).
// A NaN makes its whole series NaN in both (detrending_cF sets such columns to NaN for the line fit by hand).
// out may be in.
template <int ORDER, bool RECT>
__global__ void detrend_kernel(const float* in, float* out, int ntrials, int nsamp, int nchan, int* flag) {
    const Series s = my_series(ntrials, nsamp, nchan);
    if (!s.valid) return;
    const float* x = in + s.base;
    float* y = out + s.base;
    bool nan = false;
    if (ORDER == 0) {
        const float m = np_mean(x, nsamp, nchan, nan);
        for (int i = 0; i < nsamp; ++i) {
            const float v = x[i * nchan] - m;
            y[i * nchan] = RECT ? fabsf(v) : v;
        }
    } else {
        const double mid = 0.5 * (double)(nsamp - 1);
        double sx = 0.0, sxt = 0.0;
        for (int i = 0; i < nsamp; ++i) {
            const float v = x[i * nchan];
            nan |= v != v;
            sx += (double)v;
            sxt += (double)v * ((double)i - mid);
        }
        // sum of (i - mid)^2 over i = 0 .. n-1
        const double stt = (double)nsamp * ((double)nsamp * (double)nsamp - 1.0) / 12.0;
        const double a = sx / (double)nsamp;
        const double b = nsamp > 1 ? sxt / stt : 0.0;
        for (int i = 0; i < nsamp; ++i) {
            const float v = (float)((double)x[i * nchan] - (a + b * ((double)i - mid)));
            y[i * nchan] = RECT ? fabsf(v) : v;
        }
    }
    if (nan) flag[s.trial] = 1;
}

// ---- z-score (standardize_cF): (x - np.mean(x, 0)) / np.std(x, 0) in float32 ----------------------------------------
// np.std: mean as above, d = x - mean, d * d, the same axis-0 sum, / n, sqrt.  The squares pass through `out` when
// there is one channel, because NumPy's pairwise sum wants them in memory; `out` must not be `in`.
template <bool RECT>
__global__ void standardize_kernel(const float* __restrict__ in, float* __restrict__ out, int ntrials, int nsamp,
                                   int nchan, int* __restrict__ flag) {
    const Series s = my_series(ntrials, nsamp, nchan);
    if (!s.valid) return;
    const float* x = in + s.base;
    float* y = out + s.base;
    bool nan = false;
    const float m = np_mean(x, nsamp, nchan, nan);
    float q = 0.f;
    int i = 0;
    for (; i + LOAD_AHEAD <= nsamp; i += LOAD_AHEAD) {
        float v[LOAD_AHEAD];
        for (int u = 0; u < LOAD_AHEAD; ++u) v[u] = x[(i + u) * nchan];
        for (int u = 0; u < LOAD_AHEAD; ++u) {
            const float d = v[u] - m;
            const float dd = d * d;
            if (nchan == 1) y[i + u] = dd;
            q = q + dd;
        }
    }
    for (; i < nsamp; ++i) {
        const float d = x[i * nchan] - m;
        const float dd = d * d;
        if (nchan == 1) y[i] = dd;
        q = q + dd;
    }
    if (nchan == 1) q = nan ? m : np_pairwise_sum(y, nsamp);
    const float sd = sqrt_f32(__fdiv_rn(q, (float)nsamp));
    for (i = 0; i < nsamp; ++i) {
        const float v = __fdiv_rn(x[i * nchan] - m, sd);
        y[i * nchan] = RECT ? fabsf(v) : v;
    }
    if (nan) flag[s.trial] = 1;
}

// ---- Butterworth: scipy.signal.sosfilt / sosfiltfilt ---------------------------------------------------------------
// c[s] = {b0, b1, b2, a1, a2} of section s (a0 = 1), zi[s] = sosfilt_zi of it.  Passed by value: every lane reads the
// same coefficients.  The kernels are compiled for NS = 2, 4, 8 and MAX_SECTIONS sections and run the first nsec <= NS of
// them, so that a short cascade keeps its coefficients in scalar registers.
struct SosCoef {
    double c[MAX_SECTIONS][5];
    double zi[MAX_SECTIONS][2];
    int nsec;
};

// run `LAUNCH(NS)` for the smallest compiled cascade length that holds nsec <= MAX_SECTIONS sections (the launchers of
// preproc.hip and the CPU emulation of the tests both dispatch through this)
#define SPY_SOS_DISPATCH(nsec, LAUNCH) \
    do {                               \
        if ((nsec) <= 2) { LAUNCH(2); } \
        else if ((nsec) <= 4) { LAUNCH(4); } \
        else if ((nsec) <= 8) { LAUNCH(8); } \
        else { LAUNCH(spypre::MAX_SECTIONS); } \
    } while (0)

// one sample through the cascade, SciPy's _sosfilt statement by statement (transposed direct form II)
template <int NS>
__device__ __forceinline__ double sos_step(const SosCoef& k, double (&z)[NS][2], double v) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s < k.nsec) {
            const double w = k.c[s][0] * v + z[s][0];
            z[s][0] = (k.c[s][1] * v - k.c[s][3] * w) + z[s][1];
            z[s][1] = k.c[s][2] * v - k.c[s][4] * w;
            v = w;
        }
    }
    return v;
}

template <int NS>
__device__ __forceinline__ void sos_start(const SosCoef& k, double (&z)[NS][2], double first) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        z[s][0] = s < k.nsec ? k.zi[s][0] * first : 0.0;
        z[s][1] = s < k.nsec ? k.zi[s][1] * first : 0.0;
    }
}

// sample i of scipy's odd_ext(x, edge): 2 * x[0] - x[edge - i] | x | 2 * x[n-1] - x[n-2-j], in the data's float32
__device__ __forceinline__ float odd_ext(const float* x, int i, int edge, int nsamp, int nchan) {
    if (i < edge) return 2.f * x[0] - x[(edge - i) * nchan];
    const int j = i - edge;
    if (j < nsamp) return x[j * nchan];
    return 2.f * x[(nsamp - 1) * nchan] - x[(2 * nsamp - 2 - j) * nchan];
}

// direction "onepass": out = sosfilt(sos, x) from a zero state; out may be in
template <int NS, bool RECT>
__global__ void sos_onepass_kernel(const float* in, float* out, SosCoef k, int ntrials, int nsamp, int nchan, int* flag) {
    const Series s = my_series(ntrials, nsamp, nchan);
    if (!s.valid) return;
    const float* x = in + s.base;
    float* y = out + s.base;
    double z[NS][2];
    sos_start(k, z, 0.0);
    bool nan = false;
    int i = 0;
    for (; i + LOAD_AHEAD <= nsamp; i += LOAD_AHEAD) {
        float v[LOAD_AHEAD];
        for (int u = 0; u < LOAD_AHEAD; ++u) v[u] = x[(i + u) * nchan];
        for (int u = 0; u < LOAD_AHEAD; ++u) {
            nan |= v[u] != v[u];
            const float r = (float)sos_step(k, z, (double)v[u]);
            y[(i + u) * nchan] = RECT ? fabsf(r) : r;
        }
    }
    for (; i < nsamp; ++i) {
        const float v = x[i * nchan];
        nan |= v != v;
        const float r = (float)sos_step(k, z, (double)v);
        y[i * nchan] = RECT ? fabsf(r) : r;
    }
    if (nan) flag[s.trial] = 1;
}

// direction "twopass", forward half of sosfiltfilt: the odd extension by `edge` samples at both ends, filtered from the
// state zi * ext[0], kept in float64 in work (ntrials, nsamp + 2 * edge, nchan)
template <int NS>
__global__ void sos_forward_kernel(const float* __restrict__ in, double* __restrict__ work, SosCoef k, int ntrials,
                                   int nsamp, int nchan, int edge, int* __restrict__ flag) {
    const Series s = my_series(ntrials, nsamp, nchan);
    if (!s.valid) return;
    const float* x = in + s.base;
    const int len = nsamp + 2 * edge;
    double* w = work + ((long long)s.trial * len * nchan + s.chan);
    double z[NS][2];
    sos_start(k, z, (double)odd_ext(x, 0, edge, nsamp, nchan));
    bool nan = false;
    int i = 0;
    for (; i + LOAD_AHEAD <= len; i += LOAD_AHEAD) {
        float v[LOAD_AHEAD];
        for (int u = 0; u < LOAD_AHEAD; ++u) v[u] = odd_ext(x, i + u, edge, nsamp, nchan);
        for (int u = 0; u < LOAD_AHEAD; ++u) {
            nan |= v[u] != v[u];
            w[(i + u) * nchan] = sos_step(k, z, (double)v[u]);
        }
    }
    for (; i < len; ++i) {
        const float v = odd_ext(x, i, edge, nsamp, nchan);
        nan |= v != v;
        w[i * nchan] = sos_step(k, z, (double)v);
    }
    if (nan) flag[s.trial] = 1;
}

// backward half: the forward result filtered from its last sample to its first, from the state zi * work[last]; the
// samples of the trial itself go to out as float32
template <int NS, bool RECT>
__global__ void sos_backward_kernel(const double* __restrict__ work, float* __restrict__ out, SosCoef k, int ntrials,
                                    int nsamp, int nchan, int edge) {
    const Series s = my_series(ntrials, nsamp, nchan);
    if (!s.valid) return;
    float* y = out + s.base;
    const int len = nsamp + 2 * edge;
    const double* w = work + ((long long)s.trial * len * nchan + s.chan);
    double z[NS][2];
    sos_start(k, z, w[(len - 1) * nchan]);
    int i = len - 1;
    for (; i - LOAD_AHEAD + 1 >= 0; i -= LOAD_AHEAD) {
        double v[LOAD_AHEAD];
        for (int u = 0; u < LOAD_AHEAD; ++u) v[u] = w[(i - u) * nchan];
        for (int u = 0; u < LOAD_AHEAD; ++u) {
            const float r = (float)sos_step(k, z, v[u]);
            const int j = i - u - edge;
            if (j >= 0 && j < nsamp) y[j * nchan] = RECT ? fabsf(r) : r;
        }
    }
    for (; i >= 0; --i) {
        const float r = (float)sos_step(k, z, w[i * nchan]);
        const int j = i - edge;
        if (j >= 0 && j < nsamp) y[j * nchan] = RECT ? fabsf(r) : r;
    }
}

// ---- windowed sinc: scipy.signal.convolve(x, h[:, None], mode="same"), direct --------------------------------------
// out[n] = sum_k h[k] * x[n + half - k], half = (ntaps - 1) / 2, x = 0 outside the trial; a float64 fma chain over the
// taps in ascending k.  A NaN sample therefore reaches exactly the ntaps outputs around it in its own channel, which is
// what the reference's switch to method="direct" is for.
//
// Workgroup = NT waves; a wave = 64 neighbouring channels, each lane R consecutive outputs of its channel, so a
// workgroup makes a tile of T = NT * R outputs x 64 channels.  The taps are walked in chunks of KC: per chunk the
// T + KC - 1 samples the tile needs are staged in LDS (row = sample, 64 floats: a wave reads one row, conflict free),
// and every lane slides a window of R samples down its column - one LDS read and R fmas per tap, the window rotating
// through R registers by unrolling R taps.  h[k] is the same for all lanes.  out must not be in.
template <int R, int NT, int KC>
struct FirTile {
    static constexpr int T = R * NT;
    static constexpr int ROWS = T + KC - 1;
    static constexpr int THREADS = 64 * NT;
    static constexpr int LDS_BYTES = ROWS * 64 * 4;
    static_assert(KC % R == 0, "tap chunk is a whole number of window rotations");
};

template <int R, int NT, int KC, bool RECT>
__global__ void __launch_bounds__(64 * NT)
fir_same_kernel(const float* __restrict__ in, float* __restrict__ out, const double* __restrict__ h, int ntaps, int nsamp,
                int nchan, int* __restrict__ flag) {
    using Tile = FirTile<R, NT, KC>;
    SPY_DYN_SMEM(float, tile);
    const int lane = threadIdx.x & 63;
    const int tg = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const bool chan_ok = c < nchan;
    const int t0 = blockIdx.y * Tile::T;
    const int trial = blockIdx.z;
    const int half = (ntaps - 1) / 2;
    const float* x = in + (long long)trial * nsamp * nchan + (chan_ok ? c : 0);
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    bool nan = false;

    for (int k0 = 0; k0 < ntaps; k0 += KC) {
        const int first = t0 + half - k0 - (KC - 1);          // sample held by tile row 0
        __syncthreads();
        for (int row = tg; row < Tile::ROWS; row += NT) {
            const int j = first + row;
            float v = 0.f;
            if (chan_ok && j >= 0 && j < nsamp) v = x[j * nchan];
            nan |= v != v;
            tile[row * 64 + lane] = v;
        }
        __syncthreads();
        // tap k0 + u, output t0 + tg*R + r  ->  row tg*R + (KC-1) + r - u
        const int row0 = tg * R + KC - 1;
        const float* col = tile + lane;
        double w[R];
#pragma unroll
        for (int r = 0; r < R; ++r) w[r] = (double)col[(row0 + r) * 64];
        for (int u0 = 0; u0 < KC && k0 + u0 < ntaps; u0 += R) {
#pragma unroll
            for (int uu = 0; uu < R; ++uu) {
                const int k = k0 + u0 + uu;
                if (k < ntaps) {
                    const double hk = h[k];
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[r] = fma(hk, w[(r - uu + R) % R], acc[r]);
                }
                // the window moves one sample back: the register of the newest sample takes the next older one
                const int row = row0 - (u0 + uu + 1);
                w[(R - 1 - uu) % R] = row >= 0 ? (double)col[row * 64] : 0.0;
            }
        }
    }
    if (chan_ok) {
        float* y = out + (long long)trial * nsamp * nchan + c;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int n = t0 + tg * R + r;
            if (n < nsamp) {
                const float v = (float)acc[r];
                y[n * nchan] = RECT ? fabsf(v) : v;
            }
        }
    }
    if (nan) flag[trial] = 1;
}

}  // namespace spypre
