// Rational resampling of spy.resampledata (preproc/resampling.py: resample = scipy.signal.resample_poly with the
// caller's window, downsample = trial[::skip]; preproc/compRoutines.py: resample_cF, downsample_cF) as one up-FIR-down
// kernel.  Kept in a header so that the CPU emulation of the tests compiles the same kernel; the launcher lives in
// resample.hip.
//
// in (ntrials, nsamp, nchan) float32 -> out (ntrials, nout, nchan) float32, channel fastest.  With half = (ntaps - 1) / 2
//
//     out[m] = sum_i h[m * down + half - i * up] * x[i]        h = 0 outside [0, ntaps), x = 0 outside the trial
//
// which is resample_poly(x, up, down, window=h / up) once SciPy's padding of the taps and its removal cancel (h arrives
// already multiplied by up).  up = 1 with the single tap 1.0 is x[::down]; up = 1 with a filter is every down-th sample
// of the "same" convolution of fir_same_kernel.  The sum is float64 with explicit fma() and has no order to keep.
//
// Mapping.  Write m = u * up + q.  The outputs of one PHASE q use the same taps h[phase + j * up], j = 0, 1, ...
// (phase = (q * down + half) % up), and output u pairs tap j with input row u * down + (q * down + half) / up - j: per
// phase the problem is a FIR of about ntaps / up taps whose outputs lie `down` rows apart.  A workgroup takes R
// consecutive u of one phase for 64 neighbouring channels (lane = channel), so that the phase, every tap address and
// every input row are uniform over a wave: the taps come through scalar loads, and one loaded tap serves R fmas.
// The taps of the phase are walked in chunks of KC; per chunk the (R - 1) * down + KC input rows the R outputs need are
// staged in LDS once (row = sample, 64 floats: a wave reads one row, conflict free), and the NT waves of the workgroup
// share the chunk, KC / NT taps each, every wave holding R partial sums per lane.  At the end the partial sums cross
// LDS and are added in wave order.  One LDS read per fma; measured times and what holds the kernel up: DESIGN.md 8.
// The number of staged rows grows with `down`, so the launcher picks the largest compiled R whose rows fit; R = 1 needs
// KC rows whatever `down` is.  All sample and tap indices are 64-bit.  out must not be in.
#pragma once

namespace spyres {

template <int R, int NT, int KC>
struct UpfirdnTile {
    static constexpr int THREADS = 64 * NT;
    static constexpr int KW = KC / NT;                                      // taps of a chunk per wave
    static_assert(KC % NT == 0, "the waves share a tap chunk evenly");
    static constexpr long long rows(long long down) { return (R - 1) * down + KC; }
    static constexpr long long lds_bytes(long long down) {
        const long long stage = rows(down) * 64 * 4, reduce = (long long)NT * R * 64 * 8;
        return stage > reduce ? stage : reduce;
    }
};

// ublocks = blocks of R outputs per phase = ceil(ceil(nout / up) / R); grid = (up * ublocks, ceil(nchan / 64), trials)
template <int R, int NT, int KC>
__global__ void __launch_bounds__(64 * NT)
upfirdn_kernel(const float* __restrict__ in, float* __restrict__ out, const double* __restrict__ h, int ntaps,
               long long nsamp, long long nchan, long long nout, int up, int down, long long ublocks) {
    using Tile = UpfirdnTile<R, NT, KC>;
    SPY_DYN_SMEM(float, tile);
    const int lane = threadIdx.x & 63;
    const int tg = spy_wave_index(threadIdx.x);
    const long long c = (long long)blockIdx.y * 64 + lane;
    const bool chan_ok = c < nchan;
    const long long q = (long long)blockIdx.x / ublocks;                    // phase class, < up
    const long long u0 = ((long long)blockIdx.x - q * ublocks) * R;         // first of the R outputs u0 + r of that class
    const long long trial = blockIdx.z;
    const long long pq = q * down + (ntaps - 1) / 2;
    const long long phase = pq % up;
    const long long base0 = u0 * down + pq / up;                            // input row that tap `phase` of output u0 meets
    // taps of this phase: phase + j * up < ntaps
    const long long ntap_q = phase < ntaps ? (ntaps - phase + up - 1) / up : 0;
    const int rows = (int)Tile::rows(down);
    const float* x = in + trial * nsamp * nchan + (chan_ok ? c : 0);
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;

    for (long long j0 = 0; j0 < ntap_q; j0 += KC) {
        const long long first = base0 - j0 - (KC - 1);                      // sample held by tile row 0
        __syncthreads();
        for (int row = tg; row < rows; row += NT) {
            const long long s = first + row;
            float v = 0.f;
            if (chan_ok && s >= 0 && s < nsamp) v = x[s * nchan];
            tile[row * 64 + lane] = v;
        }
        __syncthreads();
        // tap j0 + t of output u0 + r  ->  row r * down + (KC - 1) - t
        const float* col = tile + lane;
#pragma unroll
        for (int tt = 0; tt < Tile::KW; ++tt) {
            const int t = tg * Tile::KW + tt;
            if (j0 + t < ntap_q) {
                const double hk = h[phase + (j0 + t) * up];
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = fma(hk, (double)col[(r * down + (KC - 1) - t) * 64], acc[r]);
            }
        }
    }
    // the waves' partial sums, added in wave order
    __syncthreads();
    double* part = reinterpret_cast<double*>(tile);
#pragma unroll
    for (int r = 0; r < R; ++r) part[(tg * R + r) * 64 + lane] = acc[r];
    __syncthreads();
    for (int r = tg; r < R; r += NT) {
        double s = 0.0;
        for (int w = 0; w < NT; ++w) s += part[(w * R + r) * 64 + lane];
        const long long m = (u0 + r) * up + q;
        if (chan_ok && m < nout) out[(trial * nout + m) * nchan + c] = (float)s;
    }
}

}  // namespace spyres
