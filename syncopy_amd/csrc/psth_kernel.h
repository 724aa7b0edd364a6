// Peristimulus time histogram of spy.spike_psth (statistics/psth.py: psth, statistics/compRoutines.py: psth_cF / PSTH)
// over a spike table resident on the device.  Kept in a header so that the CPU emulation of the tests compiles the same
// kernels; the launchers live in psth.hip.
//
// The table is a structure of arrays, one entry per spike and SORTED BY SAMPLE: sample int64, channel int32, unit int32.
// Trial t owns the rows [row_lo[t], row_hi[t]) (its spikes with start <= sample < end; the same rows may belong to
// several selected trials when the selection repeats one) and has the relative time
//
//     time(r) = (double)(sample[r] - start[t] + onset[t]) / samplerate          one IEEE float64 division, as NumPy's
//
// which does not decrease along the rows.  A spike is in bin b when edges[b] <= time < edges[b + 1], the last bin also
// takes time == edges[nbins] (np.histogram2d with explicit edges), so the spikes of one (trial, bin) are a contiguous
// row range and no float arithmetic can move a count:
//
//   psth_presence_kernel    flags[channel * nunit + unit] = 1 for every row of a selected trial whose channel and unit
//                           pass the selection (plain byte stores of the same value; replaces the per-trial np.unique
//                           loop of get_chan_unit_combs).  The host turns the table into the sorted columns and the
//                           look-up table lut[channel * nunit + unit] -> column or -1.
//   psth_bin_rows_kernel    rows[t][e] = first row of trial t with time >= edges[e], for the last edge with time >
//                           edges[e]: one thread per (trial, edge), a binary search.
//   psth_count_kernel       a workgroup owns BIN_TILE bins x COL_TILE columns of one trial: uint32 counts in LDS, added
//                           with LDS atomics (integer adds: any order gives the same bits), then ONE plain store per
//                           element, finalised: NaN outside the trial's valid bins [lo, hi), else (float)(count *
//                           scale) with the product in float64.  The output needs no zeroing.
//   psth_unit_count_kernel  output "proportion": S[t][k] = number of the trial's selected spikes of unit k (dense index)
//   psth_proportion_kernel  with edges[0] <= time <= edges[nbins], or -1 when the unit does not occur in the trial; then
//                           per column, in float64: v[b] = count[b] / dt[b] / S (0 / 0 = NaN: unit present, nothing in
//                           the window; 0 for an absent unit), NaN where psth_count_kernel masked, divided by the sum
//                           of the non-NaN v[b] in bin order (1 if that is 0), one rounding to float32.
//
// No global atomics anywhere.  All row and element indices are 64-bit.  Trials ride on blockIdx.x (up to 2^31 - 1).
#pragma once

namespace spypsth {

constexpr int THREADS = 256;
constexpr int BIN_TILE = 32;         // bins of a psth_count_kernel workgroup
constexpr int COL_TILE = 128;        // columns of a psth_count_kernel workgroup: 16 KiB of LDS, ten workgroups per CU
constexpr int UNIT_TILE = 1024;      // dense units of a psth_unit_count_kernel workgroup: 8 KiB of LDS
constexpr int PROP_TILE = 64;        // columns (= threads) of a psth_proportion_kernel workgroup
constexpr int MAX_ROW_BLOCKS = 256;  // workgroups that share the rows of one trial in psth_presence_kernel

__device__ __forceinline__ double spike_time(long long sample, long long start, long long onset, double samplerate) {
    return (double)(sample - start + onset) / samplerate;
}

// grid = (trials, nblk <= MAX_ROW_BLOCKS), THREADS threads; flags zeroed by the caller
__global__ void __launch_bounds__(THREADS)
psth_presence_kernel(const int* __restrict__ chan, const int* __restrict__ unit, const long long* __restrict__ row_lo,
                     const long long* __restrict__ row_hi, const unsigned char* __restrict__ chan_ok,
                     const unsigned char* __restrict__ unit_ok, long long nchan, long long nunit,
                     unsigned char* __restrict__ flags) {
    const long long t = blockIdx.x;
    const long long r1 = row_hi[t];
    const long long step = (long long)gridDim.y * THREADS;
    for (long long r = row_lo[t] + (long long)blockIdx.y * THREADS + threadIdx.x; r < r1; r += step) {
        const long long c = chan[r], u = unit[r];
        if (c < 0 || c >= nchan || u < 0 || u >= nunit) continue;
        if (chan_ok[c] && unit_ok[u]) flags[c * nunit + u] = 1;
    }
}

// grid = ceil(trials * nedges / THREADS), THREADS threads; rows (trials, nedges)
__global__ void __launch_bounds__(THREADS)
psth_bin_rows_kernel(const long long* __restrict__ sample, const long long* __restrict__ row_lo,
                     const long long* __restrict__ row_hi, const long long* __restrict__ start,
                     const long long* __restrict__ onset, long long ntrials, const double* __restrict__ edges,
                     long long nedges, double samplerate, long long* __restrict__ rows) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= ntrials * nedges) return;
    const long long t = i / nedges, e = i - t * nedges;
    const double edge = edges[e];
    const bool last = e == nedges - 1;
    const long long s0 = start[t], on = onset[t];
    long long a = row_lo[t], b = row_hi[t];
    while (a < b) {                                     // first row in [a, b) that is not before the edge
        const long long m = a + ((b - a) >> 1);
        const double tm = spike_time(sample[m], s0, on, samplerate);
        const bool before = last ? tm <= edge : tm < edge;
        if (before) a = m + 1; else b = m;
    }
    rows[i] = a;
}

// grid = (trials, ceil(nbins / BIN_TILE), ceil(ncols / COL_TILE)), THREADS threads.  lohi: (lo, hi) int32 per trial.
__global__ void __launch_bounds__(THREADS)
psth_count_kernel(const int* __restrict__ chan, const int* __restrict__ unit, const long long* __restrict__ rows,
                  const int* __restrict__ lut, long long nchan, long long nunit, const int* __restrict__ lohi,
                  long long nbins, long long ncols, double scale, float* __restrict__ out) {
    __shared__ unsigned cnt[BIN_TILE * COL_TILE];
    __shared__ long long rb[BIN_TILE + 1];
    const int tid = threadIdx.x;
    const long long t = blockIdx.x;
    const long long b0 = (long long)blockIdx.y * BIN_TILE, c0 = (long long)blockIdx.z * COL_TILE;
    const int nb = (int)(nbins - b0 < BIN_TILE ? nbins - b0 : BIN_TILE);
    for (int i = tid; i < BIN_TILE * COL_TILE; i += THREADS) cnt[i] = 0u;
    if (tid <= nb) rb[tid] = rows[t * (nbins + 1) + b0 + tid];
    __syncthreads();
    const long long r1 = rb[nb];
    for (long long r = rb[0] + tid; r < r1; r += THREADS) {
        const long long c = chan[r], u = unit[r];
        if (c < 0 || c >= nchan || u < 0 || u >= nunit) continue;
        const long long col = (long long)lut[c * nunit + u] - c0;
        if (col < 0 || col >= COL_TILE) continue;       // not selected (-1), or another workgroup's column
        int lo = 0, hi = nb;                            // last bin with rb[bin] <= r
        while (hi - lo > 1) {
            const int m = (lo + hi) >> 1;
            if (rb[m] <= r) lo = m; else hi = m;
        }
        atomicAdd(&cnt[lo * COL_TILE + (int)col], 1u);
    }
    __syncthreads();
    const long long vlo = lohi[2 * t], vhi = lohi[2 * t + 1];
    const int nc = (int)(ncols - c0 < COL_TILE ? ncols - c0 : COL_TILE);
    for (int i = tid; i < BIN_TILE * COL_TILE; i += THREADS) {
        const int b = i / COL_TILE, c = i - b * COL_TILE;
        if (b >= nb || c >= nc) continue;
        const long long bin = b0 + b;
        const float v = (bin >= vlo && bin < vhi) ? (float)((double)cnt[i] * scale) : __int_as_float(0x7fc00000);
        out[(t * nbins + bin) * ncols + c0 + c] = v;
    }
}

// grid = (trials, ceil(nk / UNIT_TILE)), THREADS threads.  unit_k[unit] -> dense unit index of a unit that has a column.
// S (trials, nk) int32: spikes inside [rows[t][0], rows[t][nbins]), -1 for a unit without a selected spike in the trial.
__global__ void __launch_bounds__(THREADS)
psth_unit_count_kernel(const int* __restrict__ chan, const int* __restrict__ unit, const long long* __restrict__ row_lo,
                       const long long* __restrict__ row_hi, const long long* __restrict__ rows,
                       const int* __restrict__ lut, const int* __restrict__ unit_k, long long nchan, long long nunit,
                       long long nk, long long nbins, int* __restrict__ S) {
    __shared__ unsigned inwin[UNIT_TILE];
    __shared__ unsigned seen[UNIT_TILE];
    const int tid = threadIdx.x;
    const long long t = blockIdx.x, k0 = (long long)blockIdx.y * UNIT_TILE;
    for (int i = tid; i < UNIT_TILE; i += THREADS) { inwin[i] = 0u; seen[i] = 0u; }
    __syncthreads();
    const long long w0 = rows[t * (nbins + 1)], w1 = rows[t * (nbins + 1) + nbins];
    const long long r1 = row_hi[t];
    for (long long r = row_lo[t] + tid; r < r1; r += THREADS) {
        const long long c = chan[r], u = unit[r];
        if (c < 0 || c >= nchan || u < 0 || u >= nunit) continue;
        if (lut[c * nunit + u] < 0) continue;
        const long long k = (long long)unit_k[u] - k0;
        if (k < 0 || k >= UNIT_TILE) continue;
        atomicAdd(&seen[k], 1u);
        if (r >= w0 && r < w1) atomicAdd(&inwin[k], 1u);
    }
    __syncthreads();
    for (int i = tid; i < UNIT_TILE; i += THREADS)
        if (k0 + i < nk) S[t * nk + k0 + i] = seen[i] ? (int)inwin[i] : -1;
}

// grid = (trials, ceil(ncols / PROP_TILE)), PROP_TILE threads: one thread per column, the bins in order.  out holds the
// counts of psth_count_kernel (scale 1) with its NaNs, and is overwritten.  col_k[column] -> dense unit index.
__global__ void __launch_bounds__(PROP_TILE)
psth_proportion_kernel(const int* __restrict__ S, const int* __restrict__ col_k, const double* __restrict__ edges,
                       long long nk, long long nbins, long long ncols, float* __restrict__ out) {
    const long long t = blockIdx.x, c = (long long)blockIdx.y * PROP_TILE + threadIdx.x;
    if (c >= ncols) return;
    const int s = S[t * nk + col_k[c]];
    float* p = out + t * nbins * ncols + c;
    double sum = 0.0;
    for (long long b = 0; b < nbins; ++b) {
        const float n = p[b * ncols];
        if (n != n || s < 0) continue;                  // masked bin; a unit that is absent from the trial adds 0
        const double v = (double)n / (edges[b + 1] - edges[b]) / (double)s;
        if (v == v) sum += v;
    }
    const double norm = sum == 0.0 ? 1.0 : sum;
    for (long long b = 0; b < nbins; ++b) {
        const float n = p[b * ncols];
        if (n != n) continue;                           // stays NaN
        const double v = s < 0 ? 0.0 : (double)n / (edges[b + 1] - edges[b]) / (double)s;
        p[b * ncols] = (float)(v / norm);
    }
}

}  // namespace spypsth
