// How the synthetic-data kernels are launched (synth.hip, synth_kernel.h): the argument checks, the choice between the
// coupled and the uncoupled AR(2) kernel, where the coupling table lives, and the lane of the tiling kernel.  Pure integer
// logic, no HIP header and no runtime call, so that the decisions are testable on any host (tests/test_synth.py through
// tests/emu/synth_route_shim.cpp) and shared by the launcher.
//
// Every tensor is (ntrials, nsamples, nchan), C-order: the channels of a sample lie side by side.
#pragma once
#include <cstddef>
#include <cstdint>

namespace spysyn {

constexpr int MAX_CHAN = 1024;          // one thread per channel in one workgroup: the largest workgroup
constexpr int SERIES_THREADS = 256;     // a workgroup of the kernels with one thread per (trial, channel) series
constexpr int TILE_THREADS = 256;       // a workgroup of the tiling kernel

// element counts stay far from 2^63 (the guard of concat_route)
constexpr long long CAP = INT64_MAX >> 5;

// nullptr, or what is wrong with the shape of a (ntrials, nsamples, nchan) tensor; min_samples: the shortest trial
inline const char* shape_error(int64_t ntrials, int64_t nsamples, int64_t nchan, int64_t min_samples) {
    if (ntrials < 0) return "negative trial count";
    if (nsamples < min_samples) return min_samples == 2 ? "a trial has fewer than 2 samples" : "a trial has no samples";
    if (nchan < 1) return "no channels";
    if (nchan > CAP / nsamples || nchan * nsamples > CAP / (ntrials > 0 ? ntrials : 1)) return "the tensor is too large";
    return nullptr;
}

struct Ar2Route {
    const char* err = nullptr;  // what is wrong with the arguments, or nullptr
    bool coupled = false;       // an entry off the diagonal exists: one workgroup per trial, else one thread per series
    bool csr_in_lds = false;    // coupled: the coupling table lies in LDS behind the two state vectors
    int block = 0;              // threads of a workgroup
    long long grid = 0;         // workgroups
    size_t lds_bytes = 0;       // dynamic LDS of a workgroup
    long long nnz = 0;          // entries of the coupling table
};

// rowptr (nchan + 1), col (rowptr[nchan]): the non-zeros of AdjMat.T as CSR - per receiver its senders, ascending
inline Ar2Route ar2_route(int64_t ntrials, int64_t nsamples, int64_t nchan, const int32_t* rowptr, const int32_t* col,
                          size_t lds_per_block) {
    Ar2Route r;
    if ((r.err = shape_error(ntrials, nsamples, nchan, 2))) return r;
    if (nchan > MAX_CHAN) { r.err = "more than 1024 channels"; return r; }
    if (rowptr[0] != 0) { r.err = "the coupling table does not begin at 0"; return r; }
    for (int64_t c = 0; c < nchan; ++c)                         // (rows in order: every index below is < rowptr[nchan])
        if (rowptr[c + 1] < rowptr[c] || rowptr[c + 1] - rowptr[c] > nchan) { r.err = "a row of the coupling table is malformed"; return r; }
    for (int64_t c = 0; c < nchan; ++c) {
        for (int32_t k = rowptr[c]; k < rowptr[c + 1]; ++k) {
            if (col[k] < 0 || col[k] >= nchan) { r.err = "a sender lies outside the channels"; return r; }
            if (k > rowptr[c] && col[k] <= col[k - 1]) { r.err = "the senders of a receiver are not ascending"; return r; }
            if (col[k] != c) r.coupled = true;
        }
    }
    r.nnz = rowptr[nchan];
    if (r.coupled) {
        if (ntrials > INT32_MAX) { r.err = "too many trials"; return r; }
        const size_t state = 2 * sizeof(float) * (size_t)nchan;
        const size_t table = sizeof(int32_t) * (size_t)(nchan + 1) + (sizeof(int32_t) + sizeof(float)) * (size_t)r.nnz;
        r.csr_in_lds = state + table <= lds_per_block;
        r.lds_bytes = r.csr_in_lds ? state + table : state;
        r.block = (int)((nchan + 63) / 64 * 64);
        r.grid = ntrials;
    } else {
        const long long series = ntrials * nchan;
        r.block = SERIES_THREADS;
        r.grid = (series + SERIES_THREADS - 1) / SERIES_THREADS;
        if (r.grid > INT32_MAX) { r.err = "too many series"; return r; }
    }
    return r;
}

struct SeriesRoute {
    const char* err = nullptr;
    int block = 0;
    long long grid = 0;
};

// the phase-diffusion kernel: one thread per (trial, channel)
inline SeriesRoute phase_route(int64_t ntrials, int64_t nsamples, int64_t nchan) {
    SeriesRoute r;
    if ((r.err = shape_error(ntrials, nsamples, nchan, 1))) return r;
    r.block = SERIES_THREADS;
    r.grid = (ntrials * nchan + SERIES_THREADS - 1) / SERIES_THREADS;
    if (r.grid > INT32_MAX) r.err = "too many series";
    return r;
}

struct TileRoute {
    const char* err = nullptr;
    int lane_bytes = 0;         // 16 where a row of channels is whole lanes and the output lies on a 16-byte boundary, else 4
    long long lanes = 0;        // lanes of the output
    long long grid = 0;
};

inline TileRoute tile_route(int64_t ntrials, int64_t nsamples, int64_t nchan, uint64_t out_addr, int64_t max_blocks) {
    TileRoute r;
    if ((r.err = shape_error(ntrials, nsamples, nchan, 1))) return r;
    if (out_addr % 4) { r.err = "the output is not aligned to its element type"; return r; }
    r.lane_bytes = (nchan % 4 == 0 && out_addr % 16 == 0) ? 16 : 4;
    r.lanes = ntrials * nsamples * (nchan / (r.lane_bytes / 4));
    r.grid = (r.lanes + TILE_THREADS - 1) / TILE_THREADS;
    if (r.grid > max_blocks) r.grid = max_blocks;
    if (r.grid < 1) r.grid = 1;
    return r;
}

}  // namespace spysyn
