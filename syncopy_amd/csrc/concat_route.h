// How several tensors are joined along an inner axis (concat.hip, concat_kernel.h): the argument checks and the lane width.
// Pure integer logic, no HIP header and no runtime call, so that the decision is testable on any host
// (tests/test_concat.py through tests/emu/concat_route_shim.cpp) and shared by the launcher.
//
// Source s is `src_rows[s]` rows of `pre` lines of `run[s]` elements, C-order; an output row is `pre` lines of
// W = sum(run) elements, and in every line the run of source s begins at element cum[s] = run[0] + ... + run[s - 1].
// Channel as the fastest axis: pre = the axes between time and channel, run[s] = the channels of s.  Channel in the
// middle: pre = 1, run[s] = channels x the axes behind them.
#pragma once
#include <cstdint>

namespace spycat {

constexpr int MAX_SRC = 8;      // SPYHIP_CONCAT_MAX of include/spyhip.h: what travels by value in the kernel argument

struct Route {
    const char* err = nullptr;  // what is wrong with the arguments, or nullptr
    int lane_bytes = 0;         // 16, or the element size
    bool lane_aligned = false;  // 16-byte lanes on 16-byte boundaries (false: a 16-byte element on an 8-byte boundary)
    long long w = 0;            // elements of an output line
    long long cum[MAX_SRC + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // first element of each source's run in a line; cum[nsrc] = w
    long long row0 = 0, nrows = 0;      // first output row and rows of the launch
};

// desc: (ntrials, 2 + nsrc) first output row, rows, first row in each source; src_addr / out_addr: the base addresses
inline Route concat_route(int elem_bytes, int nsrc, const int64_t* src_rows, const int64_t* run, int64_t pre,
                          const int64_t* desc, int64_t ntrials, const uint64_t* src_addr, uint64_t out_addr,
                          int64_t out_rows) {
    Route r;
    if (nsrc < 2 || nsrc > MAX_SRC) { r.err = "the number of sources is not 2 to 8"; return r; }
    if (elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 16) { r.err = "element size is not 4, 8 or 16 bytes"; return r; }
    if (pre < 1) { r.err = "pre is below 1"; return r; }
    if (out_rows < 0 || ntrials < 0) { r.err = "negative row or trial count"; return r; }
    const uint64_t natural = elem_bytes < 8 ? elem_bytes : 8;
    const long long cap = INT64_MAX >> 5;                      // the guard of select_route: byte counts stay far from 2^63
    for (int s = 0; s < nsrc; ++s) {
        if (run[s] < 1) { r.err = "a run is below 1"; return r; }
        if (src_rows[s] < 0) { r.err = "negative row or trial count"; return r; }
        if (run[s] > cap / pre - r.w) { r.err = "a row is too wide"; return r; }
        r.w += run[s];
        r.cum[s + 1] = r.w;
    }
    if (out_addr % natural) { r.err = "a tensor is not aligned to its element type"; return r; }
    const long long row_o = pre * r.w;                         // elements of an output row; a source's row is no longer
    if (row_o > cap / (out_rows > 0 ? out_rows : 1)) { r.err = "the tensor is too large"; return r; }
    const uint64_t out_bytes = (uint64_t)out_rows * row_o * elem_bytes;
    for (int s = 0; s < nsrc; ++s) {
        if (src_addr[s] % natural) { r.err = "a tensor is not aligned to its element type"; return r; }
        if (pre * run[s] > cap / (src_rows[s] > 0 ? src_rows[s] : 1)) { r.err = "the tensor is too large"; return r; }
        const uint64_t src_bytes = (uint64_t)src_rows[s] * pre * run[s] * elem_bytes;
        if (src_addr[s] == out_addr) { r.err = "the output is a source"; return r; }
        if (src_addr[s] < out_addr + out_bytes && out_addr < src_addr[s] + src_bytes) { r.err = "the output overlaps a source"; return r; }
    }

    // ---- the trials: inside their tensors, output rows stacked
    const int64_t stride = 2 + nsrc;
    int64_t next = ntrials ? desc[0] : 0;
    for (int64_t k = 0; k < ntrials; ++k) {
        const int64_t o = desc[stride * k], n = desc[stride * k + 1];
        if (n < 0 || o < 0 || o > out_rows - n) { r.err = "a trial lies outside its tensor"; return r; }
        for (int s = 0; s < nsrc; ++s) {
            const int64_t a0 = desc[stride * k + 2 + s];
            if (a0 < 0 || a0 > src_rows[s] - n) { r.err = "a trial lies outside its tensor"; return r; }
        }
        if (o != next) { r.err = "the output rows are not stacked"; return r; }
        next = o + n; r.nrows += n;
    }
    r.row0 = ntrials ? desc[0] : 0;

    // ---- the lane: 16 bytes where every run is a multiple of 16 bytes and every base lies on a 16-byte boundary; every
    // line and every run of every tensor then begins on one too
    bool aligned = out_addr % 16 == 0;
    bool whole = true;
    for (int s = 0; s < nsrc; ++s) {
        aligned = aligned && src_addr[s] % 16 == 0;
        whole = whole && run[s] * elem_bytes % 16 == 0;
    }
    r.lane_aligned = elem_bytes < 16 || aligned;
    r.lane_bytes = (elem_bytes == 16 || (aligned && whole)) ? 16 : elem_bytes;
    return r;
}

}  // namespace spycat
