// How a selection of rows and inner axes is gathered (select.hip, select_kernel.h): the argument checks, the collapse of
// the axes, the innermost contiguous run and the lane width.  Pure integer logic, no HIP header and no runtime call, so
// that the decision is testable on any host (tests/test_select.py through tests/emu/select_route_shim.cpp) and shared by
// the launcher.
//
// A tensor is `src_rows` rows of (extent[0], extent[1], extent[2]) elements, C-order.  Every inner axis is taken WHOLE, as
// a RANGE [start, start + count) or through a LIST of count int32 indices; the lists of the LIST axes follow each other in
// one array, in axis order.  Axes of extent 1 drop out, unless a list repeats their one entry (such an axis stays a list:
// the output has `count` of it); a whole axis merges into a whole axis or a range to its left
// (range [s, s + c) over P whole elements = range [sP, (s + c)P)), so what is left has at most three axes, the fastest
// of them a run of `run` contiguous elements.  With nothing left but one whole axis the run is the trial itself (FLAT).
#pragma once
#include <cstdint>

namespace spysel {

enum Kind { WHOLE = 0, RANGE = 1, LIST = 2 };
enum Mode { FLAT = 0, AXES = 1, AXES_LDS = 2 };

// index-list entries (int32, all lists of a launch together) that a workgroup keeps in LDS: 16 KiB of the CU's 160, ten
// workgroups of 256 threads still fit; longer lists are read from global memory
constexpr long long LDS_CAP = 4096;

struct Route {
    const char* err = nullptr;  // what is wrong with the arguments, or nullptr
    int mode = FLAT;
    int lane_bytes = 0;         // 16, or the element size
    bool lane_aligned = false;  // 16-byte lanes on 16-byte boundaries (false: a 16-byte element on an 8-byte boundary)
    long long run = 0;          // elements of the innermost contiguous run (FLAT: of one row; the run is the trial)
    long long wo = 0, ws = 0;   // elements of an output row and of a source row
    long long n[3] = {1, 1, 1};         // AXES: the output's extent along the collapsed axes
    long long s[3] = {0, 0, 1};         // AXES: the source's element stride along them
    long long start[3] = {0, 0, 0};     // AXES: first source index of an axis without a list
    long long loff[3] = {-1, -1, -1};   // AXES: where the axis's list begins in the index array, or -1
    long long nidx = 0;         // entries of the index array
    long long row0 = 0, nrows = 0;      // first output row and rows of the launch
};

namespace detail {
struct Axis { long long ext, kind, start, cnt, loff; };

// the residue of m * stride modulo v over the source indices m of an axis if it is the same for all of them, else -1
inline long long axis_residue(const Axis& a, long long stride, const int32_t* idx, long long v) {
    if (a.kind != LIST) {
        if (a.cnt > 1 && stride % v) return -1;
        return a.start % v * (stride % v) % v;
    }
    long long res = -1;
    for (long long i = 0; i < a.cnt; ++i) {
        const long long r = idx[a.loff + i] % v * (stride % v) % v;
        if (res >= 0 && r != res) return -1;
        res = r;
    }
    return res;
}
}  // namespace detail

// desc: (ntrials, 3) first output row, first source row, rows; src_addr / out_addr: the tensors' base addresses
inline Route select_route(int elem_bytes, int64_t src_rows, int64_t out_rows, const int64_t* extent, const int32_t* kind,
                          const int64_t* start, const int64_t* count, const int32_t* idx, const int64_t* desc,
                          int64_t ntrials, uint64_t src_addr, uint64_t out_addr) {
    using detail::Axis;
    Route r;
    if (elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 16) { r.err = "element size is not 4, 8 or 16 bytes"; return r; }
    if (src_rows < 0 || out_rows < 0 || ntrials < 0) { r.err = "negative row or trial count"; return r; }
    if (src_addr == out_addr) { r.err = "the output is the source"; return r; }
    const uint64_t natural = elem_bytes < 8 ? elem_bytes : 8;
    if (src_addr % natural || out_addr % natural) { r.err = "a tensor is not aligned to its element type"; return r; }

    // ---- the axes: checks, then the collapse
    Axis ax[3];
    int nax = 0;
    r.wo = r.ws = 1;
    for (int i = 0; i < 3; ++i) {
        Axis a{extent[i], kind[i], 0, extent[i], -1};
        if (a.ext < 1) { r.err = "an extent is below 1"; return r; }
        if (a.kind != WHOLE && a.kind != RANGE && a.kind != LIST) { r.err = "unknown kind of axis"; return r; }
        if (a.kind != WHOLE) {
            a.cnt = count[i];
            if (a.cnt < 1) { r.err = "a count is 0"; return r; }
        }
        if (a.kind == RANGE) {
            a.start = start[i];
            if (a.start < 0 || a.start > a.ext - a.cnt) { r.err = "a range lies outside its extent"; return r; }
            if (a.cnt == a.ext) a.kind = WHOLE;
        }
        if (a.kind == LIST) {
            if (!idx || a.ext > INT32_MAX) { r.err = "an index list is missing"; return r; }
            a.loff = r.nidx;
            r.nidx += a.cnt;
            for (long long j = 0; j < a.cnt; ++j)
                if (idx[a.loff + j] < 0 || idx[a.loff + j] >= a.ext) { r.err = "an index lies outside its extent"; return r; }
        }
        if (a.ext > (INT64_MAX >> 5) / r.ws || a.cnt > (INT64_MAX >> 5) / r.wo) { r.err = "a row is too wide"; return r; }
        r.ws *= a.ext;
        r.wo *= a.cnt;
        if (a.ext > 1 || a.cnt > 1) ax[nax++] = a;     // (a list may repeat the one entry of an axis of extent 1)
    }
    if (r.ws > (INT64_MAX >> 5) / (src_rows > 0 ? src_rows : 1) || r.wo > (INT64_MAX >> 5) / (out_rows > 0 ? out_rows : 1)) {
        r.err = "the tensor is too large";
        return r;
    }
    const uint64_t src_bytes = (uint64_t)src_rows * r.ws * elem_bytes, out_bytes = (uint64_t)out_rows * r.wo * elem_bytes;
    if (src_addr < out_addr + out_bytes && out_addr < src_addr + src_bytes) { r.err = "the output overlaps the source"; return r; }
    Axis col[3];
    int ncol = 0;                       // collapsed axes, fastest first
    for (int i = nax - 1; i >= 0; --i) {
        Axis a = ax[i];
        if (ncol && col[ncol - 1].kind == WHOLE && a.kind != LIST) {
            const long long p = col[ncol - 1].ext;
            col[ncol - 1] = Axis{a.ext * p, a.kind, a.start * p, a.cnt * p, -1};
        } else {
            col[ncol++] = a;
        }
    }
    const bool flat = ncol == 0 || (ncol == 1 && col[0].kind == WHOLE);
    if (!flat) {
        long long stride = 1;
        for (int c = 0; c < ncol; ++c) {                // col[0] is the fastest axis: slot 2
            r.n[2 - c] = col[c].cnt; r.s[2 - c] = stride; r.start[2 - c] = col[c].start; r.loff[2 - c] = col[c].loff;
            stride *= col[c].ext;
        }
    }
    r.mode = flat ? FLAT : (r.nidx > 0 && r.nidx <= LDS_CAP ? AXES_LDS : AXES);
    r.run = flat ? r.ws : (col[0].kind == LIST ? 1 : col[0].cnt);

    // ---- the trials: inside their tensors, output rows stacked
    int64_t next = ntrials ? desc[0] : 0;
    for (int64_t k = 0; k < ntrials; ++k) {
        const int64_t o = desc[3 * k], a0 = desc[3 * k + 1], n = desc[3 * k + 2];
        if (n < 0 || o < 0 || a0 < 0 || o > out_rows - n || a0 > src_rows - n) { r.err = "a trial lies outside its tensor"; return r; }
        if (o != next) { r.err = "the output rows are not stacked"; return r; }
        next = o + n; r.nrows += n;
    }
    r.row0 = ntrials ? desc[0] : 0;

    // ---- the lane: 16 bytes where the run's length and every run's offset in both tensors are multiples of 16 bytes
    r.lane_bytes = elem_bytes;
    r.lane_aligned = elem_bytes < 16 || (src_addr % 16 == 0 && out_addr % 16 == 0);
    if (elem_bytes == 16 || src_addr % 16 || out_addr % 16) return r;
    const long long v = 16 / elem_bytes;
    long long rows_res = -1;                            // residue of the first source element of a row
    bool first = true;
    for (int64_t k = 0; k < ntrials; ++k) {
        const int64_t o = desc[3 * k], a0 = desc[3 * k + 1], n = desc[3 * k + 2];
        if (n == 0) continue;
        if (flat && (n % v * (r.ws % v) % v || o % v * (r.wo % v) % v)) return r;     // the trial is the run
        if (!flat && n > 1 && r.ws % v) return r;
        const long long res = a0 % v * (r.ws % v) % v;
        if (!first && res != rows_res) return r;
        rows_res = res; first = false;
    }
    if (first) return r;                                // no rows: nothing to widen
    long long sum = rows_res;
    if (!flat) {
        if (col[0].kind == LIST || col[0].cnt % v) return r;
        sum += col[0].start % v;                        // (a run of the fastest axis begins at its start)
        long long stride = col[0].ext;
        for (int c = 1; c < ncol; ++c) {
            const long long res = detail::axis_residue(col[c], stride, idx, v);
            if (res < 0) return r;
            sum += res;
            stride *= col[c].ext;
        }
    }
    if (sum % v == 0) r.lane_bytes = 16;
    return r;
}

}  // namespace spysel
