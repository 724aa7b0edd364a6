// Which kernels serve a cross-spectral update (K4 / K4h), over which ranges and in which order: pure integer logic, no HIP
// header and no runtime call, so that the launch policy is testable on any host (tests/test_csd_route.py) and shared by
// the library (csd.hip walks the steps with hipLaunchKernelGGL) and the kernel emulator (tests/emu/csd_emu.cpp compiles
// csd.hip for the host, so the same walk runs there).
#pragma once
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

namespace spycsd {

// lower-triangle 32 x 32 tiles of an nchan x nchan matrix
constexpr long long tri_tiles(int nchan) { return (long long)((nchan + 31) / 32) * ((nchan + 31) / 32 + 1) / 2; }

// One workgroup per CU: the workgroups beyond the last full round of the chip would run as an almost empty round of their
// own (F = 2049 frequencies on 256 CUs: a 9th round for one frequency).  When that partial round fills at most a quarter of
// the chip it goes to the re-cut tail (1 tile per wave, rows split over blockIdx.y) instead.  Returns the workgroups that
// stay in the main launch; every call site states `nwg` in its own unit (items, frequencies, packed rows).
constexpr long long recut_main(long long nwg, long long num_cu) {
    const long long rem = nwg % num_cu;
    return (nwg > num_cu && rem > 0 && rem * 4 <= num_cu) ? nwg - rem : nwg;
}

// bytes of one staged chunk of csd_accum_kernel: CSD_THREADS x CSD_PF float2 elements (csd.hip asserts the equality)
constexpr size_t ACCUM_CHUNK_BYTES = 512 * 8 * 8;
// dynamic LDS of the FAST variants: three 32 KiB buffers + one row of slack - a tile's columns past the last frequency
// of a row are read (and never stored)
constexpr size_t ACCUM_FAST_LDS = 3 * (size_t)16 * 256 * 8 + 512;

struct AccumGeometry {
    int err = 0;                // 0, -3 (LDS) or -1 (grid)
    int kb = 0;                 // rows per LDS chunk (the FAST variants fix theirs at compile time, 16 or 8 for FAST 3,
                                // and never read the argument: reported for the record only)
    size_t lds = 0;             // dynamic LDS bytes
    long long wg_items = 0;     // items per workgroup
    long long grid = 0;         // workgroups (blockIdx.x); 0: nothing to launch
};

// Launch geometry of csd_accum_kernel<TA, TB, FAST> over `nitems` items: `rows_wg` rows per workgroup (the rows of one
// split of a row-split launch), fast_per / fast_nwgf as in CsdArgs.
inline AccumGeometry accum_geometry(int TA, int TB, int FAST, int ntiles, int cpad, int F, long long rows_wg, int fast_per,
                                    int fast_nwgf, size_t lds_per_block, long long nitems) {
    AccumGeometry g;
    const int per = 4 * (TA + TB);
    // frequencies a workgroup can touch: items [i0, i0 + per) span at most this many f
    int nfb = (per + ntiles - 1) / ntiles;
    if (per % ntiles != 0 && ntiles > 1) nfb += 1;
    if (nfb > F) nfb = F;
    const size_t rowbytes = (size_t)nfb * cpad * 8;
    if (FAST) {
        g.kb = FAST == 3 ? 8 : 16;
        g.lds = ACCUM_FAST_LDS;
    } else {
        // a chunk holds at most ACCUM_CHUNK_BYTES; LDS holds three chunks
        int kb = 32;
        while (kb > 4 && (size_t)kb * rowbytes > ACCUM_CHUNK_BYTES) kb -= 4;
        if ((size_t)kb * rowbytes > ACCUM_CHUNK_BYTES || 3 * (size_t)kb * rowbytes > lds_per_block) { g.err = -3; return g; }
        if (kb > rows_wg) kb = (int)((rows_wg + 3) & ~3LL);
        g.kb = kb;
        g.lds = 3 * (size_t)kb * rowbytes;
    }
    g.wg_items = FAST ? fast_per : per;
    g.grid = FAST == 3 ? (nitems / ntiles) * fast_nwgf             // whole frequencies x workgroups each
                       : (nitems + g.wg_items - 1) / g.wg_items;
    if (g.grid < 0) g.grid = 0;
    if (g.grid > 0x7fffffffLL) g.err = -1;
    return g;
}

// Row split of a re-cut tail that starts at item `first`: the short workgroups (8 items each) fill the chip once when
// the rows are split over blockIdx.y, at least 64 rows per split.  The partial sums of the splits are reduced per whole
// frequency, so a tail that does not start on a frequency boundary is not split (the fast paths always start on one:
// their items per workgroup are a multiple of ntiles; the (5, 4) path of the blocked layout has 36 whatever ntiles is).
struct TailSplit {
    int nsplit = 1;                 // 1: no split
    long long rows_per_split = 0;   // multiple of 4; 0 without a split
};
inline TailSplit tail_split(long long nitems, long long first, int ntiles, long long nrows, long long num_cu) {
    TailSplit t;
    const long long tail_wg = (nitems - first + 7) / 8;
    long long nsplit = tail_wg > 0 ? num_cu / tail_wg : 1;
    const long long max_split = (nrows + 63) / 64;
    if (nsplit > max_split) nsplit = max_split;
    if (nsplit < 2 || first % ntiles != 0) return t;
    t.rows_per_split = ((nrows + nsplit - 1) / nsplit + 3) & ~3LL;
    t.nsplit = (int)((nrows + t.rows_per_split - 1) / t.rows_per_split);
    return t;
}

// channel count of the 3M kernel instance that serves `nchan` channels: the next multiple of 16
constexpr int m3_padded(int nchan) { return (nchan + 15) & ~15; }
// workgroups per packed row of that instance (csd3m_kernel.h: M3Tab<CH>::NP): 1 up to 256 channels, ceil(sub-tiles / 112) above
constexpr int m3_parts(int nchan) {
    return m3_padded(nchan) <= 256 ? 1 : ((m3_padded(nchan) / 16) * (m3_padded(nchan) / 16 + 1) / 2 + 111) / 112;
}
// frequencies per packed row: floor(256 / CHp) below 256 (padded) channels
constexpr int m3_freqs_per_row(int chp) { return chp < 256 ? 256 / chp : 1; }

enum class StepKind {
    ACCUM,       // csd_accum_kernel<ta, tb, fast> over the items [item0, item1)
    TAIL,        // re-cut tail: csd_accum_kernel<1, 1> from item0 to the last item, rows split `split` ways (+ reduction)
    M3_EXACT,    // csd3m_kernel<256, 8, true> over the packed rows (= frequencies) [0, nprow)
    M3_PADDED,   // csd3m_kernel<chp, 8, false> over the packed rows [0, nprow); n0 > 0: the channels [ch0, ch0 + n0) only
    M4_BLOCK,    // Hermitian block [ch0, ch0 + n0) with the 4-multiplication product, nprow = every frequency
    M3_RECT,     // rectangle (ch1, n1: rows) x (ch0, n0: columns) of the lower triangle, every frequency
    M4_RECT,     // the same with the 4-multiplication product
    RANK1        // csd_rank1_kernel: one row of spectra
};

struct CsdStep {
    StepKind kind;
    long long row0 = 0, nrows = 0;      // rows of spectra [row0, row0 + nrows) this step accumulates
    int ta = 0, tb = 0, fast = 0;       // ACCUM
    long long item0 = 0, item1 = 0;     // ACCUM, TAIL
    TailSplit split;                    // TAIL
    AccumGeometry geo;                  // ACCUM, TAIL
    int chp = 0;                        // M3_PADDED
    long long nprow = 0;                // M3_*, M4_BLOCK, *_RECT
    int ch0 = 0, n0 = 0, ch1 = 0, n1 = 0;
};

struct CsdQuery {
    int nchan = 0, nfreq = 0;
    long long nrows = 0;
    bool blocked = false;               // channel-quad-blocked spectra (spyhip_csd_accumulate_blocked)
    bool phase_exact = false;           // spyhip_csd_set_phase_exact: 4-multiplication kernels only
    long long num_cu = 256;
    size_t lds_per_block = 160 * 1024;
    bool (*have_m3)(int chp) = nullptr; // is csd3m_kernel<chp, 8, false> built (chp a multiple of 16 up to 512)?  The
                                        // library: every width; the emulator: its sample.  nullptr = every width.
};

struct CsdRoute {
    int err = 0;                        // 0, or the code spyhip_csd_accumulate returns with `message`
    std::string message;
    std::string kernel_name;            // the dominant kernel, for profile matching
    // geometry shared by the steps (CsdArgs of the same names)
    int nt = 0, ntiles = 0, cpad = 0, fast_per = 0, fast_nwgf = 0;
    long long nitems = 0;
    std::vector<CsdStep> steps;
};

namespace route_detail {

template <class... A>
std::string fmt(const char* f, A... a) {
    char buf[192];
    std::snprintf(buf, sizeof buf, f, a...);
    return buf;
}

// csd_accum_kernel<ta, tb, fast> over the items [i0, i1) and the rows [row0, row0 + nrows), with its launch geometry
inline void accum(const CsdQuery& q, CsdRoute& r, long long row0, long long nrows, int ta, int tb, int fast, long long i0,
                  long long i1, const TailSplit* split = nullptr) {
    CsdStep s{split ? StepKind::TAIL : StepKind::ACCUM};
    s.row0 = row0; s.nrows = nrows; s.ta = ta; s.tb = tb; s.fast = fast; s.item0 = i0; s.item1 = i1;
    if (split) s.split = *split;
    s.geo = accum_geometry(ta, tb, fast, r.ntiles, r.cpad, q.nfreq, s.split.nsplit > 1 ? s.split.rows_per_split : nrows,
                           r.fast_per, r.fast_nwgf, q.lds_per_block, i1 - i0);
    if (s.geo.err && !r.err) {
        r.err = s.geo.err;
        r.message = s.geo.err == -3 ? fmt("csd_accumulate: %d channels do not fit the LDS staging buffer", q.nchan)
                                    : "csd_accumulate: grid too large";
    }
    r.steps.push_back(s);
}

// the re-cut tail from item `first` on: 1 tile per wave, the rows split where that fills the chip (tail_split)
inline void tail(const CsdQuery& q, CsdRoute& r, long long row0, long long nrows, long long first) {
    const TailSplit split = tail_split(r.nitems, first, r.ntiles, nrows, q.num_cu);
    accum(q, r, row0, nrows, 1, 1, 0, first, r.nitems, &split);
}

// The 4-multiplication tiled kernel over the rows [row0, row0 + nrows): every layout and channel count up to 512
// (blocked: any count - a workgroup then stages 32-channel tiles only as far as LDS holds them).
inline void accum_steps(const CsdQuery& q, CsdRoute& r, long long row0, long long nrows) {
    auto add = [&](int ta, int tb, int fast, long long i0, long long i1) { accum(q, r, row0, nrows, ta, tb, fast, i0, i1); };
    const bool fast = !q.blocked && q.nchan <= 256;
    if (!q.blocked && q.nchan > 256 && q.nchan <= 512) {
        // 512-element LDS rows; the tiles of a frequency are shared by fast_nwgf workgroups, each staging the whole row.
        // The last partial round, re-cut, runs without a row split.
        const long long f_main = recut_main((long long)q.nfreq * r.fast_nwgf, q.num_cu) / r.fast_nwgf;
        add(5, 4, 3, 0, f_main * r.ntiles);
        if (f_main < q.nfreq) add(1, 1, 0, f_main * r.ntiles, r.nitems);
    } else if (fast || r.ntiles >= 21) {
        // tiles per wave (5, 4): the 36 tiles of C = 256 in one workgroup per frequency.  FAST 1: 36 tiles in every
        // workgroup (C = 256, no per-tile guards), 2: the instruction-lean path with any tile count.
        // (This branch used to ask for "at least one full round": nwg / num_cu > 0, i.e. nwg >= num_cu, which with a
        // non-empty partial round (rem > 0) is nwg > num_cu - the condition of recut_main.)
        const long long per = fast ? r.fast_per : 36, nwg = (r.nitems + per - 1) / per;
        const long long main = recut_main(nwg, q.num_cu);
        add(5, 4, !fast ? 0 : q.nchan == 256 ? 1 : 2, 0, main < nwg ? main * per : r.nitems);
        if (main < nwg) tail(q, r, row0, nrows, main * per);
    } else if (r.ntiles >= 6) {
        add(3, 2, 0, 0, r.nitems);
    } else {
        add(1, 1, 0, 0, r.nitems);
    }
}

}  // namespace route_detail

// The float32 route (spyhip_csd_accumulate, spyhip_csd_accumulate_blocked).  The order of the tests is the order of
// precedence between the kernel families.
inline CsdRoute csd_route(const CsdQuery& q) {
    using namespace route_detail;
    CsdRoute r;
    if (q.nrows < 0 || q.nfreq < 1 || q.nchan < 1 || q.num_cu < 1) { r.err = -1; r.message = "csd_accumulate: bad shape"; return r; }
    const int nchan = q.nchan, nfreq = q.nfreq;
    r.nt = (nchan + 31) / 32;
    r.ntiles = (int)tri_tiles(nchan);
    r.nitems = (long long)nfreq * r.ntiles;
    r.cpad = r.nt * 32;
    if (!q.blocked && nchan <= 256) {
        // The instruction-lean path: a 256-element LDS row holds nfb consecutive frequencies (1 for C > 128, 2 for
        // C = 128, 4 for C = 64, ...) and a workgroup owns their nfb * ntiles <= 40 tiles.
        int nfb = 256 / nchan;
        while (nfb > 1 && nfb * r.ntiles > 40) --nfb;
        if (nfb > nfreq) nfb = nfreq;
        r.fast_per = nfb * r.ntiles;
    } else if (!q.blocked && nchan <= 512) {
        r.fast_nwgf = (r.ntiles + 39) / 40;                  // 512 channels: 4 x 34 tiles
        r.fast_per = (r.ntiles + r.fast_nwgf - 1) / r.fast_nwgf;
    }
    const bool have = !q.have_m3 || q.have_m3(m3_padded(nchan));
    // odd channel counts: the 16-byte copy of the last channel of the 3M kernels reaches 8 bytes beyond its frequency,
    // so the last row of spectra goes to other kernels
    const long long nrows3 = (nchan & 1) ? q.nrows - 1 : q.nrows;
    if (nchan == 256 && !q.phase_exact) {
        // 256 channels, either hand-over layout (the kernel's LDS copies gather): one workgroup per frequency
        r.kernel_name = "spycsd::csd3m_kernel<256, 8, true, false, false>";
        const long long f_main = recut_main(nfreq, q.num_cu);
        CsdStep s{StepKind::M3_EXACT};
        s.nrows = q.nrows; s.nprow = f_main;
        r.steps.push_back(s);
        if (f_main < nfreq) tail(q, r, 0, q.nrows, f_main * r.ntiles);
    } else if (nchan <= 512 && !q.blocked && !q.phase_exact && have) {
        // every other channel count up to 512, row-major spectra: the 3M instance of the next multiple of 16 with the
        // narrower rows padded inside its LDS image.  Below 256 (padded) channels floor(256 / CHp) frequencies per
        // workgroup (the last packed row may be partial); above, 512-element LDS rows and several workgroups per frequency.
        const int chp = m3_padded(nchan), fpr = m3_freqs_per_row(chp), np = m3_parts(nchan);
        r.kernel_name = fmt("spycsd::csd3m_kernel<%d, 8, false>", chp);
        const long long nprow = (nfreq + fpr - 1) / fpr;
        const long long rem = nprow * np - recut_main(nprow * np, q.num_cu);
        const long long p_main = nprow - (rem + np - 1) / np;
        if (nrows3 > 0) {
            CsdStep s{StepKind::M3_PADDED};
            s.nrows = nrows3; s.chp = chp; s.nprow = p_main;
            r.steps.push_back(s);
            if (p_main < nprow) tail(q, r, 0, nrows3, fpr * p_main * r.ntiles);
        }
        if (nrows3 < q.nrows) accum_steps(q, r, nrows3, 1);
    } else if (nchan > 512 && !q.blocked) {
        // more than 512 channels, row-major spectra: the lower triangle in blocks of 256 channels - the Hermitian product
        // of every block with itself (the 3M instance of its width, reading its channel range out of the wide rows) and
        // the rectangle of every pair of blocks (csd3m_kernel<512, 8, false, true>).  A launch never stages more than 512
        // channels.  Phase-exact accumulation takes the same walk with the 4-multiplication instances.
        r.kernel_name = q.phase_exact
            ? "spycsd::csd3m_kernel<512, 8, false, true, true> (+ csd3m_kernel<256, 8, false, false, true> per 256-channel block)"
            : "spycsd::csd3m_kernel<512, 8, false, true> (+ csd3m_kernel<256, 8, false> per 256-channel block)";
        const int nb = (nchan + 255) / 256;
        for (int I = 0; I < nb && nrows3 > 0; ++I) {
            const int nI = nchan - 256 * I < 256 ? nchan - 256 * I : 256;
            const int chp = q.phase_exact ? 256 : m3_padded(nI), fpr = m3_freqs_per_row(chp);
            if (!q.phase_exact && q.have_m3 && !q.have_m3(chp)) {
                r.err = -1;
                r.message = fmt("csd_accumulate: no 3M kernel for a block of %d channels", nI);
                return r;
            }
            CsdStep s{q.phase_exact ? StepKind::M4_BLOCK : StepKind::M3_PADDED};
            s.nrows = nrows3; s.chp = chp; s.ch0 = 256 * I; s.n0 = nI;
            s.nprow = q.phase_exact ? nfreq : (nfreq + fpr - 1) / fpr;
            r.steps.push_back(s);
            for (int J = 0; J < I; ++J) {
                CsdStep t{q.phase_exact ? StepKind::M4_RECT : StepKind::M3_RECT};
                t.nrows = nrows3; t.nprow = nfreq; t.ch0 = 256 * J; t.n0 = 256; t.ch1 = 256 * I; t.n1 = nI;
                r.steps.push_back(t);
            }
        }
        if (nrows3 < q.nrows) {
            CsdStep s{StepKind::RANK1};
            s.row0 = nrows3; s.nrows = 1;
            r.steps.push_back(s);
        }
    } else {
        const int fast = q.blocked ? 0 : nchan == 256 ? 1 : nchan < 256 ? 2 : 3;
        r.kernel_name = fmt("spycsd::csd_accum_kernel<%s, %d>", fast || r.ntiles >= 21 ? "5, 4" : r.ntiles >= 6 ? "3, 2" : "1, 1", fast);
        accum_steps(q, r, 0, q.nrows);
    }
    if (q.nrows == 0) r.steps.clear();          // (nothing to add: the geometry and the name still hold)
    return r;
}

// The half-precision entry (K4h, 256 channels, one workgroup per frequency) for the frequencies [f0, f0 + nf) of an update:
// csdh_kernel serves the frequencies of the full rounds, [0, f_main); the last partial round, re-cut, goes to the float32
// tail in one piece, so a range that reaches beyond f_main must end at nfreq.
struct CsdhRoute {
    int err = 0;
    std::string message;
    int f_main = 0;             // first frequency of the re-cut tail (= nfreq: none)
    int h0 = 0, h1 = 0;         // csdh_kernel over the frequencies [h0, h1) (none if h1 <= h0)
    CsdRoute tail;              // no step, or the tail over the items [max(f0, f_main) * 36, nfreq * 36)
};
inline CsdhRoute csdh_route(const CsdQuery& q, int f0, int nf) {
    CsdhRoute r;
    r.f_main = (int)recut_main(q.nfreq, q.num_cu);
    const int f1 = f0 + nf;
    r.h0 = f0;
    r.h1 = f1 < r.f_main ? f1 : r.f_main;
    if (f1 > r.f_main && f1 != q.nfreq) {
        r.err = -1;
        r.message = route_detail::fmt("csd_accumulate_split_range: a range beyond frequency %d must end at nfreq = %d", r.f_main, q.nfreq);
        return r;
    }
    r.tail.nt = 8; r.tail.ntiles = 36; r.tail.cpad = 256; r.tail.fast_per = 36;
    r.tail.nitems = (long long)q.nfreq * 36;
    if (f1 > r.f_main) route_detail::tail(q, r.tail, 0, q.nrows, (long long)(f0 > r.f_main ? f0 : r.f_main) * 36);
    return r;
}

// Name of the dominant kernel of an update of `nchan` channels, for matching profiler rows.  `half`: the caller goes
// through the half-precision entry, which serves 256 channels of row-major spectra whatever the arithmetic setting.
inline std::string csd_kernel_name(CsdQuery q, bool half) {
    if (half && q.nchan == 256 && !q.blocked) return "spycsd::csdh_kernel";
    q.nfreq = 1; q.nrows = 2;
    return csd_route(q).kernel_name;
}

}  // namespace spycsd
