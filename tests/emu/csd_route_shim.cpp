// C view of the pure route of the cross-spectral update (syncopy_amd/csrc/csd_route.h) for tests/test_csd_route.py
// (TEST INFRASTRUCTURE ONLY).  Built with the host compiler alone: the header must not need HIP.
#include <cstdio>
#include <cstring>
#include <map>
#include <utility>

#include "../../syncopy_amd/csrc/csd_route.h"
#include "emu_m3_widths.h"

using namespace spycsd;

namespace {

bool no_m3(int) { return false; }

CsdQuery query(int nchan, int nfreq, long long nrows, int blocked, int phase_exact, long long num_cu, int m3) {
    CsdQuery q;
    q.nchan = nchan; q.nfreq = nfreq; q.nrows = nrows;
    q.blocked = blocked != 0; q.phase_exact = phase_exact != 0;
    q.num_cu = num_cu;
    q.have_m3 = m3 == 0 ? nullptr : m3 == 1 ? emu_have_m3 : no_m3;      // (1: the emulator's sample, emu_m3_widths.h)
    return q;
}

std::string render(const CsdStep& s) {
    char b[256];
    const long long r0 = s.row0, nr = s.nrows;
    switch (s.kind) {
        case StepKind::ACCUM:
            std::snprintf(b, sizeof b, "ACCUM<%d,%d,%d> rows %lld+%lld items %lld:%lld grid %lld lds %zu kb %d", s.ta, s.tb, s.fast,
                          r0, nr, s.item0, s.item1, s.geo.grid, s.geo.lds, s.geo.kb);
            break;
        case StepKind::TAIL:
            std::snprintf(b, sizeof b, "TAIL rows %lld+%lld items %lld:%lld split %dx%lld grid %lld lds %zu kb %d", r0, nr, s.item0,
                          s.item1, s.split.nsplit, s.split.rows_per_split, s.geo.grid, s.geo.lds, s.geo.kb);
            break;
        case StepKind::M3_EXACT: std::snprintf(b, sizeof b, "M3_EXACT rows %lld+%lld nprow %lld", r0, nr, s.nprow); break;
        case StepKind::M3_PADDED:
            if (s.n0) std::snprintf(b, sizeof b, "M3_PADDED<%d> rows %lld+%lld nprow %lld ch %d+%d", s.chp, r0, nr, s.nprow, s.ch0, s.n0);
            else std::snprintf(b, sizeof b, "M3_PADDED<%d> rows %lld+%lld nprow %lld", s.chp, r0, nr, s.nprow);
            break;
        case StepKind::M4_BLOCK: std::snprintf(b, sizeof b, "M4_BLOCK rows %lld+%lld nfreq %lld ch %d+%d", r0, nr, s.nprow, s.ch0, s.n0); break;
        case StepKind::M3_RECT:
        case StepKind::M4_RECT:
            std::snprintf(b, sizeof b, "%s rows %lld+%lld nfreq %lld ch %d+%d x %d+%d", s.kind == StepKind::M3_RECT ? "M3_RECT" : "M4_RECT",
                          r0, nr, s.nprow, s.ch1, s.n1, s.ch0, s.n0);
            break;
        case StepKind::RANK1: std::snprintf(b, sizeof b, "RANK1 rows %lld+%lld", r0, nr); break;
    }
    return b;
}

// Do the steps of a route cover every (frequency, lower-triangle tile, row) exactly once?  Empty string, or what is wrong.
// Tiled steps are intervals of items (frequency x 32 x 32 tile); the block walk above 512 channels is counted per pair of
// 256-channel blocks, every pair over all frequencies.
std::string check_cover(const CsdQuery& q, const CsdRoute& r) {
    using route_detail::fmt;
    if (r.err) return "";
    std::map<std::pair<long long, long long>, std::vector<const CsdStep*>> by_rows;
    for (const CsdStep& s : r.steps) by_rows[{s.row0, s.nrows}].push_back(&s);
    long long next_row = 0;
    for (const auto& kv : by_rows) {                          // (ordered by row0: the row ranges must tile [0, nrows))
        if (kv.first.first != next_row || kv.first.second < 1) return fmt("rows %lld+%lld after row %lld", kv.first.first, kv.first.second, next_row);
        next_row += kv.first.second;
        long long item = 0;                                   // items [0, item) are covered so far
        std::map<std::pair<int, int>, int> pairs;             // block walk: (I, J) -> times covered
        bool rank1 = false;
        for (const CsdStep* sp : kv.second) {
            const CsdStep& s = *sp;
            switch (s.kind) {
                case StepKind::ACCUM:
                case StepKind::TAIL: {
                    if (s.item0 != item || s.item1 <= s.item0) return fmt("items %lld:%lld after item %lld", s.item0, s.item1, item);
                    item = s.item1;
                    const long long wg = s.geo.wg_items;
                    const long long reach = s.fast == 3 ? (s.geo.grid / r.fast_nwgf) * r.ntiles
                                                        : s.geo.grid * wg;         // items the grid reaches
                    if (reach < s.item1 - s.item0) return fmt("grid %lld reaches %lld of %lld items", s.geo.grid, reach, s.item1 - s.item0);
                    if (s.fast == 3 && (long long)r.fast_per * r.fast_nwgf < r.ntiles) return std::string("wide workgroups miss tiles");
                    if (s.fast && s.fast != 3 && s.item0 % wg != 0) return std::string("fast launch off its workgroup grid");
                    const int n = s.split.nsplit;
                    if (s.kind == StepKind::ACCUM && n != 1) return std::string("split outside a tail");
                    if (n > 1) {
                        const long long rps = s.split.rows_per_split;
                        if (s.item0 % r.ntiles != 0) return fmt("split tail starts at item %lld: not a frequency boundary", s.item0);
                        if (rps < 1 || rps % 4 != 0 || n * rps < s.nrows || (n - 1) * rps >= s.nrows)
                            return fmt("%d splits of %lld rows do not tile %lld rows", n, rps, s.nrows);
                    } else if (s.split.rows_per_split != 0) return std::string("rows_per_split without a split");
                    break;
                }
                case StepKind::M3_EXACT:
                case StepKind::M3_PADDED:
                case StepKind::M4_BLOCK: {
                    const int chp = s.kind == StepKind::M3_PADDED ? s.chp : 256;
                    const int fpr = m3_freqs_per_row(chp);
                    long long nf = s.nprow * fpr < q.nfreq ? s.nprow * fpr : q.nfreq;
                    if (s.n0 == 0) {                          // whole rows of spectra
                        if (item != 0 || q.nchan > 512 || chp < q.nchan || (q.nchan & 1 && s.row0 + s.nrows == q.nrows))
                            return std::string("3M launch out of place");
                        if (s.kind == StepKind::M3_PADDED && (chp != m3_padded(q.nchan) || (q.have_m3 && !q.have_m3(chp)))) return std::string("wrong 3M instance");
                        item = nf * r.ntiles;
                    } else {
                        if (nf != q.nfreq || s.ch0 % 256 || s.n0 > 256 || s.n0 > chp || s.ch0 + s.n0 > q.nchan) return std::string("bad block");
                        if (s.n0 != 256 && s.ch0 + s.n0 != q.nchan) return std::string("short block inside");
                        ++pairs[{s.ch0 / 256, s.ch0 / 256}];
                    }
                    break;
                }
                case StepKind::M3_RECT:
                case StepKind::M4_RECT:
                    if (s.nprow != q.nfreq || s.ch0 % 256 || s.ch1 % 256 || s.n0 != 256 || s.ch1 <= s.ch0 || s.ch1 + s.n1 > q.nchan ||
                        (s.n1 != 256 && s.ch1 + s.n1 != q.nchan))
                        return std::string("bad rectangle");
                    ++pairs[{s.ch1 / 256, s.ch0 / 256}];
                    break;
                case StepKind::RANK1:
                    if (s.nrows != 1 || rank1) return std::string("bad rank-1 step");
                    rank1 = true;
                    break;
            }
        }
        const int nb = (q.nchan + 255) / 256;
        const bool walked = !pairs.empty();
        if (walked) {
            for (int I = 0; I < nb; ++I)
                for (int J = 0; J <= I; ++J)
                    if (pairs[{I, J}] != 1) return fmt("block pair (%d, %d) covered %d times", I, J, pairs[{I, J}]);
            if ((int)pairs.size() != nb * (nb + 1) / 2) return std::string("stray block pair");
        }
        if ((item == r.nitems) + walked + rank1 != 1) return fmt("rows %lld+%lld: items up to %lld of %lld, block walk %d, rank-1 %d", kv.first.first, kv.first.second, item, r.nitems, (int)walked, (int)rank1);
    }
    if (next_row != q.nrows) return fmt("rows up to %lld of %lld", next_row, q.nrows);
    return "";
}

void put(char* dst, int cap, const std::string& s) { std::snprintf(dst, cap, "%s", s.c_str()); }

}  // namespace

extern "C" {

long long csd_recut_main(long long nwg, long long num_cu) { return recut_main(nwg, num_cu); }
long long csd_tri_tiles(int nchan) { return tri_tiles(nchan); }

// m3: 0 every padded 3M width, 1 the emulator's sample, 2 none.  steps: one line per step.  geom: nt, ntiles, cpad, fast_per, fast_nwgf, nitems
int csd_route_text(int nchan, int nfreq, long long nrows, int blocked, int phase_exact, long long num_cu, int m3, long long* geom,
                   char* name, char* steps, char* message, int cap) {
    const CsdQuery q = query(nchan, nfreq, nrows, blocked, phase_exact, num_cu, m3);
    const CsdRoute r = csd_route(q);
    const long long g[6] = {r.nt, r.ntiles, r.cpad, r.fast_per, r.fast_nwgf, r.nitems};
    std::memcpy(geom, g, sizeof g);
    std::string t;
    for (const CsdStep& s : r.steps) t += render(s) + "\n";
    put(name, cap, r.kernel_name);
    put(steps, cap, t);
    put(message, cap, r.err ? r.message : check_cover(q, r));
    return r.err;
}

int csd_name(int nchan, int blocked, int phase_exact, int half, char* name, int cap) {
    put(name, cap, csd_kernel_name(query(nchan, 1, 1, blocked, phase_exact, 256, 0), half != 0));
    return 0;
}

// out: f_main, h0, h1, tail steps (0 / 1), tail item0, nsplit, rows_per_split, grid
int csdh_route_c(int nfreq, long long nrows, int f0, int nf, long long num_cu, long long* out, char* message, int cap) {
    const CsdhRoute r = csdh_route(query(256, nfreq, nrows, 0, 0, num_cu, 0), f0, nf);
    put(message, cap, r.message);
    out[0] = r.f_main; out[1] = r.h0; out[2] = r.h1; out[3] = (long long)r.tail.steps.size();
    out[4] = out[5] = out[6] = out[7] = 0;
    if (!r.tail.steps.empty()) {
        const CsdStep& s = r.tail.steps[0];
        out[4] = s.item0; out[5] = s.split.nsplit; out[6] = s.split.rows_per_split; out[7] = s.geo.grid;
    }
    return r.err;
}

// The invariant sweep: nchan 1 ... max_chan, both layouts, both arithmetic settings, the frequency counts around the re-cut
// boundary of `num_cu`, two row counts (one odd, one that a tail splits).  Returns the queries asked, -1 with `message` at
// the first route whose steps do not cover every (frequency, tile, row) exactly once.
long long csd_route_sweep(long long num_cu, int max_chan, int m3, long long* tails, long long* split_tails, char* message, int cap) {
    const int cu = (int)num_cu;
    const int freqs[8] = {1, 2, cu - 1, cu, cu + 1, cu + cu / 4, cu + cu / 4 + 1, 2049};
    const long long rows[3] = {1, 70, 301};
    long long n = 0;
    *tails = *split_tails = 0;
    for (int nchan = 1; nchan <= max_chan; ++nchan)
        for (int blocked = 0; blocked < 2; ++blocked)
            for (int exact = 0; exact < 2; ++exact)
                for (int nfreq : freqs)
                    for (long long nrows : rows) {
                        if (nfreq < 1) continue;
                        const CsdQuery q = query(nchan, nfreq, nrows, blocked, exact, num_cu, m3);
                        const CsdRoute r = csd_route(q);
                        ++n;
                        const std::string bad = r.err == -3 && blocked ? "" : r.err ? r.message : check_cover(q, r);
                        if (!bad.empty()) {
                            std::snprintf(message, cap, "nchan %d nfreq %d nrows %lld blocked %d exact %d num_cu %lld: %s", nchan, nfreq,
                                          nrows, blocked, exact, num_cu, bad.c_str());
                            return -1;
                        }
                        for (const CsdStep& s : r.steps)
                            if (s.kind == StepKind::TAIL) { ++*tails; *split_tails += s.split.nsplit > 1; }
                    }
    return n;
}
}
