// C view of the pure route of the wavelet transform (syncopy_amd/csrc/cwt_route.h) for tests/test_cwt_route.py (TEST
// INFRASTRUCTURE ONLY).  Built with the host compiler alone: the header must not need HIP.  With -DCWT_ROUTE_MAIN the file
// is a stand-alone program that runs the invariant sweep (for a sanitizer build outside Python).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>

#include "cwt_route_text.h"

using namespace spycwt;

namespace {

struct Case {
    int family = 0;
    double p0 = 6.0, p1 = 0.0, dt = 1e-3;
    std::vector<double> scales;
    int nsig = 0, nchan = 1, output = 0, detrend = -1;
    std::vector<int> tpos;          // empty: identity
};

Plan make_plan(const Case& c) {
    std::vector<int> ntaps, centre;
    for (double sc : c.scales) {
        const Taps k = sample_taps(c.family, c.p0, c.p1, sc, c.dt, c.nsig);
        ntaps.push_back((int)k.re.size());
        centre.push_back(k.c);
    }
    return plan_route(c.nsig, c.nchan, c.output, c.detrend, ntaps, centre, c.tpos.empty() ? nullptr : c.tpos.data());
}

// ---- the invariants of a plan; empty string, or what is wrong
std::string check_groups(const Plan& p, const std::vector<Group>& set, bool with_pieces) {
    std::vector<int> seen(p.nscales, 0);
    std::vector<std::vector<std::pair<int, int>>> pieces(p.nscales);
    for (const Group& g : set) {
        const int NB = 1 << g.log2n;
        if (!engine(g.log2n)) return fmt("no engine for 2^%d", g.log2n);
        if (g.V < 1) return fmt("V %d", g.V);
        if ((long long)(g.nblocks - 1) * g.V >= p.nsig || (long long)g.nblocks * g.V < p.nsig) return fmt("%d blocks of %d outputs for %d samples", g.nblocks, g.V, p.nsig);
        if ((int)g.cshift.size() != g.nscales() || (int)g.sidx.size() != g.nscales()) return std::string("table sizes");
        if (g.long_idx >= 0) {
            if (!with_pieces) return std::string("piece in a sum set");
            const int sc = g.scale_ids[0];
            if (g.nscales() != 1 || p.long_scales[g.long_idx] != sc || g.log2n != MAX_LOG2N) return std::string("bad piece");
            if (g.ntaps < 1 || g.ntaps > CWT_PIECE || g.V != NB - (g.ntaps - 1) || g.cshift[0] != g.ntaps - 1) return std::string("piece geometry");
            // window [o0 - halo, o0 - halo + NB) must hold every input of the V outputs: taps tap0 ... tap0 + ntaps - 1 about centre c
            if (g.halo != g.ntaps - 1 - (p.centre[sc] - g.tap0)) return std::string("piece halo");
            pieces[sc].push_back({g.tap0, g.ntaps});
            continue;
        }
        int halo = 0, reach = 0;
        for (int q = 0; q < g.nscales(); ++q) {
            const int sc = g.scale_ids[q];
            if (sc < 0 || sc >= p.nscales) return std::string("scale id");
            ++seen[sc];
            if (2 * (p.ntaps[sc] + 1) > NB) return fmt("%d taps on a %d-point block", p.ntaps[sc], NB);
            halo = std::max(halo, p.ntaps[sc] - 1 - p.centre[sc]);
            reach = std::max(reach, p.centre[sc]);
            if (g.cshift[q] != g.halo + p.centre[sc]) return std::string("cshift");
        }
        if (g.halo != halo || g.halo + g.V + reach != NB) return fmt("halo %d + V %d + reach %d != %d", g.halo, g.V, reach, NB);
        if (g.direct != (engine(g.log2n)->Gd > 0)) return std::string("direct flag");
    }
    for (int sc = 0; sc < p.nscales; ++sc) {
        int next = 0;
        for (const auto& pc : pieces[sc]) {                     // pieces in order, covering the taps exactly once
            if (pc.first != next) return fmt("scale %d: piece at tap %d after %d", sc, pc.first, next);
            next += pc.second;
        }
        const bool cut = !pieces[sc].empty();
        if (cut && (next != p.ntaps[sc] || seen[sc])) return fmt("scale %d: pieces cover %d of %d taps", sc, next, p.ntaps[sc]);
        if (!cut && seen[sc] != 1) return fmt("scale %d in %d groups", sc, seen[sc]);
    }
    return "";
}

std::string check_plan(const Plan& p) {
    std::string bad = check_groups(p, p.groups, true);
    if (!bad.empty()) return bad;
    if (!p.groups_sum.empty()) {
        bad = check_groups(p, p.groups_sum, false);
        if (!bad.empty()) return "sum set: " + bad;
        for (const Group& g : p.groups_sum)
            if (g.log2n < 12 || g.log2n > 13) return std::string("sum set off the packed engine / below its floor");
        if (!p.sum_pairs || !p.long_scales.empty() || p.nsig < SUM_FLOOR_FROM) return std::string("sum set that no trial sum uses");
    }
    bool all13 = true;
    for (const Group& g : p.sum_set()) all13 = all13 && g.log2n <= 13;
    if (p.sum_pairs != all13) return std::string("sum_pairs");
    // staging rows: a bijection of the scales no direct group serves
    std::vector<int> row(p.nscales, -1);
    std::set<int> rows;
    for (size_t r = 0; r < p.staged.size(); ++r) {
        if (p.staged[r] < 0 || p.staged[r] >= p.nscales || row[p.staged[r]] >= 0) return std::string("staged scale twice");
        row[p.staged[r]] = (int)r;
    }
    const bool fourier = p.output == OUT_FOURIER;
    for (const Group& g : p.groups) {
        if (g.direct != g.sidx_stage.empty()) return std::string("compact rows of a direct group");
        for (int q = 0; q < g.nscales(); ++q) {
            const int sc = g.scale_ids[q];
            if (g.direct) { if (row[sc] >= 0) return std::string("direct scale staged"); continue; }
            if (row[sc] < 0) return fmt("scale %d has no staging row", sc);
            const bool side = g.long_idx >= 0 && !fourier;      // real outputs of a piece: row of the side buffer
            if (g.sidx_stage[q] != (side ? g.long_idx : row[sc]) || g.sidx[q] != (side ? g.long_idx : sc)) return std::string("row tables");
            rows.insert(row[sc]);
        }
    }
    if (rows.size() != p.staged.size()) return std::string("staging row without a scale");
    if (p.lrow.size() != p.long_scales.size()) return std::string("lrow size");
    for (size_t li = 0; li < p.lrow.size(); ++li)
        if (p.lrow[li] != row[p.long_scales[li]]) return std::string("lrow");
    return "";
}

// ---- the invariants of the steps of a call
std::string check_exec(const Plan& p, const ExecQuery& q, const ExecRoute& r) {
    const std::vector<Group>& groups = r.sum_set ? p.groups_sum : p.groups;
    const size_t esz = p.output == OUT_FOURIER ? 8 : 4, per = (size_t)p.nchan * p.nsig;
    const int nlong = (int)p.long_scales.size();
    int next_seg = 0, cur0 = -1, cur_n = 0;
    long long next_item = 0;
    std::vector<int> done;                  // groups run in the current chunk
    bool scattered = false;
    auto close_chunk = [&]() -> std::string {
        if (cur0 < 0) return "";
        if (!q.precision64 && done.size() != groups.size()) return fmt("chunk at %d ran %zu of %zu groups", cur0, done.size(), groups.size());
        if (q.precision64 && next_item != (long long)cur_n * p.nchan) return fmt("chunk at %d: items up to %lld", cur0, next_item);
        const bool staged = q.precision64 || !(q.direct && q.accumulate != 2) || !p.staged.empty();
        if (scattered != staged) return fmt("chunk at %d: transposition %d, staged rows %d", cur0, (int)scattered, (int)staged);
        return "";
    };
    for (const Step& s : r.steps) {
        if (s.gx < 1 || s.gx > 0x7fffffffLL || s.gy < 1 || s.gy > 65535 || s.gz < 1 || s.gz > 65535) return fmt("grid %lldx%lldx%lld", s.gx, s.gy, s.gz);
        if (s.kind == StepKind::MEAN_NP || s.kind == StepKind::TREND) {
            if (s.seg0 != 0 || s.nseg != q.nseg || (size_t)q.nseg * p.nchan * 2 > r.trend || cur0 >= 0) return std::string("trend step");
            continue;
        }
        if (s.seg0 != cur0) {               // a new chunk
            const std::string bad = close_chunk();
            if (!bad.empty()) return bad;
            if (s.seg0 != next_seg || s.nseg < 1 || s.nseg > r.chunk) return fmt("chunk %d+%d after segment %d", s.seg0, s.nseg, next_seg);
            cur0 = s.seg0; cur_n = s.nseg; next_seg = s.seg0 + s.nseg;
            done.clear(); next_item = 0; scattered = false;
        } else if (s.nseg != cur_n) return std::string("chunk length changes");
        const size_t ns = (size_t)s.nseg, nsets = r.pairs ? (ns + 1) / 2 : ns;
        switch (s.kind) {
            case StepKind::INPUT_COPY:
                if (q.precision64 || p.nchan < 2 || ns * per > r.xt) return std::string("input copy");
                if (s.gx * 64 < p.nsig || s.gy * 64 < p.nchan || s.gz != (long long)ns) return std::string("input copy grid");
                break;
            case StepKind::CWT64:
                if (!q.precision64 || s.wg0 != next_item || (size_t)s.gx * 3 * q.L64 > r.work64) return std::string("cwt64 launch");
                next_item += s.gx;
                if (ns * p.nscales * per * esz > r.stage_bytes) return std::string("cwt64 staging");
                break;
            case StepKind::TRANSFORM: {
                if (q.precision64 || s.group != (int)done.size()) return std::string("group order");
                done.push_back(s.group);
                const Group& g = groups[s.group];
                const Engine& e = *engine(g.log2n);
                const bool direct = s.engine == EngineKind::DIRECT, pairs = s.engine == EngineKind::PACKED_PAIRS;
                if (pairs != r.pairs || (pairs && q.accumulate != 2)) return std::string("pairs");
                if (direct && (!g.direct || !q.direct || q.accumulate == 2 || s.target != Target::OUTPUT || s.G != e.Gd)) return std::string("direct step");
                if (!direct && (s.G != e.G || s.target == Target::OUTPUT)) return std::string("staged step");
                if ((s.engine == EngineKind::PLAIN14) != (!direct && g.log2n == 14)) return std::string("engine kind");
                if (s.outk != (g.long_idx >= 0 ? 2 : outk_of(p.output))) return std::string("outk");
                const long long units = s.engine == EngineKind::PLAIN14 || pairs ? p.nchan : (p.nchan + 1) / 2;
                if (s.gx != (long long)(direct ? ns : nsets) * ((units + s.G - 1) / s.G) * g.nblocks) return std::string("transform grid");
                if (direct) break;
                const std::vector<int>& tab = s.sidx == Sidx::COMPACT ? g.sidx_stage : g.sidx;
                if ((int)tab.size() != g.nscales()) return std::string("index table");
                for (int v : tab)
                    if (v < 0 || v >= s.nrows) return fmt("row %d of %d", v, s.nrows);
                if (s.add != (g.long_idx >= 0 && g.piece > 0)) return std::string("add");
                if (s.target == Target::LONG_SIDE) {
                    if (g.long_idx < 0 || esz != 4 || s.nrows != nlong || ns * nlong * per > r.stage_long) return std::string("side buffer");
                } else if (nsets * s.nrows * per * (g.long_idx >= 0 ? 8 : esz) > r.stage_bytes) return std::string("staging size");
                break;
            }
            case StepKind::LONG_CONVERT:
                if (!nlong || esz != 4 || done.size() != groups.size() || (size_t)s.gx * 256 < ns * nlong * per) return std::string("long convert");
                for (int v : s.sidx == Sidx::COMPACT ? p.lrow : p.long_scales)
                    if (v < 0 || v >= s.nrows) return std::string("long row");
                if (ns * s.nrows * per * 4 > r.stage_bytes || ns * nlong * per > r.stage_long) return std::string("long convert sizes");
                break;
            case StepKind::SCATTER:
                if (scattered || s.nsets != (int)nsets || (size_t)s.nsets * s.nrows * per * esz > r.stage_bytes) return std::string("transposition");
                if (s.nrows != (s.compact ? (int)p.staged.size() : p.nscales) || s.gy != s.nrows) return std::string("transposition rows");
                if ((s.scatter == Scatter::COMPLEX) != (esz == 8) || s.gx * (s.scatter == Scatter::WIDE ? 256 : 64) < p.nsig) return std::string("transposition kernel");
                if (s.scatter == Scatter::WIDE && (p.nsig & 3)) return std::string("wide transposition of a ragged length");
                if (s.gz != (q.accumulate == 2 ? 1 : (long long)ns)) return std::string("transposition grid");
                scattered = true;
                break;
            default: return std::string("step kind");
        }
    }
    if (r.err) return "";                   // (the steps up to the error were checked)
    const std::string bad = close_chunk();
    if (!bad.empty()) return bad;
    if (next_seg != q.nseg) return fmt("chunks up to segment %d of %d", next_seg, q.nseg);
    return "";
}

void put(char* dst, int cap, const std::string& s) { std::snprintf(dst, cap, "%s", s.c_str()); }

Case make_case(int family, double p0, double p1, const double* scales, int nscales, double dt, int nsig, int nchan, int output,
               int detrend, const int* tpos) {
    Case c;
    c.family = family; c.p0 = p0; c.p1 = p1; c.dt = dt; c.scales.assign(scales, scales + nscales);
    c.nsig = nsig; c.nchan = nchan; c.output = output; c.detrend = detrend;
    if (tpos) c.tpos.assign(tpos, tpos + nsig);
    return c;
}

}  // namespace

extern "C" {

// the sampled taps of one scale: returns the count; re / im hold up to `cap`
int cwt_taps(int family, double p0, double p1, double scale, double dt, int nsig, double* re, double* im, int cap, int* centre) {
    const Taps k = sample_taps(family, p0, p1, scale, dt, nsig);
    for (size_t m = 0; m < k.re.size() && (int)m < cap; ++m) { re[m] = k.re[m]; im[m] = k.im[m]; }
    *centre = k.c;
    return (int)k.re.size();
}

int cwt_block_length(int ntaps, int floor) { return block_length(ntaps, floor); }

// L of spyhip_cwt_plan_set_precision for these tap counts
long long cwt_conv_length64(int nsig, const int* ntaps, int nscales) { return conv_length64(nsig, std::vector<int>(ntaps, ntaps + nscales)); }

// the plan-creation rule for the direct kernels
int cwt_direct_fits(const int* tpos, int nsig, const int* V, int ngroups, unsigned long long rowb, unsigned long long chanb) {
    return spycwt::cwt_direct_fits(tpos, nsig, V, ngroups, rowb, chanb) ? 1 : 0;
}

// plan: one line per group (cwt_route_text.h); message: the plan's error text, or the shim's verdict on its invariants
int cwt_plan_text(int family, double p0, double p1, const double* scales, int nscales, double dt, int nsig, int nchan, int output,
                  int detrend, const int* tpos, char* plan, char* message, int cap) {
    const Plan p = make_plan(make_case(family, p0, p1, scales, nscales, dt, nsig, nchan, output, detrend, tpos));
    put(plan, cap, p.err ? "" : render_plan(p));
    put(message, cap, p.err ? p.message : check_plan(p));
    return p.err;
}

// steps: one line per step; sizes: chunk, trend, stage bytes, long side buffer, input copy, float64 work (elements), pairs, sum set
int cwt_exec_text(int family, double p0, double p1, const double* scales, int nscales, double dt, int nsig, int nchan, int output,
                  int detrend, const int* tpos, int nseg, int accumulate, int direct, int precision64, long long num_cu,
                  long long stage_budget, long long work_budget, long long* sizes, char* steps, char* message, int cap) {
    const Plan p = make_plan(make_case(family, p0, p1, scales, nscales, dt, nsig, nchan, output, detrend, tpos));
    if (p.err) { put(message, cap, p.message); return p.err; }
    ExecQuery q;
    q.nseg = nseg; q.accumulate = accumulate; q.direct = direct && p.direct_ok; q.precision64 = precision64 != 0;
    q.L64 = precision64 ? conv_length64(nsig, p.ntaps) : 0;
    if (num_cu > 0) q.num_cu = num_cu;
    if (stage_budget > 0) q.stage_budget = (size_t)stage_budget;
    if (work_budget > 0) q.work_budget = (size_t)work_budget;
    const ExecRoute r = exec_route(p, q);
    const long long z[8] = {r.chunk, (long long)r.trend, (long long)r.stage_bytes, (long long)r.stage_long, (long long)r.xt,
                            (long long)r.work64, r.pairs, r.sum_set};
    std::memcpy(sizes, z, sizeof z);
    std::string t;
    for (const Step& s : r.steps) t += render_step(p, r, s) + "\n";
    put(steps, cap, t);
    put(message, cap, r.err ? r.message : check_exec(p, q, r));
    return r.err;
}

// The invariant sweep: `nplans` seeded random plans (every family, 1 ... 30 scales of 5 ... 40000 taps, signals of 1 ... 20000
// samples with the lengths around the thresholds favoured, 1 ... 130 channels, every output class, slots identity / thinned /
// gapped / not increasing), each asked for accumulate 0 / 1 / 2 x direct on / off x both precisions x the library's and
// small budgets.  Returns the queries asked (plans + calls), -1 with `message` at the first violated invariant.
// stats: plans with pieces, with several groups, with a sum set of their own, calls in several chunks, calls on pairs
long long cwt_route_sweep(unsigned seed, int nplans, long long* stats, char* message, int cap) {
    std::mt19937 rng(seed);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    auto unit = [&] { return (rng() >> 8) * (1.0 / 16777216.0); };
    const int edges[] = {1, 2, 3, 63, 64, 255, 1023, 1024, 1025, 2048, 4095, 4096, 4097, 4100, 8192, 16384, 20000};
    long long n = 0;
    for (int i = 0; i < 5; ++i) stats[i] = 0;
    for (int it = 0; it < nplans; ++it) {
        Case c;
        c.family = pick(0, 3);
        c.p0 = c.family == 0 ? 6.0 : c.family == 1 ? pick(1, 4) : pick(1, 6);
        c.p1 = c.family == 1 ? 5.0 : 0.0;
        c.nsig = pick(0, 2) ? edges[pick(0, 16)] : pick(1, 20000);
        c.nchan = pick(0, 3) ? pick(1, 5) : pick(1, 130);
        const int outs[] = {0, 1, 2, 5};
        c.output = outs[pick(0, 3)];
        c.detrend = pick(-1, 1);
        const int nscales = pick(0, 2) ? pick(1, 4) : pick(1, 30);
        const double top = pick(0, 3) ? 0.2 : 4.0;          // (long kernels are the expensive ones to sample: one plan in four)
        for (int s = 0; s < nscales; ++s) {
            double sc = 0.0005 * std::exp(unit() * std::log(top / 0.0005));
            if (c.family == 1) sc /= c.p0;
            c.scales.push_back(sc);
        }
        const int slots = pick(0, 5);
        if (slots >= 3) {
            c.tpos.resize(c.nsig);
            int next = 0;
            for (int t = 0; t < c.nsig; ++t) {
                if (slots == 3) c.tpos[t] = pick(0, 2) ? next++ : -1;               // thinned
                else if (slots == 4) { c.tpos[t] = next; next += 1 + pick(0, 40000); if (next > 2000000000) next = 2000000000; }
                else c.tpos[t] = pick(0, 9) ? t : std::max(0, t - 1);                // some slot twice
            }
        }
        const Plan p = make_plan(c);
        ++n;
        std::string bad = p.err ? (p.err == -3 ? "" : p.message) : check_plan(p);
        bool pieces = false;
        for (const Group& g : p.groups) pieces = pieces || g.long_idx >= 0;
        stats[0] += pieces; stats[1] += p.groups.size() > 1; stats[2] += !p.groups_sum.empty();
        for (int acc = 0; acc < 3 && bad.empty() && !p.err; ++acc)
            for (int direct = 0; direct < 2 && bad.empty(); ++direct)
                for (int p64 = 0; p64 < 2 && bad.empty(); ++p64)
                    for (int small = 0; small < 3 && bad.empty(); ++small) {
                        ExecQuery q;
                        q.nseg = small == 2 && it % 8 == 0 ? pick(60000, 70000) : pick(1, 40);
                        q.accumulate = acc; q.direct = direct && p.direct_ok; q.precision64 = p64 != 0;
                        q.L64 = p64 ? conv_length64(c.nsig, p.ntaps) : 0;
                        q.num_cu = small ? pick(1, 8) : 256;
                        if (small) {
                            const size_t per_seg = (size_t)p.nscales * c.nchan * c.nsig * 8;
                            q.stage_budget = (size_t)(unit() * 6 * per_seg) + 1;
                            q.work_budget = (size_t)(unit() * 40 * 48 * (p64 ? q.L64 : 16)) + 1;
                        }
                        const ExecRoute r = exec_route(p, q);
                        ++n;
                        bad = check_exec(p, q, r);
                        if (r.err && r.err != -1) bad = "error code";
                        int chunks = 0;
                        for (const Step& s : r.steps) chunks += s.kind == StepKind::SCATTER;
                        stats[3] += chunks > 1; stats[4] += r.pairs;
                        if (!bad.empty()) bad += fmt(" (nseg %d accumulate %d direct %d precision64 %d num_cu %lld budgets %zu %zu)", q.nseg, acc,
                                                     direct, p64, q.num_cu, q.stage_budget, q.work_budget);
                    }
        if (!bad.empty()) {
            std::string sc;
            for (double v : c.scales) sc += fmt(" %.9g", v);
            put(message, cap, fmt("plan %d: family %d p0 %g nsig %d nchan %d output %d slots %d scales", it, c.family, c.p0, c.nsig,
                                  c.nchan, c.output, slots) + sc + ": " + bad);
            return -1;
        }
    }
    return n;
}
}

#ifdef CWT_ROUTE_MAIN
int main(int argc, char** argv) {
    const int nplans = argc > 1 ? std::atoi(argv[1]) : 400;
    long long stats[5];
    char msg[4096] = "";
    const long long n = cwt_route_sweep(20261018u, nplans, stats, msg, sizeof msg);
    std::printf("queries %lld (plans with pieces %lld, several groups %lld, own sum set %lld; calls in chunks %lld, on pairs %lld) %s\n", n,
                stats[0], stats[1], stats[2], stats[3], stats[4], msg);
    return n < 0;
}
#endif
