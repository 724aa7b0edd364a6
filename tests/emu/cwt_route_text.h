// Text form of the wavelet route (syncopy_amd/csrc/cwt_route.h), one line per group and per step, for the pinned plans of
// tests/test_cwt_route.py and the emulator's record of what it ran (TEST INFRASTRUCTURE ONLY).
#pragma once
#include <string>

#include "../../syncopy_amd/csrc/cwt_route.h"

namespace spycwt {

inline std::string join(const std::vector<int>& v) {
    std::string t;
    for (size_t i = 0; i < v.size(); ++i) t += (i ? "," : "") + std::to_string(v[i]);
    return t.empty() ? "-" : t;
}

inline std::string render_group(const Group& g) {
    const std::string head = g.long_idx >= 0 ? fmt("piece %d of long scale %d taps %d+%d", g.piece, g.long_idx, g.tap0, g.ntaps)
                                             : fmt("group 2^%d%s", g.log2n, g.direct ? " direct" : "");
    return head + fmt(" V %d halo %d nblocks %d", g.V, g.halo, g.nblocks) + " scales " + join(g.scale_ids) + " cshift " +
           join(g.cshift) + " sidx " + join(g.sidx) + " compact " + join(g.sidx_stage);
}

inline std::string render_plan(const Plan& p) {
    std::string t = "taps " + join(p.ntaps) + "\n";
    for (const Group& g : p.groups) t += render_group(g) + "\n";
    for (const Group& g : p.groups_sum) t += "sum " + render_group(g) + "\n";
    t += "staged " + join(p.staged) + " long " + join(p.long_scales) + " lrow " + join(p.lrow) +
         fmt(" sum_pairs %d direct_ok %d\n", (int)p.sum_pairs, (int)p.direct_ok);
    return t;
}

// (the kernel instance first, as the kernel's template arguments)
inline std::string render_step(const Plan& p, const ExecRoute& r, const Step& s) {
    const std::string seg = fmt(" seg %d+%d", s.seg0, s.nseg), grid = fmt(" grid %lldx%lldx%lld", s.gx, s.gy, s.gz);
    switch (s.kind) {
        case StepKind::MEAN_NP: return "cwt_mean_np" + seg + grid;
        case StepKind::TREND: return "cwt_trend" + seg + grid;
        case StepKind::INPUT_COPY: return "cwt_stage_input" + seg + grid;
        case StepKind::CWT64: return fmt("cwt64<%d>", s.outk) + seg + fmt(" wg0 %lld", s.wg0) + grid;
        case StepKind::TRANSFORM: {
            const Group& g = (r.sum_set ? p.groups_sum : p.groups)[s.group];
            const char* kern = s.engine == EngineKind::DIRECT ? "cwt2d" : s.engine == EngineKind::PLAIN14 ? "cwt" : "cwt2";
            return fmt("%s<%d,%d,%d%s>", kern, g.log2n, s.G, s.outk, s.engine == EngineKind::PACKED_PAIRS ? ",pairs" : "") + seg +
                   fmt(" %sgroup %d sidx %s rows %d -> %s%s", r.sum_set ? "sum " : "", s.group, s.sidx == Sidx::COMPACT ? "compact" : "full",
                       s.nrows, s.target == Target::OUTPUT ? "output" : s.target == Target::STAGE ? "stage" : "long side", s.add ? " add" : "") +
                   grid;
        }
        case StepKind::LONG_CONVERT:
            return "cwt_long_convert" + seg + fmt(" lidx %s rows %d", s.sidx == Sidx::COMPACT ? "compact" : "full", s.nrows) + grid;
        case StepKind::SCATTER:
            return fmt("cwt_scatter<%s>", s.scatter == Scatter::COMPLEX ? "float2" : s.scatter == Scatter::WIDE ? "wide" : "float") + seg +
                   fmt(" sets %d rows %d%s", s.nsets, s.nrows, s.compact ? " compact" : "") + grid;
    }
    return "";
}

}  // namespace spycwt
