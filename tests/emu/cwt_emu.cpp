// CPU emulation of the wavelet plan (K3), TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's own plan and exec entry
// points (syncopy_amd/csrc/cwt.hip) and kernels, on the runtime stand-in hip/hip_runtime.h.  Built by
// __graft_entry__.build() and tests/cwt_drive.py.
#include "hip_emu.h"
#include "../../syncopy_amd/csrc/cwt.hip"
#include "emu_unit.h"
#include "cwt_route_text.h"

// the two byte budgets of spyhip_cwt_exec, which like the other launch limits no API sets: a value > 0 replaces the route's own
extern "C" void emu_ctx_set_cwt_budgets(spyhip_ctx* ctx, long long stage_bytes, long long work64_bytes) {
    if (stage_bytes > 0) ctx->limits.cwt_stage_bytes = stage_bytes;
    if (work64_bytes > 0) ctx->limits.cwt_work64_bytes = work64_bytes;
}

// the steps spyhip_cwt_exec(plan, ..., nseg, ..., accumulate) walks, one line each (cwt_route_text.h), from the query that
// call makes; returns the route's error code
extern "C" int emu_cwt_trace(const spyhip_cwt_plan* p, int nseg, int accumulate, char* text, int cap) {
    const spycwt::ExecRoute r = spycwt::exec_route(p->r, exec_query(p, nseg, accumulate));
    std::string t;
    for (const spycwt::Step& s : r.steps) t += spycwt::render_step(p->r, r, s) + "\n";
    std::snprintf(text, cap, "%s", t.c_str());
    return r.err;
}
