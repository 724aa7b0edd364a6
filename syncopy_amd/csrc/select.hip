// Launcher of the data selection (kernels in select_kernel.h, decisions in select_route.h): one launch per call, whatever
// the number of trials.  Every buffer belongs to the caller; nothing here allocates or synchronises.
#include "spy_common.h"
#include "select_kernel.h"

namespace {

using namespace spysel;

template <class L>
void launch(spyhip_ctx* ctx, const Args& g, int mode) {
    const long long nitem = (g.nrows * g.wo) >> g.vshift;
    long long blocks = (nitem + THREADS - 1) / THREADS;
    if (blocks > ctx->limits.elementwise_blocks) blocks = ctx->limits.elementwise_blocks;
    const dim3 grid((unsigned)(blocks < 1 ? 1 : blocks)), block(THREADS);
    if (mode == FLAT)
        hipLaunchKernelGGL((select_kernel<L, FLAT>), grid, block, 0, ctx->stream, g);
    else if (mode == AXES_LDS)
        hipLaunchKernelGGL((select_kernel<L, AXES_LDS>), grid, block, 0, ctx->stream, g);
    else
        hipLaunchKernelGGL((select_kernel<L, AXES>), grid, block, 0, ctx->stream, g);
}

}  // namespace

extern "C" int spyhip_select(spyhip_ctx* ctx, int elem_bytes, const void* src_d, int64_t src_rows, const int64_t* extent,
                             const int32_t* kind, const int64_t* start, const int64_t* count, const int32_t* idx,
                             const int32_t* idx_d, const int64_t* desc, const int64_t* desc_d, int64_t ntrials, void* out_d,
                             int64_t out_rows) {
    if (!ctx || !src_d || !out_d || !extent || !kind || !start || !count || !desc || !desc_d || (!idx != !idx_d)) {
        spy::set_error("select: bad argument");
        return -1;
    }
    const Route r = select_route(elem_bytes, src_rows, out_rows, extent, kind, start, count, idx, desc, ntrials,
                                 (uint64_t)reinterpret_cast<uintptr_t>(src_d), (uint64_t)reinterpret_cast<uintptr_t>(out_d));
    if (r.err) {
        spy::set_error("select: %s", r.err);
        return -1;
    }
    if (r.nrows == 0) return 0;
    Args g;
    g.src = src_d; g.out = out_d; g.desc = (const long long*)desc_d; g.idx = idx_d;
    g.ntrials = ntrials; g.row0 = r.row0; g.nrows = r.nrows; g.wo = r.wo; g.ws = r.ws;
    for (int i = 0; i < 3; ++i) { g.n[i] = r.n[i]; g.s[i] = r.s[i]; g.start[i] = r.start[i]; g.loff[i] = r.loff[i]; }
    g.nidx = (int)(r.mode == AXES_LDS ? r.nidx : 0);
    g.vshift = 0;
    for (int v = r.lane_bytes / elem_bytes; v > 1; v >>= 1) ++g.vshift;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    if (r.lane_bytes == 16) {
        if (r.lane_aligned) launch<Lane16>(ctx, g, r.mode); else launch<Lane16e>(ctx, g, r.mode);
    } else if (r.lane_bytes == 8) {
        launch<Lane8>(ctx, g, r.mode);
    } else {
        launch<Lane4>(ctx, g, r.mode);
    }
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}
