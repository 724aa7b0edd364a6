// Launcher of the channel concatenation (kernel in concat_kernel.h, decisions in concat_route.h): one launch per call,
// whatever the number of trials or sources.  Every buffer belongs to the caller; nothing here allocates or synchronises.
#include "spy_common.h"
#include "concat_kernel.h"

namespace {

using namespace spycat;

template <class L>
void launch(spyhip_ctx* ctx, const Args& g) {
    const long long nitem = g.nrows * g.pre * g.w;
    long long blocks = (nitem + THREADS - 1) / THREADS;
    if (blocks > ctx->limits.elementwise_blocks) blocks = ctx->limits.elementwise_blocks;
    const dim3 grid((unsigned)(blocks < 1 ? 1 : blocks)), block(THREADS);
    hipLaunchKernelGGL((concat_kernel<L>), grid, block, 0, ctx->stream, g);
}

}  // namespace

extern "C" int spyhip_concat(spyhip_ctx* ctx, int elem_bytes, int nsrc, const void* const* src_d, const int64_t* src_rows,
                             const int64_t* run, int64_t pre, const int64_t* desc, const int64_t* desc_d, int64_t ntrials,
                             void* out_d, int64_t out_rows) {
    if (!ctx || !src_d || !src_rows || !run || !desc || !desc_d || !out_d) {
        spy::set_error("concat: bad argument");
        return -1;
    }
    uint64_t addr[MAX_SRC] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < nsrc && s < MAX_SRC; ++s) {
        if (!src_d[s]) {
            spy::set_error("concat: bad argument");
            return -1;
        }
        addr[s] = (uint64_t)reinterpret_cast<uintptr_t>(src_d[s]);
    }
    const Route r = concat_route(elem_bytes, nsrc, src_rows, run, pre, desc, ntrials, addr,
                                 (uint64_t)reinterpret_cast<uintptr_t>(out_d), out_rows);
    if (r.err) {
        spy::set_error("concat: %s", r.err);
        return -1;
    }
    if (r.nrows == 0) return 0;
    const long long v = r.lane_bytes / elem_bytes;              // elements of a lane: every run is a multiple
    Args g;
    for (int s = 0; s < MAX_SRC; ++s) g.src[s] = src_d[s < nsrc ? s : nsrc - 1];
    for (int s = 0; s <= MAX_SRC; ++s) g.cum[s] = r.cum[s < nsrc ? s : nsrc] / v;
    g.out = out_d; g.desc = (const long long*)desc_d;
    g.ntrials = ntrials; g.row0 = r.row0; g.nrows = r.nrows; g.pre = pre; g.w = r.w / v;
    g.nsrc = nsrc;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    if (r.lane_bytes == 16) {
        if (r.lane_aligned) launch<Lane16>(ctx, g); else launch<Lane16e>(ctx, g);
    } else if (r.lane_bytes == 8) {
        launch<Lane8>(ctx, g);
    } else {
        launch<Lane4>(ctx, g);
    }
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}
