// Launchers of the synthetic-data kernels (kernels in synth_kernel.h, decisions in synth_route.h): one launch per call.
// Every buffer belongs to the caller; nothing here allocates or synchronises.
#include "spy_common.h"
#include "synth_kernel.h"

namespace {

using namespace spysyn;

template <bool CSR_LDS>
int launch_coupled(spyhip_ctx* ctx, const Ar2Route& r, const Ar2Args& g) {
    auto kern = ar2_coupled_kernel<CSR_LDS>;
    SPY_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)r.lds_bytes));
    hipLaunchKernelGGL(kern, dim3((unsigned)r.grid), dim3((unsigned)r.block), r.lds_bytes, ctx->stream, g);
    return 0;
}

template <class L>
void launch_tile(spyhip_ctx* ctx, const TileRoute& r, const float* col_d, int64_t nsamples, int64_t nchan, float* out_d) {
    hipLaunchKernelGGL((tile_kernel<L>), dim3((unsigned)r.grid), dim3(TILE_THREADS), 0, ctx->stream, col_d,
                       (long long)nsamples, (long long)(nchan / (int64_t)(sizeof(L) / 4)), r.lanes, reinterpret_cast<L*>(out_d));
}

}  // namespace

extern "C" int spyhip_synth_ar2(spyhip_ctx* ctx, const double* noise_d, int64_t ntrials, int64_t nsamples, int nchan,
                                double alpha1, double alpha2, const int32_t* rowptr, const int32_t* col,
                                const int32_t* rowptr_d, const int32_t* col_d, const float* w_d, float* out_d) {
    if (!ctx || !noise_d || !rowptr || !rowptr_d || !out_d) {
        spy::set_error("synth_ar2: bad argument");
        return -1;
    }
    // (an empty table may come without its arrays)
    if (nchan >= 1 && nchan <= MAX_CHAN && rowptr[nchan] != 0 && (!col || !col_d || !w_d)) {
        spy::set_error("synth_ar2: bad argument");
        return -1;
    }
    const Ar2Route r = ar2_route(ntrials, nsamples, nchan, rowptr, col, ctx->lds_per_block);
    if (r.err) {
        spy::set_error("synth_ar2: %s", r.err);
        return -1;
    }
    if (ntrials == 0) return 0;
    Ar2Args g;
    g.noise = noise_d; g.rowptr = rowptr_d; g.col = col_d; g.w = w_d; g.out = out_d;
    g.alpha1 = alpha1; g.alpha2 = (float)alpha2; g.nsamples = nsamples; g.nchan = nchan; g.nnz = (int)r.nnz;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    if (!r.coupled) {
        hipLaunchKernelGGL(ar2_series_kernel, dim3((unsigned)r.grid), dim3((unsigned)r.block), 0, ctx->stream, g,
                           (long long)(ntrials * nchan));
    } else if (r.csr_in_lds) {
        if (int rc = launch_coupled<true>(ctx, r, g)) return rc;
    } else {
        if (int rc = launch_coupled<false>(ctx, r, g)) return rc;
    }
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_synth_phase(spyhip_ctx* ctx, const float* wn_d, const float* lin_d, const float* ps0_d, double rel_eps,
                                  int64_t ntrials, int64_t nsamples, int nchan, int want_cos, float* out_d) {
    if (!ctx || !wn_d || !lin_d || !ps0_d || !out_d) {
        spy::set_error("synth_phase: bad argument");
        return -1;
    }
    const SeriesRoute r = phase_route(ntrials, nsamples, nchan);
    if (r.err) {
        spy::set_error("synth_phase: %s", r.err);
        return -1;
    }
    if (ntrials == 0) return 0;
    PhaseArgs g;
    g.wn = wn_d; g.lin = lin_d; g.ps0 = ps0_d; g.out = out_d; g.rel_eps = (float)rel_eps;
    g.nsamples = nsamples; g.nseries = ntrials * nchan; g.nchan = nchan; g.want_cos = want_cos != 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(phase_kernel, dim3((unsigned)r.grid), dim3((unsigned)r.block), 0, ctx->stream, g);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_synth_tile(spyhip_ctx* ctx, const float* col_d, int64_t ntrials, int64_t nsamples, int nchan,
                                 float* out_d) {
    if (!ctx || !col_d || !out_d) {
        spy::set_error("synth_tile: bad argument");
        return -1;
    }
    const TileRoute r = tile_route(ntrials, nsamples, nchan, (uint64_t)reinterpret_cast<uintptr_t>(out_d),
                                   ctx->limits.elementwise_blocks);
    if (r.err) {
        spy::set_error("synth_tile: %s", r.err);
        return -1;
    }
    if (r.lanes == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    if (r.lane_bytes == 16) launch_tile<Lane16>(ctx, r, col_d, nsamples, nchan, out_d);
    else launch_tile<Lane4>(ctx, r, col_d, nsamples, nchan, out_d);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}
