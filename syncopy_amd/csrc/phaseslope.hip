// Host side of K13: the phase slope index (spyhip_phaseslope / spyhip_phaseslope_from_accumulator).
#include "spy_common.h"
#include <algorithm>
#include "phaseslope_kernel.h"

template <bool RAW>
static int phaseslope_impl(spyhip_ctx* ctx, const char* who, const void* in_d, int nfreq, int nchan, double scale, int half,
                           void* out_d) {
    if (!ctx || !in_d || !out_d) { spy::set_error("%s: null argument", who); return -1; }
    if (nfreq < 2 || nchan < 1) { spy::set_error("%s: bad shape", who); return -1; }
    if (half < 0 || 2LL * half > (long long)nfreq - 1) {
        spy::set_error("%s: a band of 2 x %d bins does not fit %d frequencies", who, half, nfreq);
        return -1;
    }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const long long nt = (nchan + 31) / 32, ntiles = nt * (nt + 1) / 2;
    spyphaseslope::PhaseSlopeArgs a{};
    a.in = reinterpret_cast<const float2*>(in_d);
    a.F = nfreq; a.C = nchan; a.scale = (float)scale; a.half = half;
    a.out = reinterpret_cast<float*>(out_d);
    if (half > 0)
        a.nruns = spyphaseslope::plan_runs(nfreq - 2 * half, std::max(2 * half, spyphaseslope::MIN_RUN), ntiles, ctx->num_cu, a.run);
    else
        a.nruns = spyphaseslope::plan_runs(nfreq - 1, spyphaseslope::MIN_RUN0, ntiles, ctx->num_cu, a.run);
    const long long blocks = ntiles * a.nruns;
    if (blocks > 0x7fffffffLL) { spy::set_error("%s: grid too large", who); return -1; }
    if (half == 0 && a.nruns > 1) {
        if (spy::reserve_scratch(ctx, (size_t)a.nruns * nchan * nchan * sizeof(double))) return -2;
        a.part = reinterpret_cast<double*>(ctx->scratch);
    }
    hipLaunchKernelGGL(spyphaseslope::phaseslope_kernel<RAW>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, a);
    SPY_HIP_CHECK(hipGetLastError());
    if (a.part) {
        hipLaunchKernelGGL(spyphaseslope::phaseslope_reduce_kernel, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream,
                           a.part, a.nruns, nchan, a.out);
        SPY_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

extern "C" int spyhip_phaseslope(spyhip_ctx* ctx, const void* csd_d, int nfreq, int nchan, int half, void* out_d) {
    return phaseslope_impl<false>(ctx, "phaseslope", csd_d, nfreq, nchan, 1.0, half, out_d);
}

extern "C" int spyhip_phaseslope_from_accumulator(spyhip_ctx* ctx, const void* acc_d, int nfreq, int nchan, double scale,
                                                  int half, void* out_d) {
    return phaseslope_impl<true>(ctx, "phaseslope_from_accumulator", acc_d, nfreq, nchan, scale, half, out_d);
}
