// Host side of K12: the envelope correlations (spyhip_envcorr_accumulate / spyhip_envcorr_finalize).
#include "spy_common.h"
#include "envcorr_kernel.h"

static bool known_measure(int measure) {
    return measure == SPYHIP_ENVCORR_AMPL || measure == SPYHIP_ENVCORR_POW || measure == SPYHIP_ENVCORR_POW_ORTHO;
}

template <int M>
static int launch_accumulate(spyhip_ctx* ctx, const spyenvcorr::EnvcorrArgs& a, unsigned blocks) {
    // two buffers of 2 x 32 channels x ntaper staged values: 1 KiB per taper (amplcorr, powcorr), 2 KiB (powcorr_ortho)
    const size_t lds = 2 * (size_t)2 * a.ntaper * 32 * sizeof(typename spyenvcorr::Staged<M>::type);
    if (lds > ctx->lds_per_block) { spy::set_error("envcorr_accumulate: %d tapers do not fit the LDS staging buffer", a.ntaper); return -3; }
    SPY_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(spyenvcorr::envcorr_accum_kernel<M>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(spyenvcorr::envcorr_accum_kernel<M>, dim3(blocks), dim3(256), lds, ctx->stream, a);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_envcorr_accumulate(spyhip_ctx* ctx, const void* spec_d, int ntrials, int ntaper, int nfreq, int nchan,
                                         int measure, void* pair_d, void* chan_d) {
    if (!ctx || !spec_d || !pair_d || !chan_d) { spy::set_error("envcorr_accumulate: null argument"); return -1; }
    if (ntrials < 0 || ntaper < 1 || nfreq < 1 || nchan < 1) { spy::set_error("envcorr_accumulate: bad shape"); return -1; }
    if (!known_measure(measure)) { spy::set_error("envcorr_accumulate: unknown measure %d", measure); return -1; }
    if (ntrials == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    spyenvcorr::EnvcorrArgs a{};
    a.spec = reinterpret_cast<const float2*>(spec_d);
    a.ntrials = ntrials; a.ntaper = ntaper; a.F = nfreq; a.C = nchan;
    a.pair = reinterpret_cast<double*>(pair_d);
    a.chan = reinterpret_cast<double*>(chan_d);
    const long long nt = (nchan + 31) / 32, blocks = 8LL * ((nfreq + 7) / 8) * (nt * (nt + 1) / 2);   // 8 XCDs x frequencies each
    if (blocks > 0x7fffffffLL) { spy::set_error("envcorr_accumulate: grid too large"); return -1; }
    if (measure == SPYHIP_ENVCORR_AMPL) return launch_accumulate<SPYHIP_ENVCORR_AMPL>(ctx, a, (unsigned)blocks);
    if (measure == SPYHIP_ENVCORR_POW) return launch_accumulate<SPYHIP_ENVCORR_POW>(ctx, a, (unsigned)blocks);
    return launch_accumulate<SPYHIP_ENVCORR_POW_ORTHO>(ctx, a, (unsigned)blocks);
}

extern "C" int spyhip_envcorr_finalize(spyhip_ctx* ctx, const void* pair_d, const void* chan_d, int nfreq, int nchan,
                                       int64_t nrep, int measure, void* out_d) {
    if (!ctx || !pair_d || !chan_d || !out_d) { spy::set_error("envcorr_finalize: null argument"); return -1; }
    if (nfreq < 1 || nchan < 1) { spy::set_error("envcorr_finalize: bad shape"); return -1; }
    if (nrep < 2) { spy::set_error("envcorr_finalize: at least two repetitions are needed"); return -1; }
    if (!known_measure(measure)) { spy::set_error("envcorr_finalize: unknown measure %d", measure); return -1; }
    const long long blocks = ((long long)nfreq * nchan * nchan + 255) / 256;
    if (blocks > 0x7fffffffLL) { spy::set_error("envcorr_finalize: grid too large"); return -1; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(spyenvcorr::envcorr_finalize_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const double*>(pair_d), reinterpret_cast<const double*>(chan_d), nfreq, nchan,
                       (double)nrep, measure, reinterpret_cast<float*>(out_d));
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}
