// Launchers of spy.preprocessing: detrending, z-score, Butterworth (second-order sections) and windowed-sinc filtering
// of batches of equal-length trials (kernels in preproc_kernel.h).
#include "spy_common.h"
#include "preproc_kernel.h"

#include <climits>

namespace {

using spypre::SosCoef;

// the FIR tile the library launches: 16 outputs per lane, 8 waves, 128 taps per LDS stage (65 280 bytes of LDS, two
// workgroups per CU)
constexpr int FIR_R = 16, FIR_NT = 8, FIR_KC = 128;

// shapes every kernel here can address: offsets inside one trial are 32-bit, one thread per series
int check_batch(const char* who, int64_t ntrials, int64_t nsamp, int64_t nchan, int64_t extra_rows) {
    if (ntrials < 0 || nsamp < 1 || nchan < 1) { spy::set_error("%s: bad shape", who); return -1; }
    if ((nsamp + extra_rows) * nchan > (int64_t)INT_MAX) {
        spy::set_error("%s: %lld samples x %lld channels per trial (at most 2^31 - 1 elements)", who,
                       (long long)(nsamp + extra_rows), (long long)nchan);
        return -1;
    }
    if (ntrials > INT_MAX || (ntrials * nchan + spypre::SERIES_THREADS - 1) / spypre::SERIES_THREADS > (int64_t)INT_MAX) {
        spy::set_error("%s: %lld trials x %lld channels in one call", who, (long long)ntrials, (long long)nchan);
        return -1;
    }
    return 0;
}

dim3 series_grid(int64_t ntrials, int64_t nchan) {
    return dim3((unsigned)((ntrials * nchan + spypre::SERIES_THREADS - 1) / spypre::SERIES_THREADS));
}

int fill_sos(const char* who, const double* sos, const double* zi, int nsec, SosCoef* k) {
    if (!sos || nsec < 1 || nsec > spypre::MAX_SECTIONS) {
        spy::set_error("%s: %d second-order sections (1 ... %d)", who, nsec, spypre::MAX_SECTIONS);
        return -1;
    }
    std::memset(k, 0, sizeof(*k));
    k->nsec = nsec;
    for (int s = 0; s < nsec; ++s) {
        const double* r = sos + 6 * s;
        if (r[3] != 1.0) { spy::set_error("%s: section %d is not normalised (a0 = %g)", who, s, r[3]); return -1; }
        k->c[s][0] = r[0]; k->c[s][1] = r[1]; k->c[s][2] = r[2]; k->c[s][3] = r[4]; k->c[s][4] = r[5];
        if (zi) { k->zi[s][0] = zi[2 * s]; k->zi[s][1] = zi[2 * s + 1]; }
    }
    return 0;
}

// spyhip_fir_same behind its pointer checks, on the tile FirTile<R, NT, KC>
template <int R, int NT, int KC>
int fir_launch(spyhip_ctx* ctx, const float* in_d, float* out_d, int64_t ntrials, int64_t nsamp, int64_t nchan,
               const double* taps_d, int ntaps, int rectify, int32_t* nan_d) {
    using Tile = spypre::FirTile<R, NT, KC>;
    if (check_batch("fir_same", ntrials, nsamp, nchan, 0)) return -1;
    // the staging of a tile looks (ntaps + tile) samples to either side of it
    if (nsamp + (int64_t)ntaps + Tile::T + KC > (int64_t)INT_MAX / 2) { spy::set_error("fir_same: %d taps on %lld samples", ntaps, (long long)nsamp); return -1; }
    const int64_t max_yz = ctx->limits.grid_yz;
    const int64_t ytiles = (nsamp + Tile::T - 1) / Tile::T;
    if (ytiles > max_yz) { spy::set_error("fir_same: %lld samples per trial (at most %lld)", (long long)nsamp, (long long)(max_yz * Tile::T)); return -1; }
    if (ntrials == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const int N = (int)nsamp, C = (int)nchan;
    for (int64_t t0 = 0; t0 < ntrials; t0 += max_yz) {          // grid.z carries the trial
        const unsigned nz = (unsigned)((ntrials - t0) < max_yz ? (ntrials - t0) : max_yz);
        const dim3 g((unsigned)((nchan + 63) / 64), (unsigned)ytiles, nz), b(Tile::THREADS);
        const float* in = in_d + t0 * nsamp * nchan;
        float* out = out_d + t0 * nsamp * nchan;
        if (rectify)
            hipLaunchKernelGGL((spypre::fir_same_kernel<R, NT, KC, true>), g, b, Tile::LDS_BYTES, ctx->stream,
                               in, out, taps_d, ntaps, N, C, nan_d + t0);
        else
            hipLaunchKernelGGL((spypre::fir_same_kernel<R, NT, KC, false>), g, b, Tile::LDS_BYTES, ctx->stream,
                               in, out, taps_d, ntaps, N, C, nan_d + t0);
        SPY_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" int spyhip_detrend(spyhip_ctx* ctx, const float* in_d, float* out_d, int64_t ntrials, int64_t nsamp,
                              int64_t nchan, int order, int rectify, int32_t* nan_d) {
    if (!ctx || !in_d || !out_d || !nan_d || (order != 0 && order != 1)) { spy::set_error("detrend: bad argument"); return -1; }
    if (check_batch("detrend", ntrials, nsamp, nchan, 0)) return -1;
    if (ntrials == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const dim3 g = series_grid(ntrials, nchan), b(spypre::SERIES_THREADS);
    const int T = (int)ntrials, N = (int)nsamp, C = (int)nchan;
    switch (2 * order + (rectify ? 1 : 0)) {
        case 0: hipLaunchKernelGGL((spypre::detrend_kernel<0, false>), g, b, 0, ctx->stream, in_d, out_d, T, N, C, nan_d); break;
        case 1: hipLaunchKernelGGL((spypre::detrend_kernel<0, true>), g, b, 0, ctx->stream, in_d, out_d, T, N, C, nan_d); break;
        case 2: hipLaunchKernelGGL((spypre::detrend_kernel<1, false>), g, b, 0, ctx->stream, in_d, out_d, T, N, C, nan_d); break;
        default: hipLaunchKernelGGL((spypre::detrend_kernel<1, true>), g, b, 0, ctx->stream, in_d, out_d, T, N, C, nan_d); break;
    }
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_standardize(spyhip_ctx* ctx, const float* in_d, float* out_d, int64_t ntrials, int64_t nsamp,
                                  int64_t nchan, int rectify, int32_t* nan_d) {
    if (!ctx || !in_d || !out_d || !nan_d || in_d == out_d) { spy::set_error("standardize: bad argument"); return -1; }
    if (check_batch("standardize", ntrials, nsamp, nchan, 0)) return -1;
    if (ntrials == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const dim3 g = series_grid(ntrials, nchan), b(spypre::SERIES_THREADS);
    const int T = (int)ntrials, N = (int)nsamp, C = (int)nchan;
    if (rectify) hipLaunchKernelGGL(spypre::standardize_kernel<true>, g, b, 0, ctx->stream, in_d, out_d, T, N, C, nan_d);
    else hipLaunchKernelGGL(spypre::standardize_kernel<false>, g, b, 0, ctx->stream, in_d, out_d, T, N, C, nan_d);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_sosfilt(spyhip_ctx* ctx, const float* in_d, float* out_d, int64_t ntrials, int64_t nsamp,
                              int64_t nchan, const double* sos, int nsec, int rectify, int32_t* nan_d) {
    if (!ctx || !in_d || !out_d || !nan_d) { spy::set_error("sosfilt: bad argument"); return -1; }
    if (check_batch("sosfilt", ntrials, nsamp, nchan, 0)) return -1;
    SosCoef k;
    if (fill_sos("sosfilt", sos, nullptr, nsec, &k)) return -1;
    if (ntrials == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const dim3 g = series_grid(ntrials, nchan), b(spypre::SERIES_THREADS);
    const int T = (int)ntrials, N = (int)nsamp, C = (int)nchan;
#define SPY_ONEPASS(NS)                                                                                                  \
    if (rectify) hipLaunchKernelGGL((spypre::sos_onepass_kernel<NS, true>), g, b, 0, ctx->stream, in_d, out_d, k, T, N, C, nan_d); \
    else hipLaunchKernelGGL((spypre::sos_onepass_kernel<NS, false>), g, b, 0, ctx->stream, in_d, out_d, k, T, N, C, nan_d)
    SPY_SOS_DISPATCH(nsec, SPY_ONEPASS);
#undef SPY_ONEPASS
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_sosfiltfilt(spyhip_ctx* ctx, const float* in_d, float* out_d, double* work_d, int64_t ntrials,
                                  int64_t nsamp, int64_t nchan, const double* sos, const double* zi, int nsec, int edge,
                                  int rectify, int32_t* nan_d) {
    if (!ctx || !in_d || !out_d || !work_d || !nan_d || !zi || edge < 0) { spy::set_error("sosfiltfilt: bad argument"); return -1; }
    if (check_batch("sosfiltfilt", ntrials, nsamp, nchan, 2 * (int64_t)edge)) return -1;
    if (nsamp <= edge) {
        spy::set_error("sosfiltfilt: the trials (%lld samples) must be longer than the padding (%d)", (long long)nsamp, edge);
        return -1;
    }
    SosCoef k;
    if (fill_sos("sosfiltfilt", sos, zi, nsec, &k)) return -1;
    if (ntrials == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const dim3 g = series_grid(ntrials, nchan), b(spypre::SERIES_THREADS);
    const int T = (int)ntrials, N = (int)nsamp, C = (int)nchan;
#define SPY_FORWARD(NS) hipLaunchKernelGGL(spypre::sos_forward_kernel<NS>, g, b, 0, ctx->stream, in_d, work_d, k, T, N, C, edge, nan_d)
    SPY_SOS_DISPATCH(nsec, SPY_FORWARD);
#undef SPY_FORWARD
    SPY_HIP_CHECK(hipGetLastError());
#define SPY_BACKWARD(NS)                                                                                                 \
    if (rectify) hipLaunchKernelGGL((spypre::sos_backward_kernel<NS, true>), g, b, 0, ctx->stream, work_d, out_d, k, T, N, C, edge); \
    else hipLaunchKernelGGL((spypre::sos_backward_kernel<NS, false>), g, b, 0, ctx->stream, work_d, out_d, k, T, N, C, edge)
    SPY_SOS_DISPATCH(nsec, SPY_BACKWARD);
#undef SPY_BACKWARD
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_fir_same(spyhip_ctx* ctx, const float* in_d, float* out_d, int64_t ntrials, int64_t nsamp,
                               int64_t nchan, const double* taps_d, int ntaps, int rectify, int32_t* nan_d) {
    if (!ctx || !in_d || !out_d || !nan_d || !taps_d || ntaps < 1 || in_d == out_d) { spy::set_error("fir_same: bad argument"); return -1; }
    return fir_launch<FIR_R, FIR_NT, FIR_KC>(ctx, in_d, out_d, ntrials, nsamp, nchan, taps_d, ntaps, rectify, nan_d);
}
