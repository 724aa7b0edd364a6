// Launcher of spy.resampledata: the up-FIR-down kernel of resample_kernel.h over batches of equal-length trials.
#include "spy_common.h"
#include "resample_kernel.h"

#include <climits>

namespace {

// the tiles the library launches: 8 waves share chunks of 128 taps of a phase; 8, 4 or 1 outputs per lane, the most
// whose (R - 1) * down + 128 staged rows fit MAX_ROWS (64 KiB of LDS, two workgroups per CU)
constexpr int UFD_NT = 8, UFD_KC = 128;
constexpr long long MAX_ROWS = 256;

template <int R>
int launch(spyhip_ctx* ctx, const float* in_d, float* out_d, int64_t ntrials, int64_t nsamp, int64_t nchan, int64_t nout,
           const double* taps_d, int ntaps, int up, int down) {
    using Tile = spyres::UpfirdnTile<R, UFD_NT, UFD_KC>;
    const int64_t per_phase = (nout + up - 1) / up;
    const int64_t ublocks = (per_phase + R - 1) / R;
    if (ublocks > (int64_t)INT_MAX / up) {
        spy::set_error("upfirdn: %lld outputs in %d phases per trial", (long long)nout, up);
        return -1;
    }
    const unsigned lds = (unsigned)Tile::lds_bytes(down);
    for (int64_t t0 = 0; t0 < ntrials; t0 += 65535) {          // grid.z carries the trial
        const unsigned nz = (unsigned)((ntrials - t0) < 65535 ? (ntrials - t0) : 65535);
        const dim3 g((unsigned)(ublocks * up), (unsigned)((nchan + 63) / 64), nz), b(Tile::THREADS);
        hipLaunchKernelGGL((spyres::upfirdn_kernel<R, UFD_NT, UFD_KC>), g, b, lds, ctx->stream, in_d + t0 * nsamp * nchan,
                           out_d + t0 * nout * nchan, taps_d, ntaps, (long long)nsamp, (long long)nchan, (long long)nout,
                           up, down, (long long)ublocks);
        SPY_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" int spyhip_upfirdn(spyhip_ctx* ctx, const float* in_d, float* out_d, int64_t ntrials, int64_t nsamp,
                              int64_t nchan, int64_t nout, const double* taps_d, int ntaps, int up, int down) {
    if (!ctx || !in_d || !out_d || !taps_d || ntaps < 1 || up < 1 || down < 1 || (const void*)in_d == (const void*)out_d) {
        spy::set_error("upfirdn: bad argument");
        return -1;
    }
    if (ntrials < 0 || nsamp < 1 || nchan < 1 || nout < 1) { spy::set_error("upfirdn: bad shape"); return -1; }
    if ((nchan + 63) / 64 > 65535) { spy::set_error("upfirdn: %lld channels (at most %d)", (long long)nchan, 65535 * 64); return -1; }
    // every output meets input rows near m * down / up: keep m * down and the rows of a tile inside 64 bits
    if (nout > (INT64_MAX >> 2) / down || nsamp > (INT64_MAX >> 2)) {
        spy::set_error("upfirdn: %lld outputs at a step of %d", (long long)nout, down);
        return -1;
    }
    if (ntrials == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    if (spyres::UpfirdnTile<8, UFD_NT, UFD_KC>::rows(down) <= MAX_ROWS)
        return launch<8>(ctx, in_d, out_d, ntrials, nsamp, nchan, nout, taps_d, ntaps, up, down);
    if (spyres::UpfirdnTile<4, UFD_NT, UFD_KC>::rows(down) <= MAX_ROWS)
        return launch<4>(ctx, in_d, out_d, ntrials, nsamp, nchan, nout, taps_d, ntaps, up, down);
    return launch<1>(ctx, in_d, out_d, ntrials, nsamp, nchan, nout, taps_d, ntaps, up, down);
}
