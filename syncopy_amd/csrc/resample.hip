// Launcher of spy.resampledata: the up-FIR-down kernel of resample_kernel.h over batches of equal-length trials.
#include "spy_common.h"
#include "resample_kernel.h"

#include <climits>

namespace {

// A tile configuration: NT waves share chunks of KC taps of a phase; R0, R1 or 1 outputs per lane, the most whose
// (R - 1) * down + KC staged rows fit ROWS.  The library launches 8 waves on chunks of 128 taps, 8, 4 or 1 outputs per
// lane and at most 256 rows (64 KiB of LDS, two workgroups per CU).
template <int NT_, int KC_, long long ROWS_, int R0_, int R1_>
struct UfdCfg {
    static constexpr int NT = NT_, KC = KC_, R0 = R0_, R1 = R1_;
    static constexpr long long ROWS = ROWS_;
};
using UfdLib = UfdCfg<8, 128, 256, 8, 4>;

template <class Cfg, int R>
int launch(spyhip_ctx* ctx, const float* in_d, float* out_d, int64_t ntrials, int64_t nsamp, int64_t nchan, int64_t nout,
           const double* taps_d, int ntaps, int up, int down) {
    using Tile = spyres::UpfirdnTile<R, Cfg::NT, Cfg::KC>;
    const int64_t per_phase = (nout + up - 1) / up;
    const int64_t ublocks = (per_phase + R - 1) / R;
    if (ublocks > (int64_t)INT_MAX / up) {
        spy::set_error("upfirdn: %lld outputs in %d phases per trial", (long long)nout, up);
        return -1;
    }
    const unsigned lds = (unsigned)Tile::lds_bytes(down);
    const int64_t max_z = ctx->limits.grid_yz;
    for (int64_t t0 = 0; t0 < ntrials; t0 += max_z) {          // grid.z carries the trial
        const unsigned nz = (unsigned)((ntrials - t0) < max_z ? (ntrials - t0) : max_z);
        const dim3 g((unsigned)(ublocks * up), (unsigned)((nchan + 63) / 64), nz), b(Tile::THREADS);
        hipLaunchKernelGGL((spyres::upfirdn_kernel<R, Cfg::NT, Cfg::KC>), g, b, lds, ctx->stream, in_d + t0 * nsamp * nchan,
                           out_d + t0 * nout * nchan, taps_d, ntaps, (long long)nsamp, (long long)nchan, (long long)nout,
                           up, down, (long long)ublocks);
        SPY_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

// everything behind the pointer checks, on the tiles of Cfg
template <class Cfg>
int upfirdn_launch(spyhip_ctx* ctx, const float* in_d, float* out_d, int64_t ntrials, int64_t nsamp, int64_t nchan,
                   int64_t nout, const double* taps_d, int ntaps, int up, int down) {
    if (ntrials < 0 || nsamp < 1 || nchan < 1 || nout < 1) { spy::set_error("upfirdn: bad shape"); return -1; }
    const int64_t max_y = ctx->limits.grid_yz;
    if ((nchan + 63) / 64 > max_y) { spy::set_error("upfirdn: %lld channels (at most %lld)", (long long)nchan, (long long)(max_y * 64)); return -1; }
    // every output meets input rows near m * down / up: keep m * down and the rows of a tile inside 64 bits
    if (nout > (INT64_MAX >> 2) / down || nsamp > (INT64_MAX >> 2)) {
        spy::set_error("upfirdn: %lld outputs at a step of %d", (long long)nout, down);
        return -1;
    }
    if (ntrials == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    if (spyres::UpfirdnTile<Cfg::R0, Cfg::NT, Cfg::KC>::rows(down) <= Cfg::ROWS)
        return launch<Cfg, Cfg::R0>(ctx, in_d, out_d, ntrials, nsamp, nchan, nout, taps_d, ntaps, up, down);
    if (spyres::UpfirdnTile<Cfg::R1, Cfg::NT, Cfg::KC>::rows(down) <= Cfg::ROWS)
        return launch<Cfg, Cfg::R1>(ctx, in_d, out_d, ntrials, nsamp, nchan, nout, taps_d, ntaps, up, down);
    return launch<Cfg, 1>(ctx, in_d, out_d, ntrials, nsamp, nchan, nout, taps_d, ntaps, up, down);
}

}  // namespace

extern "C" int spyhip_upfirdn(spyhip_ctx* ctx, const float* in_d, float* out_d, int64_t ntrials, int64_t nsamp,
                              int64_t nchan, int64_t nout, const double* taps_d, int ntaps, int up, int down) {
    if (!ctx || !in_d || !out_d || !taps_d || ntaps < 1 || up < 1 || down < 1 || (const void*)in_d == (const void*)out_d) {
        spy::set_error("upfirdn: bad argument");
        return -1;
    }
    return upfirdn_launch<UfdLib>(ctx, in_d, out_d, ntrials, nsamp, nchan, nout, taps_d, ntaps, up, down);
}
