// Launchers of the peristimulus time histogram of spy.spike_psth: the kernels of psth_kernel.h over a spike table that is
// resident on the device.  Every buffer belongs to the caller; nothing here allocates or synchronises.
#include "spy_common.h"
#include "psth_kernel.h"

#include <climits>

namespace {

constexpr int64_t MAX_TABLE = 1LL << 24;     // entries of the (channel, unit) tables

bool table_ok(const char* what, int64_t nchan, int64_t nunit) {
    if (nchan < 1 || nunit < 1 || nchan > MAX_TABLE || nunit > MAX_TABLE || nchan * nunit > MAX_TABLE) {
        spy::set_error("%s: a (channel, unit) table of %lld x %lld entries (at most %lld)", what, (long long)nchan,
                       (long long)nunit, (long long)MAX_TABLE);
        return false;
    }
    return true;
}

bool trials_ok(const char* what, int64_t ntrials) {
    if (ntrials < 0 || ntrials > INT_MAX) { spy::set_error("%s: %lld trials", what, (long long)ntrials); return false; }
    return true;
}

bool shape_ok(const spyhip_ctx* ctx, const char* what, int64_t ntrials, int64_t nbins, int64_t ncols) {
    if (!trials_ok(what, ntrials)) return false;
    const int64_t max_yz = ctx->limits.grid_yz;         // blocks along grid.y / grid.z
    if (nbins < 1 || ncols < 1 || (nbins + spypsth::BIN_TILE - 1) / spypsth::BIN_TILE > max_yz ||
        (ncols + spypsth::PROP_TILE - 1) / spypsth::PROP_TILE > max_yz ||
        (ntrials > 0 && nbins + 1 > (INT64_MAX >> 3) / ntrials / ncols)) {
        spy::set_error("%s: %lld trials of %lld bins x %lld columns", what, (long long)ntrials, (long long)nbins,
                       (long long)ncols);
        return false;
    }
    return true;
}

}  // namespace

extern "C" int spyhip_psth_presence(spyhip_ctx* ctx, const int32_t* chan_d, const int32_t* unit_d, const int64_t* row_lo_d,
                                    const int64_t* row_hi_d, int64_t ntrials, int64_t max_rows, const uint8_t* chan_ok_d,
                                    int64_t nchan, const uint8_t* unit_ok_d, int64_t nunit, uint8_t* flags_d) {
    if (!ctx || !chan_d || !unit_d || !row_lo_d || !row_hi_d || !chan_ok_d || !unit_ok_d || !flags_d) {
        spy::set_error("psth_presence: bad argument");
        return -1;
    }
    if (!trials_ok("psth_presence", ntrials) || !table_ok("psth_presence", nchan, nunit)) return -1;
    if (ntrials == 0 || max_rows < 1) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    int64_t nblk = (max_rows + 16 * spypsth::THREADS - 1) / (16 * spypsth::THREADS);
    if (nblk > spypsth::MAX_ROW_BLOCKS) nblk = spypsth::MAX_ROW_BLOCKS;
    hipLaunchKernelGGL(spypsth::psth_presence_kernel, dim3((unsigned)ntrials, (unsigned)nblk), dim3(spypsth::THREADS), 0,
                       ctx->stream, chan_d, unit_d, (const long long*)row_lo_d, (const long long*)row_hi_d, chan_ok_d,
                       unit_ok_d, (long long)nchan, (long long)nunit, flags_d);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_psth_bin_rows(spyhip_ctx* ctx, const int64_t* sample_d, const int64_t* row_lo_d,
                                    const int64_t* row_hi_d, const int64_t* start_d, const int64_t* onset_d,
                                    int64_t ntrials, const double* edges_d, int64_t nedges, double samplerate,
                                    int64_t* rows_d) {
    if (!ctx || !sample_d || !row_lo_d || !row_hi_d || !start_d || !onset_d || !edges_d || !rows_d) {
        spy::set_error("psth_bin_rows: bad argument");
        return -1;
    }
    if (!trials_ok("psth_bin_rows", ntrials)) return -1;
    if (nedges < 2 || !(samplerate > 0.0) || (ntrials > 0 && nedges > (int64_t)INT_MAX * spypsth::THREADS / ntrials)) {
        spy::set_error("psth_bin_rows: %lld trials, %lld edges, samplerate %g", (long long)ntrials, (long long)nedges,
                       samplerate);
        return -1;
    }
    if (ntrials == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t nblk = (ntrials * nedges + spypsth::THREADS - 1) / spypsth::THREADS;
    hipLaunchKernelGGL(spypsth::psth_bin_rows_kernel, dim3((unsigned)nblk), dim3(spypsth::THREADS), 0, ctx->stream,
                       (const long long*)sample_d, (const long long*)row_lo_d, (const long long*)row_hi_d,
                       (const long long*)start_d, (const long long*)onset_d, (long long)ntrials, edges_d,
                       (long long)nedges, samplerate, (long long*)rows_d);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_psth_count(spyhip_ctx* ctx, const int32_t* chan_d, const int32_t* unit_d, const int64_t* rows_d,
                                 const int32_t* lut_d, int64_t nchan, int64_t nunit, const int32_t* lohi_d,
                                 int64_t ntrials, int64_t nbins, int64_t ncols, double scale, float* out_d) {
    if (!ctx || !chan_d || !unit_d || !rows_d || !lut_d || !lohi_d || !out_d) {
        spy::set_error("psth_count: bad argument");
        return -1;
    }
    if (!shape_ok(ctx, "psth_count", ntrials, nbins, ncols) || !table_ok("psth_count", nchan, nunit)) return -1;
    if (ntrials == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const dim3 grid((unsigned)ntrials, (unsigned)((nbins + spypsth::BIN_TILE - 1) / spypsth::BIN_TILE),
                    (unsigned)((ncols + spypsth::COL_TILE - 1) / spypsth::COL_TILE));
    hipLaunchKernelGGL(spypsth::psth_count_kernel, grid, dim3(spypsth::THREADS), 0, ctx->stream, chan_d, unit_d,
                       (const long long*)rows_d, lut_d, (long long)nchan, (long long)nunit, lohi_d, (long long)nbins,
                       (long long)ncols, scale, out_d);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_psth_proportion(spyhip_ctx* ctx, const int32_t* chan_d, const int32_t* unit_d,
                                      const int64_t* row_lo_d, const int64_t* row_hi_d, const int64_t* rows_d,
                                      const int32_t* lut_d, int64_t nchan, int64_t nunit, const int32_t* unit_k_d,
                                      const int32_t* col_k_d, int64_t nk, const double* edges_d, int64_t ntrials,
                                      int64_t nbins, int64_t ncols, int32_t* s_d, float* out_d) {
    if (!ctx || !chan_d || !unit_d || !row_lo_d || !row_hi_d || !rows_d || !lut_d || !unit_k_d || !col_k_d || !edges_d ||
        !s_d || !out_d) {
        spy::set_error("psth_proportion: bad argument");
        return -1;
    }
    if (!shape_ok(ctx, "psth_proportion", ntrials, nbins, ncols) || !table_ok("psth_proportion", nchan, nunit)) return -1;
    if (nk < 1 || nk > nunit || (nk + spypsth::UNIT_TILE - 1) / spypsth::UNIT_TILE > ctx->limits.grid_yz) {
        spy::set_error("psth_proportion: %lld units with a column", (long long)nk);
        return -1;
    }
    if (ntrials == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(spypsth::psth_unit_count_kernel,
                       dim3((unsigned)ntrials, (unsigned)((nk + spypsth::UNIT_TILE - 1) / spypsth::UNIT_TILE)),
                       dim3(spypsth::THREADS), 0, ctx->stream, chan_d, unit_d, (const long long*)row_lo_d,
                       (const long long*)row_hi_d, (const long long*)rows_d, lut_d, unit_k_d, (long long)nchan,
                       (long long)nunit, (long long)nk, (long long)nbins, s_d);
    SPY_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(spypsth::psth_proportion_kernel,
                       dim3((unsigned)ntrials, (unsigned)((ncols + spypsth::PROP_TILE - 1) / spypsth::PROP_TILE)),
                       dim3(spypsth::PROP_TILE), 0, ctx->stream, (const int*)s_d, col_k_d, edges_d, (long long)nk,
                       (long long)nbins, (long long)ncols, out_d);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}
