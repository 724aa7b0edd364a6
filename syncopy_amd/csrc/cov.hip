// Launcher of the channel covariance of spy.timelockanalysis: the kernels of cov_kernel.h over a batch of equal-length
// trials.  The column means live in the context's scratch buffer between the two kernels of a launch.
#include "spy_common.h"
#include "cov_kernel.h"

#include <climits>

namespace {

// the tiles the library launches: 8 waves add the rows of a mean; chunks of 32 rows, 40 KiB of LDS, four workgroups per CU
constexpr int COV_NW = 8, COV_KC = 32;

// everything behind the pointer checks, with NW waves per mean
template <int NW>
int cov_launch(spyhip_ctx* ctx, const float* x_d, float* out_d, int64_t ntrials, int64_t n, int64_t nchan, int64_t ddof) {
    if (ntrials < 0 || n < 1 || nchan < 1) { spy::set_error("cov: bad shape"); return -1; }
    if (ddof < 0 || n - ddof <= 0) {
        spy::set_error("cov: %lld samples leave no degree of freedom at ddof %lld", (long long)n, (long long)ddof);
        return -1;
    }
    // element indices stay inside 64 bits, the blocks of a trial inside a grid dimension
    if (nchan > INT_MAX || n > (INT64_MAX >> 2) / nchan || spycov::cov_blocks(nchan) > INT_MAX) {
        spy::set_error("cov: %lld samples of %lld channels", (long long)n, (long long)nchan);
        return -1;
    }
    if (ntrials == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t max_z = ctx->limits.grid_yz;          // trials per launch (grid.y)
    const int64_t per = ntrials < max_z ? ntrials : max_z;
    if (spy::reserve_scratch(ctx, (size_t)per * (size_t)nchan * sizeof(double))) return -2;
    double* mean_d = reinterpret_cast<double*>(ctx->scratch);
    const double scale = 1.0 / (double)(n - ddof);
    const unsigned lds = (unsigned)spycov::CovTile<COV_KC>::lds_bytes();
    for (int64_t t0 = 0; t0 < ntrials; t0 += max_z) {
        const unsigned nz = (unsigned)((ntrials - t0) < max_z ? (ntrials - t0) : max_z);
        const float* x = x_d + t0 * n * nchan;
        hipLaunchKernelGGL((spycov::cov_mean_kernel<NW>), dim3((unsigned)((nchan + 63) / 64), nz), dim3(64 * NW), 0,
                           ctx->stream, x, mean_d, (long long)n, (long long)nchan);
        SPY_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL((spycov::cov_kernel<COV_KC>), dim3((unsigned)spycov::cov_blocks(nchan), nz),
                           dim3(spycov::CovTile<COV_KC>::THREADS), lds, ctx->stream, x, (const double*)mean_d,
                           out_d + t0 * nchan * nchan, (long long)n, (long long)nchan, scale);
        SPY_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" int spyhip_cov_f32(spyhip_ctx* ctx, const float* x_d, float* out_d, int64_t ntrials, int64_t n, int64_t nchan,
                              int64_t ddof) {
    if (!ctx || !x_d || !out_d || (const void*)x_d == (const void*)out_d) { spy::set_error("cov: bad argument"); return -1; }
    return cov_launch<COV_NW>(ctx, x_d, out_d, ntrials, n, nchan, ddof);
}
