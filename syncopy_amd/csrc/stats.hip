// Launchers of the summary statistics spy.var / spy.std / spy.median / spy.itc (kernels in stats_kernel.h).
#include "spy_common.h"
#include "stats_kernel.h"

namespace {

unsigned elementwise_blocks(const spyhip_ctx* ctx, long long n) {
    long long blocks = (n + 255) / 256;
    if (blocks > ctx->limits.elementwise_blocks) blocks = ctx->limits.elementwise_blocks;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

}  // namespace

extern "C" int spyhip_trial_sum(spyhip_ctx* ctx, const void* in_d, float* acc_d, int64_t ntrials, int64_t nfloat) {
    if (!ctx || !in_d || !acc_d || ntrials < 0 || nfloat < 0) { spy::set_error("trial_sum: bad argument"); return -1; }
    if (ntrials == 0 || nfloat == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(spystat::trial_sum_kernel, dim3(elementwise_blocks(ctx, nfloat)), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const float*>(in_d), acc_d, (long long)ntrials, (long long)nfloat);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_trial_sum_finalize(spyhip_ctx* ctx, const float* acc_d, void* mean_d, int64_t ntotal, int64_t n,
                                         int is_complex) {
    if (!ctx || !acc_d || !mean_d || ntotal < 1 || n < 0) { spy::set_error("trial_sum_finalize: bad argument"); return -1; }
    if (n == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const long long nf = is_complex ? 2 * n : n;
    float* out = reinterpret_cast<float*>(mean_d);
    if (is_complex)
        hipLaunchKernelGGL(spystat::trial_scale_kernel<true>, dim3(elementwise_blocks(ctx, nf)), dim3(256), 0, ctx->stream,
                           acc_d, out, (long long)ntotal, nf);
    else
        hipLaunchKernelGGL(spystat::trial_scale_kernel<false>, dim3(elementwise_blocks(ctx, nf)), dim3(256), 0, ctx->stream,
                           acc_d, out, (long long)ntotal, nf);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_trial_sqdev(spyhip_ctx* ctx, const void* in_d, const void* mean_d, float* acc_d, int64_t ntrials,
                                  int64_t n, int is_complex) {
    if (!ctx || !in_d || !mean_d || !acc_d || ntrials < 0 || n < 0) { spy::set_error("trial_sqdev: bad argument"); return -1; }
    if (ntrials == 0 || n == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const float* in = reinterpret_cast<const float*>(in_d);
    const float* mean = reinterpret_cast<const float*>(mean_d);
    if (is_complex)
        hipLaunchKernelGGL(spystat::trial_sqdev_kernel<true>, dim3(elementwise_blocks(ctx, n)), dim3(256), 0, ctx->stream, in,
                           mean, acc_d, (long long)ntrials, (long long)n);
    else
        hipLaunchKernelGGL(spystat::trial_sqdev_kernel<false>, dim3(elementwise_blocks(ctx, n)), dim3(256), 0, ctx->stream, in,
                           mean, acc_d, (long long)ntrials, (long long)n);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_trial_var_finalize(spyhip_ctx* ctx, const float* acc_d, void* out_d, int64_t ntotal, int64_t n,
                                         int is_complex, int take_sqrt) {
    if (!ctx || !acc_d || !out_d || ntotal < 1 || n < 0) { spy::set_error("trial_var_finalize: bad argument"); return -1; }
    if (n == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    float* out = reinterpret_cast<float*>(out_d);
    const dim3 g(elementwise_blocks(ctx, n)), b(256);
    const long long T = ntotal, N = n;
    switch ((is_complex ? 2 : 0) + (take_sqrt ? 1 : 0)) {
        case 0: hipLaunchKernelGGL((spystat::trial_var_finalize_kernel<false, false>), g, b, 0, ctx->stream, acc_d, out, T, N); break;
        case 1: hipLaunchKernelGGL((spystat::trial_var_finalize_kernel<false, true>), g, b, 0, ctx->stream, acc_d, out, T, N); break;
        case 2: hipLaunchKernelGGL((spystat::trial_var_finalize_kernel<true, false>), g, b, 0, ctx->stream, acc_d, out, T, N); break;
        default: hipLaunchKernelGGL((spystat::trial_var_finalize_kernel<true, true>), g, b, 0, ctx->stream, acc_d, out, T, N); break;
    }
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_itc_accumulate(spyhip_ctx* ctx, const void* in_d, void* acc_d, int64_t ntrials, int64_t n) {
    if (!ctx || !in_d || !acc_d || ntrials < 0 || n < 0) { spy::set_error("itc_accumulate: bad argument"); return -1; }
    if (ntrials == 0 || n == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(spystat::itc_accum_kernel, dim3(elementwise_blocks(ctx, n)), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const float2*>(in_d), reinterpret_cast<float2*>(acc_d), (long long)ntrials,
                       (long long)n);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_itc_finalize(spyhip_ctx* ctx, const void* acc_d, float* out_d, int64_t ntotal, int64_t outer,
                                   int64_t ntaper, int64_t inner) {
    if (!ctx || !acc_d || !out_d || ntotal < 1 || outer < 0 || ntaper < 1 || inner < 0) {
        spy::set_error("itc_finalize: bad argument");
        return -1;
    }
    if (outer == 0 || inner == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(spystat::itc_finalize_kernel, dim3(elementwise_blocks(ctx, outer * inner)), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const float2*>(acc_d), out_d, (long long)ntotal, (long long)outer,
                       (long long)ntaper, (long long)inner);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_axis_nanvar(spyhip_ctx* ctx, const void* x_d, int64_t outer, int64_t n, int64_t inner, int is_complex,
                                  int take_sqrt, void* out_d) {
    if (!ctx || !x_d || !out_d || outer < 1 || n < 1 || inner < 1) { spy::set_error("axis_nanvar: bad argument"); return -1; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    long long blocks = (outer * inner + 255) / 256;
    if (blocks > ctx->limits.workgroups) blocks = ctx->limits.workgroups;
    const dim3 g((unsigned)blocks), b(256);
    const float* x = reinterpret_cast<const float*>(x_d);
    float* out = reinterpret_cast<float*>(out_d);
    const long long O = outer, N = n, I = inner;
    switch ((is_complex ? 2 : 0) + (take_sqrt ? 1 : 0)) {
        case 0: hipLaunchKernelGGL((spystat::axis_nanvar_kernel<false, false>), g, b, 0, ctx->stream, x, O, N, I, out); break;
        case 1: hipLaunchKernelGGL((spystat::axis_nanvar_kernel<false, true>), g, b, 0, ctx->stream, x, O, N, I, out); break;
        case 2: hipLaunchKernelGGL((spystat::axis_nanvar_kernel<true, false>), g, b, 0, ctx->stream, x, O, N, I, out); break;
        default: hipLaunchKernelGGL((spystat::axis_nanvar_kernel<true, true>), g, b, 0, ctx->stream, x, O, N, I, out); break;
    }
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_axis_nanmedian(spyhip_ctx* ctx, const void* x_d, int64_t outer, int64_t n, int64_t inner,
                                     int is_complex, void* work_d, void* out_d) {
    if (!ctx || !x_d || !out_d || outer < 1 || n < 1 || inner < 1) { spy::set_error("axis_nanmedian: bad argument"); return -1; }
    if (n > 0x7fffffffLL) { spy::set_error("axis_nanmedian: %lld elements along the axis (at most 2^31 - 1)", (long long)n); return -1; }
    if (inner > 1 && !work_d) { spy::set_error("axis_nanmedian: inner = %lld needs a work buffer of the input's size", (long long)inner); return -1; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const void* slices = x_d;
    if (inner > 1) {                    // slices contiguous first: (outer, n, inner) -> (outer, inner, n)
        const long long ntile = (long long)outer * ((n + 31) / 32) * ((inner + 31) / 32);
        const unsigned tb = (unsigned)(ntile > ctx->limits.workgroups ? ctx->limits.workgroups : ntile);
        if (is_complex)
            hipLaunchKernelGGL(spystat::axis_transpose_kernel<float2>, dim3(tb), dim3(256), 0, ctx->stream,
                               reinterpret_cast<const float2*>(x_d), reinterpret_cast<float2*>(work_d), (long long)outer,
                               (long long)n, (long long)inner);
        else
            hipLaunchKernelGGL(spystat::axis_transpose_kernel<float>, dim3(tb), dim3(256), 0, ctx->stream,
                               reinterpret_cast<const float*>(x_d), reinterpret_cast<float*>(work_d), (long long)outer,
                               (long long)n, (long long)inner);
        SPY_HIP_CHECK(hipGetLastError());
        slices = work_d;
    }
    const long long nslice = (long long)outer * inner;
    const unsigned mb = (unsigned)(nslice > ctx->limits.workgroups ? ctx->limits.workgroups : nslice);
    if (is_complex)
        hipLaunchKernelGGL(spystat::axis_nanmedian_kernel<true>, dim3(mb), dim3(spystat::MED_THREADS), 0, ctx->stream,
                           reinterpret_cast<const float*>(slices), nslice, (long long)n, reinterpret_cast<float*>(out_d));
    else
        hipLaunchKernelGGL(spystat::axis_nanmedian_kernel<false>, dim3(mb), dim3(spystat::MED_THREADS), 0, ctx->stream,
                           reinterpret_cast<const float*>(slices), nslice, (long long)n, reinterpret_cast<float*>(out_d));
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}
