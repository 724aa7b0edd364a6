// Host side of K11: spyhip_directed_norm of include/spyhip.h (directed transfer function / partial directed coherence from
// the factors of the Wilson stage).  Grid, tile and LDS come from directed_route.h.
#include "spy_common.h"
#include "directed_kernel.h"

extern "C" int spyhip_directed_norm(spyhip_ctx* ctx, const void* M_d, const void* w_d, int nfreq, int n, int axis, int squared,
                                    void* out_d) {
    if (!ctx || !M_d || !out_d) { spy::set_error("directed_norm: null argument"); return -1; }
    if (nfreq < 1 || n < 1) { spy::set_error("directed_norm: bad shape"); return -1; }
    if (axis != 0 && axis != 1) { spy::set_error("directed_norm: axis %d is neither 0 (rows, DTF) nor 1 (columns, PDC)", axis); return -1; }
    if (M_d == out_d) { spy::set_error("directed_norm: the output must not alias the input"); return -1; }
    const spydir::NormRoute r = spydir::norm_route(n, nfreq, ctx->lds_per_block);
    if (!r.ok) { spy::set_error("directed_norm: no tile of %d lines fits %zu bytes of LDS", spydir::DL, ctx->lds_per_block); return -3; }
    if (r.grid > 0x7fffffffLL) { spy::set_error("directed_norm: grid too large"); return -1; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const auto kernel = axis == 0 ? spydir::directed_norm_kernel<0> : spydir::directed_norm_kernel<1>;
    SPY_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)r.grid), dim3(r.threads), r.lds, ctx->stream, reinterpret_cast<const spydir::cd*>(M_d),
                       reinterpret_cast<const double*>(w_d), nfreq, n, r.kc, (int)r.cached, squared != 0, reinterpret_cast<float*>(out_d));
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}
