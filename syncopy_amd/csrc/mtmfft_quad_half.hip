// mtmfft_quad_kernel<13, 1, ..., HALF>: 2^14 samples as channel pairs through the 8192-point radix-16 engine (mtmfft2_kernel.h)
#include "spy_common.h"
#include "mtmfft2_kernel.h"

namespace spyfft {

template <int OUTK, bool MEAN>
static int quad_half_launch_one(hipStream_t stream, MtmArgs a, int npairs) {
    using C = Cfg2<13, 1>;
    unsigned grid;
    if (spy::xcd_grid(a, npairs, 1, 16, a.nseg, &grid)) return -1;
    auto kern = mtmfft_quad_kernel<13, 1, OUTK, MEAN, true>;
    SPY_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)C::LDS_BYTES));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(C::NTHREADS), C::LDS_BYTES, stream, a);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

// `a.tapers` = the windows times scale / 2 (the plan's pre-scaled table), `a.tw` = exp(-2 pi i m / 8192), `a.twh` the half-step table
int quad_half_launch(hipStream_t stream, const MtmArgs& a, int npairs, int outk, bool mean) {
    return spy::dispatch_mode(outk, mean, [&](auto K, auto Mn) {
        return quad_half_launch_one<decltype(K)::value, decltype(Mn)::value>(stream, a, npairs);
    });
}

}  // namespace spyfft
