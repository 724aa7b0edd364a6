// Launch plumbing shared by the translation units of the decimal-length kernel (mtmfft_dec_kernel.h)
#pragma once
#include "spy_common.h"
#include "mtmfft_dec_cfg.h"     // mtmfft_dec_kernel.h + the named schedules

namespace spyfft {

template <class Cf, int OUTK, bool MEAN>
int dec_launch_one(hipStream_t stream, MtmArgs a, int nquads) {        // (Cf::HALF: channel PAIRS)
    unsigned grid;
    if (spy::xcd_grid(a, nquads, Cf::G, Cf::HALF ? 16 : 8, a.nseg, &grid)) return -1;
    auto kern = mtmfft_dec_kernel<Cf, OUTK, MEAN>;
    SPY_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)Cf::LDS_BYTES));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cf::NTHREADS), Cf::LDS_BYTES, stream, a);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

template <class Cf>
int dec_launch_mode(hipStream_t stream, const MtmArgs& a, int nquads, int outk, bool mean) {
    return spy::dispatch_mode(outk, mean, [&](auto K, auto Mn) {
        return dec_launch_one<Cf, decltype(K)::value, decltype(Mn)::value>(stream, a, nquads);
    });
}

}  // namespace spyfft
