// Launch plumbing shared by the translation units of the reference-precision compile-time-schedule kernel
// (mtmfft_dec64_kernel.h)
#pragma once
#include "spy_common.h"
#include "mtmfft_dec64_cfg.h"

namespace spyfft {

template <class Cf, int OUTK, bool MEAN>
int dec64_launch_one(hipStream_t stream, F64Args fa, int npairs) {      // (Cf::HALF: single channels)
    unsigned grid;
    if (spy::xcd_grid(fa.m, npairs, Cf::G, Cf::HALF ? 32 : 16, fa.m.nseg, &grid)) return -1;
    auto kern = mtmfft_dec64_kernel<Cf, OUTK, MEAN>;
    SPY_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)Cf::LDS_BYTES));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cf::NTHREADS), Cf::LDS_BYTES, stream, fa);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

template <class Cf>
int dec64_launch_mode(hipStream_t stream, const F64Args& a, int npairs, int outk, bool mean) {
    return spy::dispatch_mode(outk, mean, [&](auto K, auto Mn) {
        return dec64_launch_one<Cf, decltype(K)::value, decltype(Mn)::value>(stream, a, npairs);
    });
}

}  // namespace spyfft
