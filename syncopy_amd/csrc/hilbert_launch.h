// Launchers of the packed Hilbert kernels (hilbert_kernel.h), one translation unit per family so that they compile side
// by side: hilbert_packed.hip (N = 2^k) and hilbert_blue.hip (Bluestein).  NO_INSTANCE: no kernel of that length.
#pragma once
#include "spy_common.h"
#include "hilbert_kernel.h"

namespace spyhil {

constexpr int NO_INSTANCE = -100;

int launch_packed(hipStream_t stream, const HilArgs& a, int log2n, bool cplx, unsigned grid);
int launch_blue(hipStream_t stream, const HilArgs& a, int log2n, bool cplx, unsigned grid);

template <int LOG2N, bool BLUE>
int launch_one(hipStream_t stream, const HilArgs& a, bool cplx, unsigned grid) {
    constexpr int G = route_detail::packed_G(LOG2N);
    using C = Cfg2<LOG2N, G>;
    auto go = [&](auto kern) {
        // (per device, cheap: set at every launch)
        SPY_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)C::LDS_BYTES));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(C::NTHREADS), C::LDS_BYTES, stream, a);
        SPY_HIP_CHECK(hipGetLastError());
        return 0;
    };
    return cplx ? go(hilbert_packed_kernel<LOG2N, G, BLUE, true>) : go(hilbert_packed_kernel<LOG2N, G, BLUE, false>);
}

}  // namespace spyhil
