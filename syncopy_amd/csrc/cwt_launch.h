// The kernel instance behind a step of the wavelet route (cwt_route.h), declared once from the engine list for
// cwt.hip: f(kernel, threads per workgroup, dynamic LDS bytes).  -1: no such instance.
#pragma once
#include "cwt_kernel.h"
#include "cwt64_kernel.h"
#include "cwt_route.h"

namespace spycwt {

template <class F>
int with_outk(int outk, F&& f) {
    switch (outk) {
        case 0: return f(std::integral_constant<int, 0>{});
        case 1: return f(std::integral_constant<int, 1>{});
        default: return f(std::integral_constant<int, 2>{});
    }
}

template <class F>
int with_transform_kernel(int log2n, EngineKind kind, int outk, F&& f) {
    return for_engine(log2n, [&](auto L, auto G, auto GD) -> int {
        return with_outk(outk, [&](auto K) -> int {
            constexpr int l = decltype(L)::value, g = decltype(G)::value, gd = decltype(GD)::value, k = decltype(K)::value;
            if constexpr (gd > 0) {
                using C = spyfft::Cfg2<l, gd>;
                if (kind == EngineKind::DIRECT) return f(spyfft::cwt2d_kernel<l, gd, k>, (int)C::NTHREADS, (size_t)C::LDS_BYTES);
            }
            if constexpr (l <= 13) {        // the packed engine: two channels (or two trials of a channel) per transform
                using C = spyfft::Cfg2<l, g>;
                if (kind == EngineKind::PACKED) return f(spyfft::cwt2_kernel<l, g, k, false>, (int)C::NTHREADS, (size_t)C::LDS_BYTES);
                if (kind == EngineKind::PACKED_PAIRS) return f(spyfft::cwt2_kernel<l, g, k, true>, (int)C::NTHREADS, (size_t)C::LDS_BYTES);
            } else {
                using C = spyfft::Cfg<l, g>;
                if (kind == EngineKind::PLAIN14) return f(spyfft::cwt_kernel<l, g, k>, (int)C::NTHREADS, (size_t)C::LDS_BYTES);
            }
            return -1;
        });
    });
}

template <class F>
int with_cwt64_kernel(int outk, F&& f) {
    return with_outk(outk, [&](auto K) -> int { return f(spyfft::cwt64_kernel<decltype(K)::value>); });
}

// f(kernel): all three take the staging rows of CwtArgs, 256 threads and no dynamic LDS
template <class F>
int with_scatter_kernel(Scatter kind, F&& f) {
    switch (kind) {
        case Scatter::COMPLEX: return f(spyfft::cwt_scatter_kernel<float2>);
        case Scatter::WIDE: return f(spyfft::cwt_scatter_wide_kernel);
        default: return f(spyfft::cwt_scatter_kernel<float>);
    }
}

}  // namespace spycwt
