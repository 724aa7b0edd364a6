// CPU emulation of the summary-statistics kernels (syncopy_amd/csrc/stats_kernel.h), TEST INFRASTRUCTURE ONLY (see
// hip_emu.h).  A translation unit of its own: it defines the emulator's thread-locals, adds the few device functions
// these kernels need beyond hip_emu.h, and launches the kernels as stats.hip does.  Built by tests/test_stats.py.
#include "hip_emu.h"

namespace emu {
thread_local dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
thread_local BlockCtx* t_ctx = nullptr;
}  // namespace emu

// shims: LDS integer atomics, the float64 square root, bit casts
static inline unsigned atomicAdd(unsigned* p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline double __dsqrt_rn(double a) { return std::sqrt(a); }
static inline float __uint_as_float(unsigned u) { float f; std::memcpy(&f, &u, 4); return f; }

#include "../../syncopy_amd/csrc/stats_kernel.h"

namespace {
constexpr unsigned EMU_THREADS = 64;        // one OS thread per lane: small workgroups keep the emulation quick

unsigned blocks_for(long long n) { return (unsigned)std::max(1LL, std::min(8LL, (n + EMU_THREADS - 1) / EMU_THREADS)); }
}  // namespace

extern "C" {

void emu_trial_var(const float* in, float* mean, float* acc, float* out, long long T, long long n, int cplx,
                   int take_sqrt, long long chunk) {
    const long long nf = cplx ? 2 * n : n;
    const dim3 b(EMU_THREADS);
    for (long long a = 0; a < T; a += chunk) {
        const long long k = std::min(chunk, T - a);
        emu::launch(dim3(blocks_for(nf)), b, 0, [&] { spystat::trial_sum_kernel(in + a * nf, mean, k, nf); });
    }
    if (cplx) emu::launch(dim3(blocks_for(nf)), b, 0, [&] { spystat::trial_scale_kernel<true>(mean, mean, T, nf); });
    else emu::launch(dim3(blocks_for(nf)), b, 0, [&] { spystat::trial_scale_kernel<false>(mean, mean, T, nf); });
    for (long long a = 0; a < T; a += chunk) {
        const long long k = std::min(chunk, T - a);
        if (cplx) emu::launch(dim3(blocks_for(n)), b, 0, [&] { spystat::trial_sqdev_kernel<true>(in + a * nf, mean, acc, k, n); });
        else emu::launch(dim3(blocks_for(n)), b, 0, [&] { spystat::trial_sqdev_kernel<false>(in + a * nf, mean, acc, k, n); });
    }
    switch ((cplx ? 2 : 0) + (take_sqrt ? 1 : 0)) {
        case 0: emu::launch(dim3(blocks_for(n)), b, 0, [&] { spystat::trial_var_finalize_kernel<false, false>(acc, out, T, n); }); break;
        case 1: emu::launch(dim3(blocks_for(n)), b, 0, [&] { spystat::trial_var_finalize_kernel<false, true>(acc, out, T, n); }); break;
        case 2: emu::launch(dim3(blocks_for(n)), b, 0, [&] { spystat::trial_var_finalize_kernel<true, false>(acc, out, T, n); }); break;
        default: emu::launch(dim3(blocks_for(n)), b, 0, [&] { spystat::trial_var_finalize_kernel<true, true>(acc, out, T, n); }); break;
    }
}

void emu_itc(const float* in, float* acc, float* out, long long T, long long outer, long long ntaper, long long inner,
             long long chunk) {
    const long long n = outer * ntaper * inner;
    const float2* z = reinterpret_cast<const float2*>(in);
    float2* a2 = reinterpret_cast<float2*>(acc);
    for (long long a = 0; a < T; a += chunk) {
        const long long k = std::min(chunk, T - a);
        emu::launch(dim3(blocks_for(n)), dim3(EMU_THREADS), 0, [&] { spystat::itc_accum_kernel(z + a * n, a2, k, n); });
    }
    emu::launch(dim3(blocks_for(outer * inner)), dim3(EMU_THREADS), 0,
                [&] { spystat::itc_finalize_kernel(a2, out, T, outer, ntaper, inner); });
}

void emu_axis_nanvar(const float* x, long long outer, long long n, long long inner, int cplx, int take_sqrt, float* out) {
    const dim3 g(blocks_for(outer * inner)), b(EMU_THREADS);
    switch ((cplx ? 2 : 0) + (take_sqrt ? 1 : 0)) {
        case 0: emu::launch(g, b, 0, [&] { spystat::axis_nanvar_kernel<false, false>(x, outer, n, inner, out); }); break;
        case 1: emu::launch(g, b, 0, [&] { spystat::axis_nanvar_kernel<false, true>(x, outer, n, inner, out); }); break;
        case 2: emu::launch(g, b, 0, [&] { spystat::axis_nanvar_kernel<true, false>(x, outer, n, inner, out); }); break;
        default: emu::launch(g, b, 0, [&] { spystat::axis_nanvar_kernel<true, true>(x, outer, n, inner, out); }); break;
    }
}

// work: outer * n * inner elements when inner > 1; nblocks: workgroups of the median kernel (each walks several slices
// when fewer than the slices)
void emu_axis_nanmedian(const float* x, long long outer, long long n, long long inner, int cplx, float* work, float* out,
                        unsigned nblocks) {
    const float* slices = x;
    if (inner > 1) {
        const unsigned tb = (unsigned)std::min(4LL, outer * ((n + 31) / 32) * ((inner + 31) / 32));
        if (cplx)
            emu::launch(dim3(tb), dim3(256), 0, [&] {
                spystat::axis_transpose_kernel<float2>(reinterpret_cast<const float2*>(x), reinterpret_cast<float2*>(work),
                                                       outer, n, inner);
            });
        else
            emu::launch(dim3(tb), dim3(256), 0, [&] { spystat::axis_transpose_kernel<float>(x, work, outer, n, inner); });
        slices = work;
    }
    const long long nslice = outer * inner;
    const dim3 g((unsigned)std::max(1LL, std::min((long long)nblocks, nslice))), b(EMU_THREADS);
    if (cplx) emu::launch(g, b, 0, [&] { spystat::axis_nanmedian_kernel<true>(slices, nslice, n, out); });
    else emu::launch(g, b, 0, [&] { spystat::axis_nanmedian_kernel<false>(slices, nslice, n, out); });
}

}  // extern "C"
