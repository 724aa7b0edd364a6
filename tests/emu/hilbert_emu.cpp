// CPU emulation of the Hilbert kernels (syncopy_amd/csrc/hilbert_kernel.h), TEST INFRASTRUCTURE ONLY (see hip_emu.h).
// Routes, sizes its tables and launches as hilbert.hip does, from the same hilbert_route.h.  Built by tests/test_hilbert.py.
#include "hip_emu.h"

#include <string>
#include <vector>

namespace emu {
thread_local dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
thread_local BlockCtx* t_ctx = nullptr;
}  // namespace emu

#include "../../syncopy_amd/csrc/hilbert_kernel.h"
#include "../../syncopy_amd/csrc/host_fft.h"

namespace {
using spyhil::Family;
using spyhil::HilArgs;

template <int LOG2N, bool BLUE>
void run_packed(const HilArgs& a, bool cplx, unsigned grid) {
    constexpr int G = spyhil::route_detail::packed_G(LOG2N);
    using C = spyfft::Cfg2<LOG2N, G>;
    if (cplx) emu::launch(dim3(grid), dim3(C::NTHREADS), C::LDS_BYTES, [&] { spyhil::hilbert_packed_kernel<LOG2N, G, BLUE, true>(a); });
    else emu::launch(dim3(grid), dim3(C::NTHREADS), C::LDS_BYTES, [&] { spyhil::hilbert_packed_kernel<LOG2N, G, BLUE, false>(a); });
}
}  // namespace

extern "C" {

// 0, or the route's error code; `name` (>= 192 bytes) receives the kernel name
int emu_hilbert(const float* in, void* out, int* nan, int ntrials, long long nsamp, int nchan, int output, char* name) {
    const spyhil::Route r = spyhil::hilbert_route(nsamp);
    if (r.err) return r.err;
    if (name) std::snprintf(name, 192, "%s", r.kernel_name.c_str());
    const bool cplx = output == SPYHIP_OUT_FOURIER;
    const int N = (int)nsamp;
    HilArgs a{};
    a.in = in; a.out = out; a.nan = nan;
    a.ntrials = ntrials; a.nsamp = N; a.nchan = nchan; a.kind = output;
    if (r.family == Family::COPY) {
        const unsigned g = (unsigned)(((long long)ntrials * nchan + 255) / 256);
        if (cplx) emu::launch(dim3(g), dim3(256), 0, [&] { spyhil::hilbert_copy_kernel<true>(a); });
        else emu::launch(dim3(g), dim3(256), 0, [&] { spyhil::hilbert_copy_kernel<false>(a); });
        return 0;
    }
    if (r.family == Family::ANY64) {
        spyhil::HilArgs64 b{};
        b.in = in; b.out = out; b.nan = nan;
        b.ntrials = ntrials; b.nsamp = N; b.nchan = nchan; b.kind = output;
        b.blue = r.bluestein ? 1 : 0;
        b.plan = r.plan;
        const std::vector<double2> tw = spy::twiddle_table<double2>(r.M);
        std::vector<double2> chirp, bhat;
        if (r.bluestein) spy::bluestein_tables(N, r.M, 0, &chirp, &bhat);
        b.tw = tw.data(); b.chirp = chirp.data(); b.bhat = bhat.data();
        const long long total = (long long)ntrials * ((nchan + 1) / 2);
        long long chunk = 3;                                // (several launches, as a long batch takes on the device)
        if (chunk > spyhil::any64_chunk(r.M)) chunk = spyhil::any64_chunk(r.M);
        std::vector<double2> work((size_t)chunk * 2 * (size_t)r.M);
        b.work = work.data();
        for (long long w0 = 0; w0 < total; w0 += chunk) {
            b.wg0 = w0;
            const unsigned g = (unsigned)(total - w0 < chunk ? total - w0 : chunk);
            if (cplx) emu::launch(dim3(g), dim3(256), 0, [&] { spyhil::hilbert_any64_kernel<true>(b); });
            else emu::launch(dim3(g), dim3(256), 0, [&] { spyhil::hilbert_any64_kernel<false>(b); });
        }
        return 0;
    }
    const spyhil::PackedGrid g = spyhil::packed_grid(ntrials, nchan, r.G);
    a.npg = g.npg; a.S = g.S; a.ncl = g.ncl;
    const std::vector<float2> tw = spy::twiddle_table<float2>(r.M);
    std::vector<float2> chirp, bhat;
    if (r.family == Family::BLUE) spy::bluestein_tables(N, r.M, 0, &chirp, &bhat);
    a.tw = tw.data(); a.chirp = chirp.data(); a.bhat = bhat.data();
    a.inv_n = 1.0f / (float)N;
    const bool blue = r.family == Family::BLUE;
#define EMU_HIL(L)                                                   \
    case L:                                                          \
        if (!blue) run_packed<L, false>(a, cplx, g.grid);            \
        else if constexpr (L >= 8) run_packed<L, true>(a, cplx, g.grid); \
        break
    switch (r.log2n) {
        EMU_HIL(4); EMU_HIL(5); EMU_HIL(6); EMU_HIL(7); EMU_HIL(8); EMU_HIL(9); EMU_HIL(10); EMU_HIL(11); EMU_HIL(12);
        default: return -100;                               // (8192 points = 512 OS threads per block: not emulated)
    }
#undef EMU_HIL
    return 0;
}

}  // extern "C"
