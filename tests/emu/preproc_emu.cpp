// CPU emulation of the preprocessing kernels (syncopy_amd/csrc/preproc_kernel.h), TEST INFRASTRUCTURE ONLY (see
// hip_emu.h).  Launches the kernels as preproc.hip does, the FIR kernel on a small tile.  Built by tests/test_preproc.py.
#include "hip_emu.h"

namespace emu {
thread_local dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
thread_local BlockCtx* t_ctx = nullptr;
}  // namespace emu

#include "../../syncopy_amd/csrc/preproc_kernel.h"

namespace {
using spypre::SosCoef;
dim3 series_grid(long long ntrials, long long nchan) {
    return dim3((unsigned)((ntrials * nchan + spypre::SERIES_THREADS - 1) / spypre::SERIES_THREADS));
}
SosCoef coef(const double* sos, const double* zi, int nsec) {
    SosCoef k;
    std::memset(&k, 0, sizeof(k));
    k.nsec = nsec;
    for (int s = 0; s < nsec; ++s) {
        const double* r = sos + 6 * s;
        k.c[s][0] = r[0]; k.c[s][1] = r[1]; k.c[s][2] = r[2]; k.c[s][3] = r[4]; k.c[s][4] = r[5];
        if (zi) { k.zi[s][0] = zi[2 * s]; k.zi[s][1] = zi[2 * s + 1]; }
    }
    return k;
}
constexpr int R = 4, NT = 2, KC = 8;      // tile of 8 outputs, 8 taps per stage
using Tile = spypre::FirTile<R, NT, KC>;
}  // namespace

extern "C" {

void emu_detrend(const float* in, float* out, int T, int N, int C, int order, int rect, int* flag) {
    const dim3 g = series_grid(T, C), b(spypre::SERIES_THREADS);
    switch (2 * order + (rect ? 1 : 0)) {
        case 0: emu::launch(g, b, 0, [&] { spypre::detrend_kernel<0, false>(in, out, T, N, C, flag); }); break;
        case 1: emu::launch(g, b, 0, [&] { spypre::detrend_kernel<0, true>(in, out, T, N, C, flag); }); break;
        case 2: emu::launch(g, b, 0, [&] { spypre::detrend_kernel<1, false>(in, out, T, N, C, flag); }); break;
        default: emu::launch(g, b, 0, [&] { spypre::detrend_kernel<1, true>(in, out, T, N, C, flag); }); break;
    }
}

void emu_standardize(const float* in, float* out, int T, int N, int C, int rect, int* flag) {
    const dim3 g = series_grid(T, C), b(spypre::SERIES_THREADS);
    if (rect) emu::launch(g, b, 0, [&] { spypre::standardize_kernel<true>(in, out, T, N, C, flag); });
    else emu::launch(g, b, 0, [&] { spypre::standardize_kernel<false>(in, out, T, N, C, flag); });
}

void emu_sosfilt(const float* in, float* out, int T, int N, int C, const double* sos, int nsec, int rect, int* flag) {
    const SosCoef k = coef(sos, nullptr, nsec);
    const dim3 g = series_grid(T, C), b(spypre::SERIES_THREADS);
    if (rect) emu::launch(g, b, 0, [&] { spypre::sos_onepass_kernel<8, true>(in, out, k, T, N, C, flag); });
    else emu::launch(g, b, 0, [&] { spypre::sos_onepass_kernel<8, false>(in, out, k, T, N, C, flag); });
}

void emu_sosfiltfilt(const float* in, float* out, double* work, int T, int N, int C, const double* sos, const double* zi,
                     int nsec, int edge, int rect, int* flag) {
    const SosCoef k = coef(sos, zi, nsec);
    const dim3 g = series_grid(T, C), b(spypre::SERIES_THREADS);
    emu::launch(g, b, 0, [&] { spypre::sos_forward_kernel<8>(in, work, k, T, N, C, edge, flag); });
    if (rect) emu::launch(g, b, 0, [&] { spypre::sos_backward_kernel<8, true>(work, out, k, T, N, C, edge); });
    else emu::launch(g, b, 0, [&] { spypre::sos_backward_kernel<8, false>(work, out, k, T, N, C, edge); });
}

void emu_fir_same(const float* in, float* out, int T, int N, int C, const double* taps, int ntaps, int rect, int* flag) {
    const dim3 g((unsigned)((C + 63) / 64), (unsigned)((N + Tile::T - 1) / Tile::T), (unsigned)T), b(Tile::THREADS);
    if (rect) emu::launch(g, b, Tile::LDS_BYTES, [&] { spypre::fir_same_kernel<R, NT, KC, true>(in, out, taps, ntaps, N, C, flag); });
    else emu::launch(g, b, Tile::LDS_BYTES, [&] { spypre::fir_same_kernel<R, NT, KC, false>(in, out, taps, ntaps, N, C, flag); });
}

}  // extern "C"
