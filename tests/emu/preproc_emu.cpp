// CPU emulation of the preprocessing kernels (syncopy_amd/csrc/preproc_kernel.h), TEST INFRASTRUCTURE ONLY (see
// hip_emu.h).  Launches the kernels as preproc.hip does, the FIR kernel on a small tile.  Built by tests/test_preproc.py.
#include "hip_emu.h"

#include <algorithm>

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

// ---- plain models of the cascade, for the error bound of the tests (not the kernels) --------------------------------
// One (time, channel) float32 trial through sosfilt (edge < 0, zero start state) or sosfiltfilt (odd extension by `edge`,
// start states zi * first sample, float64 between the passes), result rounded to float32 (out64, if given: unrounded).  `how`: 0 = float64 with
// separate multiplies and adds (SciPy's statements), 1 and 2 = float64 with every multiply-add that a compiler may
// contract fused, in its two possible pairings, 3 = float64 arithmetic with the state z kept in float32.
namespace {
template <int HOW>
double model_step(const double* sos, int nsec, double* z, double v) {
    for (int s = 0; s < nsec; ++s) {
        const double* r = sos + 6 * s;
        double w, z0, z1;
        if (HOW == 1) {
            w = std::fma(r[0], v, z[2 * s]);
            z0 = std::fma(r[1], v, -(r[4] * w)) + z[2 * s + 1];
            z1 = std::fma(r[2], v, -(r[5] * w));
        } else if (HOW == 2) {
            w = std::fma(r[0], v, z[2 * s]);
            z0 = std::fma(-r[4], w, r[1] * v) + z[2 * s + 1];
            z1 = std::fma(-r[5], w, r[2] * v);
        } else {
            // separate operations: this file is compiled without contraction (the kernel header's pragma, no -mfma)
            w = r[0] * v + z[2 * s];
            z0 = (r[1] * v - r[4] * w) + z[2 * s + 1];
            z1 = r[2] * v - r[5] * w;
        }
        if (HOW == 3) { z0 = (double)(float)z0; z1 = (double)(float)z1; }
        z[2 * s] = z0;
        z[2 * s + 1] = z1;
        v = w;
    }
    return v;
}

template <int HOW>
void model_sos(const float* x, float* out, double* out64, int N, int C, const double* sos, const double* zi, int nsec,
               int edge) {
    std::vector<double> z(2 * nsec), ext, fwd;
    for (int c = 0; c < C; ++c) {
        if (edge < 0) {
            std::fill(z.begin(), z.end(), 0.0);
            for (int i = 0; i < N; ++i) {
                const double r = model_step<HOW>(sos, nsec, z.data(), (double)x[i * C + c]);
                out[i * C + c] = (float)r;
                if (out64) out64[i * C + c] = r;
            }
            continue;
        }
        const int len = N + 2 * edge;
        ext.resize(len);
        fwd.resize(len);
        for (int i = 0; i < edge; ++i) ext[i] = (double)(2.f * x[c] - x[(edge - i) * C + c]);
        for (int i = 0; i < N; ++i) ext[edge + i] = (double)x[i * C + c];
        for (int i = 0; i < edge; ++i) ext[edge + N + i] = (double)(2.f * x[(N - 1) * C + c] - x[(N - 2 - i) * C + c]);
        for (int s = 0; s < 2 * nsec; ++s) z[s] = zi[s] * ext[0];
        if (HOW == 3) for (auto& v : z) v = (double)(float)v;
        for (int i = 0; i < len; ++i) fwd[i] = model_step<HOW>(sos, nsec, z.data(), ext[i]);
        for (int s = 0; s < 2 * nsec; ++s) z[s] = zi[s] * fwd[len - 1];
        if (HOW == 3) for (auto& v : z) v = (double)(float)v;
        for (int i = len - 1; i >= 0; --i) {
            const double r = model_step<HOW>(sos, nsec, z.data(), fwd[i]);
            if (i >= edge && i < edge + N) {
                out[(i - edge) * C + c] = (float)r;
                if (out64) out64[(i - edge) * C + c] = r;
            }
        }
    }
}
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

// the cascade kernels are launched through the launcher's own dispatch (SPY_SOS_DISPATCH: NS = 2, 4, 8, MAX_SECTIONS);
// more sections than are compiled return -1, as fill_sos() of preproc.hip does
int emu_sosfilt(const float* in, float* out, int T, int N, int C, const double* sos, int nsec, int rect, int* flag) {
    if (nsec < 1 || nsec > spypre::MAX_SECTIONS) return -1;
    const SosCoef k = coef(sos, nullptr, nsec);
    const dim3 g = series_grid(T, C), b(spypre::SERIES_THREADS);
#define EMU_ONEPASS(NS)                                                                                          \
    if (rect) emu::launch(g, b, 0, [&] { spypre::sos_onepass_kernel<NS, true>(in, out, k, T, N, C, flag); });    \
    else emu::launch(g, b, 0, [&] { spypre::sos_onepass_kernel<NS, false>(in, out, k, T, N, C, flag); })
    SPY_SOS_DISPATCH(nsec, EMU_ONEPASS);
#undef EMU_ONEPASS
    return 0;
}

int emu_sosfiltfilt(const float* in, float* out, double* work, int T, int N, int C, const double* sos, const double* zi,
                    int nsec, int edge, int rect, int* flag) {
    if (nsec < 1 || nsec > spypre::MAX_SECTIONS || edge < 0 || N <= edge) return -1;
    const SosCoef k = coef(sos, zi, nsec);
    const dim3 g = series_grid(T, C), b(spypre::SERIES_THREADS);
#define EMU_FORWARD(NS) emu::launch(g, b, 0, [&] { spypre::sos_forward_kernel<NS>(in, work, k, T, N, C, edge, flag); })
    SPY_SOS_DISPATCH(nsec, EMU_FORWARD);
#undef EMU_FORWARD
#define EMU_BACKWARD(NS)                                                                                             \
    if (rect) emu::launch(g, b, 0, [&] { spypre::sos_backward_kernel<NS, true>(work, out, k, T, N, C, edge); });     \
    else emu::launch(g, b, 0, [&] { spypre::sos_backward_kernel<NS, false>(work, out, k, T, N, C, edge); })
    SPY_SOS_DISPATCH(nsec, EMU_BACKWARD);
#undef EMU_BACKWARD
    return 0;
}

int model_sosfilt(const float* x, float* out, double* out64, int N, int C, const double* sos, const double* zi, int nsec,
                  int edge, int how) {
    if (nsec < 1 || (edge >= 0 && (!zi || N <= edge))) return -1;
    switch (how) {
        case 0: model_sos<0>(x, out, out64, N, C, sos, zi, nsec, edge); return 0;
        case 1: model_sos<1>(x, out, out64, N, C, sos, zi, nsec, edge); return 0;
        case 2: model_sos<2>(x, out, out64, N, C, sos, zi, nsec, edge); return 0;
        case 3: model_sos<3>(x, out, out64, N, C, sos, zi, nsec, edge); return 0;
    }
    return -1;
}

void emu_fir_same(const float* in, float* out, int T, int N, int C, const double* taps, int ntaps, int rect, int* flag) {
    const dim3 g((unsigned)((C + 63) / 64), (unsigned)((N + Tile::T - 1) / Tile::T), (unsigned)T), b(Tile::THREADS);
    if (rect) emu::launch(g, b, Tile::LDS_BYTES, [&] { spypre::fir_same_kernel<R, NT, KC, true>(in, out, taps, ntaps, N, C, flag); });
    else emu::launch(g, b, Tile::LDS_BYTES, [&] { spypre::fir_same_kernel<R, NT, KC, false>(in, out, taps, ntaps, N, C, flag); });
}

}  // extern "C"
