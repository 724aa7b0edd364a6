// CPU emulation of spy.preprocessing, TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's own launchers
// (syncopy_amd/csrc/preproc.hip) and kernels, on the runtime stand-in hip/hip_runtime.h, and plain models of the
// second-order-section cascade.  Built by tests/test_preproc.py.
#include "../../syncopy_amd/csrc/preproc.hip"
#include "emu_unit.h"

#include <algorithm>

// the same launcher on a tile of 8 outputs, 2 waves and 8 taps per stage (the cases of test_emu_fir are tuned to it)
extern "C" int emu_fir_same_small(spyhip_ctx* ctx, const float* in, float* out, int64_t ntrials, int64_t nsamp, int64_t nchan,
                                  const double* taps, int ntaps, int rectify, int32_t* nan) {
    return fir_launch<4, 2, 8>(ctx, in, out, ntrials, nsamp, nchan, taps, ntaps, rectify, nan);
}

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

extern "C" int model_sosfilt(const float* x, float* out, double* out64, int N, int C, const double* sos, const double* zi, int nsec,
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
