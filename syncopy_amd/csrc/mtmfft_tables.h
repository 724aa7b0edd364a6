// The host tables of a tapered-FFT plan, per kernel family: what spyhip_fft_plan_create / spyhip_fft_plan_set_precision
// upload for a route of mtmfft_route.h, and what the CPU kernel emulator of the tests points its arguments at.  Pure
// functions of the route (no HIP header); T2 is float2 with a Route and double2 with a Route64.
#pragma once
#include <vector>

#include "host_fft.h"
#include "mtmfft_route.h"

namespace spyfft {

// An empty vector: the family does not read that table.
template <class T2>
struct FftTables {
    std::vector<T2> tw;              // exp(-2 pi i m / n), n = the length of the in-LDS transform: nfft, nfft / 2 in the float32
                                     // HALF forms, the Bluestein length (float64: nfft, or the Bluestein length of ANY)
    std::vector<T2> twh;             // HALF forms: float32 exp(-2 pi i f / nfft), f <= nfft / 4; float64 the table of nfft / 2
    std::vector<T2> chirp, bhat;     // Bluestein (spy::bluestein_tables)
    std::vector<T2> tw1, tw2, twM;   // DECLONG: of M, P, nfft.  LONG: of 2^l1, 2^l2, M.  DECLONG64: of M, P
    std::vector<float> tapers_half;  // QUAD, QUAD_HALF: the windows times scale / 2
    std::vector<double> wsum;        // DECLONG, LONG: spy::taper_moments
};

// `tapers`: the (ntaper x nsig) windows as given, `tf` the same rounded to float32
template <class T2>
FftTables<T2> fft_tables(const Route& r, int nfft, int nsig, int ntaper, const double* tapers, double scale, const std::vector<float>& tf) {
    using spy::twiddle_table;
    FftTables<T2> t;
    switch (r.family) {
        case Family::QUAD: case Family::DEC: case Family::MIXED:
            t.tw = twiddle_table<T2>(nfft);
            break;
        case Family::QUAD_HALF: case Family::DEC_HALF:
            t.tw = twiddle_table<T2>(nfft / 2);
            t.twh = twiddle_table<T2>(nfft, nfft / 4 + 1);
            break;
        case Family::BLUE:
            spy::bluestein_tables(nfft, r.M, 0, &t.chirp, &t.bhat);
            t.tw = twiddle_table<T2>(r.M);
            break;
        case Family::DECLONG:
            t.tw1 = twiddle_table<T2>(r.M);
            t.tw2 = twiddle_table<T2>(r.P);
            t.twM = twiddle_table<T2>(nfft);
            break;
        case Family::LONG:
            spy::bluestein_tables(nfft, r.M, 1 << r.l1, &t.chirp, &t.bhat);      // bhat in [k1][k2] order, 1/M folded in
            t.tw1 = twiddle_table<T2>(1 << r.l1);
            t.tw2 = twiddle_table<T2>(1 << r.l2);
            t.twM = twiddle_table<T2>(r.M);
            break;
        case Family::GENERIC:
            if (!r.direct) spy::bluestein_tables(nfft, r.M, 0, &t.chirp, &t.bhat);
            t.tw = twiddle_table<T2>(r.M);
            break;
    }
    if (r.family == Family::QUAD || r.family == Family::QUAD_HALF) t.tapers_half = spy::taper_half_table(tapers, (size_t)ntaper * nsig, scale);
    if (r.family == Family::DECLONG || r.family == Family::LONG) t.wsum = spy::taper_moments(tf, ntaper, nsig);
    return t;
}

// GENERIC: the route's radix list with the tables where they were put, as the kernel takes it (GenPlan of mtmfft_generic.h)
template <class GenPlan, class T2>
GenPlan gen_plan(const Route& r, int nfft, const T2* chirp, const T2* bhat) {
    GenPlan g{};
    g.n = r.M;
    g.nfac = r.nfac;
    for (int i = 0; i < ROUTE_MAXFAC; ++i) g.radix[i] = r.radix[i];
    g.nfft = nfft;
    g.bluestein = r.direct ? 0 : 1;
    g.chirp = chirp;
    g.bhat = bhat;
    g.stage_x = r.stage_x ? 1 : 0;
    return g;
}

// (DECLONG64 is chosen only with Family::DECLONG of the float32 route, whose taper moments `wsum` it shares)
template <class T2>
FftTables<T2> fft_tables64(const Route64& r, int nfft) {
    using spy::twiddle_table;
    FftTables<T2> t;
    if (r.family == Family64::DEC64_HALF) t.twh = twiddle_table<T2>(nfft / 2);
    if (r.family == Family64::DECLONG64) { t.tw1 = twiddle_table<T2>(r.M); t.tw2 = twiddle_table<T2>(r.P); }
    if (r.blue_M) spy::bluestein_tables(nfft, r.blue_M, 0, &t.chirp, &t.bhat);
    t.tw = twiddle_table<T2>(r.blue_M ? r.blue_M : nfft);
    return t;
}

}  // namespace spyfft
