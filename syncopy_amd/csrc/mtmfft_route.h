// Which kernel family serves a tapered FFT (K1): pure integer logic, no HIP header and no runtime call, so that the
// selection is testable on any host (tests/test_fft_route.py).  Two readers: mtmfft.hip uploads the tables a route needs
// (mtmfft_tables.h) and launches it; the CPU kernel emulator of the tests (tests/emu/emu_kernels.cpp: emu_fft_exec) asks the
// same route, points its arguments at the same tables and walks the same steps on host memory.
//
// The length tables below are the only place the host code asks "is this length scheduled"; the instance translation
// units (mtmfft_dec_*.hip, mtmfft_dec64_*.hip) hold the matching `case`s, and tests/test_gpu_fft_schedules.py runs every
// entry, so a table entry without an instance fails there.
#pragma once
#include <cstddef>
#include <cstdio>
#include <string>

#include "f64_plus_plan.h"
#include "mtmfft_mixed_plan.h"

namespace spyfft {

// float32 compile-time radix schedules (mtmfft_dec_{a..l}.hip): decimal trial lengths (1 kHz x 0.1 ... 10 s) and 3 x 2^k
constexpr int DEC_LENGTHS[] = {100,  200,  300,  400,  500,  600,  768,  800,  1000, 1200, 1500, 1536, 1600, 2000,
                               2400, 2500, 3000, 3072, 3200, 4000, 4800, 5000, 6000, 6144, 7500, 8000, 10000};
// beyond one workgroup's LDS in quad form, but a channel pair (float64: a single channel) fits through the schedule of
// nfft / 2 (mtmfft_dec_{m,n}.hip, mtmfft_quad_half.hip, mtmfft_dec64_{o,p}.hip)
constexpr int HALF_LENGTHS[] = {12000, 12288, 15000, 16000, 16384, 20000};
// reference-precision compile-time schedules (mtmfft_dec64_{a..n}.hip)
constexpr int DEC64_LENGTHS[] = {100,  200,  256,  300,  400,  500,  512,  600,  768,  800,  1000,
                                 1024, 1200, 1500, 1536, 1600, 2000, 2048, 2400, 2500, 3000, 3072,
                                 3200, 4000, 4096, 4800, 5000, 6000, 6144, 7500, 8000, 8192, 10000};

template <size_t K>
constexpr bool in_table(const int (&t)[K], int n) {
    for (int v : t)
        if (v == n) return true;
    return false;
}

constexpr int ROUTE_MAXFAC = 20;                        // (= GEN_MAXFAC of mtmfft_generic.h)

// SPYHIP_OUT_* of include/spyhip.h -> the OUTK template argument of the kernels: 0 power, 1 other real kinds, 2 complex
constexpr int outk_of(int output) { return output == 2 ? 2 : (output == 0 ? 0 : 1); }

enum class Family { QUAD, QUAD_HALF, DEC, DEC_HALF, MIXED, BLUE, DECLONG, LONG, GENERIC };

struct Route {
    Family family = Family::GENERIC;
    int err = 0;                // 0, or the code spyhip_fft_plan_create returns with `message`
    std::string message;
    std::string kernel_name;
    int log2n = 0, G = 1;       // QUAD, BLUE: packed power-of-two engine of length 2^log2n, G quads per workgroup; MIXED: G
    int P = 0, M = 0;           // DECLONG: nfft = P M.  BLUE, LONG, GENERIC: the transform length (Bluestein: M >= 2 nfft - 1)
    int l1 = 0, l2 = 0;         // LONG: M = 2^l1 x 2^l2
    bool direct = false;        // LONG: nfft == M, one plain four-step transform; GENERIC: no Bluestein either
    MixPlan mix{};              // MIXED
    int mix_threads = 0;
    int radix[ROUTE_MAXFAC] = {};  // GENERIC: Stockham passes of length M
    int nfac = 0;
    bool stage_x = false;       // GENERIC: the segment is staged in LDS
    size_t lds_bytes = 0;       // MIXED, GENERIC
};

enum class Family64 { DEC64, DEC64_HALF, DECLONG64, ANY };

struct Route64 {
    Family64 family = Family64::ANY;
    int err = 0;
    std::string message;
    std::string kernel_name;
    int P = 0, M = 0;           // DECLONG64: nfft = P M
    int blue_M = 0;             // ANY in Bluestein form: M = 2^m >= 2 nfft - 1, else 0
    spywil::PlusPlan plan{};    // ANY: factor schedule of nfft (of blue_M)
};

namespace route_detail {

constexpr bool pow2(int v) { return v > 0 && !(v & (v - 1)); }
inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// radix schedule of the generic Stockham passes; false if n has a prime factor > 13
inline bool factorize(int n, int* radix, int* nfac) {
    static const int cand[] = {16, 8, 4, 2, 3, 5, 7, 11, 13};
    int k = 0;
    for (int c : cand) {
        while (n % c == 0 && n > 1) {
            if (k >= ROUTE_MAXFAC) return false;
            radix[k++] = c;
            n /= c;
        }
    }
    *nfac = k;
    return n == 1;
}

// N = P M with M a sub-transform length of mtmfft_declong.h (in order of preference: cost per point of the schedule,
// then the fewest radix-P terms) and P in {2, 3, 4, 5, 6, 8}
inline bool declong_split(int nfft, int* P, int* M) {
    static const int subs[] = {4096, 2000, 5000, 4000, 10000, 8000};
    for (int m : subs) {
        if (nfft % m) continue;
        const int q = nfft / m;
        if (q == 2 || q == 3 || q == 4 || q == 5 || q == 6 || q == 8) { *P = q; *M = m; return true; }
    }
    return false;
}

// channel quads interleaved per workgroup of the packed kernel (256 threads up to N = 4096)
constexpr int default_G(int log2n) { return log2n >= 12 ? 1 : log2n == 11 ? 2 : log2n == 10 ? 4 : log2n == 9 ? 8 : 16; }

template <class... A>
std::string fmt(const char* f, A... a) {
    char buf[192];
    std::snprintf(buf, sizeof buf, f, a...);
    return buf;
}

}  // namespace route_detail

// "OUTK, MEAN" as the kernel names spell the output mode
inline std::string route_mode(int output, int keeptapers) {
    return route_detail::fmt("%d, %s", outk_of(output), keeptapers ? "false" : "true");
}

// ---- One filler per family: the parameters that family launches by, and its kernel name.  fft_route() below calls them in
// the order of precedence; the kernel emulator of the tests calls one directly to run a family on a shape the route gives
// to another (LONG at 1500 samples, BLUE instead of MIXED at 500, DECLONG at 6 x 2000).

// QUAD: power-of-two nfft in 256 ... 8192 on the packed engine; QUAD_HALF: 2^14 as channel pairs through the 8192-point
// schedule (mtmfft_quad_half.hip)
inline void route_quad(Route& r, int nfft, int output, int keeptapers) {
    using namespace route_detail;
    const std::string mode = route_mode(output, keeptapers);
    r.log2n = ilog2(nfft);
    if (r.log2n == 14) {
        r.family = Family::QUAD_HALF;
        r.kernel_name = fmt("mtmfft_quad_kernel<13, 1, %s, HALF of N = %d>", mode.c_str(), nfft);
        return;
    }
    r.family = Family::QUAD;
    r.G = default_G(r.log2n);
    // complex spectra of every taper at N = 4096 are store-bound: two quads per workgroup (one workgroup per
    // CU) write 64 contiguous bytes per bin row and are 13 % faster; everything else prefers two independent
    // 256-thread workgroups per CU
    if (r.log2n == 12 && outk_of(output) == 2 && keeptapers) r.G = 2;
    r.kernel_name = fmt("mtmfft_quad_kernel<%d, %d, %s>", r.log2n, r.G, mode.c_str());
}

// DEC / DEC_HALF: the compile-time schedule of nfft (HALF: channel pairs through the schedule of nfft / 2)
inline void route_dec(Route& r, int nfft, bool half, const std::string& mode) {
    r.family = half ? Family::DEC_HALF : Family::DEC;
    r.kernel_name = route_detail::fmt(half ? "mtmfft_dec_kernel<HALF of N = %d, %s>" : "mtmfft_dec_kernel<N = %d, %s>", nfft, mode.c_str());
}

// MIXED: the packed mixed-radix engine, if it has a schedule for nfft that fits the LDS
inline bool route_mixed(Route& r, int nfft, int nchan, size_t lds_per_block, const std::string& mode) {
    if (!mix_schedule(nfft, (nchan + 3) / 4, &r.mix, &r.mix_threads, &r.lds_bytes) || r.lds_bytes > lds_per_block) return false;
    r.family = Family::MIXED;
    r.G = 1 << r.mix.lg;
    std::string sched;
    for (int i = 0; i < r.mix.npass; ++i) sched += (i ? "x" : "") + std::to_string(r.mix.radix[i]);
    r.kernel_name = route_detail::fmt("mtmfft_mixed_kernel<%s> N=%d (%s) %d threads x %d quads", mode.c_str(), nfft, sched.c_str(),
                                      r.mix.th, r.G);
    return true;
}

// BLUE: Bluestein on the packed power-of-two engine: M = 2^log2n >= 2 nfft - 1 (at least 256, at most 8192)
inline void route_blue(Route& r, int nfft, const std::string& mode) {
    using namespace route_detail;
    r.family = Family::BLUE;
    r.M = 256;
    while (r.M < 2 * nfft - 1) r.M <<= 1;
    r.log2n = ilog2(r.M);
    r.G = default_G(r.log2n);
    r.kernel_name = fmt("mtmfft_blue_kernel<%d, %d, %s>", r.log2n, r.G, mode.c_str());
}

// DECLONG: longer than one workgroup's LDS, N = P M with M a scheduled length: decimation in time through HBM
inline bool route_declong(Route& r, int nfft, const std::string& mode) {
    if (!route_detail::declong_split(nfft, &r.P, &r.M)) return false;
    r.family = Family::DECLONG;
    r.kernel_name = route_detail::fmt("declong<%d x %d, %s>", r.P, r.M, mode.c_str());
    return true;
}

// LONG: Bluestein with four-step transforms through HBM: M = 2^m >= 2 nfft - 1 (>= 4096), M1 = 2^ceil(m/2), M2 = M / M1;
// a power-of-two nfft is one plain four-step transform
inline void route_long(Route& r, int nfft, const std::string& mode) {
    using namespace route_detail;
    r.family = Family::LONG;
    r.direct = pow2(nfft) && nfft >= 4096;
    int m = 12;
    while ((1LL << m) < (r.direct ? (long long)nfft : 2LL * nfft - 1)) ++m;
    r.M = 1 << m;
    r.l1 = (m + 1) / 2;
    r.l2 = m / 2;
    r.kernel_name = fmt("mtmfft_long<%d x %d, %s>", 1 << r.l1, 1 << r.l2, mode.c_str());
}

// GENERIC: Stockham passes in LDS over the radix list of nfft, or of the Bluestein length where nfft has a prime factor > 13
inline void route_generic(Route& r, int nsig, int nfft, size_t lds_per_block, const std::string& mode) {
    using namespace route_detail;
    r.family = Family::GENERIC;
    if (nfft < 16) { r.err = -1; r.message = fmt("nfft=%d too short (need >= 16)", nfft); return; }
    r.M = nfft;
    r.direct = factorize(nfft, r.radix, &r.nfac);
    if (!r.direct) {            // Bluestein: circular convolution of length M = pow2 >= 2*nfft-1
        r.M = 16;
        while (r.M < 2 * nfft - 1) r.M <<= 1;
        factorize(r.M, r.radix, &r.nfac);
    }
    const size_t work = (size_t)2 * r.M * 8, staged = work + (size_t)nsig * 8;      // float2 elements
    r.stage_x = staged <= lds_per_block;
    r.lds_bytes = r.stage_x ? staged : work;
    if (r.lds_bytes > lds_per_block) {
        r.err = -3;
        r.message = fmt("nfft=%d needs %zu bytes of LDS (> %zu): unsupported length", nfft, r.lds_bytes, lds_per_block);
        return;
    }
    r.kernel_name = fmt("mtmfft_generic_kernel<%s>", mode.c_str());
}

// The float32 route.  The order of the tests is the order of precedence between the families.
inline Route fft_route(int nsig, int nfft, int nchan, int ntaper, int output, int keeptapers, size_t lds_per_block,
                       bool force_generic) {
    using namespace route_detail;
    (void)ntaper;               // (reserved: no family depends on the taper count today)
    Route r;
    const std::string mode = route_mode(output, keeptapers);
    if (force_generic) { route_generic(r, nsig, nfft, lds_per_block, mode); return r; }
    if (pow2(nfft) && nfft >= 256 && nfft <= 16384) { route_quad(r, nfft, output, keeptapers); return r; }
    if (in_table(DEC_LENGTHS, nfft)) {
        // decimal trial lengths: radix schedules fixed at compile time, 10 values per thread.
        // HALF form where it measured faster than the quad form (tools/half_probe.py): 5000 (88 KB of LDS per quad: one
        // workgroup per CU; pairs 12.8 vs 16.0 us/trial at 256 channels) and 10000 with the taper mean (split exchanges
        // in quad form: 39.3 vs 43.9, complex 42.6 vs 61.7; with every taper kept the 8-byte stores of a pair cost more)
        route_dec(r, nfft, nfft == 5000 || (nfft == 10000 && !keeptapers), mode);
        return r;
    }
    // 5-smooth lengths take the mixed-radix engine whatever the taper count: the chirp-z kernel's two length-M transforms
    // and three pointwise products leave ~4x the float32 error of a direct transform
    if (route_mixed(r, nfft, nchan, lds_per_block, mode)) return r;
    if (nfft >= 2 && 2 * nfft - 1 <= 8192) { route_blue(r, nfft, mode); return r; }
    if (nfft > 10240 && route_declong(r, nfft, mode)) {
        // up to 20480 samples a channel PAIR still fits one workgroup's LDS: the real transform through the schedule
        // of nfft / 2 (CfgD::HALF)
        if (in_table(HALF_LENGTHS, nfft)) { r.P = r.M = 0; route_dec(r, nfft, true, mode); }
        return r;
    }
    // (lengths up to 10240 with prime factors <= 13 stay on the generic LDS kernel below: measured 10-20 % faster than the
    // HBM round trips of the long path; everything longer, and awkward lengths, go there)
    if (nfft <= (1 << 19) && !(nfft <= 10240 && factorize(nfft, r.radix, &r.nfac))) { route_long(r, nfft, mode); return r; }
    route_generic(r, nsig, nfft, lds_per_block, mode);
    return r;
}

// DEC64 / DEC64_HALF: the reference-precision compile-time schedule of nfft (filler, as the float32 ones above)
inline void route64_dec(Route64& r, int nfft, bool half, const std::string& mode) {
    r.family = half ? Family64::DEC64_HALF : Family64::DEC64;
    r.kernel_name = route_detail::fmt(half ? "mtmfft_dec64_kernel<HALF of N = %d, %s>" : "mtmfft_dec64_kernel<N = %d, %s>", nfft, mode.c_str());
}

// The reference-precision route (spyhip_fft_plan_set_precision): float64 taper product and transform.  `f32` is the
// float32 route of the same plan: the decimation through HBM serves both precisions or neither (they share the plan's
// taper moments).
inline Route64 fft_route64(int nfft, int output, int keeptapers, const Route& f32) {
    using namespace route_detail;
    Route64 r;
    const std::string mode = route_mode(output, keeptapers);
    // (HALF: single channels through the schedule of nfft / 2, CfgD64::HALF)
    if (in_table(HALF_LENGTHS, nfft)) { route64_dec(r, nfft, true, mode); return r; }
    if (in_table(DEC64_LENGTHS, nfft)) { route64_dec(r, nfft, false, mode); return r; }
    if (f32.family == Family::DECLONG) {
        r.family = Family64::DECLONG64;
        r.P = f32.P;
        r.M = f32.M;
        r.kernel_name = fmt("declong64_kernel<%d x %d, %s>", r.P, r.M, mode.c_str());
        return r;
    }
    // any other length: generic Stockham passes over work arrays in LDS / global memory; the O(R^2) pass of a prime
    // factor R is only reasonable for small R - beyond 61 the transform takes Bluestein's form on M = 2^m >= 2 nfft - 1
    r.family = Family64::ANY;
    if (nfft < 2 || nfft > (1 << 20)) {
        r.err = -3;
        r.message = fmt("fft_plan_set_precision: the reference-precision kernels serve transform lengths 2 ... 2^20 (nfft = %d)", nfft);
        return r;
    }
    int big = 1;
    if (!spywil::plus_plan(nfft, &r.plan)) big = 1 << 30;
    else for (int i = 0; i < r.plan.nfac; ++i) big = r.plan.radix[i] > big ? r.plan.radix[i] : big;
    if (big > 61) {
        r.blue_M = 16;
        while (r.blue_M < 2 * nfft - 1) r.blue_M <<= 1;
        spywil::plus_plan(r.blue_M, &r.plan);
        r.kernel_name = fmt("mtmfft_f64_any_kernel<%s> N=%d (Bluestein, M = %d)", mode.c_str(), nfft, r.blue_M);
    } else {
        r.kernel_name = fmt("mtmfft_f64_any_kernel<%s> N=%d", mode.c_str(), nfft);
    }
    return r;
}

}  // namespace spyfft
