// Which kernel family computes the analytic signal (scipy.signal.hilbert, circular over the trial length N, no padding)
// of the Hilbert option of spy.preprocessing: pure integer logic, no HIP header and no runtime call, so that the launcher
// (hilbert.hip), the kernel emulator (tests/emu/hilbert_emu.cpp) and the route test (tests/emu/hilbert_route_shim.cpp)
// read one decision.
//
//   PACKED  N = 2^k, 16 ... 8192      forward FFT, times h, inverse FFT on the packed radix-16 engine (fft2_device.h)
//   BLUE    other N with 2N - 1 <= 8192  the same through Bluestein's chirp-z form: four transforms of M = 2^m >= 2N - 1
//   ANY64   everything else <= 2^20   complex128 Stockham passes over global work arrays (f64_stockham.h), in Bluestein's
//                                     form when the largest prime factor exceeds 61, as fft_route64 decides for Family64::ANY
//   COPY    N = 1                     the analytic signal of one sample is the sample: a conversion of x + 0j
#pragma once
#include <cstddef>
#include <cstdio>
#include <string>

#include "f64_plus_plan.h"

namespace spyhil {

constexpr int HILBERT_MAX_N = 1 << 20;
constexpr int PACKED_MIN_N = 16, PACKED_MAX_N = 8192;
constexpr int BLUE_MAX_M = 8192, BLUE_MIN_M = 256;
constexpr int ANY64_MAX_PRIME = 61;
// bytes of complex128 work arrays one ANY64 launch may hold (two arrays of length L per workgroup)
constexpr size_t ANY64_WORK_BYTES = (size_t)512 << 20;

enum class Family { COPY, PACKED, BLUE, ANY64 };

struct Route {
    Family family = Family::COPY;
    int err = 0;                // 0, or the code spyhip_hilbert_plan_create returns with `message`
    std::string message;
    std::string kernel_name;
    int M = 0;                  // transform length: N (PACKED, ANY64 in radix form), the Bluestein length (BLUE, ANY64)
    int log2n = 0, G = 1;       // PACKED, BLUE: engine of length 2^log2n, G channel quads per workgroup
    int threads = 0;            // threads per workgroup
    size_t lds_bytes = 0;       // dynamic LDS per workgroup
    bool bluestein = false;     // ANY64: chirp-z form
    spywil::PlusPlan plan{};    // ANY64: factor schedule of M
};

namespace route_detail {

constexpr bool pow2(int v) { return v > 0 && !(v & (v - 1)); }
inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// channel quads interleaved per workgroup of the packed engine: 256 threads up to 4096 points, one quad per thread row
// below 64 points
constexpr int packed_G(int log2n) {
    return log2n >= 12 ? 1 : log2n == 11 ? 2 : log2n == 10 ? 4 : log2n == 9 ? 8 : log2n == 8 ? 16 : log2n == 7 ? 32 : 64;
}
// (= Cfg2<log2n, G>::LDS_BYTES of fft2_device.h; hilbert_kernel.h asserts the equality)
constexpr size_t packed_lds(int log2n, int G) {
    const int N = 1 << log2n, T = N / 16;
    const bool pad = (T % 16) == 0;
    return (size_t)((N + (pad ? N / 16 : 0)) * G + G) * 16;
}

template <class... A>
std::string fmt(const char* f, A... a) {
    char buf[192];
    std::snprintf(buf, sizeof buf, f, a...);
    return buf;
}

}  // namespace route_detail

// (the kernel name leaves the output out: every family has one instance for complex64 and one for the real kinds)
inline Route hilbert_route(long long nsamp) {
    using namespace route_detail;
    Route r;
    if (nsamp < 1 || nsamp > HILBERT_MAX_N) {
        r.err = -3;
        r.message = fmt("hilbert: trials of 1 ... %d (2^20) samples are served (nsamp = %lld)", HILBERT_MAX_N, nsamp);
        return r;
    }
    const int N = (int)nsamp;
    if (N == 1) {
        r.family = Family::COPY;
        r.M = 1;
        r.threads = 256;
        r.kernel_name = "hilbert_copy_kernel";
        return r;
    }
    if (pow2(N) && N >= PACKED_MIN_N && N <= PACKED_MAX_N) {
        r.family = Family::PACKED;
        r.M = N;
        r.log2n = ilog2(N);
    } else if (2 * N - 1 <= BLUE_MAX_M) {
        r.family = Family::BLUE;
        r.M = BLUE_MIN_M;
        while (r.M < 2 * N - 1) r.M <<= 1;
        r.log2n = ilog2(r.M);
    }
    if (r.family != Family::COPY) {
        r.G = packed_G(r.log2n);
        r.threads = (r.M / 16) * r.G;
        r.lds_bytes = packed_lds(r.log2n, r.G);
        r.kernel_name = r.family == Family::PACKED ? fmt("hilbert_packed_kernel<%d, %d>", r.log2n, r.G)
                                                   : fmt("hilbert_packed_kernel<%d, %d, Bluestein> N=%d", r.log2n, r.G, N);
        return r;
    }
    r.family = Family::ANY64;
    r.threads = 256;
    int big = 1;
    if (!spywil::plus_plan(N, &r.plan)) big = 1 << 30;
    else for (int i = 0; i < r.plan.nfac; ++i) big = r.plan.radix[i] > big ? r.plan.radix[i] : big;
    if (big > ANY64_MAX_PRIME) {
        r.bluestein = true;
        r.M = 16;
        while (r.M < 2 * N - 1) r.M <<= 1;
        spywil::plus_plan(r.M, &r.plan);
        r.kernel_name = fmt("hilbert_any64_kernel N=%d (Bluestein, M = %d)", N, r.M);
    } else {
        r.M = N;
        r.kernel_name = fmt("hilbert_any64_kernel N=%d", N);
    }
    return r;
}

// Launch geometry of the packed families: `nquad` channel quads per trial, G per workgroup; the S workgroups that share
// the 128-byte lines of a trial's rows form a cluster, clusters go round robin over the 8 XCDs (the block map of the
// tapered-FFT kernels, spy::xcd_grid).  grid = 0: too many blocks for one launch.
struct PackedGrid {
    int npg = 0, S = 1, ncl = 0;
    unsigned grid = 0;
};
inline PackedGrid packed_grid(long long ntrials, int nchan, int G) {
    PackedGrid g;
    const int nquad = (nchan + 3) / 4;
    g.npg = (nquad + G - 1) / G;
    int S = 8 / G; if (S < 1) S = 1; if (S > g.npg) S = g.npg;
    g.S = S;
    g.ncl = (g.npg + S - 1) / S;
    const long long nclusters = ntrials * g.ncl;
    const long long n = ((nclusters + 7) / 8) * S * 8;
    g.grid = n > 0x7fffffffLL ? 0u : (unsigned)n;
    return g;
}

// Workgroups (one per channel pair and trial) one ANY64 launch may run at once within ANY64_WORK_BYTES, at least one
inline long long any64_chunk(int M) {
    const size_t per = (size_t)2 * (size_t)M * 16;
    const long long c = (long long)(ANY64_WORK_BYTES / per);
    return c < 1 ? 1 : c;
}

// the spectral weight of scipy.signal.hilbert: h[0] = 1, h[k] = 2 for 1 <= k < ceil(N / 2), h[N / 2] = 1 for even N, else 0
constexpr int hilbert_weight(int k, int N) { return (k == 0 || 2 * k == N) ? 1 : (2 * k < N ? 2 : 0); }

}  // namespace spyhil
