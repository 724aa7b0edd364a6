// Launch geometry and mode dispatch shared by the transform kernels' host code: no HIP header and no runtime call, so
// that the library (through spy_common.h) and the CPU kernel emulator of the tests take their grids from the same lines.
#pragma once
#include <type_traits>

namespace spy {

void set_error(const char* fmt, ...);

// f(integral_constant<int, OUTK>, bool_constant<MEAN>) for the run-time output mode: OUTK = 0 power, 1 other real kinds,
// 2 complex; MEAN = average over the tapers
template <class F>
auto dispatch_mode(int outk, bool mean, F&& f) {
    switch (outk * 2 + (mean ? 1 : 0)) {
        case 0: return f(std::integral_constant<int, 0>{}, std::bool_constant<false>{});
        case 1: return f(std::integral_constant<int, 0>{}, std::bool_constant<true>{});
        case 2: return f(std::integral_constant<int, 1>{}, std::bool_constant<false>{});
        case 3: return f(std::integral_constant<int, 1>{}, std::bool_constant<true>{});
        case 4: return f(std::integral_constant<int, 2>{}, std::bool_constant<false>{});
        default: return f(std::integral_constant<int, 2>{}, std::bool_constant<true>{});
    }
}

// XCD cluster grid of the transform kernels: `nitems` work items (channel quads, pairs or single channels) per segment, G
// per workgroup; S workgroups that share `rows_shared / G` 128-byte rows form a cluster, clusters go round robin over the
// 8 XCDs.  Fills a.npg, a.S, a.ncl.
template <class Args>
int xcd_grid(Args& a, int nitems, int G, int rows_shared, int nseg, unsigned* grid) {
    a.npg = (nitems + G - 1) / G;
    int S = rows_shared / G; if (S < 1) S = 1; if (S > a.npg) S = a.npg;
    a.S = S;
    a.ncl = (a.npg + S - 1) / S;
    const long long nclusters = (long long)nseg * a.ncl;
    const long long g = ((nclusters + 7) / 8) * S * 8;
    if (g > 0x7fffffffLL) { set_error("fft_exec: grid too large (%lld blocks)", g); return -1; }
    *grid = (unsigned)g;
    return 0;
}

// f(args, s0, ns) for the segments [s0, s0 + ns) of launches with the segment on a grid axis (at most 65535 per launch):
// `args` is `a` with seg_start / seg_lo / seg_hi moved to s0
template <class Args, class F>
void for_seg_launches(const Args& a, int nseg, F&& f) {
    for (int s0 = 0; s0 < nseg; s0 += 65535) {
        Args m = a;
        m.seg_start += s0; m.seg_lo += s0; m.seg_hi += s0;
        f(m, s0, nseg - s0 < 65535 ? nseg - s0 : 65535);
    }
}

}  // namespace spy
