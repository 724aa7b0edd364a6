// How spyhip_directed_norm (K11: directed transfer function / partial directed coherence from a stack of complex128
// matrices) is launched: pure integer logic, no HIP header and no runtime call, so that the launcher (directed.hip), the
// kernel under the CPU emulator (tests/emu/directed_emu.cpp) and the route test (tests/emu/directed_route_shim.cpp) read one
// decision.  The constexpr functions are callable from device code as they stand (directed_kernel.h).
//
// A workgroup owns a strip of DL "lines" of one matrix - rows for axis 0 (the norm runs along a row of M), columns for
// axis 1 (along a column) - and all n entries along them.  It reads the strip once with 16-byte loads, keeps
// w_k^2 |M|^2 (8 bytes per entry) in LDS next to the DL sums, and writes the transposed, normalised float32 values from
// LDS.  A strip that does not fit is worked through in chunks of `kc` entries along the line: the sums come from a first
// sweep, the second sweep re-reads each chunk (the strip is DL n 16 bytes, 0.5 MB at n = 1024: L2) into the LDS tile.
#pragma once
#include <cstddef>

namespace spydir {

constexpr int DL = 32;       // lines per workgroup: 128-byte runs of float32 (axis 0) / 512-byte runs of complex128 (axis 1)
constexpr int DT = 256;      // threads per workgroup
constexpr int DW = DT / 64;  // waves
constexpr int DKC = 256;     // largest chunk along the line of a strip that is not kept whole

// row stride of the LDS tile in doubles: odd, so that the DL lines of one column fall into DL different bank pairs
constexpr int norm_ld(int kc) { return kc | 1; }
// the tile, the DL sums and the DW x DL partial sums of axis 1
constexpr size_t norm_lds(int kc) { return ((size_t)DL * norm_ld(kc) + DL + (size_t)DW * DL) * sizeof(double); }
constexpr int norm_strips(int n) { return (n + DL - 1) / DL; }

struct NormRoute {
    bool ok = false;            // false: not even the smallest tile fits the LDS of a workgroup
    bool cached = false;        // the whole strip stays in LDS: every element of M is read once
    int kc = 0;                 // entries along the line per LDS tile (n when cached)
    int strips = 0;             // workgroups per matrix
    long long grid = 0;         // XCD-aware 1-D grid: strips x the matrices rounded up to the 8 XCDs (see the kernel)
    unsigned threads = DT;
    size_t lds = 0;
};
// Two workgroups per CU are wanted (the loads of one hide behind the stores of the other), so a strip is kept whole
// only in half of the LDS; at 160 KiB that is n <= 315.
inline NormRoute norm_route(int n, int nfreq, size_t lds_per_block) {
    NormRoute r;
    r.strips = norm_strips(n);
    r.grid = (long long)r.strips * ((nfreq + 7) / 8) * 8;
    if (norm_lds(n) <= lds_per_block / 2) {
        r.ok = r.cached = true; r.kc = n; r.lds = norm_lds(n);
        return r;
    }
    for (int pass = 0; pass < 2 && !r.ok; ++pass)
        for (int kc = DKC; kc >= 64 && !r.ok; kc /= 2)
            if (kc < n && norm_lds(kc) <= (pass == 0 ? lds_per_block / 2 : lds_per_block)) {
                r.ok = true; r.kc = kc; r.lds = norm_lds(kc);
            }
    if (!r.ok && norm_lds(n) <= lds_per_block) {       // a small matrix on a tiny LDS: whole after all
        r.ok = r.cached = true; r.kc = n; r.lds = norm_lds(n);
    }
    return r;
}

}  // namespace spydir
