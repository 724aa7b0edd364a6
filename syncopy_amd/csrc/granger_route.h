// Which kernels serve the Wilson / Granger stage (K6), with which grid and how much LDS, and where the work arrays of
// spyhip_granger lie: pure integer logic, no HIP header and no runtime call, so that the launcher (granger.hip, which
// the kernel emulator runs: tests/emu/granger_emu.cpp) and the route test (tests/emu/granger_route_shim.cpp) read one decision.
// The constexpr functions are callable from device code as they stand (granger_kernels.h, wilson_plus_kernel.h).
// tests/test_granger_route.py holds the resulting table of size classes for the 160 KiB of LDS of the MI355X.
#pragma once
#include <cstddef>

namespace spywil {

constexpr int GT = 32;       // output tile of zgemm_kernel
constexpr int MT = 64;       // output tile of zgemm_mfma_kernel
constexpr int ZB = 16;       // rows per block of zinv_blocked_kernel
constexpr int ZM = 32;       // rows per block of zinv_mfma_kernel
constexpr int ZT = 512;      // threads of the matrix-core inverses: 8 waves = two per SIMD (an MFMA blocks its wave; the
                             // partner keeps the pipe busy)
constexpr int ZW = 64;       // rows per block of zinv64_mfma_kernel
constexpr int CHP = 32;      // columns per panel of zchol_panel_kernel
constexpr int NRED = 1024;   // workgroups (= partial maxima) of relerr_kernel
constexpr size_t CD = 16;    // bytes of a complex128

struct Grid3 { unsigned x = 1, y = 1, z = 1; };

// ---- products
// 64 x 64 output tiles per matrix: all of them, or the lower triangle for the Hermitian modes (2: error check, 3: X X^H)
constexpr int zgemm_tiles(int n, bool hermitian) {
    return hermitian ? ((n + 63) / 64) * ((n + 63) / 64 + 1) / 2 : ((n + 63) / 64) * ((n + 63) / 64);
}
// tiles a workgroup works through (measured per mode at 2049 x 256 x 256: the plain product - whose four tiles of a row
// share the A panel - likes 4 tiles per workgroup, 3.66 -> 2.84 ms with the triangular factor; the others are best with 2)
constexpr int zgemm_tpw(int mode) { return mode == 0 ? 4 : 2; }
constexpr int zgemm_groups(int n, int mode) {
    return (zgemm_tiles(n, mode == 2 || mode == 3) + zgemm_tpw(mode) - 1) / zgemm_tpw(mode);
}

enum class Gemm { TILED, MFMA0, MFMA1, MFMA2, MFMA3 };
struct GemmRoute {
    Gemm kernel = Gemm::TILED;
    const char* name = "";
    Grid3 grid;
    unsigned threads = 256;
    size_t lds = 0;             // dynamic LDS (the tiles are static)
    int mode = -1;              // the MODE of zgemm_mfma_kernel, -1 for zgemm_kernel
    int ntiles = 0;             // MFMA2: partial maxima per matrix
};
// C[b] = A[b] op(B[b]).  n >= 48: the fp64 matrix cores, 64 x 64 tiles on the XCD-aware 1-D grid (groups of tiles x the
// batch rounded up to the 8 XCDs, see the kernel).  `same`: A == B && sA == sB, with opB = 1 the Hermitian product X X^H;
// `badd`: a matrix joins op(B); `ref`: per-workgroup maxima of |Ref - C| / |Ref| instead of C (both: matrix cores only)
inline GemmRoute gemm_route(int n, int batch, int opB, bool same, bool badd, bool ref) {
    GemmRoute r;
    if (n < 48) {
        r.name = "spywil::zgemm_kernel";
        r.grid.x = r.grid.y = (unsigned)((n + GT - 1) / GT);
        r.grid.z = (unsigned)batch;
        return r;
    }
    static const char* const names[4] = {"spywil::zgemm_mfma_kernel<0>", "spywil::zgemm_mfma_kernel<1>",
                                         "spywil::zgemm_mfma_kernel<2>", "spywil::zgemm_mfma_kernel<3>"};
    r.mode = ref ? 2 : (badd ? 1 : ((opB == 1 && same) ? 3 : 0));
    r.kernel = (Gemm)((int)Gemm::MFMA0 + r.mode);
    r.name = names[r.mode];
    r.grid.x = (unsigned)(zgemm_groups(n, r.mode) * ((batch + 7) / 8) * 8);
    r.ntiles = zgemm_tiles(n, r.mode == 2 || r.mode == 3);
    return r;
}

// ---- inverse: one workgroup per matrix
enum class Inv { MFMA64, MFMA32, BLOCKED16, PIVOTED };
struct InvRoute {
    Inv kernel = Inv::PIVOTED;
    const char* name = "";
    unsigned threads = 256;
    size_t lds = 0;
    bool copy_src = false;      // the kernel works in place: `src` is copied into M first
};
// blocked: block Gauss-Jordan (pivots inside the diagonal blocks only; info = 2 where a tiny pivot showed up and the
// caller must repeat with blocked = false); false: partial pivoting, 16x the traffic.  has_src: out of place.
inline InvRoute inv_route(int n, bool blocked, bool has_src, size_t lds_per_block) {
    InvRoute r;
    // 64-row blocks (half the sweeps over the matrices) where they pad no more than the 32-row blocks would
    // (its 130 KiB fit every device this library was built for; a smaller LDS falls through to the kernels below)
    if (blocked && n >= 2 * ZW && (n + 63) / 64 * 64 == (n + 31) / 32 * 32 && (size_t)2 * ZW * (ZW + 1) * CD <= lds_per_block) {
        r.kernel = Inv::MFMA64; r.name = "spywil::zinv64_mfma_kernel"; r.threads = ZT;
        r.lds = (size_t)2 * ZW * (ZW + 1) * CD;
        return r;
    }
    if (blocked && n >= 2 * ZM) {
        const int npad = ((n + ZM - 1) / ZM) * ZM;
        const size_t lds = ((size_t)ZM * (npad + 1) + ZM * (ZM + 1)) * CD;
        if (lds <= lds_per_block) {
            r.kernel = Inv::MFMA32; r.name = "spywil::zinv_mfma_kernel"; r.threads = ZT; r.lds = lds;
            return r;
        }
    }
    r.copy_src = has_src;
    if (blocked && n >= 2 * ZB) {
        const int npad = ((n + ZB - 1) / ZB) * ZB;
        const size_t lds = ((size_t)ZB * npad + ZB * ZB) * CD;
        if (lds <= lds_per_block) {
            r.kernel = Inv::BLOCKED16; r.name = "spywil::zinv_blocked_kernel"; r.lds = lds;
            return r;
        }
    }
    r.name = "spywil::zinv_kernel";
    r.lds = (size_t)n * (2 * CD + sizeof(int));
    return r;
}

// ---- Cholesky factor in place: one workgroup of 256 threads per matrix
enum class Chol { PANEL, COLUMN };
struct CholRoute {
    Chol kernel = Chol::COLUMN;
    const char* name = "";
    unsigned threads = 256;
    size_t lds = 0;
};
inline CholRoute chol_route(int n, size_t lds_per_block) {
    CholRoute r;
    const size_t plds = ((size_t)n * (CHP + 1) + CHP * (CHP + 1)) * CD;
    if (n <= 256 && n >= 2 * CHP && plds <= lds_per_block) {      // panels of 32 columns
        r.kernel = Chol::PANEL; r.name = "spywil::zchol_panel_kernel"; r.lds = plds;
        return r;
    }
    r.name = "spywil::zchol_kernel";
    r.lds = (size_t)n * CD;
    return r;
}

// ---- plus operator for nent entries over the lag-domain length L
// workgroups of plus4_kernel: ONE entry pair each, in groups of 32 (four pairs share the 128-byte lines of a row)
constexpr long long plus4_grid(long long nent) { return (((nent + 1) / 2 + 31) / 32) * 32; }
// (= PCfg<log2l>::LDS_BYTES of wilson_plus_kernel.h; granger.hip asserts the equality)
constexpr size_t plus4_lds(int log2l) {
    const int L = 1 << log2l, T = L / 16;
    const int xelems = L + (T % 16 == 0 ? L / 16 : 0) + 1, selems = 2 * (L / 2 + 1);
    return (size_t)(xelems > selems ? xelems : selems) * CD;
}

enum class Plus { PLUS4, LDS, LONG };
struct PlusRoute {
    Plus kernel = Plus::LDS;
    const char* name = "";
    int log2l = 0;              // PLUS4: the instance
    long long grid = 0;         // workgroups of one launch (LONG: of a full one)
    unsigned threads = 256;
    size_t lds = 0;
    long long chunk = 0;        // LONG: entries per launch
    size_t scratch_bytes = 0;   // LONG: global work arrays, 2 L complex128 per workgroup
};
// the radix-16 LDS kernel for power-of-two lengths 256 ... 4096, the generic LDS kernel while two length-L arrays fit
// LDS, global scratch beyond (any length)
inline PlusRoute plus_route(int L, long long nent, size_t lds_per_block, int num_cu) {
    static const char* const names4[5] = {"spywil::plus4_kernel<8>", "spywil::plus4_kernel<9>", "spywil::plus4_kernel<10>",
                                          "spywil::plus4_kernel<11>", "spywil::plus4_kernel<12>"};
    PlusRoute r;
    for (int l = 8; l <= 12; ++l)
        if (L == 1 << l && plus4_lds(l) <= lds_per_block) {
            r.kernel = Plus::PLUS4; r.name = names4[l - 8]; r.log2l = l;
            r.grid = plus4_grid(nent); r.threads = (unsigned)(L / 16); r.lds = plus4_lds(l);
            return r;
        }
    const size_t two = (size_t)2 * L * CD;
    if (two <= lds_per_block) {
        r.name = "spywil::plus_kernel"; r.grid = nent; r.lds = two;
        return r;
    }
    // entries per launch: scratch of at most 1 GiB (at least one workgroup per CU if that is more)
    r.kernel = Plus::LONG; r.name = "spywil::plus_long_kernel";
    r.chunk = (long long)(((size_t)1 << 30) / two);
    if (r.chunk < num_cu) r.chunk = num_cu;
    if (r.chunk > nent) r.chunk = nent;
    r.grid = r.chunk;
    r.scratch_bytes = (size_t)r.chunk * two;
    return r;
}

// ---- convergence check max |A - psi psi^H| / |A| (max_rel_err, wilson_sf.py:99-103,190-194)
struct ErrRoute {
    bool fused = false;         // the matrix-core product takes S and the error check along (no product is stored)
    bool subset_first = false;  // every 8th bin first: a lower bound; the full check runs only once the subset passes
    int subset_bins = 0;
};
inline ErrRoute err_route(int n, int F, bool full_check_forced) {
    ErrRoute r;
    r.fused = n >= 48;
    r.subset_first = r.fused && F >= 64 && !full_check_forced;
    r.subset_bins = (F + 7) / 8;
    return r;
}

// ---- work arrays of spyhip_granger: byte offsets into the context's arena, each a multiple of 256
struct Arena {
    size_t A = 0, U = 0, psi = 0, T1 = 0, T2 = 0;      // F x n x n complex128 each
    size_t small = 0;           // 7 n x n complex128: g0, psi0, psi0 next, g0 + S, Sigma, scratch, psi0 of iteration 0
    size_t tw = 0;              // L complex128 twiddles
    size_t lam = 0;             // 2 F doubles: eigenvalue estimates
    size_t inf = 0;             // F ints: flags of the inverse / Cholesky kernels
    size_t part = 0;            // NRED doubles: partial maxima of relerr_kernel, the reduced maximum in part[0]
    size_t bigpart = 0;         // ceil(n / 64)^2 F doubles: per-tile maxima of the fused error check
    size_t total = 0;
};
inline Arena granger_arena(int n, int F) {
    Arena a;
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
    const size_t nn = (size_t)n * n, tot = (size_t)F * nn, mt = (size_t)(n + MT - 1) / MT;
    a.A = take(tot * CD); a.U = take(tot * CD); a.psi = take(tot * CD); a.T1 = take(tot * CD); a.T2 = take(tot * CD);
    a.small = take(7 * nn * CD);
    a.tw = take((size_t)2 * (F - 1) * CD);
    a.lam = take(2 * (size_t)F * sizeof(double));
    a.inf = take((size_t)F * sizeof(int));
    a.part = take(NRED * sizeof(double));
    a.bigpart = take(mt * mt * F * sizeof(double));
    a.total = off;
    return a;
}

}  // namespace spywil
