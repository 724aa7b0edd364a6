// C view of the pure route of the Wilson / Granger stage (syncopy_amd/csrc/granger_route.h) for
// tests/test_granger_route.py (TEST INFRASTRUCTURE ONLY).  Built with the host compiler alone: the header must not need HIP.
#include <cstdio>

#include "../../syncopy_amd/csrc/granger_route.h"

using namespace spywil;

extern "C" {

// out: {kernel, threads, lds, copy_src}
void wr_inv(int n, int blocked, int has_src, unsigned long long lds_per_block, long long* out, char* name, int cap) {
    const InvRoute r = inv_route(n, blocked != 0, has_src != 0, (size_t)lds_per_block);
    out[0] = (int)r.kernel; out[1] = r.threads; out[2] = (long long)r.lds; out[3] = r.copy_src;
    std::snprintf(name, cap, "%s", r.name);
}

// out: {kernel, threads, lds}
void wr_chol(int n, unsigned long long lds_per_block, long long* out, char* name, int cap) {
    const CholRoute r = chol_route(n, (size_t)lds_per_block);
    out[0] = (int)r.kernel; out[1] = r.threads; out[2] = (long long)r.lds;
    std::snprintf(name, cap, "%s", r.name);
}

// out: {kernel, mode, grid x, y, z, threads, lds, partial maxima per matrix, tiles per matrix, tiles per workgroup}
void wr_gemm(int n, int batch, int opB, int same, int badd, int ref, long long* out, char* name, int cap) {
    const GemmRoute r = gemm_route(n, batch, opB, same != 0, badd != 0, ref != 0);
    out[0] = (int)r.kernel; out[1] = r.mode; out[2] = r.grid.x; out[3] = r.grid.y; out[4] = r.grid.z; out[5] = r.threads;
    out[6] = (long long)r.lds; out[7] = r.ntiles;
    out[8] = r.mode < 0 ? 0 : zgemm_tiles(n, r.mode == 2 || r.mode == 3);
    out[9] = r.mode < 0 ? 0 : zgemm_tpw(r.mode);
    std::snprintf(name, cap, "%s", r.name);
}

// out: {kernel, log2l, grid, threads, lds, chunk, scratch bytes}
void wr_plus(int L, long long nent, unsigned long long lds_per_block, int num_cu, long long* out, char* name, int cap) {
    const PlusRoute r = plus_route(L, nent, (size_t)lds_per_block, num_cu);
    out[0] = (int)r.kernel; out[1] = r.log2l; out[2] = r.grid; out[3] = r.threads; out[4] = (long long)r.lds; out[5] = r.chunk;
    out[6] = (long long)r.scratch_bytes;
    std::snprintf(name, cap, "%s", r.name);
}

// out: {fused, subset first, subset bins}
void wr_err(int n, int F, int forced, int* out) {
    const ErrRoute r = err_route(n, F, forced != 0);
    out[0] = r.fused; out[1] = r.subset_first; out[2] = r.subset_bins;
}

// off: the 11 offsets in the order of the struct and the total; size: the bytes every array needs
void wr_arena(int n, int F, unsigned long long* off, unsigned long long* size) {
    const Arena a = granger_arena(n, F);
    const unsigned long long nn = (unsigned long long)n * n, tot = nn * F, mt = (n + MT - 1) / MT;
    const size_t o[12] = {a.A, a.U, a.psi, a.T1, a.T2, a.small, a.tw, a.lam, a.inf, a.part, a.bigpart, a.total};
    const unsigned long long s[11] = {tot * 16, tot * 16, tot * 16, tot * 16, tot * 16, 7 * nn * 16, 2ULL * (F - 1) * 16, 2ULL * F * 8,
                                      4ULL * F, NRED * 8ULL, mt * mt * F * 8};
    for (int i = 0; i < 12; ++i) off[i] = o[i];
    for (int i = 0; i < 11; ++i) size[i] = s[i];
}

int wr_const(int which) {
    const int c[7] = {GT, MT, ZB, ZM, ZT, ZW, CHP};
    return c[which];
}

}  // extern "C"
