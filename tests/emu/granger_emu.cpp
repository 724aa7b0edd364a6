// CPU emulation of the Wilson / Granger stage (K6), TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's own entry
// points, launchers (syncopy_amd/csrc/granger.hip) and kernels, on the runtime stand-in hip/hip_runtime.h.  The entries
// below reach launchers that have no public entry point of their own; they hand pointers on and decide nothing.  Built by
// __graft_entry__.build() and tests/granger_drive.py.
#include "hip_emu.h"
#include "../../syncopy_amd/csrc/granger.hip"
#include "emu_unit.h"

extern "C" {

// C[b] = A[b] op(B[b]) (+ I), Badd joining op(B): gemm
int emu_w_gemm(spyhip_ctx* ctx, const cd* A, const cd* B, cd* C, int n, int batch, long long sA, long long sB, long long sC, int opB,
               int addI, const cd* Badd) {
    return gemm(ctx, A, B, C, n, batch, sA, sB, sC, opB, addI, Badd);
}

// max |ref - psi psi^H| / |ref| over `batch` matrices into part[0]: fused_check (bigpart: the per-tile maxima)
int emu_w_fused_check(spyhip_ctx* ctx, const cd* psi, const cd* ref, int n, int batch, double* bigpart, double* part) {
    Wilson w;
    w.ctx = ctx; w.n = n; w.F = batch;
    w.psi = as_cd(psi); w.A = as_cd(ref); w.bigpart = bigpart; w.part = part;
    return fused_check(w, batch, 1);
}

// M = src^-1 out of place with the kernel of (n, blocked): invert
int emu_w_inv(spyhip_ctx* ctx, cd* M, const cd* src, int n, int batch, int* info, int blocked) {
    return invert(ctx, M, n, batch, info, blocked != 0, src);
}

int emu_w_chol(spyhip_ctx* ctx, cd* M, int n, int batch, int* info) { return cholesky(ctx, M, n, batch, info); }

// S = triu(g0) - triu(g0)^H and g0 + S, as step_update launches it
int emu_w_skew(spyhip_ctx* ctx, const cd* g0, cd* S, cd* g0S, int n) {
    return launch(ctx, spywil::skew_kernel, dim3(nnblocks((long long)n * n)), 256, 0, g0, S, g0S, n);
}

// spywil::plus_kernel at a length the route gives to plus4_kernel, which the tests compare with it: the one launch here
// that no route describes (one workgroup per entry, two length-L arrays in LDS)
int emu_w_plus_generic(spyhip_ctx* ctx, const cd* g, int F, long long nent, cd* gp, cd* g0) {
    const int L = 2 * (F - 1);
    spywil::PlusPlan pl;
    if (!plus_plan(L, &pl)) return -3;
    const std::vector<cd> tw = twiddles(L);
    return launch(ctx, spywil::plus_kernel, dim3((unsigned)nent), 256, (size_t)2 * L * sizeof(cd), g, F, nent, pl, tw.data(), gp, g0);
}

}  // extern "C"
