// Host side of K6: regularisation, Wilson iteration and Granger causality on the device (spyhip_granger of
// include/spyhip.h) and the same iteration in steps for frequency shards (spyhip_wilson_*).  Which kernel serves a step,
// with which grid and LDS, is decided in granger_route.h; the iteration body is written once, as step functions over a
// workspace of device pointers (Wilson), and both entry points run it.  One scalar (the convergence error) is read back
// per iteration, as is one vector of F eigenvalue estimates per condition-number evaluation.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "spy_common.h"
#include "granger_route.h"
#include "granger_kernels.h"
#include "wilson_plus_kernel.h"

using spywil::cd;
using spywil::plus_plan;          // f64_stockham.h

namespace {
const double PI = 3.14159265358979323846264338327950288;

// one launch site per kernel instance goes through here (the opt-in to more than 64 KiB of dynamic LDS is per device and
// cheap: set at every launch)
template <class K, class... Args>
int launch(spyhip_ctx* ctx, K kernel, dim3 grid, unsigned threads, size_t lds, Args... args) {
    if (lds) SPY_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, ctx->stream, args...);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

// grid of the elementwise kernels over `count` elements (grid-stride loops)
unsigned eblocks(size_t count) { return (unsigned)std::min<size_t>((count + 255) / 256, 8192); }
// grid of the kernels with one thread per entry of an n x n matrix
unsigned nnblocks(long long nn) { return (unsigned)((nn + 255) / 256); }

// Badd joins op(B); Ref / part: per-workgroup maxima of |Ref - C| / |Ref| instead of C (matrix-core path only, n >= 48)
int gemm(spyhip_ctx* ctx, const cd* A, const cd* B, cd* C, int n, int batch, long long sA, long long sB, long long sC,
         int opB, int addI, const cd* Badd = nullptr, const cd* Ref = nullptr, double* part = nullptr) {
    const spywil::GemmRoute r = spywil::gemm_route(n, batch, opB, A == B && sA == sB, Badd != nullptr, part != nullptr);
    const dim3 grid(r.grid.x, r.grid.y, r.grid.z);
    auto mfma = [&](auto kernel) {
        return launch(ctx, kernel, grid, r.threads, r.lds, A, B, C, n, sA, sB, sC, opB, addI, Badd, Ref, part, batch);
    };
    switch (r.kernel) {
        case spywil::Gemm::TILED: return launch(ctx, spywil::zgemm_kernel, grid, r.threads, r.lds, A, B, C, n, sA, sB, sC, opB, addI);
        case spywil::Gemm::MFMA3: return mfma(spywil::zgemm_mfma_kernel<3>);
        case spywil::Gemm::MFMA2: return mfma(spywil::zgemm_mfma_kernel<2>);
        case spywil::Gemm::MFMA1: return mfma(spywil::zgemm_mfma_kernel<1>);
        case spywil::Gemm::MFMA0: return mfma(spywil::zgemm_mfma_kernel<0>);
    }
    return -1;
}

int check_info(spyhip_ctx* ctx, int* info_d, int batch, const char* what) {
    std::vector<int> h(batch);
    SPY_HIP_CHECK(hipMemcpyAsync(h.data(), info_d, batch * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SPY_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < batch; ++b)
        if (h[b]) { spy::set_error("%s failed for matrix %d of %d", what, b, batch); return -6; }
    return 0;
}

// blocked / src: see inv_route.  `src`: invert src into M (out of place) instead of M in place
int invert(spyhip_ctx* ctx, cd* M, int n, int batch, int* info_d, bool blocked = false, const cd* src = nullptr) {
    const spywil::InvRoute r = spywil::inv_route(n, blocked, src != nullptr, ctx->lds_per_block);
    if (r.copy_src) SPY_HIP_CHECK(hipMemcpyAsync(M, src, (size_t)batch * n * n * sizeof(cd), hipMemcpyDeviceToDevice, ctx->stream));
    switch (r.kernel) {
        case spywil::Inv::MFMA64: return launch(ctx, spywil::zinv64_mfma_kernel, dim3(batch), r.threads, r.lds, M, src, n, info_d);
        case spywil::Inv::MFMA32: return launch(ctx, spywil::zinv_mfma_kernel, dim3(batch), r.threads, r.lds, M, src, n, info_d);
        case spywil::Inv::BLOCKED16: return launch(ctx, spywil::zinv_blocked_kernel, dim3(batch), r.threads, r.lds, M, n, info_d);
        case spywil::Inv::PIVOTED: return launch(ctx, spywil::zinv_kernel, dim3(batch), r.threads, r.lds, M, n, info_d);
    }
    return -1;
}

// inverse of ONE matrix (psi0): block Gauss-Jordan first (the pivoted kernel is a 256-step serial chain, 17.6 ms at
// n = 256 against < 1 ms), the pivoted kernel only if a diagonal block met a tiny pivot
int invert_one(spyhip_ctx* ctx, cd* dst, const cd* src, int n, int* inf) {
    if (invert(ctx, dst, n, 1, inf, true, src)) return -2;
    int h = 0;
    SPY_HIP_CHECK(hipMemcpyAsync(&h, inf, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SPY_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (h == 0) return 0;
    return invert(ctx, dst, n, 1, inf, false, src);
}

int cholesky(spyhip_ctx* ctx, cd* M, int n, int batch, int* info_d) {
    const spywil::CholRoute r = spywil::chol_route(n, ctx->lds_per_block);
    switch (r.kernel) {
        case spywil::Chol::PANEL: return launch(ctx, spywil::zchol_panel_kernel, dim3(batch), r.threads, r.lds, M, n, info_d);
        case spywil::Chol::COLUMN: return launch(ctx, spywil::zchol_kernel, dim3(batch), r.threads, r.lds, M, n, info_d);
    }
    return -1;
}

// max_f cond_2(A_f) for Hermitian A_f: |lambda|_max(A) * |lambda|_max(A^-1) by power iteration - on the EIGHTH powers:
// three squarings on the matrix cores (13 ms at 2049 x 256 x 256) make the iteration converge eight times faster
// (the ratio of the two largest eigenvalues is raised to the 8th power; ~100 ms per call before), and the 8th root
// divides the estimate's relative error by 8.  `w1`, `w2`: two more work arrays of the size of A.
int max_cond(spyhip_ctx* ctx, const cd* A, cd* work, cd* w1, cd* w2, int n, int F, double* lam_d, int* info_d, double* out) {
    const long long nn = (long long)n * n;
    const int iters = 400;
    std::vector<double> h(2 * (size_t)F);
    std::vector<int> hi(F);
    auto power8 = [&](const cd* X, double* lam) -> int {
        // (X is Hermitian: X^2 = X X^H, the product that computes the lower-triangle tiles only)
        if (gemm(ctx, X, X, w1, n, F, nn, nn, nn, 1, 0)) return -2;        // X^2
        if (gemm(ctx, w1, w1, w2, n, F, nn, nn, nn, 1, 0)) return -2;      // X^4
        if (gemm(ctx, w2, w2, w1, n, F, nn, nn, nn, 1, 0)) return -2;      // X^8
        return launch(ctx, spywil::power_kernel, dim3(F), 256, (size_t)2 * n * sizeof(cd), w1, n, iters, lam);
    };
    if (power8(A, lam_d)) return -2;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (invert(ctx, work, n, F, info_d, attempt == 0, A)) return -2;
        if (power8(work, lam_d + F)) return -2;
        SPY_HIP_CHECK(hipMemcpyAsync(h.data(), lam_d, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        SPY_HIP_CHECK(hipMemcpyAsync(hi.data(), info_d, F * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        SPY_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        bool retry = false;
        for (int f = 0; f < F; ++f) retry = retry || hi[f] == 2;
        if (!retry) break;
    }
    double m = 0.0;
    for (int f = 0; f < F; ++f) {
        double c = hi[f] ? INFINITY : std::pow(h[f], 0.125) * std::pow(h[F + f], 0.125);
        if (!(c == c)) c = INFINITY;
        m = std::max(m, c);
    }
    *out = m;
    return 0;
}

template <int LOG2L>
int launch_plus4(spyhip_ctx* ctx, const spywil::PlusRoute& r, const cd* g, int F, long long nent, const cd* tw, cd* gp, cd* g0) {
    using C = spywil::PCfg<LOG2L>;
    static_assert(spywil::plus4_lds(LOG2L) == C::LDS_BYTES, "granger_route.h restates PCfg::LDS_BYTES");
    return launch(ctx, spywil::plus4_kernel<LOG2L>, dim3((unsigned)r.grid), C::T, r.lds, g, F, nent, tw, gp, g0);
}

// [g]^+ for nent entries over F rfft bins, lag-domain length L = 2 (F - 1) with the radix schedule pl and the
// twiddles tw[m] = exp(-2 pi i m / L)
int plus(spyhip_ctx* ctx, int L, const spywil::PlusPlan& pl, const cd* g, int F, long long nent, const cd* tw, cd* gp, cd* g0) {
    const spywil::PlusRoute r = spywil::plus_route(L, nent, ctx->lds_per_block, ctx->num_cu);
    switch (r.kernel) {
        case spywil::Plus::PLUS4:
            switch (r.log2l) {
                case 8: return launch_plus4<8>(ctx, r, g, F, nent, tw, gp, g0);
                case 9: return launch_plus4<9>(ctx, r, g, F, nent, tw, gp, g0);
                case 10: return launch_plus4<10>(ctx, r, g, F, nent, tw, gp, g0);
                case 11: return launch_plus4<11>(ctx, r, g, F, nent, tw, gp, g0);
                default: return launch_plus4<12>(ctx, r, g, F, nent, tw, gp, g0);
            }
        case spywil::Plus::LDS:
            return launch(ctx, spywil::plus_kernel, dim3((unsigned)r.grid), r.threads, r.lds, g, F, nent, pl, tw, gp, g0);
        case spywil::Plus::LONG:
            if (spy::reserve_scratch(ctx, r.scratch_bytes)) return -2;
            for (long long e0 = 0; e0 < nent; e0 += r.chunk)
                if (launch(ctx, spywil::plus_long_kernel, dim3((unsigned)std::min(r.chunk, nent - e0)), r.threads, 0, g, F, nent, pl, tw,
                           gp, g0, reinterpret_cast<cd*>(ctx->scratch), e0))
                    return -2;
            return 0;
    }
    return -1;
}

// tw[m] = exp(-2 pi i m / L)
std::vector<cd> twiddles(int L) {
    std::vector<cd> h(L);
    for (int m = 0; m < L; ++m) { const double a = -2.0 * PI * m / L; h[m] = make_double2(std::cos(a), std::sin(a)); }
    return h;
}

// ---------------------------------------------------------------------------------------------------------------------
// The Wilson factorisation (wilson_sf.py:16-120) of F bins of n x n matrices as steps over device pointers.
// spyhip_granger carves the arrays out of the context's arena and owns psi / psi0, so an update swaps pointers; the
// stepped entry points fill in what their step touches from the caller's arrays and their work_d, and an update copies.
// ---------------------------------------------------------------------------------------------------------------------
struct Wilson {
    spyhip_ctx* ctx = nullptr;
    int n = 0, F = 0;
    cd *A = nullptr, *U = nullptr;              // the (regularised) CSD and its Cholesky factor, F x n x n
    cd *psi = nullptr, *psi0 = nullptr;         // F x n x n, n x n
    cd *T1 = nullptr, *T2 = nullptr;            // F x n x n work arrays
    cd *S = nullptr, *g0S = nullptr, *psi0n = nullptr;      // n x n: skew part of g0 (or scratch), g0 + S, psi0 next
    double* lam = nullptr;                      // 2 F
    int* inf = nullptr;                         // F
    double *part = nullptr, *bigpart = nullptr; // NRED, ceil(n / 64)^2 F
    bool owns_psi = false;
    long long nn() const { return (long long)n * n; }
    size_t tot() const { return (size_t)F * n * n; }
};

// w.psi <- next (w.T1) / w.psi0 <- w.psi0n
int commit(Wilson& w, cd*& cur, cd*& next, size_t count) {
    if (w.owns_psi) { std::swap(cur, next); return 0; }
    SPY_HIP_CHECK(hipMemcpyAsync(cur, next, count * sizeof(cd), hipMemcpyDeviceToDevice, w.ctx->stream));
    return 0;
}

// A = widen(csd) + eps I (regularize_csd's CSD + eps*eye, wilson_sf.py:244) and the largest 2-norm condition number of
// its bins.  T1, T2 and psi (not in use yet) are the work arrays.
int step_cond(Wilson& w, const float2* csd, double eps, double* cond) {
    if (launch(w.ctx, spywil::widen_kernel, dim3(eblocks(w.tot())), 256, 0, csd, w.A, w.n, (long long)w.tot(), eps)) return -2;
    return max_cond(w.ctx, w.A, w.T1, w.T2, w.psi, w.n, w.F, w.lam, w.inf, cond);
}

// U = Cholesky factor of A per bin (wilson_sf.py:76) and the bins' part of gamma_0 = fft(CSD_full)[0] (:135-140,
// symmetrised real part), the bins being [f_lo, f_lo + F) of Ftot
int step_init(Wilson& w, cd* gamma, int f_lo, int Ftot) {
    SPY_HIP_CHECK(hipMemcpyAsync(w.U, w.A, w.tot() * sizeof(cd), hipMemcpyDeviceToDevice, w.ctx->stream));
    if (cholesky(w.ctx, w.U, w.n, w.F, w.inf)) return -2;
    if (int rc = check_info(w.ctx, w.inf, w.F, "Cholesky factorisation of the CSD (not positive definite)")) return rc;
    return launch(w.ctx, spywil::gamma0_kernel, dim3(nnblocks(w.nn())), 256, 0, w.A, w.F, w.n, gamma, f_lo, Ftot);
}

// psi0 = chol(gamma_0)^T (wilson_sf.py:144-151); gamma_0 is overwritten by its factor
int step_psi0(Wilson& w, cd* gamma0) {
    if (cholesky(w.ctx, gamma0, w.n, 1, w.inf)) return -2;
    if (int rc = check_info(w.ctx, w.inf, 1, "Cholesky factorisation of gamma_0 (not positive definite)")) return rc;
    return launch(w.ctx, spywil::transpose_kernel, dim3(nnblocks(w.nn())), 256, 0, gamma0, w.psi0, w.n);
}

// psi = psi0 at every bin
int step_tile(Wilson& w) { return launch(w.ctx, spywil::tile_kernel, dim3(eblocks(w.tot())), 256, 0, w.psi0, w.psi, w.F, w.n); }

// g = (psi^-1 U)(psi^-1 U)^H + I (wilson_sf.py:80-92) through T1, T2.  `blocked`: the block Gauss-Jordan inverse; its
// flags travel to hinf behind the products (2: a tiny pivot, repeat the whole factorisation with blocked = false) and
// are the host's after the next synchronize.
int step_g(Wilson& w, bool blocked, cd* g, std::vector<int>& hinf) {
    const long long nn = w.nn();
    if (invert(w.ctx, w.T1, w.n, w.F, w.inf, blocked, w.psi)) return -2;                              // T1 = psi^-1
    SPY_HIP_CHECK(hipMemcpyAsync(hinf.data(), w.inf, w.F * sizeof(int), hipMemcpyDeviceToHost, w.ctx->stream));
    if (gemm(w.ctx, w.T1, w.U, w.T2, w.n, w.F, nn, nn, nn, 0, w.n >= 48 ? 2 : 0)) return -2;          // psi^-1 U (U lower triangular)
    return gemm(w.ctx, w.T2, w.T2, g, w.n, w.F, nn, nn, nn, 1, 1);                                    // g + I
}

// psi <- psi (g+ + S), psi0 <- psi0 (g0 + S) with S = triu(g0) - triu(g0)^H (wilson_sf.py:97-101).  Fused: the
// matrix-core product takes S along; else g+ + S is formed in `gp`, in a pass of its own.
int step_update(Wilson& w, const spywil::ErrRoute& er, cd* gp, const cd* g0) {
    const long long nn = w.nn();
    if (er.fused) {
        if (launch(w.ctx, spywil::skew_kernel, dim3(nnblocks(nn)), 256, 0, g0, w.S, w.g0S, w.n)) return -2;
        if (gemm(w.ctx, w.psi, gp, w.T1, w.n, w.F, nn, nn, nn, 0, 0, w.S)) return -2;
    } else {
        if (launch(w.ctx, spywil::add_S_kernel, dim3(eblocks(w.tot())), 256, 0, gp, g0, w.g0S, w.F, w.n)) return -2;
        if (gemm(w.ctx, w.psi, gp, w.T1, w.n, w.F, nn, nn, nn, 0, 0)) return -2;
    }
    if (commit(w, w.psi, w.T1, w.tot())) return -2;
    if (gemm(w.ctx, w.psi0, w.g0S, w.psi0n, w.n, 1, nn, nn, nn, 0, 0)) return -2;
    return commit(w, w.psi0, w.psi0n, (size_t)nn);
}

// fused check over every `stride`-th of `nbins` bins: the per-tile maxima of |A - psi psi^H| / |A| reduced into part[0]
int fused_check(Wilson& w, int nbins, long long stride) {
    const long long s = stride * w.nn();
    if (gemm(w.ctx, w.psi, w.psi, nullptr, w.n, nbins, s, s, s, 1, 0, nullptr, w.A, w.bigpart)) return -2;
    return launch(w.ctx, spywil::maxred_kernel, dim3(1), 256, 0, w.bigpart, spywil::zgemm_tiles(w.n, true) * nbins, w.part);
}

// err = max_rel_err(A, psi psi^H) (wilson_sf.py:99-103,190-194), which decides whether the loop stops.  The maximum over
// a SUBSET of the frequencies is a lower bound of it: while every 8th bin alone is still at or above rtol the iteration
// cannot have converged and the other 7/8 of the product need not be formed (*subset_only: err is that lower bound);
// the full check runs as soon as the subset passes - same decisions, ~1/8 of the 3.1 ms per iteration at 256 channels x
// 2049 frequencies.  Ends with the iteration's synchronize.
int step_error(Wilson& w, const spywil::ErrRoute& er, double rtol, double* err, bool* subset_only) {
    const size_t nred = (size_t)std::min<int64_t>(spywil::NRED, w.ctx->limits.elementwise_blocks);     // (relerr_kernel strides)
    std::vector<double> hp(er.fused ? 1 : nred);
    *subset_only = false;
    if (er.subset_first) {
        if (fused_check(w, er.subset_bins, 8)) return -2;
        SPY_HIP_CHECK(hipMemcpyAsync(hp.data(), w.part, sizeof(double), hipMemcpyDeviceToHost, w.ctx->stream));
        SPY_HIP_CHECK(hipStreamSynchronize(w.ctx->stream));
        *subset_only = hp[0] >= rtol || hp[0] != hp[0];
    }
    if (er.fused) {
        if (!*subset_only && fused_check(w, w.F, 1)) return -2;
    } else {
        if (gemm(w.ctx, w.psi, w.psi, w.T1, w.n, w.F, w.nn(), w.nn(), w.nn(), 1, 0)) return -2;          // psi psi^H
        if (launch(w.ctx, spywil::relerr_kernel, dim3((unsigned)nred), 256, 0, w.A, w.T1, (long long)w.tot(), w.part)) return -2;
    }
    SPY_HIP_CHECK(hipMemcpyAsync(hp.data(), w.part, hp.size() * sizeof(double), hipMemcpyDeviceToHost, w.ctx->stream));
    SPY_HIP_CHECK(hipStreamSynchronize(w.ctx->stream));
    *err = 0.0;
    for (double v : hp) if (v > *err || v != v) *err = v;
    return 0;
}

// Sigma = psi0 psi0^T (psi0 is real), H = psi psi0^-1 (into T1), Granger-Geweke causality (wilson_sf.py:113-120,
// granger.py:53-77).  Sig, inv0: n x n.  H_d / Sigma_d may be NULL.  Ends with a synchronize.
int step_finish(Wilson& w, cd* Sig, cd* inv0, void* granger_d, void* H_d, void* Sigma_d) {
    const long long nn = w.nn();
    if (gemm(w.ctx, w.psi0, w.psi0, Sig, w.n, 1, nn, nn, nn, 1, 0)) return -2;
    if (invert_one(w.ctx, inv0, w.psi0, w.n, w.inf)) return -2;
    if (gemm(w.ctx, w.psi, inv0, w.T1, w.n, w.F, nn, 0, nn, 0, 0)) return -2;
    if (launch(w.ctx, spywil::granger_kernel, dim3(eblocks(w.tot())), 256, 0, w.A, w.T1, Sig, w.F, w.n, reinterpret_cast<float*>(granger_d)))
        return -2;
    if (H_d) SPY_HIP_CHECK(hipMemcpyAsync(H_d, w.T1, w.tot() * sizeof(cd), hipMemcpyDeviceToDevice, w.ctx->stream));
    if (Sigma_d) SPY_HIP_CHECK(hipMemcpyAsync(Sigma_d, Sig, nn * sizeof(cd), hipMemcpyDeviceToDevice, w.ctx->stream));
    SPY_HIP_CHECK(hipStreamSynchronize(w.ctx->stream));
    return 0;
}

// the context's arena (grown on demand, kept between calls: allocating and freeing 11 GB per call cost between 0.05 and
// 1 s at 256 channels x 2049 frequencies) with room for `need` bytes
bool reserve_arena(spyhip_ctx* ctx, size_t need) {
    if (need <= ctx->arena_bytes) return true;
    if (ctx->arena) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(ctx->arena); ctx->arena = nullptr; ctx->arena_bytes = 0; }
    if (hipMalloc(&ctx->arena, need) != hipSuccess) return false;
    ctx->arena_bytes = need;
    return true;
}

struct Tmp {        // small per-call device scratch of the stepped entry points
    void* p = nullptr;
    ~Tmp() { if (p) (void)hipFree(p); }
    int get(size_t bytes) { return hipMalloc(&p, bytes) == hipSuccess ? 0 : -2; }
};

// (a wrapper runs only steps that read what its caller declared const)
cd* as_cd(const void* p) { return reinterpret_cast<cd*>(const_cast<void*>(p)); }

}  // namespace

extern "C" int spyhip_granger(spyhip_ctx* ctx, const void* csd_d, int nfreq, int nchan, double rtol, int niter,
                              double cond_max, double eps_max, void* granger_d, void* H_d, void* Sigma_d,
                              double* info) {
    if (!ctx || !csd_d || !granger_d || !info) { spy::set_error("granger: null argument"); return -1; }
    if (nfreq < 3 || nchan < 1) { spy::set_error("granger: need nfreq >= 3 and nchan >= 1"); return -1; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const int F = nfreq, n = nchan, L = 2 * (F - 1);
    const size_t nn = (size_t)n * n;
    spywil::PlusPlan pl;
    if (!plus_plan(L, &pl)) {
        spy::set_error("granger: no radix schedule for the lag-domain length %d (%d frequencies)", L, F);
        return -3;
    }
    const spywil::Arena ar = spywil::granger_arena(n, F);
    if (!reserve_arena(ctx, ar.total)) {
        spy::set_error("granger: out of device memory (%zu bytes per work array)", (size_t)F * nn * sizeof(cd));
        return -2;
    }
    char* const base = static_cast<char*>(ctx->arena);
    cd* const small = reinterpret_cast<cd*>(base + ar.small);
    cd *g0 = small, *Sig = small + 4 * nn, *scr2 = small + 6 * nn;       // scr2: psi0 of iteration 0
    Wilson w;
    w.ctx = ctx; w.n = n; w.F = F; w.owns_psi = true;
    w.A = reinterpret_cast<cd*>(base + ar.A); w.U = reinterpret_cast<cd*>(base + ar.U);
    w.psi = reinterpret_cast<cd*>(base + ar.psi); w.T1 = reinterpret_cast<cd*>(base + ar.T1);
    w.T2 = reinterpret_cast<cd*>(base + ar.T2);
    w.psi0 = small + nn; w.psi0n = small + 2 * nn; w.g0S = small + 3 * nn; w.S = small + 5 * nn;
    w.lam = reinterpret_cast<double*>(base + ar.lam); w.inf = reinterpret_cast<int*>(base + ar.inf);
    w.part = reinterpret_cast<double*>(base + ar.part); w.bigpart = reinterpret_cast<double*>(base + ar.bigpart);
    cd* const tw = reinterpret_cast<cd*>(base + ar.tw);
    {
        const std::vector<cd> h = twiddles(L);
        SPY_HIP_CHECK(hipMemcpyAsync(tw, h.data(), L * sizeof(cd), hipMemcpyHostToDevice, ctx->stream));
        SPY_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    const float2* csd = reinterpret_cast<const float2*>(csd_d);

    // ---- regularize_csd (wilson_sf.py:197-254)
    double cond0 = 0.0, factor = 0.0;
    if (step_cond(w, csd, 0.0, &cond0)) return -2;
    if (!(cond0 < cond_max)) {
        factor = -1.0;
        const int nsteps = 15;
        for (int s = 0; s < nsteps; ++s) {
            const double e10 = -10.0 + (std::log10(eps_max) + 10.0) * s / (nsteps - 1);
            const double eps = std::pow(10.0, e10);
            double c = 0.0;
            if (step_cond(w, csd, eps, &c)) return -2;
            if (c < cond_max) { factor = eps; break; }
        }
    }

    // ---- Wilson factorisation (wilson_sf.py:16-120)
    if (int rc = step_init(w, w.S, 0, F)) return rc;
    if (int rc = step_psi0(w, w.S)) return rc;
    SPY_HIP_CHECK(hipMemcpyAsync(scr2, w.psi0, nn * sizeof(cd), hipMemcpyDeviceToDevice, ctx->stream));   // keep psi0 of iteration 0
    const spywil::ErrRoute er = spywil::err_route(n, F, std::getenv("SPYHIP_WILSON_FULL_CHECK") != nullptr);
    bool converged = false;
    double err = INFINITY;
    bool subset_only = false;            // the last error came from the frequency subset only (a lower bound)
    std::vector<int> hinf(F);
    for (int attempt = 0; attempt < 2 && !converged; ++attempt) {
        // attempt 0 inverts psi with the block Gauss-Jordan kernel; if one of its diagonal blocks was (nearly)
        // singular anywhere, the whole iteration restarts with the partially pivoted kernel
        bool tiny_pivot = false;
        SPY_HIP_CHECK(hipMemcpyAsync(w.psi0, scr2, nn * sizeof(cd), hipMemcpyDeviceToDevice, ctx->stream));
        if (step_tile(w)) return -2;
        err = INFINITY;
        ctx->granger_iters = 0;
        for (int it = 0; it < niter; ++it) {
            ctx->granger_iters = it + 1;
            if (step_g(w, attempt == 0, w.T1, hinf)) return -2;
            if (int rc = plus(ctx, L, pl, w.T1, F, (long long)nn, tw, w.T2, g0)) return rc;      // T2 = [g+I]^+
            if (step_update(w, er, w.T2, g0)) return -2;
            if (step_error(w, er, rtol, &err, &subset_only)) return -2;
            for (int f = 0; f < F; ++f) tiny_pivot = tiny_pivot || hinf[f] == 2;
            if (tiny_pivot) break;
            if (err < rtol) { converged = true; break; }
        }
        if (!tiny_pivot) break;
    }
    if (!converged && subset_only) {      // the loop ran out of iterations: report the error over ALL frequencies
        if (fused_check(w, F, 1)) return -2;
        SPY_HIP_CHECK(hipMemcpyAsync(&err, w.part, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        SPY_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    // ---- noise covariance, transfer function, Granger causality
    if (step_finish(w, Sig, w.S, granger_d, H_d, Sigma_d)) return -2;
    info[0] = converged ? 1.0 : 0.0;
    info[1] = err;
    info[2] = factor;
    info[3] = cond0;
    return 0;
}

extern "C" int spyhip_granger_last_iterations(const spyhip_ctx* ctx) { return ctx ? ctx->granger_iters : -1; }

// Batched inverse of `batch` n x n complex128 matrices with the kernels of the iteration: the block kernel of the size
// class (inv_route) first, the partially pivoted kernel for the whole batch if any matrix flagged a tiny pivot - what
// step_g's callers do.  The flags, and for dst == src a copy of the input (the repeat starts from it), live in the
// context's arena.  A zero pivot of the pivoted kernel is a singular matrix: -7.
extern "C" int spyhip_zinv(spyhip_ctx* ctx, const void* src_d, void* dst_d, int batch, int n) {
    if (!ctx || !src_d || !dst_d) { spy::set_error("zinv: null argument"); return -1; }
    if (batch < 1 || n < 1) { spy::set_error("zinv: bad shape"); return -1; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)batch * n * n * sizeof(cd), flags = ((size_t)batch * sizeof(int) + 255) & ~(size_t)255;
    const bool in_place = src_d == dst_d;
    if (!reserve_arena(ctx, flags + (in_place ? bytes : 0))) { spy::set_error("zinv: out of device memory (%zu bytes)", flags + bytes); return -2; }
    int* const inf = static_cast<int*>(ctx->arena);
    const cd* src = as_cd(src_d);
    if (in_place) {
        cd* const keep = reinterpret_cast<cd*>(static_cast<char*>(ctx->arena) + flags);
        SPY_HIP_CHECK(hipMemcpyAsync(keep, src_d, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        src = keep;
    }
    std::vector<int> h(batch);
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (invert(ctx, as_cd(dst_d), n, batch, inf, attempt == 0, src)) return -2;
        SPY_HIP_CHECK(hipMemcpyAsync(h.data(), inf, batch * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        SPY_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        bool tiny_pivot = false;
        for (int b = 0; b < batch; ++b) tiny_pivot = tiny_pivot || h[b] == 2;
        if (!tiny_pivot) break;
    }
    for (int b = 0; b < batch; ++b)
        if (h[b]) { spy::set_error("zinv: matrix %d of %d is singular", b, batch); return -7; }
    return 0;
}

// =====================================================================================================================
// The Wilson factorisation in steps, for frequency shards: every rank holds the bins [f_lo, f_lo + nf) of
// the nftot rfft bins of the CSD.  Everything per frequency (regularisation, Cholesky factor, inverse, products, error)
// is local; the plus operator works along the frequency axis, so the host transposes g = psi^-1 S psi^-H between
// "frequency shards x all entries" and "all frequencies x entry shards" around spyhip_wilson_plus (an all-to-all),
// and sums / maximises three small quantities over ranks (gamma_0, the condition number, the error).  The host side
// is syncopy_amd/connectivity/wilson_sharded.py; with one rank the sequence is the one of spyhip_granger: the entry
// points below wrap the same step functions.
// All arrays are complex128 on the device unless stated; work_d: 3 x nf x n x n complex128.
// =====================================================================================================================

// A = widen(csd) + eps I on the local bins (regularize_csd's CSD + eps*eye, wilson_sf.py:244); cond_out (host): the
// largest 2-norm condition number of the local bins.  work_d as above.
extern "C" int spyhip_wilson_cond(spyhip_ctx* ctx, const void* csd_c64_d, int nf, int n, double eps, void* A_d, void* work_d,
                                  double* cond_out) {
    if (!ctx || !csd_c64_d || !A_d || !work_d || !cond_out) { spy::set_error("wilson_cond: null argument"); return -1; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    Wilson w;
    w.ctx = ctx; w.n = n; w.F = nf;
    w.A = as_cd(A_d); w.T1 = as_cd(work_d); w.T2 = w.T1 + w.tot(); w.psi = w.T2 + w.tot();
    Tmp t;
    if (t.get(2 * (size_t)nf * sizeof(double) + nf * sizeof(int))) { spy::set_error("wilson_cond: out of device memory"); return -2; }
    w.lam = reinterpret_cast<double*>(t.p);
    w.inf = reinterpret_cast<int*>(w.lam + 2 * (size_t)nf);
    return step_cond(w, reinterpret_cast<const float2*>(csd_c64_d), eps, cond_out);
}

// U = Cholesky factor of A per local bin (wilson_sf.py:76) and this shard's part of gamma_0 = fft(CSD_full)[0]
// (wilson_sf.py:135-140, symmetrised real part): gamma_part_d (n x n) is to be summed over ranks.
extern "C" int spyhip_wilson_init(spyhip_ctx* ctx, const void* A_d, int nf, int n, int f_lo, int nftot, void* U_d,
                                  void* gamma_part_d) {
    if (!ctx || !A_d || !U_d || !gamma_part_d) { spy::set_error("wilson_init: null argument"); return -1; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    Wilson w;
    w.ctx = ctx; w.n = n; w.F = nf;
    w.A = as_cd(A_d); w.U = as_cd(U_d);
    Tmp t;
    if (t.get((size_t)nf * sizeof(int))) return -2;
    w.inf = reinterpret_cast<int*>(t.p);
    return step_init(w, as_cd(gamma_part_d), f_lo, nftot);
}

// psi0 = chol(gamma_0)^T (wilson_sf.py:144-151) from the summed gamma_0, tiled over the local bins into psi_d
extern "C" int spyhip_wilson_psi0(spyhip_ctx* ctx, void* gamma0_d, int n, int nf, void* psi0_d, void* psi_d) {
    if (!ctx || !gamma0_d || !psi0_d || !psi_d) { spy::set_error("wilson_psi0: null argument"); return -1; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    Wilson w;
    w.ctx = ctx; w.n = n; w.F = nf;
    w.psi0 = as_cd(psi0_d); w.psi = as_cd(psi_d);
    Tmp t;
    if (t.get(sizeof(int))) return -2;
    w.inf = reinterpret_cast<int*>(t.p);
    if (int rc = step_psi0(w, as_cd(gamma0_d))) return rc;
    return step_tile(w);
}

// g = (psi^-1 U)(psi^-1 U)^H + I on the local bins (wilson_sf.py:80-92).  work_d: 2 x nf x n x n.  Returns 1 (not an
// error) if the block inverse met a tiny pivot: repeat the whole factorisation with pivoted = 1.
extern "C" int spyhip_wilson_g(spyhip_ctx* ctx, const void* psi_d, const void* U_d, int nf, int n, int pivoted, void* work_d,
                               void* g_d) {
    if (!ctx || !psi_d || !U_d || !work_d || !g_d) { spy::set_error("wilson_g: null argument"); return -1; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    Wilson w;
    w.ctx = ctx; w.n = n; w.F = nf;
    w.psi = as_cd(psi_d); w.U = as_cd(U_d); w.T1 = as_cd(work_d); w.T2 = w.T1 + w.tot();
    Tmp t;
    if (t.get((size_t)nf * sizeof(int))) return -2;
    w.inf = reinterpret_cast<int*>(t.p);
    std::vector<int> h(nf);
    if (step_g(w, !pivoted, as_cd(g_d), h)) return -2;
    SPY_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int f = 0; f < nf; ++f)
        if (h[f] == 2) return 1;
    return 0;
}

// plus operator (wilson_sf.py:154-184) for nent matrix entries over ALL nftot frequencies: g_d, gp_d (nftot, nent),
// g0_d (nent): the zero-lag coefficients (halved, real).
extern "C" int spyhip_wilson_plus(spyhip_ctx* ctx, const void* g_d, int nftot, int64_t nent, void* gp_d, void* g0_d) {
    if (!ctx || !g_d || !gp_d || !g0_d) { spy::set_error("wilson_plus: null argument"); return -1; }
    if (nent <= 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const int L = 2 * (nftot - 1);
    spywil::PlusPlan pl;
    if (!plus_plan(L, &pl)) {
        spy::set_error("wilson_plus: no radix schedule for the lag-domain length %d", L);
        return -3;
    }
    Tmp t;
    if (t.get((size_t)L * sizeof(cd))) return -2;
    cd* tw = reinterpret_cast<cd*>(t.p);
    const std::vector<cd> h = twiddles(L);
    SPY_HIP_CHECK(hipMemcpyAsync(tw, h.data(), L * sizeof(cd), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = plus(ctx, L, pl, as_cd(g_d), nftot, (long long)nent, tw, as_cd(gp_d), as_cd(g0_d))) return rc;
    SPY_HIP_CHECK(hipStreamSynchronize(ctx->stream));        // h and tw are freed on return
    return 0;
}

// psi <- psi (g+ + S), psi0 <- psi0 (g0 + S) with S = triu(g0) - triu(g0)^H (wilson_sf.py:97-101); err_out (host): this
// shard's max |A - psi psi^H| / |A| (:103, :190-194) over all of its bins.  g0_d (n x n) holds ALL entries (gathered
// by the host).  work_d: nf x n x n.
extern "C" int spyhip_wilson_update(spyhip_ctx* ctx, void* psi_d, const void* gp_d, const void* g0_d, void* psi0_d,
                                    const void* A_d, int nf, int n, void* work_d, double* err_out) {
    if (!ctx || !psi_d || !gp_d || !g0_d || !psi0_d || !A_d || !work_d || !err_out) { spy::set_error("wilson_update: null argument"); return -1; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    Wilson w;
    w.ctx = ctx; w.n = n; w.F = nf;
    w.A = as_cd(A_d); w.psi = as_cd(psi_d); w.psi0 = as_cd(psi0_d); w.T1 = as_cd(work_d);
    const spywil::ErrRoute er = spywil::err_route(n, nf, true);      // a shard reports the maximum over all of its bins
    const size_t nn = (size_t)w.nn(), mt = (size_t)(n + spywil::MT - 1) / spywil::MT;
    Tmp t, t2;
    if (t.get(3 * nn * sizeof(cd) + (mt * mt * nf + spywil::NRED) * sizeof(double))) return -2;
    w.S = reinterpret_cast<cd*>(t.p); w.g0S = w.S + nn; w.psi0n = w.g0S + nn;
    w.bigpart = reinterpret_cast<double*>(w.psi0n + nn);
    w.part = w.bigpart + mt * mt * nf;
    cd* gp = as_cd(gp_d);
    if (!er.fused) {
        // small matrices: g+ + S is formed in place, in a copy (gp_d is left alone)
        if (t2.get(w.tot() * sizeof(cd))) return -2;
        gp = reinterpret_cast<cd*>(t2.p);
        SPY_HIP_CHECK(hipMemcpyAsync(gp, gp_d, w.tot() * sizeof(cd), hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (step_update(w, er, gp, as_cd(g0_d))) return -2;
    bool subset_only = false;
    return step_error(w, er, INFINITY, err_out, &subset_only);       // ends with the synchronize
}

// Sigma = psi0 psi0^T, H = psi psi0^-1, Granger-Geweke causality on the local bins (wilson_sf.py:113-120,
// granger.py:53-77).  granger_d float32 (nf, n, n); H_d (nf, n, n) / Sigma_d (n, n) complex128 may be NULL.
extern "C" int spyhip_wilson_finish(spyhip_ctx* ctx, const void* A_d, const void* psi_d, const void* psi0_d, int nf, int n,
                                    void* work_d, void* granger_d, void* H_d, void* Sigma_d) {
    if (!ctx || !A_d || !psi_d || !psi0_d || !work_d || !granger_d) { spy::set_error("wilson_finish: null argument"); return -1; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    Wilson w;
    w.ctx = ctx; w.n = n; w.F = nf;
    w.A = as_cd(A_d); w.psi = as_cd(psi_d); w.psi0 = as_cd(psi0_d); w.T1 = as_cd(work_d);
    const size_t nn = (size_t)w.nn();
    Tmp t;
    if (t.get(2 * nn * sizeof(cd) + sizeof(int))) return -2;
    cd* Sig = reinterpret_cast<cd*>(t.p);
    w.inf = reinterpret_cast<int*>(Sig + 2 * nn);
    return step_finish(w, Sig, Sig + nn, granger_d, H_d, Sigma_d);
}
