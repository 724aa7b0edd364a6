// Host side of K1/K2: plan construction and kernel dispatch for the tapered-FFT
// kernels (spyhip_fft_plan_create / spyhip_fft_exec of include/spyhip.h).
//
// mtmfft_route.h decides which kernel family serves a plan (pure integer logic) and mtmfft_tables.h builds the host tables
// the family needs; this file uploads them and launches the family: one exec_* function per family.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <string>

#include "spy_common.h"
#include "mtmfft_tables.h"    // mtmfft_route.h, host_fft.h
#include "mtmfft_kernel.h"
#include "mtmfft2_kernel.h"
#include "mtmfft_blue_kernel.h"
#include "mtmfft_long_launch.h"
#include "mtmfft_generic.h"
#include "mtmfft_f64_args.h"  // F64Args (the kernels themselves stay out of this translation unit: they pull in the Wilson kernels)

namespace spyfft {
struct Long64Args {           // mtmfft_declong64.h (kept out of this translation unit, as F64Args)
    MtmArgs m;
    const double* tapers64;
    const double2* twM;
    const double2* twN;
    const double2* twP;
    double2* scratch;
    const double* stats;
    const double* wsum;
    int seg0, nsegc;
    int npair;
};

// The instance translation units: each serves the lengths of its own `switch` and answers NO_INSTANCE for the others.
// One list per family; the declarations and the tables launch_unit() walks both expand from it.
#define SPY_DEC_UNITS(X) X(h) X(a) X(b) X(c) X(d) X(e) X(f) X(g) X(i) X(j) X(k) X(l)               /* mtmfft_dec_{a..l}.hip */
#define SPY_DEC_HALF_UNITS(X) X(half_a) X(half_b) X(half_c)                                        /* mtmfft_dec_{m,n,o}.hip */
#define SPY_DEC64_UNITS(X) X(a) X(b) X(c) X(d) X(e) X(f) X(g) X(h) X(i) X(j) X(k) X(l) X(m) X(n)   /* mtmfft_dec64_{a..n}.hip */
#define SPY_DEC64_HALF_UNITS(X) X(half_a) X(half_b)                                                /* mtmfft_dec64_{o,p}.hip */
#define SPY_DECLONG_UNITS(X) X(a) X(b)                              /* mtmfft_declong_{a,b}.hip, mtmfft_declong64_{a,b}.hip */
using DecLaunch = int(hipStream_t stream, const MtmArgs& a, int nfft, int nitems, int outk, bool mean);
using Dec64Launch = int(hipStream_t stream, const F64Args& a, int nfft, int nitems, int outk, bool mean);
using DeclongSub = int(hipStream_t stream, const LongArgs& a, int M, int P, long long nblocks);
using Declong64Sub = int(hipStream_t stream, const Long64Args& a, int M, int P, long long nblocks);
#define X(u) DecLaunch dec_launch_##u;
SPY_DEC_UNITS(X) SPY_DEC_HALF_UNITS(X)
#undef X
#define X(u) Dec64Launch dec64_launch_##u;
SPY_DEC64_UNITS(X) SPY_DEC64_HALF_UNITS(X)
#undef X
#define X(u) DeclongSub declong_launch_sub_##u; Declong64Sub declong64_launch_sub_##u;
SPY_DECLONG_UNITS(X)
#undef X
#define X(u) dec_launch_##u,
DecLaunch* const DEC_UNITS[] = {SPY_DEC_UNITS(X)};
DecLaunch* const DEC_HALF_UNITS[] = {SPY_DEC_HALF_UNITS(X)};
#undef X
#define X(u) dec64_launch_##u,
Dec64Launch* const DEC64_UNITS[] = {SPY_DEC64_UNITS(X)};
Dec64Launch* const DEC64_HALF_UNITS[] = {SPY_DEC64_HALF_UNITS(X)};
#undef X
#define X(u) declong_launch_sub_##u,
DeclongSub* const DECLONG_UNITS[] = {SPY_DECLONG_UNITS(X)};
#undef X
#define X(u) declong64_launch_sub_##u,
Declong64Sub* const DECLONG64_UNITS[] = {SPY_DECLONG_UNITS(X)};
#undef X

int dec_launch_c2(hipStream_t stream, const MtmArgs& a, int nquads);
int quad_half_launch(hipStream_t stream, const MtmArgs& a, int npairs, int outk, bool mean);
int declong_group(int M);
int declong_launch_post(hipStream_t stream, const LongArgs& a, int P, int M, int outk, bool mean);
int declong64_group(int M);
int declong64_launch_post(hipStream_t stream, const Long64Args& a, int P, int M, int outk, bool mean);
int f64_any_launch(hipStream_t stream, F64Args a, long long grid, long long chunk, int outk, bool mean);
int mixed_launch(hipStream_t stream, const MtmArgs& a, const MixPlan& g, int threads, size_t lds, unsigned grid, int outk,
                 bool mean);
}  // namespace spyfft

using spyfft::Family;
using spyfft::Family64;
using spyfft::MtmArgs;

static_assert(spyfft::ROUTE_MAXFAC == spyfft::GEN_MAXFAC, "the route's radix list is the generic kernel's");

struct spyhip_fft_plan {
    spyhip_ctx* ctx = nullptr;
    int nsig = 0, nfft = 0, nchan = 0, ntaper = 0, nfsel = 0, output = 0, keeptapers = 1;
    int detrend = -1, demean_taper = 0;
    float scale = 1.f;
    bool force_generic = false;       // SPYHIP_FORCE_GENERIC was set when the plan was made
    spyfft::Route r;                  // the float32 route
    spyfft::Route64 r64;              // the reference-precision route, in use while precision64
    spyfft::GenPlan gen{};            // GENERIC: the route's radix list with the device tables, as the kernel takes it
    bool precision64 = false;         // float64 taper product + FFT, complex64 rounding where the reference rounds
    spy::DevBuf<float> tapers;
    spy::DevBuf<float> tapers_half;   // tapers * scale / 2 (mtmfft_quad_kernel: no scaling left in its epilogue)
    spy::DevBuf<double> tapers64;     // the windows as the reference holds them
    spy::DevBuf<float2> tw, chirp, bhat;
    spy::DevBuf<float2> twh;          // HALF forms: exp(-2 pi i f / nfft), f <= nfft / 4 (tw then belongs to nfft / 2)
    spy::DevBuf<float2> tw1, tw2, twM;           // DECLONG, LONG
    spy::DevBuf<double> wsum, stats, stats_part;
    spy::DevBuf<float4> scratch;
    spy::DevBuf<int> fpos;
    bool identity_freq = true;
    bool blocked = false;
    unsigned* absmax = nullptr;  // spyhip_fft_plan_set_absmax: where the exec calls leave the range of the spectra
    float wnorm = 0.f;           // max_k || w_k scale ||_2
    spy::DevBuf<double2> tw64;        // exp(-2 pi i m / nfft) (ANY in Bluestein form: / M)
    spy::DevBuf<double2> tw64h;       // DEC64_HALF: exp(-2 pi i m / (nfft / 2)) (tw64 then serves as the half-step table)
    spy::DevBuf<double2> tw64_sub, tw64_P, scratch64;          // DECLONG64
    spy::DevBuf<double2> chirp64, bhat64, f64_work;            // ANY
    std::string kernel_name;
    bool ref_mean = false;      // constant detrending with the reference's float32 row-order means (seq_mean_kernel)
    bool seg_f64 = false;       // the reference holds the segments as float64 arrays (padded sliding windows)
    spy::DevBuf<float> means;
    spy::DevBuf<float2> xpair;  // pair-major copy of the segments of a launch (pair forms of trials beyond 10240 samples)
};

namespace {

int outk_of(const spyhip_fft_plan* p) { return spyfft::outk_of(p->output); }

// the unit of `units` that holds an instance for these arguments
constexpr int NO_INSTANCE = -100;
template <class Fn, size_t K, class... A>
int launch_unit(Fn* const (&units)[K], const char* what, int n, const A&... args) {
    for (Fn* u : units) {
        const int rc = u(args...);
        if (rc != NO_INSTANCE) return rc;
    }
    spy::set_error("fft_exec: no %s %d", what, n);
    return -1;
}

// ---- packed power-of-two engine (mtmfft2_kernel.h), plain or as the transform of Bluestein's convolution
template <int LOG2N, int G, bool BLUE, int OUTK, bool MEAN>
int launch_packed(const spyhip_fft_plan* p, MtmArgs a, unsigned grid) {
    using C = spyfft::Cfg2<LOG2N, G>;
    auto kern = [] {
        if constexpr (BLUE) return spyfft::mtmfft_blue_kernel<LOG2N, G, OUTK, MEAN>;
        else return spyfft::mtmfft_quad_kernel<LOG2N, G, OUTK, MEAN>;
    }();
    // (per device, cheap: set at every launch)
    SPY_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS_BYTES));
    if (!BLUE) {
        a.tapers = p->tapers_half.p;          // this kernel expects the scale / 2 folded into the window
        if (!a.tapers) { spy::set_error("fft_exec: plan without the pre-scaled taper table"); return -1; }
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(C::NTHREADS), C::LDS_BYTES, p->ctx->stream, a);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

template <int LOG2N, int G, bool BLUE>
int launch_packed_mode(const spyhip_fft_plan* p, const MtmArgs& a, unsigned grid) {
    return spy::dispatch_mode(outk_of(p), !p->keeptapers, [&](auto K, auto Mn) {
        return launch_packed<LOG2N, G, BLUE, decltype(K)::value, decltype(Mn)::value>(p, a, grid);
    });
}

template <bool BLUE>
int exec_packed(spyhip_fft_plan* p, MtmArgs& a, int nseg) {
    const int G = p->r.G;
    unsigned g;
    if (spy::xcd_grid(a, (p->nchan + 3) / 4, G, 8, nseg, &g)) return -1;      // work items per segment: channel quads
    switch (p->r.log2n) {
        case 8: return launch_packed_mode<8, 16, BLUE>(p, a, g);
        case 9: return launch_packed_mode<9, 8, BLUE>(p, a, g);
        case 10: return launch_packed_mode<10, 4, BLUE>(p, a, g);
        case 11: return launch_packed_mode<11, 2, BLUE>(p, a, g);
        case 12:
            if constexpr (!BLUE) if (G == 2) return launch_packed<12, 2, false, 2, false>(p, a, g);
            return launch_packed_mode<12, 1, BLUE>(p, a, g);
        case 13: return launch_packed_mode<13, 1, BLUE>(p, a, g);
        default: spy::set_error("no packed kernel for 2^%d", p->r.log2n); return -1;
    }
}

int exec_blue(spyhip_fft_plan* p, MtmArgs& a, int nseg) {
    a.nfft = p->nfft; a.chirp = p->chirp.p; a.bhat = p->bhat.p;
    return exec_packed<true>(p, a, nseg);
}

// ---- long transforms (mtmfft_long.h): one instantiation per factor length
// interleave per factor length: 64 -> 64 ... 1024 -> 4 (256 threads per workgroup, length/16 threads per FFT)
template <int L>
int launch_long_stage(spyhip_ctx* ctx, const spyfft::LongArgs& a, int stage, long long items) {
    constexpr int G = 4096 >> L;
    using C = spyfft::Cfg2<L, G>;
    const long long grid = items * ((stage == 1 ? a.M1 : a.M2) / G);
    if (grid > 0x7fffffffLL) { spy::set_error("fft_exec: grid too large"); return -1; }
    auto kern = stage == 0 ? spyfft::long_cols_kernel<L, G> : stage == 1 ? spyfft::long_rows_kernel<L, G> : spyfft::long_cols_inv_kernel<L, G>;
    SPY_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS_BYTES));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(C::NTHREADS), C::LDS_BYTES, ctx->stream, a);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_long(spyhip_ctx* ctx, const spyfft::LongArgs& a, int l, int stage, long long items) {
    switch (l) {
        case 6: return launch_long_stage<6>(ctx, a, stage, items);
        case 7: return launch_long_stage<7>(ctx, a, stage, items);
        case 8: return launch_long_stage<8>(ctx, a, stage, items);
        case 9: return launch_long_stage<9>(ctx, a, stage, items);
        case 10: return launch_long_stage<10>(ctx, a, stage, items);
        default: spy::set_error("fft_exec: no long-transform stage for 2^%d", l); return -1;
    }
}

// segments per launch of a transform through HBM: `buf` holds ~2 GiB of them (at least one segment)
template <class T>
int hbm_chunk(spyhip_fft_plan* p, spy::DevBuf<T>& buf, size_t per_seg, int nseg, int* chunk) {
    const size_t c = std::max<size_t>(1, std::min<size_t>((size_t)nseg, (((size_t)2 << 30) / sizeof(T)) / std::max<size_t>(per_seg, 1)));
    *chunk = (int)c;
    return buf.reserve(c * per_seg, p->ctx->stream);
}

// N = P M with M a scheduled length: sub-transforms of the decimated samples, then one radix-P pass (mtmfft_declong.h)
int exec_declong(spyhip_fft_plan* p, MtmArgs& a, int nseg) {
    const int P = p->r.P, M = p->r.M;
    spyfft::LongArgs L{};
    a.nfft = p->nfft;
    L.m = a;
    L.M1 = p->nfft; L.M2 = 1;                  // long_post_kernel: natural-order spectrum of length N
    L.tw1 = p->tw1.p; L.tw2 = p->tw2.p; L.twM = p->twM.p;
    L.wsum = p->wsum.p;
    L.direct = 0;
    L.nquad = (p->nchan + 3) / 4;
    if (int rc = spyfft::long_stats_pass(p->ctx->stream, a, p->stats, p->stats_part)) return rc;
    L.stats = p->stats.p;
    int chunk;
    if (hbm_chunk(p, p->scratch, (size_t)L.nquad * p->ntaper * p->nfft, nseg, &chunk)) return -2;      // float4 elements
    L.scratch = p->scratch.p;
    const int G = spyfft::declong_group(M);
    const long long ngrp = (L.nquad + G - 1) / G;
    for (int s0 = 0; s0 < nseg; s0 += chunk) {
        L.seg0 = s0;
        L.nsegc = std::min(chunk, nseg - s0);
        int rc = launch_unit(spyfft::DECLONG_UNITS, "sub-transform of length", M, p->ctx->stream, L, M, P, (long long)L.nsegc * P * ngrp);
        if (!rc) rc = spyfft::declong_launch_post(p->ctx->stream, L, P, M, outk_of(p), !p->keeptapers);
        if (rc) return rc;
    }
    return 0;
}

// Bluestein with four-step transforms of length M = M1 M2 through HBM, or one such transform of a power-of-two nfft
int exec_long(spyhip_fft_plan* p, MtmArgs& a, int nseg) {
    spyfft::LongArgs L{};
    a.nfft = p->nfft;
    L.m = a;
    L.M1 = 1 << p->r.l1; L.M2 = 1 << p->r.l2;
    L.tw1 = p->tw1.p; L.tw2 = p->tw2.p; L.twM = p->twM.p; L.chirp = p->chirp.p; L.bhat = p->bhat.p;
    L.wsum = p->wsum.p;
    L.direct = p->r.direct ? 1 : 0;
    L.nquad = (p->nchan + 3) / 4;
    if (int rc = spyfft::long_stats_pass(p->ctx->stream, a, p->stats, p->stats_part)) return rc;
    L.stats = p->stats.p;
    int chunk;
    if (hbm_chunk(p, p->scratch, (size_t)L.nquad * p->ntaper * p->r.M, nseg, &chunk)) return -2;       // float4 elements
    L.scratch = p->scratch.p;
    for (int s0 = 0; s0 < nseg; s0 += chunk) {
        L.seg0 = s0;
        L.nsegc = std::min(chunk, nseg - s0);
        const long long items = (long long)L.nsegc * L.nquad * p->ntaper;
        int rc = launch_long(p->ctx, L, p->r.l1, 0, items);
        if (!rc) rc = launch_long(p->ctx, L, p->r.l2, 1, items);
        if (!rc && !L.direct) rc = launch_long(p->ctx, L, p->r.l1, 2, items);
        if (!rc) rc = spy::dispatch_mode(outk_of(p), !p->keeptapers, [&](auto K, auto Mn) {
            const long long tot = (long long)L.nsegc * L.nquad * (L.m.nfft / 2 + 1);
            hipLaunchKernelGGL((spyfft::long_post_kernel<decltype(K)::value, decltype(Mn)::value>), dim3((unsigned)((tot + 255) / 256)),
                               dim3(256), 0, p->ctx->stream, L);
            SPY_HIP_CHECK(hipGetLastError());
            return 0;
        });
        if (rc) return rc;
    }
    return 0;
}

// HALF forms: channel pairs, the real transform through the schedule of nfft / 2 (CfgD::HALF, or the 8192-point packed
// engine for 2^14)
int exec_half(spyhip_fft_plan* p, MtmArgs& a, int nseg) {
    const bool mean = !p->keeptapers;
    const int outk = outk_of(p), npairs = (p->nchan + 1) / 2;
    a.twh = p->twh.p;
    // (up to 10240 samples: 5000 and 10000 in HALF form, rows gathered straight from the trial queue.  Both forms walk the
    // one list of HALF units; each unit answers NO_INSTANCE for the lengths of the others)
    if (p->nfft <= 10240)
        return launch_unit(spyfft::DEC_HALF_UNITS, "half-length schedule for nfft =", p->nfft, p->ctx->stream, a, p->nfft, npairs, outk, mean);
    // long trials: a pair workgroup's 8 bytes per row come from a pair-major copy of the segments (pair_stage_kernel)
    // instead of one L2 request per row and lane; launches of at most 4 GiB of it.  256 ch x 7 tapers incl. the
    // copy: 12000 51.2 -> 46.4, 16384 49.8 -> 46.6, 20000 102.1 -> 94.9 us/trial (what is left per segment is
    // what a quad workgroup of the same engine pays as well)
    const long long xstride = ((long long)p->nsig + 1) & ~1LL;
    const size_t per_seg = (size_t)npairs * (size_t)xstride;                     // float2 elements
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)nseg, (((size_t)4 << 30) / sizeof(float2)) / per_seg));
    if (p->xpair.reserve((size_t)chunk * per_seg, p->ctx->stream)) return -2;
    const size_t oelem = (size_t)(mean ? 1 : p->ntaper) * p->nfsel * p->nchan * (outk == 2 ? 8 : 4);
    for (int s0 = 0; s0 < nseg; s0 += chunk) {
        MtmArgs m = a;
        m.seg_start += s0; m.seg_lo += s0; m.seg_hi += s0;
        m.nseg = std::min(chunk, nseg - s0);
        m.out = reinterpret_cast<char*>(a.out) + (size_t)s0 * oelem;
        if (m.means) m.means += (size_t)s0 * p->nchan;
        spy::for_seg_launches(m, m.nseg, [&](const MtmArgs& z, int z0, int nz) {
            hipLaunchKernelGGL(spyfft::pair_stage_kernel, dim3((unsigned)((xstride + 63) / 64), (p->nchan + 63) / 64, nz), dim3(256), 0,
                               p->ctx->stream, z, p->xpair.p + (size_t)z0 * per_seg, xstride, npairs);
        });
        SPY_HIP_CHECK(hipGetLastError());
        m.xpair = p->xpair.p;
        m.xstride = xstride;
        m.chan_idx = nullptr;                    // (the copy is in selected-channel order already)
        int rc;
        if (p->r.family == Family::QUAD_HALF) {
            m.tapers = p->tapers_half.p;
            rc = spyfft::quad_half_launch(p->ctx->stream, m, npairs, outk, mean);
        } else {
            rc = launch_unit(spyfft::DEC_HALF_UNITS, "half-length schedule for nfft =", p->nfft, p->ctx->stream, m, p->nfft, npairs, outk, mean);
        }
        if (rc) return rc;
    }
    return 0;
}

int exec_dec(spyhip_fft_plan* p, MtmArgs& a, int) {
    const int nquads = (p->nchan + 3) / 4, outk = outk_of(p);
    const bool mean = !p->keeptapers;
    if (p->nfft == 2000 && outk == 2 && !mean && nquads >= 2) return spyfft::dec_launch_c2(p->ctx->stream, a, nquads);
    return launch_unit(spyfft::DEC_UNITS, "decimal-length kernel for nfft =", p->nfft, p->ctx->stream, a, p->nfft, nquads, outk, mean);
}

int exec_mixed(spyhip_fft_plan* p, MtmArgs& a, int nseg) {
    unsigned grid;
    if (spy::xcd_grid(a, (p->nchan + 3) / 4, p->r.G, 8, nseg, &grid)) return -1;
    return spyfft::mixed_launch(p->ctx->stream, a, p->r.mix, p->r.mix_threads, p->r.lds_bytes, grid, outk_of(p), !p->keeptapers);
}

int exec_generic(spyhip_fft_plan* p, MtmArgs& a, int nseg) {
    const long long grid = (long long)nseg * ((p->nchan + 1) / 2);
    if (grid > 0x7fffffffLL) { spy::set_error("fft_exec: grid too large (%lld blocks)", grid); return -1; }
    return spy::dispatch_mode(outk_of(p), !p->keeptapers, [&](auto K, auto Mn) {
        auto kern = spyfft::mtmfft_generic_kernel<decltype(K)::value, decltype(Mn)::value>;
        SPY_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->r.lds_bytes));
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(spyfft::GEN_THREADS), p->r.lds_bytes, p->ctx->stream, a, p->gen);
        SPY_HIP_CHECK(hipGetLastError());
        return 0;
    });
}

// ---- reference precision
int exec_dec64(spyhip_fft_plan* p, spyfft::F64Args& fa, int) {
    const int outk = outk_of(p);
    const bool mean = !p->keeptapers;
    if (p->r64.family == Family64::DEC64)
        return launch_unit(spyfft::DEC64_UNITS, "reference-precision schedule for nfft =", p->nfft, p->ctx->stream, fa, p->nfft,
                           (p->nchan + 1) / 2, outk, mean);
    fa.tw64 = p->tw64h.p;              // DEC64_HALF: single channels
    fa.tw64_full = p->tw64.p;
    return launch_unit(spyfft::DEC64_HALF_UNITS, "half-length reference-precision schedule for nfft =", p->nfft, p->ctx->stream, fa,
                       p->nfft, p->nchan, outk, mean);
}

// N = P M through HBM (mtmfft_declong64.h); trend and post-taper mean from the float64 sums of long_stats_kernel.
// (float64 segments of padded sliding windows, seg_f64, are treated as float32 trials here: the nuance is one
// rounding of the trend and such windows are not this long)
int exec_declong64(spyhip_fft_plan* p, spyfft::F64Args& fa, int nseg) {
    const int P = p->r64.P, M = p->r64.M, npairs = (p->nchan + 1) / 2;
    MtmArgs& a = fa.m;
    spyfft::Long64Args L{};
    a.nfft = p->nfft;
    L.m = a;
    L.tapers64 = p->tapers64.p;
    L.twM = p->tw64_sub.p; L.twN = p->tw64.p; L.twP = p->tw64_P.p;
    L.wsum = p->wsum.p;
    L.npair = npairs;
    if (int rc = spyfft::long_stats_pass(p->ctx->stream, a, p->stats, p->stats_part)) return rc;
    L.stats = p->stats.p;
    int chunk;
    if (hbm_chunk(p, p->scratch64, (size_t)npairs * p->ntaper * p->nfft, nseg, &chunk)) return -2;     // double2 elements
    L.scratch = p->scratch64.p;
    const int G = spyfft::declong64_group(M);
    const long long ngrp = (npairs + G - 1) / G;
    for (int s0 = 0; s0 < nseg; s0 += chunk) {
        L.seg0 = s0;
        L.nsegc = std::min(chunk, nseg - s0);
        int rc = launch_unit(spyfft::DECLONG64_UNITS, "float64 sub-transform of length", M, p->ctx->stream, L, M, P, (long long)L.nsegc * P * ngrp);
        if (!rc) rc = spyfft::declong64_launch_post(p->ctx->stream, L, P, M, outk_of(p), !p->keeptapers);
        if (rc) return rc;
    }
    return 0;
}

// two complex128 work arrays (length nfft, or the Bluestein length M) per workgroup: in LDS while they fit
// (leaving room for the static reduction scratch), else in global memory, launches of at most 1 GiB of them
int exec_f64_any(spyhip_fft_plan* p, spyfft::F64Args& fa, int nseg) {
    const int blue_M = p->r64.blue_M;
    const size_t wlen = blue_M ? (size_t)blue_M : (size_t)p->nfft;
    const size_t per = (size_t)2 * wlen * sizeof(double2);
    const long long grid = (long long)nseg * ((p->nchan + 1) / 2);
    fa.plan = p->r64.plan;
    fa.blue_n = blue_M ? p->nfft : 0;
    fa.chirp64 = p->chirp64.p;
    fa.bhat64 = p->bhat64.p;
    if (per + 1024 <= (size_t)p->ctx->lds_per_block) {
        fa.work = nullptr;
        if (grid > 0x7fffffffLL) { spy::set_error("fft_exec: grid too large (%lld blocks)", grid); return -1; }
        return spyfft::f64_any_launch(p->ctx->stream, fa, grid, grid, outk_of(p), !p->keeptapers);
    }
    const long long chunk = std::min<long long>(grid, std::max<long long>(p->ctx->num_cu, ((size_t)1 << 30) / per));
    if (p->f64_work.reserve((size_t)chunk * 2 * wlen, p->ctx->stream)) return -2;
    fa.work = p->f64_work.p;
    return spyfft::f64_any_launch(p->ctx->stream, fa, grid, (long long)(p->f64_work.n / (2 * wlen)), outk_of(p), !p->keeptapers);
}

}  // namespace

extern "C" int spyhip_fft_plan_create(spyhip_ctx* ctx, int nsig, int nfft, int nchan, int ntaper,
                                      const double* tapers, double scale, int detrend, int demean_taper,
                                      const int32_t* freq_idx, int nfsel, int output, int keeptapers,
                                      spyhip_fft_plan** out) {
    if (!ctx || !out || !tapers) { spy::set_error("fft_plan_create: null argument"); return -1; }
    if (nsig < 1 || nfft < nsig || nchan < 1 || ntaper < 1) {
        spy::set_error("fft_plan_create: need 1 <= nsig <= nfft, nchan >= 1, ntaper >= 1 (got %d %d %d %d)",
                       nsig, nfft, nchan, ntaper);
        return -1;
    }
    if (output < SPYHIP_OUT_POW || output > SPYHIP_OUT_ABSIMAG) { spy::set_error("bad output kind %d", output); return -1; }
    if (detrend < -1 || detrend > 1) { spy::set_error("bad detrend %d", detrend); return -1; }
    const int nf = nfft / 2 + 1;
    std::unique_ptr<spyhip_fft_plan> p(new spyhip_fft_plan());
    p->ctx = ctx;
    p->nsig = nsig; p->nfft = nfft; p->nchan = nchan; p->ntaper = ntaper;
    p->output = output; p->keeptapers = keeptapers ? 1 : 0;
    p->detrend = detrend; p->demean_taper = demean_taper ? 1 : 0;
    p->scale = (float)scale;
    p->force_generic = std::getenv("SPYHIP_FORCE_GENERIC") != nullptr;
    p->r = spyfft::fft_route(nsig, nfft, nchan, ntaper, output, p->keeptapers, ctx->lds_per_block, p->force_generic);
    const spyfft::Route& r = p->r;
    hipStream_t s = ctx->stream;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));

    {
        double wmax = 0.0;
        for (int k = 0; k < ntaper; ++k) {
            double q = 0.0;
            for (int n = 0; n < nsig; ++n) q += tapers[(size_t)k * nsig + n] * tapers[(size_t)k * nsig + n];
            wmax = std::max(wmax, q);
        }
        p->wnorm = (float)(std::sqrt(wmax) * std::fabs(scale) * (1.0 + 1e-6));
    }
    std::vector<float> tf((size_t)ntaper * nsig);
    for (size_t i = 0; i < tf.size(); ++i) tf[i] = (float)tapers[i];
    if (p->tapers.upload(tf, s)) return -2;
    {   // the windows as the reference holds them (float64), for spyhip_fft_plan_set_precision
        std::vector<double> td(tapers, tapers + (size_t)ntaper * nsig);
        if (p->tapers64.upload(td, s)) return -2;
    }

    // frequency selection -> inverse map bin -> output slot
    p->identity_freq = (freq_idx == nullptr);
    p->nfsel = freq_idx ? nfsel : nf;
    if (freq_idx) {
        std::string err;
        const std::vector<int> fpos = spy::fpos_map(freq_idx, nfsel, nf, &p->identity_freq, &err);
        if (!err.empty()) { spy::set_error("%s", err.c_str()); return -1; }
        if (!p->identity_freq && p->fpos.upload(fpos, s)) return -2;
    }

    if (r.err) { spy::set_error("%s", r.message.c_str()); return r.err; }
    p->kernel_name = r.kernel_name;
    const spyfft::FftTables<float2> t = spyfft::fft_tables<float2>(r, nfft, nsig, ntaper, tapers, scale, tf);
    auto up = [s](auto& buf, const auto& v) { return !v.empty() && buf.upload(v, s); };      // (a table the family does not read stays unallocated)
    if (up(p->tapers_half, t.tapers_half) || up(p->tw, t.tw) || up(p->twh, t.twh) || up(p->chirp, t.chirp) || up(p->bhat, t.bhat) ||
        up(p->tw1, t.tw1) || up(p->tw2, t.tw2) || up(p->twM, t.twM) || up(p->wsum, t.wsum)) return -2;
    if (r.family == Family::GENERIC) p->gen = spyfft::gen_plan<spyfft::GenPlan>(r, nfft, p->chirp.p, p->bhat.p);
    *out = p.release();
    return 0;
}

extern "C" int spyhip_fft_plan_destroy(spyhip_fft_plan* p) {
    delete p;
    return 0;
}

extern "C" int spyhip_fft_plan_set_blocked(spyhip_fft_plan* p, int on) {
    if (!p) { spy::set_error("fft_plan_set_blocked: null plan"); return -1; }
    if (on && p->precision64) { spy::set_error("fft_plan_set_blocked: not with the reference-precision kernel"); return -3; }
    if (on && !(p->r.family == Family::QUAD && p->output == SPYHIP_OUT_FOURIER && p->keeptapers)) {
        spy::set_error("fft_plan_set_blocked: the channel-blocked layout needs output=FOURIER, keeptapers=1 and a "
                       "power-of-two nfft in 256..8192");
        return -3;
    }
    p->blocked = on != 0;
    return 0;
}

extern "C" int spyhip_fft_plan_set_absmax(spyhip_fft_plan* p, float* absmax_d) {
    if (!p) { spy::set_error("fft_plan_set_absmax: null plan"); return -1; }
    if (!absmax_d) { p->absmax = nullptr; return 0; }
    // the packed power-of-two kernel (mtmfft2_kernel.h) bounds its spectra from the samples it holds; every other family
    // (other lengths, float64 transforms) gets a pass over the segments ahead of the transform (seg_range_kernel)
    const bool ok = !p->blocked && p->output == SPYHIP_OUT_FOURIER && p->keeptapers;
    if (!ok) {                 // a documented answer ("not tracked"), not a failure: the error string stays as it is
        p->absmax = nullptr;
        return -3;
    }
    p->absmax = reinterpret_cast<unsigned*>(absmax_d);
    return 0;
}

extern "C" int spyhip_fft_plan_set_precision(spyhip_fft_plan* p, int reference) {
    if (!p) { spy::set_error("fft_plan_set_precision: null plan"); return -1; }
    if (!reference) {
        p->precision64 = false;
        p->kernel_name = p->r.kernel_name;
        return 0;
    }
    if (p->blocked) {
        spy::set_error("fft_plan_set_precision: the reference-precision kernels write the standard layout");
        return -3;
    }
    SPY_HIP_CHECK(hipSetDevice(p->ctx->device));
    const spyfft::Route64 r = spyfft::fft_route64(p->nfft, p->output, p->keeptapers, p->r);
    if (r.err) { spy::set_error("%s", r.message.c_str()); return r.err; }
    hipStream_t s = p->ctx->stream;
    if (!p->tw64.p) {           // (the route is a function of the plan: its tables are built once; tw64 goes up last)
        const spyfft::FftTables<double2> t = spyfft::fft_tables64<double2>(r, p->nfft);
        auto up = [s](auto& buf, const auto& v) { return !buf.p && !v.empty() && buf.upload(v, s); };
        if (up(p->tw64h, t.twh) || up(p->tw64_sub, t.tw1) || up(p->tw64_P, t.tw2) || up(p->chirp64, t.chirp) || up(p->bhat64, t.bhat) ||
            up(p->tw64, t.tw)) return -2;
    }
    p->r64 = r;
    p->precision64 = true;
    p->kernel_name = r.kernel_name;
    return 0;
}

extern "C" int spyhip_fft_plan_set_reference_mean(spyhip_fft_plan* p, int on) {
    if (!p) { spy::set_error("fft_plan_set_reference_mean: null plan"); return -1; }
    p->ref_mean = on == 1;
    p->seg_f64 = on == 2;
    return 0;
}

extern "C" const char* spyhip_fft_plan_kernel_name(const spyhip_fft_plan* p) {
    return p ? p->kernel_name.c_str() : "";
}

extern "C" int spyhip_fft_exec(spyhip_fft_plan* p, const float* data_d, int64_t ld, const int32_t* chan_idx_d,
                               const int64_t* seg_start_d, const int64_t* seg_lo_d, const int64_t* seg_hi_d,
                               int nseg, void* out_d) {
    if (!p || !data_d || !seg_start_d || !seg_lo_d || !seg_hi_d || !out_d) { spy::set_error("fft_exec: null argument"); return -1; }
    if (nseg <= 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(p->ctx->device));
    MtmArgs a{};
    a.data = data_d; a.ld = ld; a.chan_idx = chan_idx_d;
    a.seg_start = reinterpret_cast<const long long*>(seg_start_d);
    a.seg_lo = reinterpret_cast<const long long*>(seg_lo_d);
    a.seg_hi = reinterpret_cast<const long long*>(seg_hi_d);
    a.nseg = nseg; a.nsig = p->nsig; a.nchan = p->nchan; a.ntaper = p->ntaper;
    a.tapers = p->tapers.p; a.tw = p->tw.p; a.scale = p->scale;
    a.detrend = p->detrend; a.demean_taper = p->demean_taper;
    a.fpos = p->identity_freq ? nullptr : p->fpos.p;
    a.nfsel = p->nfsel; a.out_kind = p->output; a.out = out_d;
    a.blocked = p->blocked ? 1 : 0;
    a.means = nullptr;
    a.seg_f64 = p->seg_f64 ? 1 : 0;
    a.absmax = (p->absmax && !p->blocked) ? p->absmax : nullptr;
    a.wnorm = p->wnorm;
    const int bt = std::min(256, ((p->nchan + 63) / 64) * 64);      // threads per workgroup of the passes below: whole waves, up to four
    const int ncb = (p->nchan + bt - 1) / bt;
    if (a.absmax && !(p->r.family == Family::QUAD && !p->precision64)) {
        // every family but the packed power-of-two kernel (which bounds its spectra from the samples it holds): a pass
        // over the segments ahead of the transform
        spy::for_seg_launches(a, nseg, [&](const MtmArgs& m, int, int ns) {
            hipLaunchKernelGGL(spyfft::seg_range_kernel, dim3(ncb, ns), dim3(bt), 0, p->ctx->stream, m);
        });
        SPY_HIP_CHECK(hipGetLastError());
        a.absmax = nullptr;                      // (the transform kernels of these families do not look at it)
    }
    if (p->ref_mean && p->detrend == 0) {
        // the per-channel means of every segment in the reference's summation order, ahead of the transform
        if (p->means.reserve((size_t)nseg * p->nchan, p->ctx->stream)) return -2;
        spy::for_seg_launches(a, nseg, [&](const MtmArgs& m, int s0, int ns) {
            hipLaunchKernelGGL(spyfft::seq_mean_kernel, dim3(ncb, ns), dim3(bt), 0, p->ctx->stream, m,
                               p->means.p + (size_t)s0 * p->nchan);
        });
        SPY_HIP_CHECK(hipGetLastError());
        a.means = p->means.p;
    }
    if (p->precision64) {
        spyfft::F64Args fa{};
        fa.m = a;
        fa.tapers64 = p->tapers64.p;
        fa.tw64 = p->tw64.p;
        fa.scale64 = (double)p->scale;
        switch (p->r64.family) {
            case Family64::DEC64: case Family64::DEC64_HALF: return exec_dec64(p, fa, nseg);
            case Family64::DECLONG64: return exec_declong64(p, fa, nseg);
            case Family64::ANY: return exec_f64_any(p, fa, nseg);
        }
    }
    switch (p->r.family) {
        case Family::QUAD: return exec_packed<false>(p, a, nseg);
        case Family::QUAD_HALF: case Family::DEC_HALF: return exec_half(p, a, nseg);
        case Family::DEC: return exec_dec(p, a, nseg);
        case Family::MIXED: return exec_mixed(p, a, nseg);
        case Family::BLUE: return exec_blue(p, a, nseg);
        case Family::DECLONG: return exec_declong(p, a, nseg);
        case Family::LONG: return exec_long(p, a, nseg);
        case Family::GENERIC: return exec_generic(p, a, nseg);
    }
    return -1;
}
