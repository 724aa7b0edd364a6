// CPU emulation driver for the HIP kernels (TEST INFRASTRUCTURE ONLY, see hip_emu.h).
// Compiles the kernel headers of syncopy_amd/csrc unchanged and runs them
// workgroup by workgroup on OS threads.  Built by tests/emu/build_emu.py into
// tests/emu/_build/libspyemu.so; only tests/ load it.
#include "hip_emu.h"
#include <algorithm>
using std::max;
using std::min;

namespace emu {
thread_local dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
thread_local BlockCtx* t_ctx = nullptr;
}  // namespace emu

#include "../../include/spyhip.h"
#include "../../syncopy_amd/csrc/mtmfft_kernel.h"
#include "../../syncopy_amd/csrc/mtmfft_generic.h"
#include "../../syncopy_amd/csrc/mtmfft2_kernel.h"
#include "../../syncopy_amd/csrc/mtmfft_blue_kernel.h"
#include "../../syncopy_amd/csrc/mtmfft_mixed.h"
#include "../../syncopy_amd/csrc/mtmfft_long.h"
#include "../../syncopy_amd/csrc/mtmfft_declong.h"
#include "../../syncopy_amd/csrc/mtmfft_dec64_cfg.h"
#include "../../syncopy_amd/csrc/mtmfft_dec_cfg.h"
#include "../../syncopy_amd/csrc/mtmfft_tables.h"
#include "../../syncopy_amd/csrc/spy_launch.h"

namespace spy {
void set_error(const char*, ...) {}
}  // namespace spy

using spyfft::GenPlan;
using spyfft::MtmArgs;

// ---- The tapered FFT (K1): one emulated spyhip_fft_plan_create + plan options + spyhip_fft_exec.  The route
// (mtmfft_route.h), the tables (mtmfft_tables.h), the grids and the mode dispatch (spy_launch.h) and the schedule names
// (mtmfft_dec_cfg.h, mtmfft_dec64_cfg.h) are the library's own; what follows are the steps of the exec_* functions of
// mtmfft.hip with emu::launch in place of the HIP launch, on host memory.
namespace {

constexpr int EMU_NO_INSTANCE = -100;     // the route chose a kernel the emulator holds no instance of (compile and run time)
constexpr size_t EMU_LDS = 160 * 1024;    // spyhip_ctx::lds_per_block
constexpr long long EMU_NUM_CU = 256;     // spyhip_ctx::num_cu

// what a test may ask for in place of the route's choice (emu_driver.py: FORCE)
enum Force { F_ROUTE, F_GENERIC, F_LONG, F_BLUE, F_MIXED, F_DECLONG, F_DEC, F64_DEC, F64_HALF, F64_PLAIN };

template <class K>
int go(unsigned grid, int threads, size_t lds, K&& body) {
    emu::launch(dim3(grid), dim3(threads), lds, body);
    return 0;
}

// the pass of spyhip_fft_exec ahead of the transform: per-channel means in the reference's summation order
void run_seq_mean(const MtmArgs& a, int nseg, float* means) {
    const int bt = std::min(256, ((a.nchan + 63) / 64) * 64), ncb = (a.nchan + bt - 1) / bt;
    spy::for_seg_launches(a, nseg, [&](const MtmArgs& m, int s0, int ns) {
        emu::launch(dim3(ncb, ns), dim3(bt), 0, [&] { spyfft::seq_mean_kernel(m, means + (size_t)s0 * a.nchan); });
    });
}

// ---- exec_packed: the packed power-of-two engine, plain or as the transform of Bluestein's convolution
template <int LOG2N, int G, bool BLUE, int OUTK, bool MEAN, bool HALF = false>
int run_packed(const MtmArgs& a, unsigned grid) {
    using C = spyfft::Cfg2<LOG2N, G>;
    return go(grid, C::NTHREADS, C::LDS_BYTES, [&] {
        if constexpr (BLUE) spyfft::mtmfft_blue_kernel<LOG2N, G, OUTK, MEAN>(a);
        else spyfft::mtmfft_quad_kernel<LOG2N, G, OUTK, MEAN, HALF>(a);
    });
}

template <int LOG2N, int G, bool BLUE>
int run_packed_mode(const MtmArgs& a, unsigned grid, int outk, bool mean) {
    return spy::dispatch_mode(outk, mean, [&](auto K, auto Mn) {
        return run_packed<LOG2N, G, BLUE, decltype(K)::value, decltype(Mn)::value>(a, grid);
    });
}

template <bool BLUE>
int exec_packed(const spyfft::Route& r, MtmArgs& a, int nseg, int outk, bool mean) {
    unsigned g;
    if (spy::xcd_grid(a, (a.nchan + 3) / 4, r.G, 8, nseg, &g)) return -1;
    switch (r.log2n) {
        case 8: return run_packed_mode<8, 16, BLUE>(a, g, outk, mean);
        case 9: return run_packed_mode<9, 8, BLUE>(a, g, outk, mean);
        case 10: return run_packed_mode<10, 4, BLUE>(a, g, outk, mean);
        case 11: return run_packed_mode<11, 2, BLUE>(a, g, outk, mean);
        case 12:
            if constexpr (!BLUE) if (r.G == 2) return run_packed<12, 2, false, 2, false>(a, g);
            return run_packed_mode<12, 1, BLUE>(a, g, outk, mean);
        case 13: return run_packed_mode<13, 1, BLUE>(a, g, outk, mean);
        default: return EMU_NO_INSTANCE;
    }
}

// ---- exec_dec, exec_half: compile-time schedules.  dec_launch_one of mtmfft_dec_launch.h:
template <class Cf>
int run_dec(MtmArgs a, int outk, bool mean) {
    unsigned grid;
    if (spy::xcd_grid(a, Cf::HALF ? (a.nchan + 1) / 2 : (a.nchan + 3) / 4, Cf::G, Cf::HALF ? 16 : 8, a.nseg, &grid)) return -1;
    return spy::dispatch_mode(outk, mean, [&](auto K, auto Mn) {
        constexpr int OUTK = decltype(K)::value;
        constexpr bool MEAN = decltype(Mn)::value;
        return go(grid, Cf::NTHREADS, Cf::LDS_BYTES, [&] { spyfft::mtmfft_dec_kernel<Cf, OUTK, MEAN>(a); });
    });
}

// id > 0: the schedule of nfft = id in quad form, id < 0: the HALF form of nfft = -id - a sample of the library's list
// (compile time), by the names the instance units use.  The ids below the line are VARIANTS the library does not launch:
// they exist so that a code path of the kernel (split exchanges, V = 8, a HALF decimation) runs on a short length.
int run_dec_id(int id, const MtmArgs& a, int outk, bool mean) {
    using namespace spyfft;
    switch (id) {
        case 100: return run_dec<D_100>(a, outk, mean);
        case 300: return run_dec<D_300>(a, outk, mean);
        case 400: return run_dec<D_400>(a, outk, mean);
        case 600: return run_dec<D_600>(a, outk, mean);
        case 768: return run_dec<D_768>(a, outk, mean);
        case 1000: return run_dec<D_1000>(a, outk, mean);
        case 1500: return run_dec<D_1500>(a, outk, mean);
        case 2000: return run_dec<D_2000>(a, outk, mean);
        case 2001: return run_dec<D_2000_C2>(a, outk, mean);      // (dec_launch_c2: nfft = 2000, complex spectra of every taper)
        case 2400: return run_dec<D_2400>(a, outk, mean);
        case 3000: return run_dec<D_3000>(a, outk, mean);
        case 3072: return run_dec<D_3072>(a, outk, mean);
        case 3200: return run_dec<D_3200>(a, outk, mean);
        case 5000: return run_dec<D_5000>(a, outk, mean);
        case 6000: return run_dec<D_6000>(a, outk, mean);
        case 10000: return run_dec<D_10000>(a, outk, mean);
        case -5000: return run_dec<DH_5000>(a, outk, mean);
        case -12000: return run_dec<DH_12000>(a, outk, mean);
        // ---- variants (test only)
        case 1001: return run_dec<CfgD<10, 10, 10, 1, 2, 1, true>>(a, outk, mean);            // 1000 with split exchanges
        case 512: return run_dec<CfgD<8, 8, 8, 1, 4>>(a, outk, mean);                          // V = 8
        case 4096: return run_dec<CfgD<8, 8, 8, 8, 1>>(a, outk, mean);
        case -2000: return run_dec<CfgD<10, 10, 10, 1, 2, 1, false, true>>(a, outk, mean);     // HALF through the 1000-point schedule
        case -2002: return run_dec<CfgD<10, 10, 10, 1, 2, 1, true, true>>(a, outk, mean);      // ... with split exchanges
        case -1200: return run_dec<CfgD<10, 10, 2, 1, 4, 3, false, true>>(a, outk, mean);      // HALF of 3 x 200
        case -1024: return run_dec<CfgD<16, 16, 2, 1, 2, 1, false, true>>(a, outk, mean);
        default: return EMU_NO_INSTANCE;
    }
}

int exec_half(const spyfft::Route& r, int id, int nfft, const MtmArgs& a, int nseg, int outk, bool mean, const float* tapers_half) {
    if (nfft <= 10240) return run_dec_id(id, a, outk, mean);
    // long trials: the pair-major copy of the segments (one launch holds every segment: host memory)
    const int npairs = (a.nchan + 1) / 2;
    const long long xstride = ((long long)a.nsig + 1) & ~1LL;
    const size_t per_seg = (size_t)npairs * (size_t)xstride;
    std::vector<float2> xpair((size_t)nseg * per_seg);
    MtmArgs m = a;
    spy::for_seg_launches(m, nseg, [&](const MtmArgs& z, int z0, int nz) {
        emu::launch(dim3((unsigned)((xstride + 63) / 64), (a.nchan + 63) / 64, nz), dim3(256), 0,
                    [&] { spyfft::pair_stage_kernel(z, xpair.data() + (size_t)z0 * per_seg, xstride, npairs); });
    });
    m.xpair = xpair.data();
    m.xstride = xstride;
    m.chan_idx = nullptr;
    if (r.family != spyfft::Family::QUAD_HALF) return run_dec_id(id, m, outk, mean);
    m.tapers = tapers_half;                    // quad_half_launch of mtmfft_quad_half.hip
    unsigned grid;
    if (spy::xcd_grid(m, npairs, 1, 16, m.nseg, &grid)) return -1;
    return spy::dispatch_mode(outk, mean, [&](auto K, auto Mn) {
        return run_packed<13, 1, false, decltype(K)::value, decltype(Mn)::value, true>(m, grid);
    });
}

// ---- exec_mixed (mixed_launch: its two instances differ in the launch bound only)
int exec_mixed(const spyfft::Route& r, MtmArgs& a, int nseg, int outk, bool mean) {
    unsigned grid;
    if (spy::xcd_grid(a, (a.nchan + 3) / 4, r.G, 8, nseg, &grid)) return -1;
    return spy::dispatch_mode(outk, mean, [&](auto K, auto Mn) {
        constexpr int OUTK = decltype(K)::value;
        constexpr bool MEAN = decltype(Mn)::value;
        return go(grid, r.mix_threads, r.lds_bytes, [&] { spyfft::mtmfft_mixed_kernel<OUTK, MEAN, 1024>(a, r.mix); });
    });
}

// ---- exec_generic
int exec_generic(const spyfft::Route& r, const MtmArgs& a, const GenPlan& g, int nseg, int outk, bool mean) {
    const long long grid = (long long)nseg * ((a.nchan + 1) / 2);
    if (grid > 0x7fffffffLL) return -1;
    return spy::dispatch_mode(outk, mean, [&](auto K, auto Mn) {
        constexpr int OUTK = decltype(K)::value;
        constexpr bool MEAN = decltype(Mn)::value;
        return go((unsigned)grid, spyfft::GEN_THREADS, r.lds_bytes, [&] { spyfft::mtmfft_generic_kernel<OUTK, MEAN>(a, g); });
    });
}

// ---- exec_long, exec_declong: transforms through (host memory standing in for) HBM, every segment in one chunk.
// long_stats_pass of mtmfft_long_launch.h:
void run_long_stats(const MtmArgs& a, std::vector<double>& stats) {
    const int nz = a.demean_taper ? a.ntaper + 1 : 1;
    stats.assign((size_t)a.nseg * a.nchan * (2 + a.ntaper), 0.0);
    if (!((a.detrend >= 0 && !(a.detrend == 0 && a.means)) || a.demean_taper)) return;
    std::vector<double> part((size_t)a.nseg * (a.ntaper + 1) * spyfft::LONG_SPLITS * a.nchan * 2, 0.0);
    emu::launch(dim3((a.nchan + 63) / 64, a.nseg, nz * spyfft::LONG_SPLITS), dim3(256), 0,
                [&] { spyfft::long_stats_kernel(a, part.data(), nz); });
    emu::launch(dim3((unsigned)(((size_t)a.nseg * a.nchan + 255) / 256)), dim3(256), 0,
                [&] { spyfft::long_stats_final_kernel(a, part.data(), nz, stats.data()); });
}

template <int L>
int run_long_stage(const spyfft::LongArgs& a, int stage, long long items) {
    constexpr int G = 4096 >> L;
    using C = spyfft::Cfg2<L, G>;
    const unsigned grid = (unsigned)(items * ((stage == 1 ? a.M1 : a.M2) / G));
    if (stage == 0) return go(grid, C::NTHREADS, C::LDS_BYTES, [&] { spyfft::long_cols_kernel<L, G>(a); });
    if (stage == 1) return go(grid, C::NTHREADS, C::LDS_BYTES, [&] { spyfft::long_rows_kernel<L, G>(a); });
    return go(grid, C::NTHREADS, C::LDS_BYTES, [&] { spyfft::long_cols_inv_kernel<L, G>(a); });
}

int run_long(const spyfft::LongArgs& a, int l, int stage, long long items) {
    switch (l) {
        case 6: return run_long_stage<6>(a, stage, items);
        case 7: return run_long_stage<7>(a, stage, items);
        case 8: return run_long_stage<8>(a, stage, items);
        default: return EMU_NO_INSTANCE;          // (longer factors run on the GPU only: emulation time)
    }
}

int exec_long(const spyfft::Route& r, const spyfft::FftTables<float2>& t, int nfft, MtmArgs& a, int nseg, int outk, bool mean) {
    if (r.l1 > 8) return EMU_NO_INSTANCE;
    spyfft::LongArgs L{};
    a.nfft = nfft;
    L.m = a;
    L.M1 = 1 << r.l1; L.M2 = 1 << r.l2;
    L.tw1 = t.tw1.data(); L.tw2 = t.tw2.data(); L.twM = t.twM.data(); L.chirp = t.chirp.data(); L.bhat = t.bhat.data();
    L.wsum = t.wsum.data();
    L.direct = r.direct ? 1 : 0;
    L.nquad = (a.nchan + 3) / 4;
    std::vector<double> stats;
    run_long_stats(a, stats);
    L.stats = stats.data();
    std::vector<float4> scratch((size_t)nseg * L.nquad * a.ntaper * r.M);
    L.scratch = scratch.data();
    L.seg0 = 0;
    L.nsegc = nseg;
    const long long items = (long long)L.nsegc * L.nquad * a.ntaper;
    int rc = run_long(L, r.l1, 0, items);
    if (!rc) rc = run_long(L, r.l2, 1, items);
    if (!rc && !L.direct) rc = run_long(L, r.l1, 2, items);
    if (rc) return rc;
    const long long tot = (long long)L.nsegc * L.nquad * (nfft / 2 + 1);
    return spy::dispatch_mode(outk, mean, [&](auto K, auto Mn) {
        constexpr int OUTK = decltype(K)::value;
        constexpr bool MEAN = decltype(Mn)::value;
        return go((unsigned)((tot + 255) / 256), 256, 0, [&] { spyfft::long_post_kernel<OUTK, MEAN>(L); });
    });
}

template <class C>
int run_declong_sub(const spyfft::LongArgs& L, int P, long long nblocks) {
    return go((unsigned)nblocks, C::NTHREADS, C::LDS_BYTES, [&] { spyfft::declong_sub_kernel<C>(L, P); });
}

template <int P>
int run_declong_post(const spyfft::LongArgs& L, int M, int outk, bool mean) {
    const long long tot = (long long)L.nsegc * L.nquad * (M / 2 + 1);
    return spy::dispatch_mode(outk, mean, [&](auto K, auto Mn) {
        constexpr int OUTK = decltype(K)::value;
        constexpr bool MEAN = decltype(Mn)::value;
        return go((unsigned)((tot + 255) / 256), 256, 0, [&] { spyfft::declong_post_kernel<P, OUTK, MEAN>(L, M); });
    });
}

int exec_declong(const spyfft::Route& r, const spyfft::FftTables<float2>& t, int nfft, MtmArgs& a, int nseg, int outk, bool mean) {
    using namespace spyfft;
    const int P = r.P, M = r.M;
    LongArgs L{};
    a.nfft = nfft;
    L.m = a;
    L.M1 = nfft; L.M2 = 1;
    L.tw1 = t.tw1.data(); L.tw2 = t.tw2.data(); L.twM = t.twM.data();
    L.wsum = t.wsum.data();
    L.direct = 0;
    L.nquad = (a.nchan + 3) / 4;
    std::vector<double> stats;
    run_long_stats(a, stats);
    L.stats = stats.data();
    std::vector<float4> scratch((size_t)nseg * L.nquad * a.ntaper * nfft);
    L.scratch = scratch.data();
    L.seg0 = 0;
    L.nsegc = nseg;
    int G, rc;                                     // (declong_group: quads per workgroup of the sub-transform's schedule)
    switch (M) {
        case 2000: G = D_2000::G; break;
        case 4096: G = D_4096::G; break;
        case 5000: G = D_5000::G; break;
        case 10000: G = D_10000::G; break;
        default: return EMU_NO_INSTANCE;
    }
    const long long nblocks = (long long)L.nsegc * P * ((L.nquad + G - 1) / G);
    switch (M) {
        case 2000: rc = run_declong_sub<D_2000>(L, P, nblocks); break;
        case 4096: rc = run_declong_sub<D_4096>(L, P, nblocks); break;
        case 5000: rc = run_declong_sub<D_5000>(L, P, nblocks); break;
        default: rc = run_declong_sub<D_10000>(L, P, nblocks); break;
    }
    if (rc) return rc;
    switch (P) {
        case 2: return run_declong_post<2>(L, M, outk, mean);
        case 3: return run_declong_post<3>(L, M, outk, mean);
        case 4: return run_declong_post<4>(L, M, outk, mean);
        case 6: return run_declong_post<6>(L, M, outk, mean);
        default: return EMU_NO_INSTANCE;
    }
}

// ---- reference precision: exec_dec64 (dec64_launch_one of mtmfft_dec64_launch.h), exec_f64_any
template <class Cf>
int run_dec64(spyfft::F64Args fa, int outk, bool mean) {
    unsigned grid;
    if (spy::xcd_grid(fa.m, Cf::HALF ? fa.m.nchan : (fa.m.nchan + 1) / 2, Cf::G, Cf::HALF ? 32 : 16, fa.m.nseg, &grid)) return -1;
    return spy::dispatch_mode(outk, mean, [&](auto K, auto Mn) {
        constexpr int OUTK = decltype(K)::value;
        constexpr bool MEAN = decltype(Mn)::value;
        return go(grid, Cf::NTHREADS, Cf::LDS_BYTES, [&] { spyfft::mtmfft_dec64_kernel<Cf, OUTK, MEAN>(fa); });
    });
}

// id > 0: the schedule of nfft = id (512 / 2048 / 500 differ from 1024 / 4096 / 1000 in one radix only: left to the GPU
// tests), id < 0: the HALF form of nfft = -id; below the line VARIANTS, as in run_dec_id
int run_dec64_id(int id, const spyfft::F64Args& fa, int outk, bool mean) {
    using namespace spyfft;
    switch (id) {
#define EMU_D64(N) case N: return run_dec64<D64_##N>(fa, outk, mean);
        EMU_D64(100) EMU_D64(200) EMU_D64(256) EMU_D64(300) EMU_D64(400) EMU_D64(600) EMU_D64(768) EMU_D64(1000) EMU_D64(1024)
        EMU_D64(1500) EMU_D64(2000) EMU_D64(2400) EMU_D64(2500) EMU_D64(3000) EMU_D64(3072) EMU_D64(3200) EMU_D64(4000)
        EMU_D64(4096) EMU_D64(5000) EMU_D64(6000) EMU_D64(7500) EMU_D64(8192) EMU_D64(10000) EMU_D64(16384)
#undef EMU_D64
        case -12000: return run_dec64<D64H_12000>(fa, outk, mean);
        // ---- variants (test only)
        case -2000: return run_dec64<CfgD64<10, 10, 10, 1, 2, false, true, true, 1, true>>(fa, outk, mean);
        case -2002: return run_dec64<CfgD64<10, 10, 10, 1, 2, true, true, true, 1, true>>(fa, outk, mean);    // split exchanges
        case -1200: return run_dec64<CfgD64<10, 10, 2, 1, 4, false, true, true, 3, true>>(fa, outk, mean);    // 3 x 200
        case -1024: return run_dec64<CfgD64<16, 16, 2, 1, 2, false, true, false, 1, true>>(fa, outk, mean);   // powers from the table
        default: return EMU_NO_INSTANCE;
    }
}

int exec_f64_any(const spyfft::Route64& r, int nfft, spyfft::F64Args& fa, int nseg, int outk, bool mean) {
    const size_t wlen = r.blue_M ? (size_t)r.blue_M : (size_t)nfft;
    const size_t per = (size_t)2 * wlen * sizeof(double2);
    const long long grid = (long long)nseg * ((fa.m.nchan + 1) / 2);
    fa.plan = r.plan;
    fa.blue_n = r.blue_M ? nfft : 0;
    std::vector<double2> work;
    long long chunk = grid;
    if (per + 1024 > EMU_LDS) {                  // work arrays in global memory, launches of `chunk` workgroups
        chunk = std::min<long long>(grid, std::max<long long>(EMU_NUM_CU, ((size_t)1 << 30) / per));
        work.resize((size_t)chunk * 2 * wlen);
    }
    fa.work = work.empty() ? nullptr : work.data();
    const size_t lds = fa.work ? 0 : (size_t)2 * fa.plan.L * sizeof(double2);
    for (long long w0 = 0; w0 < grid; w0 += chunk) {       // f64_any_launch of mtmfft_f64.hip
        fa.wg0 = w0;
        const int rc = spy::dispatch_mode(outk, mean, [&](auto K, auto Mn) {
            constexpr int OUTK = decltype(K)::value;
            constexpr bool MEAN = decltype(Mn)::value;
            return go((unsigned)std::min(chunk, grid - w0), 256, lds, [&] { spyfft::mtmfft_f64_any_kernel<OUTK, MEAN>(fa); });
        });
        if (rc) return rc;
    }
    return 0;
}

}  // namespace

extern "C" {

// spyfft::seq_mean_kernel as spyhip_fft_exec launches it (plan option spyhip_fft_plan_set_reference_mean)
void emu_seq_mean(const float* data, long long ld, const int* chan_idx, const long long* seg_start,
                  const long long* seg_lo, const long long* seg_hi, int nseg, int nsig, int nchan, float* means) {
    MtmArgs a{};
    a.data = data; a.ld = ld; a.chan_idx = chan_idx;
    a.seg_start = seg_start; a.seg_lo = seg_lo; a.seg_hi = seg_hi;
    a.nseg = nseg; a.nsig = nsig; a.nchan = nchan;
    run_seq_mean(a, nseg, means);
}

// Plan parameters as spyhip_fft_plan_create takes them, then the plan options (precision64: set_precision; ref_mean: 1 / 2 of
// set_reference_mean; blocked: set_blocked), then the exec arguments on host memory.  `force` (Force) runs the filler of
// one family in place of the route's choice; `variant`: the schedule id of a forced DEC / DEC64 family (run_dec_id,
// run_dec64_id); `nostage`: the mixed engine re-reads the segment per taper although it would fit the LDS.
// name: the route's kernel_name.  info: family (+ 100: Family64), G, and for MIXED th, npass, stage, threads, radix[0],
// radix[last].  Returns 0, the plan's error code, or EMU_NO_INSTANCE (-100) where the emulator holds no instance of what
// the route chose - it never runs another family in its place.
int emu_fft_exec(int nsig, int nfft, int nchan, int ntaper, const double* tapers, double scale, int detrend, int demean_taper,
                 const int* freq_idx, int nfsel, int output, int keeptapers, int precision64, int ref_mean, int blocked,
                 int force, int variant, int nostage, const float* data, long long ld, const int* chan_idx,
                 const long long* seg_start, const long long* seg_lo, const long long* seg_hi, int nseg, void* out,
                 char* name, int cap, int* info) {
    using namespace spyfft;
    if (nsig < 1 || nfft < nsig || nchan < 1 || ntaper < 1) return -1;
    const int nf = nfft / 2 + 1, outk = outk_of(output);
    const bool mean = !keeptapers;
    const std::string mode = route_mode(output, keeptapers);
    Route r;
    switch (force) {
        case F_GENERIC: r = fft_route(nsig, nfft, nchan, ntaper, output, keeptapers, EMU_LDS, true); break;
        case F_LONG: route_long(r, nfft, mode); break;
        case F_BLUE: route_blue(r, nfft, mode); break;
        case F_MIXED: if (!route_mixed(r, nfft, nchan, EMU_LDS, mode)) return -3; break;
        case F_DECLONG: if (!route_declong(r, nfft, mode)) return -3; break;
        case F_DEC: route_dec(r, nfft, variant < 0, mode); break;
        default: r = fft_route(nsig, nfft, nchan, ntaper, output, keeptapers, EMU_LDS, false); break;
    }
    if (nostage && r.family == Family::MIXED) r.mix.stage = 0;

    // ---- spyhip_fft_plan_create
    std::vector<float> tf((size_t)ntaper * nsig);
    for (size_t i = 0; i < tf.size(); ++i) tf[i] = (float)tapers[i];
    bool identity_freq = true;
    std::vector<int> fpos;
    if (freq_idx) {
        std::string err;
        fpos = spy::fpos_map(freq_idx, nfsel, nf, &identity_freq, &err);
        if (!err.empty()) return -1;
    }
    if (r.err) return r.err;
    const FftTables<float2> t = fft_tables<float2>(r, nfft, nsig, ntaper, tapers, scale, tf);
    if (blocked && !(r.family == Family::QUAD && output == SPYHIP_OUT_FOURIER && keeptapers && !precision64)) return -3;
    Route64 r64;
    FftTables<double2> t64;
    if (precision64) {          // ---- spyhip_fft_plan_set_precision
        switch (force) {
            case F64_DEC: route64_dec(r64, nfft, false, mode); break;
            case F64_HALF: route64_dec(r64, nfft, true, mode); break;
            default: r64 = fft_route64(nfft, output, keeptapers, r); break;
        }
        if (r64.err) return r64.err;
        if (force == F64_PLAIN && r64.blue_M) {      // VARIANT: the O(R^2) pass of a prime factor above 61
            r64.blue_M = 0;
            if (!spywil::plus_plan(nfft, &r64.plan)) return -3;
            r64.kernel_name = route_detail::fmt("mtmfft_f64_any_kernel<%s> N=%d", mode.c_str(), nfft);
        }
        t64 = fft_tables64<double2>(r64, nfft);
    }
    if (name) std::snprintf(name, cap, "%s", (precision64 ? r64.kernel_name : r.kernel_name).c_str());
    if (info) {
        info[0] = precision64 ? 100 + (int)r64.family : (int)r.family;
        info[1] = r.G;
        if (r.family == Family::MIXED) {
            info[2] = r.mix.th; info[3] = r.mix.npass; info[4] = r.mix.stage; info[5] = r.mix_threads;
            info[6] = r.mix.radix[0]; info[7] = r.mix.radix[r.mix.npass - 1];
        }
    }

    // ---- spyhip_fft_exec
    if (nseg <= 0) return 0;
    MtmArgs a{};
    a.data = data; a.ld = ld; a.chan_idx = chan_idx;
    a.seg_start = seg_start; a.seg_lo = seg_lo; a.seg_hi = seg_hi;
    a.nseg = nseg; a.nsig = nsig; a.nchan = nchan; a.ntaper = ntaper;
    a.tapers = tf.data(); a.tw = t.tw.data(); a.scale = (float)scale;
    a.detrend = detrend; a.demean_taper = demean_taper ? 1 : 0;
    a.fpos = identity_freq ? nullptr : fpos.data();
    a.nfsel = freq_idx ? nfsel : nf; a.out_kind = output; a.out = out;
    a.blocked = blocked ? 1 : 0;
    a.seg_f64 = ref_mean == 2 ? 1 : 0;
    std::vector<float> means;
    if (ref_mean == 1 && detrend == 0) {
        means.resize((size_t)nseg * nchan);
        run_seq_mean(a, nseg, means.data());
        a.means = means.data();
    }
    if (precision64) {
        F64Args fa{};
        fa.m = a;
        fa.tapers64 = tapers;
        fa.tw64 = t64.tw.data();
        fa.scale64 = (double)(float)scale;
        switch (r64.family) {
            case Family64::DEC64: return run_dec64_id(force == F64_DEC && variant ? variant : nfft, fa, outk, mean);
            case Family64::DEC64_HALF:
                fa.tw64 = t64.twh.data();
                fa.tw64_full = t64.tw.data();
                return run_dec64_id(force == F64_HALF && variant ? variant : -nfft, fa, outk, mean);
            case Family64::DECLONG64: return EMU_NO_INSTANCE;
            case Family64::ANY:
                fa.chirp64 = t64.chirp.data();
                fa.bhat64 = t64.bhat.data();
                return exec_f64_any(r64, nfft, fa, nseg, outk, mean);
        }
    }
    switch (r.family) {
        case Family::QUAD:
            a.tapers = t.tapers_half.data();       // this kernel expects the scale / 2 folded into the window
            return exec_packed<false>(r, a, nseg, outk, mean);
        case Family::QUAD_HALF: case Family::DEC_HALF:
            a.twh = t.twh.data();
            return exec_half(r, force == F_DEC ? variant : -nfft, nfft, a, nseg, outk, mean, t.tapers_half.data());
        case Family::DEC:
            if (force == F_DEC) return run_dec_id(variant, a, outk, mean);
            return run_dec_id(nfft == 2000 && outk == 2 && !mean && (nchan + 3) / 4 >= 2 ? 2001 : nfft, a, outk, mean);
        case Family::MIXED: return exec_mixed(r, a, nseg, outk, mean);
        case Family::BLUE:
            a.nfft = nfft; a.chirp = t.chirp.data(); a.bhat = t.bhat.data();
            return exec_packed<true>(r, a, nseg, outk, mean);
        case Family::DECLONG: return exec_declong(r, t, nfft, a, nseg, outk, mean);
        case Family::LONG: return exec_long(r, t, nfft, a, nseg, outk, mean);
        case Family::GENERIC:
            return exec_generic(r, a, gen_plan<GenPlan>(r, nfft, t.chirp.data(), t.bhat.data()), nseg, outk, mean);
    }
    return -1;
}

}  // extern "C"
