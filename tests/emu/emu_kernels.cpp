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
#include "../../syncopy_amd/csrc/csd_route.h"
#include "emu_m3_widths.h"
#include "../../syncopy_amd/csrc/csd_kernel.h"
#include "../../syncopy_amd/csrc/csd3m_kernel.h"
#include "../../syncopy_amd/csrc/ppc_kernel.h"
#include "../../syncopy_amd/csrc/ccov_kernel.h"
#include "../../syncopy_amd/csrc/jack_kernel.h"
#include "../../syncopy_amd/csrc/mtmfft2_kernel.h"
#include "../../syncopy_amd/csrc/mtmfft_dec_kernel.h"
#include "../../syncopy_amd/csrc/mtmfft_blue_kernel.h"
#include "../../syncopy_amd/csrc/mtmfft_mixed.h"
#include "../../syncopy_amd/csrc/mtmfft_long.h"
#include "../../syncopy_amd/csrc/mtmfft_declong.h"
#include "../../syncopy_amd/csrc/cwt_launch.h"
#include "cwt_route_text.h"
#include "../../syncopy_amd/csrc/granger_kernels.h"
#include "../../syncopy_amd/csrc/wilson_plus_kernel.h"
#include "../../syncopy_amd/csrc/mtmfft_dec64_cfg.h"

namespace spy {
void set_error(const char*, ...) {}
}  // namespace spy

using spyfft::GenPlan;
using spyfft::MtmArgs;

namespace {

template <int LOG2N, int G, int OUTK, bool MEAN>
void run_quad(const MtmArgs& a, unsigned grid, long only_block) {
    using C = spyfft::Cfg2<LOG2N, G>;
    emu::launch(dim3(grid), dim3(C::NTHREADS), C::LDS_BYTES,
                [&] { spyfft::mtmfft_quad_kernel<LOG2N, G, OUTK, MEAN>(a); }, only_block);
}

template <int LOG2N, int G>
void run_quad_mode(const MtmArgs& a, unsigned grid, int outk, int mean, long only_block) {
    switch (outk * 2 + mean) {
        case 0: run_quad<LOG2N, G, 0, false>(a, grid, only_block); break;
        case 1: run_quad<LOG2N, G, 0, true>(a, grid, only_block); break;
        case 2: run_quad<LOG2N, G, 1, false>(a, grid, only_block); break;
        case 3: run_quad<LOG2N, G, 1, true>(a, grid, only_block); break;
        case 4: run_quad<LOG2N, G, 2, false>(a, grid, only_block); break;
        default: run_quad<LOG2N, G, 2, true>(a, grid, only_block); break;
    }
}

template <int LOG2N, int G>
void run_blue_mode(const MtmArgs& a, unsigned grid, int outk, int mean) {
    using C = spyfft::Cfg2<LOG2N, G>;
    auto go = [&](auto fn) { emu::launch(dim3(grid), dim3(C::NTHREADS), C::LDS_BYTES, fn); };
    switch (outk * 2 + mean) {
        case 0: go([&] { spyfft::mtmfft_blue_kernel<LOG2N, G, 0, false>(a); }); break;
        case 1: go([&] { spyfft::mtmfft_blue_kernel<LOG2N, G, 0, true>(a); }); break;
        case 2: go([&] { spyfft::mtmfft_blue_kernel<LOG2N, G, 1, false>(a); }); break;
        case 3: go([&] { spyfft::mtmfft_blue_kernel<LOG2N, G, 1, true>(a); }); break;
        case 4: go([&] { spyfft::mtmfft_blue_kernel<LOG2N, G, 2, false>(a); }); break;
        default: go([&] { spyfft::mtmfft_blue_kernel<LOG2N, G, 2, true>(a); }); break;
    }
}

template <int L>
void run_long_stage(const spyfft::LongArgs& a, int stage, long long items) {
    constexpr int G = 4096 >> L;
    using C = spyfft::Cfg2<L, G>;
    const unsigned grid = (unsigned)(items * ((stage == 1 ? a.M1 : a.M2) / G));
    if (stage == 0) emu::launch(dim3(grid), dim3(C::NTHREADS), C::LDS_BYTES, [&] { spyfft::long_cols_kernel<L, G>(a); });
    else if (stage == 1) emu::launch(dim3(grid), dim3(C::NTHREADS), C::LDS_BYTES, [&] { spyfft::long_rows_kernel<L, G>(a); });
    else emu::launch(dim3(grid), dim3(C::NTHREADS), C::LDS_BYTES, [&] { spyfft::long_cols_inv_kernel<L, G>(a); });
}
int run_long(const spyfft::LongArgs& a, int l, int stage, long long items) {
    switch (l) {
        case 6: run_long_stage<6>(a, stage, items); return 0;
        case 7: run_long_stage<7>(a, stage, items); return 0;
        case 8: run_long_stage<8>(a, stage, items); return 0;
        default: return -1;          // longer factors are exercised on the GPU only (emulation time)
    }
}

}  // namespace

// mtmfft_dec_kernel (compile-time radix schedules): id = 1000 / 2000 / 5000 (V = 10), 2001 (20 x 10 x 10), 4096 / 512 (V = 8)
template <class Cf>
static void run_dec_mode(const MtmArgs& a0, int nseg, int nchan, int outk, int mean) {
    MtmArgs a = a0;
    const int G = Cf::G;
    const int nitem = Cf::HALF ? (nchan + 1) / 2 : (nchan + 3) / 4;      // channel pairs / quads (as mtmfft_dec_launch.h)
    a.npg = (nitem + G - 1) / G;
    int S = (Cf::HALF ? 16 : 8) / G; if (S < 1) S = 1; if (S > a.npg) S = a.npg;
    a.S = S;
    a.ncl = (a.npg + S - 1) / S;
    const long long nclusters = (long long)nseg * a.ncl;
    const unsigned grid = (unsigned)(((nclusters + 7) / 8) * S * 8);
    auto go = [&](auto fn) { emu::launch(dim3(grid), dim3(Cf::NTHREADS), Cf::LDS_BYTES, fn); };
    switch (outk * 2 + mean) {
        case 0: go([&] { spyfft::mtmfft_dec_kernel<Cf, 0, false>(a); }); break;
        case 1: go([&] { spyfft::mtmfft_dec_kernel<Cf, 0, true>(a); }); break;
        case 2: go([&] { spyfft::mtmfft_dec_kernel<Cf, 1, false>(a); }); break;
        case 3: go([&] { spyfft::mtmfft_dec_kernel<Cf, 1, true>(a); }); break;
        case 4: go([&] { spyfft::mtmfft_dec_kernel<Cf, 2, false>(a); }); break;
        default: go([&] { spyfft::mtmfft_dec_kernel<Cf, 2, true>(a); }); break;
    }
}

static int g_blocked = 0;   // hand-over layout toggle shared by the FFT and CSD entry points
static int g_force_4m = 0;  // SPYHIP_CSD_4M: 256 channels on the 4-multiplication kernel
static long long g_num_cu = 1LL << 40;  // compute units the CSD route plans for; the default is so many that nothing is re-cut
static const float* g_means = nullptr;   // (nseg x nchan) reference-order means for the next FFT call, or none
static const float* g_twh = nullptr;     // exp(-2 pi i f / nfft), f <= nfft / 4: the table of the HALF-form schedules

template <int LOG2N, int G>
static void emu_launch_ccov(const spyfft::CcovArgs& a) {
    using C = spyfft::Cfg2<LOG2N, G>;
    const long long grid = 8 * (((a.npairs + 2 * G - 1) / (2 * G) + 7) / 8);
    emu::launch(dim3((unsigned)grid), dim3(C::NTHREADS), C::LDS_BYTES, [&] { spyfft::ccov_lags_kernel<LOG2N, G>(a); });
}

// plus4_kernel<LOG2L> with the grid, threads and LDS of its route (granger_route.h)
template <int LOG2L>
void run_plus4(const spywil::PlusRoute& r, const double* g, int F, long long nent, const double* tw, double* gp, double* g0) {
    emu::launch(dim3((unsigned)r.grid), dim3(r.threads), r.lds, [&] {
        spywil::plus4_kernel<LOG2L>(reinterpret_cast<const spywil::cd*>(g), F, nent, reinterpret_cast<const spywil::cd*>(tw),
                                    reinterpret_cast<spywil::cd*>(gp), reinterpret_cast<spywil::cd*>(g0)); });
}

// K1L2 (mtmfft_declong.h): N = P M through scratch memory - statistics, scheduled sub-transforms of the decimated samples,
// radix-P step + separation + conversion.  (P, M) = (6, 2000), (3, 4096), (4, 5000), (2, 10000)
template <class C, int P>
static void run_declong(spyfft::LongArgs& L, int outk, bool mean) {
    constexpr int M = C::N, G = C::G;
    const int ngrp = (L.nquad + G - 1) / G;
    emu::launch(dim3((unsigned)((long long)L.nsegc * P * ngrp)), dim3(C::NTHREADS), C::LDS_BYTES,
                [&] { spyfft::declong_sub_kernel<C>(L, P); });
    const unsigned grid = (unsigned)(((long long)L.nsegc * L.nquad * (M / 2 + 1) + 255) / 256);
    switch (outk * 2 + (mean ? 1 : 0)) {
        case 0: emu::launch(dim3(grid), dim3(256), 0, [&] { spyfft::declong_post_kernel<P, 0, false>(L, M); }); break;
        case 1: emu::launch(dim3(grid), dim3(256), 0, [&] { spyfft::declong_post_kernel<P, 0, true>(L, M); }); break;
        case 2: emu::launch(dim3(grid), dim3(256), 0, [&] { spyfft::declong_post_kernel<P, 1, false>(L, M); }); break;
        case 3: emu::launch(dim3(grid), dim3(256), 0, [&] { spyfft::declong_post_kernel<P, 1, true>(L, M); }); break;
        case 4: emu::launch(dim3(grid), dim3(256), 0, [&] { spyfft::declong_post_kernel<P, 2, false>(L, M); }); break;
        default: emu::launch(dim3(grid), dim3(256), 0, [&] { spyfft::declong_post_kernel<P, 2, true>(L, M); }); break;
    }
}

extern "C" {

void emu_set_blocked(int on) { g_blocked = on; }
void emu_set_force_4m(int on) { g_force_4m = on; }
void emu_set_num_cu(long long n) { g_num_cu = n > 0 ? n : 1LL << 40; }
void emu_set_means(const float* m) { g_means = m; }
void emu_set_twh(const float* t) { g_twh = t; }

// spyfft::seq_mean_kernel as spyhip_fft_exec launches it (plan option spyhip_fft_plan_set_reference_mean)
void emu_seq_mean(const float* data, long long ld, const int* chan_idx, const long long* seg_start,
                  const long long* seg_lo, const long long* seg_hi, int nseg, int nsig, int nchan, float* means) {
    MtmArgs a{};
    a.data = data; a.ld = ld; a.chan_idx = chan_idx;
    a.seg_start = seg_start; a.seg_lo = seg_lo; a.seg_hi = seg_hi;
    a.nseg = nseg; a.nsig = nsig; a.nchan = nchan;
    emu::launch(dim3((nchan + 63) / 64, nseg), dim3(64), 0, [&] { spyfft::seq_mean_kernel(a, means); }, -1);
}

// Mirrors the argument marshalling of spyhip_fft_exec for the power-of-two kernels
// (packed quad kernel up to 2^13, pair kernel for 2^14).
// All pointers are host pointers.  Returns 0, or -1 for an unsupported (log2n, G).
int emu_mtmfft_pow2(int log2n, int G, const float* data, long long ld, const int* chan_idx,
                    const long long* seg_start, const long long* seg_lo, const long long* seg_hi, int nseg,
                    int nsig, int nchan, int ntaper, const float* tapers, const float* tw, float scale,
                    int detrend, int demean_taper, const int* fpos, int nfsel, int out_kind, int keeptapers,
                    void* out) {
    MtmArgs a{};
    a.data = data; a.ld = ld; a.chan_idx = chan_idx;
    a.seg_start = seg_start; a.seg_lo = seg_lo; a.seg_hi = seg_hi;
    a.nseg = nseg; a.nsig = nsig; a.nchan = nchan; a.ntaper = ntaper;
    a.tapers = tapers; a.tw = reinterpret_cast<const float2*>(tw); a.scale = scale;
    a.detrend = detrend; a.demean_taper = demean_taper; a.fpos = fpos; a.nfsel = nfsel;
    a.out_kind = out_kind; a.out = out;
    a.means = g_means;
    a.blocked = g_blocked;
    const bool quad = log2n <= 13;
    // mtmfft_quad_kernel expects the window times scale / 2 (the plan uploads that table, mtmfft.hip)
    std::vector<float> th;
    {
        th.resize((size_t)ntaper * nsig);
        for (size_t i = 0; i < th.size(); ++i) th[i] = (float)((double)tapers[i] * (0.5 * (double)scale));
        a.tapers = th.data();
    }
    const int nitem = quad ? (nchan + 3) / 4 : (nchan + 1) / 2;
    a.npg = (nitem + G - 1) / G;
    int S = (quad ? 8 : 16) / G; if (S < 1) S = 1; if (S > a.npg) S = a.npg;
    a.S = S;
    a.ncl = (a.npg + S - 1) / S;
    const long long nclusters = (long long)nseg * a.ncl;
    const unsigned grid = (unsigned)(((nclusters + 7) / 8) * S * 8);
    const int outk = out_kind == SPYHIP_OUT_FOURIER ? 2 : (out_kind == SPYHIP_OUT_POW ? 0 : 1);
    const int mean = keeptapers ? 0 : 1;
    if (log2n == 14) {
        // 2^14: channel pairs through the 8192-point engine (HALF form; `tw` belongs to 8192, the half-step table was set)
        a.twh = reinterpret_cast<const float2*>(g_twh);
        using C = spyfft::Cfg2<13, 1>;
        auto go = [&](auto fn) { emu::launch(dim3(grid), dim3(C::NTHREADS), C::LDS_BYTES, fn); };
        switch (outk * 2 + mean) {
            case 0: go([&] { spyfft::mtmfft_quad_kernel<13, 1, 0, false, true>(a); }); break;
            case 1: go([&] { spyfft::mtmfft_quad_kernel<13, 1, 0, true, true>(a); }); break;
            case 2: go([&] { spyfft::mtmfft_quad_kernel<13, 1, 1, false, true>(a); }); break;
            case 3: go([&] { spyfft::mtmfft_quad_kernel<13, 1, 1, true, true>(a); }); break;
            case 4: go([&] { spyfft::mtmfft_quad_kernel<13, 1, 2, false, true>(a); }); break;
            default: go([&] { spyfft::mtmfft_quad_kernel<13, 1, 2, true, true>(a); }); break;
        }
        return 0;
    }
    switch (log2n * 100 + G) {
        case 816: run_quad_mode<8, 16>(a, grid, outk, mean, -1); break;
        case 908: run_quad_mode<9, 8>(a, grid, outk, mean, -1); break;
        case 1004: run_quad_mode<10, 4>(a, grid, outk, mean, -1); break;
        case 1102: run_quad_mode<11, 2>(a, grid, outk, mean, -1); break;
        case 1201: run_quad_mode<12, 1>(a, grid, outk, mean, -1); break;
        case 1202: if (outk != 2 || mean) return -1; run_quad<12, 2, 2, false>(a, grid, -1); break;
        case 1301: run_quad_mode<13, 1>(a, grid, outk, mean, -1); break;
        default: return -1;
    }
    return 0;
}

int emu_mtmfft_dec(int id, const float* data, long long ld, const int* chan_idx,
                   const long long* seg_start, const long long* seg_lo, const long long* seg_hi, int nseg,
                   int nsig, int nchan, int ntaper, const float* tapers, const float* tw, float scale,
                   int detrend, int demean_taper, const int* fpos, int nfsel, int out_kind, int keeptapers,
                   void* out) {
    MtmArgs a{};
    a.data = data; a.ld = ld; a.chan_idx = chan_idx;
    a.seg_start = seg_start; a.seg_lo = seg_lo; a.seg_hi = seg_hi;
    a.nseg = nseg; a.nsig = nsig; a.nchan = nchan; a.ntaper = ntaper;
    a.tapers = tapers; a.tw = reinterpret_cast<const float2*>(tw); a.scale = scale;
    a.detrend = detrend; a.demean_taper = demean_taper; a.fpos = fpos; a.nfsel = nfsel;
    a.out_kind = out_kind; a.out = out;
    a.means = g_means;
    a.twh = reinterpret_cast<const float2*>(g_twh);
    const int outk = out_kind == SPYHIP_OUT_FOURIER ? 2 : (out_kind == SPYHIP_OUT_POW ? 0 : 1);
    const int mean = keeptapers ? 0 : 1;
    switch (id) {
        // HALF form (id = -nfft): channel pairs, the real transform of nfft samples through the schedule of nfft / 2
        case -2000: run_dec_mode<spyfft::CfgD<10, 10, 10, 1, 2, 1, false, true>>(a, nseg, nchan, outk, mean); break;
        case -2002: run_dec_mode<spyfft::CfgD<10, 10, 10, 1, 2, 1, true, true>>(a, nseg, nchan, outk, mean); break;     // split exchanges
        case -1200: run_dec_mode<spyfft::CfgD<10, 10, 2, 1, 4, 3, false, true>>(a, nseg, nchan, outk, mean); break;     // 3 x 200
        case -5000: run_dec_mode<spyfft::CfgD<10, 10, 5, 5, 1, 1, false, true>>(a, nseg, nchan, outk, mean); break;
        case -12000: run_dec_mode<spyfft::CfgD<10, 10, 10, 2, 1, 3, false, true>>(a, nseg, nchan, outk, mean); break;
        case -1024: run_dec_mode<spyfft::CfgD<16, 16, 2, 1, 2, 1, false, true>>(a, nseg, nchan, outk, mean); break;
        case 1000: run_dec_mode<spyfft::CfgD<10, 10, 10, 1, 2>>(a, nseg, nchan, outk, mean); break;
        case 2000: run_dec_mode<spyfft::CfgD<10, 10, 10, 2, 1>>(a, nseg, nchan, outk, mean); break;
        case 2001: run_dec_mode<spyfft::CfgD<20, 10, 10, 1, 2>>(a, nseg, nchan, outk, mean); break;
        case 5000: run_dec_mode<spyfft::CfgD<10, 10, 10, 5, 1>>(a, nseg, nchan, outk, mean); break;
        case 600: run_dec_mode<spyfft::CfgD<10, 10, 2, 1, 4, 3>>(a, nseg, nchan, outk, mean); break;
        case 100: run_dec_mode<spyfft::CfgD<10, 10, 1, 1, 16>>(a, nseg, nchan, outk, mean); break;
        case 400: run_dec_mode<spyfft::CfgD<10, 10, 2, 2, 8>>(a, nseg, nchan, outk, mean); break;
        case 2400: run_dec_mode<spyfft::CfgD<20, 20, 2, 1, 1, 3>>(a, nseg, nchan, outk, mean); break;
        case 3200: run_dec_mode<spyfft::CfgD<20, 20, 4, 2, 1>>(a, nseg, nchan, outk, mean); break;
        case 300: run_dec_mode<spyfft::CfgD<10, 10, 1, 1, 8, 3>>(a, nseg, nchan, outk, mean); break;
        case 768: run_dec_mode<spyfft::CfgD<16, 16, 1, 1, 4, 3>>(a, nseg, nchan, outk, mean); break;
        case 3072: run_dec_mode<spyfft::CfgD<16, 16, 4, 1, 1, 3>>(a, nseg, nchan, outk, mean); break;
        case 10000: run_dec_mode<spyfft::CfgD<20, 20, 5, 5, 1, 1, true>>(a, nseg, nchan, outk, mean); break;
        case 1001: run_dec_mode<spyfft::CfgD<10, 10, 10, 1, 2, 1, true>>(a, nseg, nchan, outk, mean); break;
        case 1500: run_dec_mode<spyfft::CfgD<10, 10, 5, 1, 2, 3>>(a, nseg, nchan, outk, mean); break;
        case 3000: run_dec_mode<spyfft::CfgD<10, 10, 10, 1, 1, 3>>(a, nseg, nchan, outk, mean); break;
        case 6000: run_dec_mode<spyfft::CfgD<10, 10, 10, 2, 1, 3>>(a, nseg, nchan, outk, mean); break;
        case 512: run_dec_mode<spyfft::CfgD<8, 8, 8, 1, 4>>(a, nseg, nchan, outk, mean); break;
        case 4096: run_dec_mode<spyfft::CfgD<8, 8, 8, 8, 1>>(a, nseg, nchan, outk, mean); break;
        default: return -1;
    }
    return 0;
}

// Mirrors spyhip_fft_exec for the Bluestein kernel (tables built by the Python mirror of mtmfft.hip).
int emu_mtmfft_blue(int log2m, int G, int nfft, const float* chirp, const float* bhat, const float* data, long long ld,
                    const int* chan_idx, const long long* seg_start, const long long* seg_lo, const long long* seg_hi,
                    int nseg, int nsig, int nchan, int ntaper, const float* tapers, const float* tw, float scale,
                    int detrend, int demean_taper, const int* fpos, int nfsel, int out_kind, int keeptapers, void* out) {
    MtmArgs a{};
    a.data = data; a.ld = ld; a.chan_idx = chan_idx;
    a.seg_start = seg_start; a.seg_lo = seg_lo; a.seg_hi = seg_hi;
    a.nseg = nseg; a.nsig = nsig; a.nchan = nchan; a.ntaper = ntaper;
    a.tapers = tapers; a.tw = reinterpret_cast<const float2*>(tw); a.scale = scale;
    a.detrend = detrend; a.demean_taper = demean_taper; a.fpos = fpos; a.nfsel = nfsel;
    a.out_kind = out_kind; a.out = out;
    a.means = g_means;
    a.nfft = nfft; a.chirp = reinterpret_cast<const float2*>(chirp); a.bhat = reinterpret_cast<const float2*>(bhat);
    const int nitem = (nchan + 3) / 4;
    a.npg = (nitem + G - 1) / G;
    int S = 8 / G; if (S < 1) S = 1; if (S > a.npg) S = a.npg;
    a.S = S;
    a.ncl = (a.npg + S - 1) / S;
    const long long nclusters = (long long)nseg * a.ncl;
    const unsigned grid = (unsigned)(((nclusters + 7) / 8) * S * 8);
    const int outk = out_kind == SPYHIP_OUT_FOURIER ? 2 : (out_kind == SPYHIP_OUT_POW ? 0 : 1);
    const int mean = keeptapers ? 0 : 1;
    switch (log2m * 100 + G) {
        case 816: run_blue_mode<8, 16>(a, grid, outk, mean); break;
        case 908: run_blue_mode<9, 8>(a, grid, outk, mean); break;
        case 1004: run_blue_mode<10, 4>(a, grid, outk, mean); break;
        case 1102: run_blue_mode<11, 2>(a, grid, outk, mean); break;
        case 1201: run_blue_mode<12, 1>(a, grid, outk, mean); break;
        case 1301: run_blue_mode<13, 1>(a, grid, outk, mean); break;
        default: return -1;
    }
    return 0;
}

// Mirrors the long-transform branch of spyhip_fft_exec (one chunk holding every segment).
int emu_mtmfft_long(int l1, int l2, int nfft, const float* chirp, const float* bhat, const float* tw1, const float* tw2,
                    const float* twM, const double* wsum, const float* data, long long ld, const int* chan_idx,
                    const long long* seg_start, const long long* seg_lo, const long long* seg_hi, int nseg, int nsig,
                    int nchan, int ntaper, const float* tapers, float scale, int detrend, int demean_taper,
                    const int* fpos, int nfsel, int out_kind, int keeptapers, void* out) {
    MtmArgs a{};
    a.data = data; a.ld = ld; a.chan_idx = chan_idx;
    a.seg_start = seg_start; a.seg_lo = seg_lo; a.seg_hi = seg_hi;
    a.nseg = nseg; a.nsig = nsig; a.nchan = nchan; a.ntaper = ntaper;
    a.tapers = tapers; a.scale = scale; a.detrend = detrend; a.demean_taper = demean_taper;
    a.fpos = fpos; a.nfsel = nfsel; a.out_kind = out_kind; a.out = out; a.nfft = nfft;
    a.means = g_means;
    spyfft::LongArgs L{};
    L.m = a;
    L.M1 = 1 << l1; L.M2 = 1 << l2;
    L.tw1 = reinterpret_cast<const float2*>(tw1); L.tw2 = reinterpret_cast<const float2*>(tw2);
    L.twM = reinterpret_cast<const float2*>(twM); L.chirp = reinterpret_cast<const float2*>(chirp);
    L.bhat = reinterpret_cast<const float2*>(bhat); L.wsum = wsum;
    L.nquad = (nchan + 3) / 4;
    std::vector<double> stats((size_t)nseg * nchan * (2 + ntaper), 0.0);
    L.stats = stats.data();
    if (detrend >= 0 || demean_taper) {
        const int nz = demean_taper ? ntaper + 1 : 1;
        std::vector<double> part((size_t)nseg * nz * spyfft::LONG_SPLITS * nchan * 2, 0.0);
        emu::launch(dim3((nchan + 63) / 64, nseg, nz * spyfft::LONG_SPLITS), dim3(256), 0,
                    [&] { spyfft::long_stats_kernel(a, part.data(), nz); });
        emu::launch(dim3((unsigned)(((size_t)nseg * nchan + 255) / 256)), dim3(256), 0,
                    [&] { spyfft::long_stats_final_kernel(a, part.data(), nz, stats.data()); });
    }
    const size_t M = (size_t)L.M1 * L.M2;
    const long long items = (long long)nseg * L.nquad * ntaper;
    std::vector<float4> scratch((size_t)items * M);
    L.scratch = scratch.data();
    L.seg0 = 0; L.nsegc = nseg;
    if (run_long(L, l1, 0, items) || run_long(L, l2, 1, items) || run_long(L, l1, 2, items)) return -1;
    const int outk = out_kind == SPYHIP_OUT_FOURIER ? 2 : (out_kind == SPYHIP_OUT_POW ? 0 : 1);
    const bool mean = !keeptapers;
    const unsigned grid = (unsigned)(((long long)nseg * L.nquad * (nfft / 2 + 1) + 255) / 256);
    switch (outk * 2 + (mean ? 1 : 0)) {
        case 0: emu::launch(dim3(grid), dim3(256), 0, [&] { spyfft::long_post_kernel<0, false>(L); }); break;
        case 1: emu::launch(dim3(grid), dim3(256), 0, [&] { spyfft::long_post_kernel<0, true>(L); }); break;
        case 2: emu::launch(dim3(grid), dim3(256), 0, [&] { spyfft::long_post_kernel<1, false>(L); }); break;
        case 3: emu::launch(dim3(grid), dim3(256), 0, [&] { spyfft::long_post_kernel<1, true>(L); }); break;
        case 4: emu::launch(dim3(grid), dim3(256), 0, [&] { spyfft::long_post_kernel<2, false>(L); }); break;
        default: emu::launch(dim3(grid), dim3(256), 0, [&] { spyfft::long_post_kernel<2, true>(L); }); break;
    }
    return 0;
}

int emu_mtmfft_declong(int P, int M, const float* twsub, const float* twN, const float* twP, const double* wsum,
                       const float* data, long long ld, const int* chan_idx, const long long* seg_start,
                       const long long* seg_lo, const long long* seg_hi, int nseg, int nsig, int nchan, int ntaper,
                       const float* tapers, float scale, int detrend, int demean_taper, const int* fpos, int nfsel,
                       int out_kind, int keeptapers, void* out) {
    MtmArgs a{};
    a.data = data; a.ld = ld; a.chan_idx = chan_idx;
    a.seg_start = seg_start; a.seg_lo = seg_lo; a.seg_hi = seg_hi;
    a.nseg = nseg; a.nsig = nsig; a.nchan = nchan; a.ntaper = ntaper;
    a.tapers = tapers; a.scale = scale; a.detrend = detrend; a.demean_taper = demean_taper;
    a.fpos = fpos; a.nfsel = nfsel; a.out_kind = out_kind; a.out = out; a.nfft = P * M;
    a.means = g_means;
    spyfft::LongArgs L{};
    L.m = a;
    L.M1 = P * M; L.M2 = 1;
    L.tw1 = reinterpret_cast<const float2*>(twsub); L.tw2 = reinterpret_cast<const float2*>(twP);
    L.twM = reinterpret_cast<const float2*>(twN); L.wsum = wsum;
    L.nquad = (nchan + 3) / 4;
    std::vector<double> stats((size_t)nseg * nchan * (2 + ntaper), 0.0);
    L.stats = stats.data();
    if ((detrend >= 0 && !(detrend == 0 && a.means)) || demean_taper) {
        const int nz = demean_taper ? ntaper + 1 : 1;
        std::vector<double> part((size_t)nseg * nz * spyfft::LONG_SPLITS * nchan * 2, 0.0);
        emu::launch(dim3((nchan + 63) / 64, nseg, nz * spyfft::LONG_SPLITS), dim3(256), 0,
                    [&] { spyfft::long_stats_kernel(a, part.data(), nz); });
        emu::launch(dim3((unsigned)(((size_t)nseg * nchan + 255) / 256)), dim3(256), 0,
                    [&] { spyfft::long_stats_final_kernel(a, part.data(), nz, stats.data()); });
    }
    std::vector<float4> scratch((size_t)nseg * L.nquad * ntaper * (size_t)P * M);
    L.scratch = scratch.data();
    L.seg0 = 0; L.nsegc = nseg;
    const int outk = out_kind == SPYHIP_OUT_FOURIER ? 2 : (out_kind == SPYHIP_OUT_POW ? 0 : 1);
    const bool mean = !keeptapers;
    if (P == 6 && M == 2000) run_declong<spyfft::CfgD<10, 10, 10, 2, 1>, 6>(L, outk, mean);
    else if (P == 3 && M == 4096) run_declong<spyfft::CfgD<16, 16, 16, 1, 1>, 3>(L, outk, mean);
    else if (P == 4 && M == 5000) run_declong<spyfft::CfgD<10, 10, 10, 5, 1>, 4>(L, outk, mean);
    else if (P == 2 && M == 10000) run_declong<spyfft::CfgD<20, 20, 5, 5, 1, 1, true>, 2>(L, outk, mean);
    else return -1;
    return 0;
}

int emu_mtmfft_generic(int n, int nfac, const int* radix, int nfft, int bluestein, const float* chirp,
                       const float* bhat, int stage_x, const float* data, long long ld, const int* chan_idx,
                       const long long* seg_start, const long long* seg_lo, const long long* seg_hi, int nseg,
                       int nsig, int nchan, int ntaper, const float* tapers, const float* tw, float scale,
                       int detrend, int demean_taper, const int* fpos, int nfsel, int out_kind, int keeptapers,
                       void* out) {
    MtmArgs a{};
    a.data = data; a.ld = ld; a.chan_idx = chan_idx;
    a.seg_start = seg_start; a.seg_lo = seg_lo; a.seg_hi = seg_hi;
    a.nseg = nseg; a.nsig = nsig; a.nchan = nchan; a.ntaper = ntaper;
    a.tapers = tapers; a.tw = reinterpret_cast<const float2*>(tw); a.scale = scale;
    a.detrend = detrend; a.demean_taper = demean_taper; a.fpos = fpos; a.nfsel = nfsel;
    a.out_kind = out_kind; a.out = out;
    a.means = g_means;
    GenPlan g{};
    g.n = n; g.nfac = nfac; g.nfft = nfft; g.bluestein = bluestein; g.stage_x = stage_x;
    for (int i = 0; i < nfac; ++i) g.radix[i] = radix[i];
    g.chirp = reinterpret_cast<const float2*>(chirp);
    g.bhat = reinterpret_cast<const float2*>(bhat);
    const size_t lds = ((size_t)2 * n + (stage_x ? nsig : 0)) * sizeof(float2);
    const unsigned grid = (unsigned)nseg * (unsigned)((nchan + 1) / 2);
    const int outk = out_kind == SPYHIP_OUT_FOURIER ? 2 : (out_kind == SPYHIP_OUT_POW ? 0 : 1);
    const bool mean = !keeptapers;
    auto go = [&](auto fn) { emu::launch(dim3(grid), dim3(spyfft::GEN_THREADS), lds, fn); };
    switch (outk * 2 + (mean ? 1 : 0)) {
        case 0: go([&] { spyfft::mtmfft_generic_kernel<0, false>(a, g); }); break;
        case 1: go([&] { spyfft::mtmfft_generic_kernel<0, true>(a, g); }); break;
        case 2: go([&] { spyfft::mtmfft_generic_kernel<1, false>(a, g); }); break;
        case 3: go([&] { spyfft::mtmfft_generic_kernel<1, true>(a, g); }); break;
        case 4: go([&] { spyfft::mtmfft_generic_kernel<2, false>(a, g); }); break;
        default: go([&] { spyfft::mtmfft_generic_kernel<2, true>(a, g); }); break;
    }
    return 0;
}

// The packed mixed-radix engine (mtmfft_mixed.h) with the schedule spyhip_fft_plan_create computes (mix_schedule).
// Returns 1 if the length is not served by it.  force_nostage: take the re-read-per-taper path although the segment
// would fit into LDS; info (7 ints): th, G, npass, stage, threads, radix[0], radix[last].
int emu_mtmfft_mixed(int nfft, int force_nostage, int* info, const float* data, long long ld, const int* chan_idx,
                     const long long* seg_start, const long long* seg_lo, const long long* seg_hi, int nseg,
                     int nsig, int nchan, int ntaper, const float* tapers, const float* tw, float scale,
                     int detrend, int demean_taper, const int* fpos, int nfsel, int out_kind, int keeptapers,
                     void* out) {
    spyfft::MixPlan g{};
    int threads = 0;
    size_t lds = 0;
    if (!spyfft::mix_schedule(nfft, (nchan + 3) / 4, &g, &threads, &lds)) return 1;
    if (force_nostage) g.stage = 0;
    if (info) {
        info[0] = g.th; info[1] = 1 << g.lg; info[2] = g.npass; info[3] = g.stage; info[4] = threads;
        info[5] = g.radix[0]; info[6] = g.radix[g.npass - 1];
    }
    MtmArgs a{};
    a.data = data; a.ld = ld; a.chan_idx = chan_idx;
    a.seg_start = seg_start; a.seg_lo = seg_lo; a.seg_hi = seg_hi;
    a.nseg = nseg; a.nsig = nsig; a.nchan = nchan; a.ntaper = ntaper;
    a.tapers = tapers; a.tw = reinterpret_cast<const float2*>(tw); a.scale = scale;
    a.detrend = detrend; a.demean_taper = demean_taper; a.fpos = fpos; a.nfsel = nfsel;
    a.out_kind = out_kind; a.out = out;
    a.means = g_means;
    const int G = 1 << g.lg;
    const int nitem = (nchan + 3) / 4;
    a.npg = (nitem + G - 1) / G;
    int S = 8 / G; if (S < 1) S = 1; if (S > a.npg) S = a.npg;
    a.S = S;
    a.ncl = (a.npg + S - 1) / S;
    const long long nclusters = (long long)nseg * a.ncl;
    const unsigned grid = (unsigned)(((nclusters + 7) / 8) * S * 8);
    const int outk = out_kind == SPYHIP_OUT_FOURIER ? 2 : (out_kind == SPYHIP_OUT_POW ? 0 : 1);
    const bool mean = !keeptapers;
    auto go = [&](auto fn) { emu::launch(dim3(grid), dim3(threads), lds, fn); };
    switch (outk * 2 + (mean ? 1 : 0)) {
        case 0: go([&] { spyfft::mtmfft_mixed_kernel<0, false, 1024>(a, g); }); break;
        case 1: go([&] { spyfft::mtmfft_mixed_kernel<0, true, 1024>(a, g); }); break;
        case 2: go([&] { spyfft::mtmfft_mixed_kernel<1, false, 1024>(a, g); }); break;
        case 3: go([&] { spyfft::mtmfft_mixed_kernel<1, true, 1024>(a, g); }); break;
        case 4: go([&] { spyfft::mtmfft_mixed_kernel<2, false, 1024>(a, g); }); break;
        default: go([&] { spyfft::mtmfft_mixed_kernel<2, true, 1024>(a, g); }); break;
    }
    return 0;
}

// spyhip_csd_accumulate for the emulated kernels: the route of csd_route.h (the one csd.hip launches), asked with the
// emulator's sample of 3M instances and walked with emu::launch.  force_tpw (1, 3, 5) is the test-only override that picks
// a generic csd_accum_kernel<TA, TB> directly.  Returns a code for the first kernel: 1 / 3 / 5 generic tiles per wave,
// 6 the instruction-lean path, 7 its wide variant, 8 / 9 the 3M kernel (exact 256 / padded), 10 / 11 the 256-channel
// block walk (3M / 4M).
}  // extern "C"

template <int TA, int TB, int FAST = 0>
static void emu_accum(spycsd::CsdArgs a, const spycsd::AccumGeometry& g, int nsplit = 1) {
    a.kb = g.kb;
    if (g.grid > 0)
        emu::launch(dim3((unsigned)g.grid, (unsigned)nsplit), dim3(spycsd::CSD_THREADS), g.lds,
                    [&] { spycsd::csd_accum_kernel<TA, TB, FAST>(a); });
}

static void emu_accum(const spycsd::CsdArgs& a, int ta, int fast, const spycsd::AccumGeometry& g) {
    switch (ta * 10 + fast) {
        case 50: emu_accum<5, 4>(a, g); break;
        case 51: emu_accum<5, 4, 1>(a, g); break;
        case 52: emu_accum<5, 4, 2>(a, g); break;
        case 53: emu_accum<5, 4, 3>(a, g); break;
        case 30: emu_accum<3, 2>(a, g); break;
        default: emu_accum<1, 1>(a, g); break;
    }
}

// grid of m3_launch_one (csd3m_launch_impl.h)
template <int CH, bool EXACT, bool RECT = false, bool M4 = false>
static void emu_m3(spycsd::CsdArgs a, long long nprow) {
    constexpr int NP = spycsd::M3Tab<CH, RECT>::NP;
    a.item_base = 0;
    a.item_end = nprow * spycsd::M3_TILES_PER_F;
    const long long grid = NP > 1 ? ((nprow + 7) / 8) * 8 * NP : (a.blocked ? ((nprow + 31) / 32) * 32 : nprow);
    if (nprow > 0)
        emu::launch(dim3((unsigned)grid), dim3(512), spycsd::M3_LDS_BYTES, [&] { spycsd::csd3m_kernel<CH, 8, EXACT, RECT, M4>(a); });
}

extern "C" {

int emu_csd_accumulate(const float* spec, long long nrows, int F, int C, float* acc, int force_tpw) {
    using spycsd::StepKind;
    spycsd::CsdQuery q;
    q.nchan = C; q.nfreq = F; q.nrows = nrows;
    q.blocked = g_blocked != 0;
    q.phase_exact = g_force_4m != 0;
    q.num_cu = g_num_cu;
    q.have_m3 = emu_have_m3;
    spycsd::CsdArgs base{};
    base.F = F; base.C = C;
    base.acc = reinterpret_cast<float2*>(acc);
    base.blocked = g_blocked;
    if (force_tpw) {                             // (asks no route: a shape the route refuses still reaches the generic kernel)
        const int ta = force_tpw, tb = force_tpw == 1 ? 1 : force_tpw - 1;
        if (ta != 1 && ta != 3 && ta != 5) return -1;
        if (nrows < 0 || F < 1 || C < 1) return -1;
        base.nt = (C + 31) / 32; base.ntiles = (int)spycsd::tri_tiles(C); base.cpad = base.nt * 32;
        base.nitems = (long long)F * base.ntiles;
        base.spec = reinterpret_cast<const float2*>(spec);
        base.nrows = nrows;
        base.item_end = base.nitems;
        const spycsd::AccumGeometry g = spycsd::accum_geometry(ta, tb, 0, base.ntiles, base.cpad, F, nrows, 0, 0, q.lds_per_block, base.nitems);
        if (g.err) return g.err;
        if (nrows > 0) emu_accum(base, ta, 0, g);
        return ta;
    }
    const spycsd::CsdRoute r = spycsd::csd_route(q);
    if (r.err) return r.err;
    base.nt = r.nt; base.ntiles = r.ntiles; base.nitems = r.nitems; base.cpad = r.cpad;
    base.fast_per = r.fast_per; base.fast_nwgf = r.fast_nwgf;
    for (const spycsd::CsdStep& s : r.steps) {
        spycsd::CsdArgs a = base;
        a.spec = reinterpret_cast<const float2*>(spec) + (size_t)s.row0 * F * C;
        a.nrows = s.nrows;
        a.item_base = s.item0; a.item_end = s.item1;
        a.ctot = s.n0 ? C : 0;
        a.ch0 = s.ch0; a.n0 = s.n0; a.ch1 = s.ch1; a.n1 = s.n1;
        switch (s.kind) {
            case StepKind::ACCUM: emu_accum(a, s.ta, s.fast, s.geo); break;
            case StepKind::TAIL: {               // launch_tail of csd.hip with the scratch on the host
                const int f0 = (int)(s.item0 / r.ntiles), nf = F - f0, nsplit = s.split.nsplit;
                const long long n = (long long)nf * C * C;
                std::vector<float2> part(nsplit > 1 ? (size_t)(nsplit - 1) * n : 0);
                if (nsplit > 1) { a.rows_per_split = s.split.rows_per_split; a.part = part.data(); a.part_f0 = f0; a.part_nf = nf; }
                emu_accum<1, 1>(a, s.geo, nsplit);
                if (nsplit > 1)
                    emu::launch(dim3((unsigned)std::min<long long>((n + 255) / 256, 4096)), dim3(256), 0,
                                [&] { spycsd::csd_reduce_parts_kernel(a.acc, a.part, nsplit - 1, f0, nf, C); });
                break;
            }
            case StepKind::M3_EXACT: emu_m3<256, true>(a, s.nprow); break;
            case StepKind::M3_PADDED:
                switch (s.chp) {
#define EMU_M3(CH) case CH: emu_m3<CH, false>(a, s.nprow); break;
                    EMU_M3_WIDTHS(EMU_M3)
#undef EMU_M3
                    default: return -1;            // (the route asked emu_have_m3, which reads the same list)
                }
                break;
            case StepKind::M4_BLOCK: emu_m3<256, false, false, true>(a, s.nprow); break;
            case StepKind::M3_RECT: emu_m3<512, false, true>(a, s.nprow); break;
            case StepKind::M4_RECT: emu_m3<512, false, true, true>(a, s.nprow); break;
            case StepKind::RANK1:                // csd_rank1_kernel of csd.hip, on the host
                for (int f = 0; f < F; ++f)
                    for (int i = 0; i < C; ++i)
                        for (int j = 0; j <= i; ++j) {
                            const float2 u = a.spec[(size_t)f * C + i], v = a.spec[(size_t)f * C + j];
                            float2& o = a.acc[((size_t)f * C + i) * C + j];
                            o.x += u.x * v.x + u.y * v.y;
                            o.y += u.y * v.x - u.x * v.y;
                        }
                break;
        }
    }
    if (r.steps.empty()) return 0;
    const spycsd::CsdStep& s0 = r.steps.front();
    switch (s0.kind) {
        case StepKind::ACCUM: return s0.fast == 3 ? 7 : s0.fast ? 6 : s0.ta;
        case StepKind::M3_EXACT: return 8;
        case StepKind::M3_PADDED: return s0.n0 ? 10 : 9;
        case StepKind::M4_BLOCK: return 11;
        case StepKind::RANK1: return g_force_4m ? 11 : 10;
        default: return -1;
    }
}

void emu_csd_finalize(float* acc, int F, int C, float scale) {
    emu::launch(dim3((unsigned)(F * spycsd::tri_tiles(C))), dim3(256), 0,
                [&] { spycsd::csd_finalize_kernel(reinterpret_cast<float2*>(acc), F, C, scale); });
}

void emu_coh_from_accumulator(const float* acc, int F, int C, float scale, int kind, void* out) {
    const dim3 grid((unsigned)(F * spycsd::tri_tiles(C)));
    if (kind == SPYHIP_OUT_FOURIER)
        emu::launch(grid, dim3(256), 0, [&] { spycsd::coh_from_acc_kernel<true>(reinterpret_cast<const float2*>(acc), F, C, scale, kind, out); });
    else
        emu::launch(grid, dim3(256), 0, [&] { spycsd::coh_from_acc_kernel<false>(reinterpret_cast<const float2*>(acc), F, C, scale, kind, out); });
}

void emu_coh_normalize(const float* csd, int F, int C, int kind, void* out) {
    if (kind == SPYHIP_OUT_FOURIER)
        emu::launch(dim3(4), dim3(256), 0, [&] { spycsd::coh_normalize_kernel<true>(reinterpret_cast<const float2*>(csd), F, C, kind, out); });
    else
        emu::launch(dim3(4), dim3(256), 0, [&] { spycsd::coh_normalize_kernel<false>(reinterpret_cast<const float2*>(csd), F, C, kind, out); });
}

// K9 (mirrors spyhip_jack_coh_accumulate)
void emu_jack_coh(const float* spec, int ntrials, int K, int F, int C, const float* S, const void* direct, int kind,
                  long long T, double* sum_d, double* sum_d2) {
    spycsd::JackArgs a{};
    a.spec = reinterpret_cast<const float2*>(spec);
    a.S = reinterpret_cast<const float2*>(S);
    a.direct = direct;
    a.ntrials = ntrials; a.K = K; a.F = F; a.C = C; a.kind = kind;
    a.T = (float)T;
    a.sum_d = sum_d; a.sum_d2 = sum_d2;
    const int nt = (C + 31) / 32;
    const size_t lds = 2 * (size_t)2 * K * 32 * sizeof(float2);
    const dim3 grid((unsigned)(8 * ((F + 7) / 8) * (nt * (nt + 1) / 2)));
    if (kind == SPYHIP_OUT_FOURIER) emu::launch(grid, dim3(256), lds, [&] { spycsd::jack_coh_kernel<true>(a); });
    else emu::launch(grid, dim3(256), lds, [&] { spycsd::jack_coh_kernel<false>(a); });
}

// K7 (mirrors ppc.hip)
void emu_ppc_accumulate(const float* spec, int ntrials, int ntaper, int F, int C, float* acc) {
    spyppc::PpcArgs a{};
    a.spec = reinterpret_cast<const float2*>(spec);
    a.ntrials = ntrials; a.ntaper = ntaper; a.F = F; a.C = C;
    a.acc = reinterpret_cast<float2*>(acc);
    const int nt = (C + 31) / 32;
    const size_t lds = 2 * (size_t)2 * ntaper * 32 * sizeof(float2);
    emu::launch(dim3((unsigned)(8 * ((F + 7) / 8) * (nt * (nt + 1) / 2))), dim3(256), lds, [&] { spyppc::ppc_accum_kernel(a); });
}

void emu_ppc_accumulate_csd(const float* csd, int ntrials, long long n, float* acc) {
    emu::launch(dim3((unsigned)((n + 255) / 256)), dim3(256), 0, [&] {
        spyppc::ppc_accum_csd_kernel(reinterpret_cast<const float2*>(csd), n, ntrials, reinterpret_cast<float2*>(acc));
    });
}

void emu_ppc_finalize(const float* acc, int F, int ni, int nj, int lower_only, long long T, float* out) {
    const long long n = (long long)F * ni * nj;
    emu::launch(dim3((unsigned)((n + 255) / 256)), dim3(256), 0, [&] {
        spyppc::ppc_finalize_kernel(reinterpret_cast<const float2*>(acc), F, ni, nj, lower_only, (double)T, out);
    });
}

// K8 (mirrors ccov.hip): tw = exp(-2 pi i m / L) from the caller; norm as spyhip_ccov_from_accumulator
int emu_ccov(const float* acc, const float* tw, int nfft, int nchan, int nsamples, double scale, int norm, float* out) {
    spyfft::CcovArgs a{};
    a.acc = reinterpret_cast<const float2*>(acc);
    a.tw = reinterpret_cast<const float2*>(tw);
    a.C = nchan; a.nsamples = nsamples;
    a.nlag = nsamples / 2 + (nsamples & 1);
    a.q = (nsamples & 1) ? 0 : 1;
    a.npairs = (long long)nchan * (nchan + 1) / 2;
    a.scale = (float)(scale / (double)nfft);
    a.out = out;
    switch (nfft) {
        case 1024: emu_launch_ccov<10, 4>(a); break;
        case 2048: emu_launch_ccov<11, 2>(a); break;
        case 4096: emu_launch_ccov<12, 1>(a); break;
        case 8192: emu_launch_ccov<13, 1>(a); break;
        default: return -1;
    }
    if (norm) {
        std::vector<float> d(nchan);
        const float dc = (float)(scale / ((double)nsamples * (double)nsamples));
        emu::launch(dim3((nchan + 255) / 256), dim3(256), 0,
                    [&] { spyfft::ccov_diag_kernel(out, a.acc, nchan, norm, dc, d.data()); });
        const long long n = (long long)a.nlag * nchan * nchan;
        emu::launch(dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                    [&] { spyfft::ccov_normalize_kernel(out, n, nchan, d.data()); });
    }
    return 0;
}

// spyhip_cwt_plan_create* + set_direct / set_precision + spyhip_cwt_exec for the emulated kernels: the taps, the plan and the
// steps of cwt_route.h (the ones cwt.hip uploads and launches), walked with emu::launch on host buffers.  family, p0, p1:
// spycwt::sample_taps; num_cu and the two byte budgets as spycwt::ExecQuery (<= 0: the library's).  `trace`: one line per
// step (cwt_route_text.h).  Returns the route's error code.
int emu_cwt(const float* data, long long ld, const int* chan_idx, const long long* seg_start, const long long* trial_lo,
            const long long* trial_hi, int nseg, int nsig, int nchan, int nscales, const double* scales, double dt, int family,
            double p0, double p1, int detrend, int out_kind, const int* tpos, int ntime_out, void* out, int accumulate,
            int direct, int precision64, long long num_cu, long long stage_budget, long long work_budget, char* trace, int cap) {
    using namespace spycwt;
    std::vector<Taps> taps;
    std::vector<int> ntaps, centre;
    for (int s = 0; s < nscales; ++s) {
        taps.push_back(sample_taps(family, p0, p1, scales[s], dt, nsig));
        ntaps.push_back((int)taps[s].re.size());
        centre.push_back(taps[s].c);
    }
    const Plan pl = plan_route(nsig, nchan, out_kind, detrend, ntaps, centre, tpos);
    if (pl.err) return pl.err;
    ExecQuery q;
    q.nseg = nseg; q.accumulate = accumulate; q.direct = direct && pl.direct_ok; q.precision64 = precision64 != 0;
    if (num_cu > 0) q.num_cu = num_cu;
    if (stage_budget > 0) q.stage_budget = (size_t)stage_budget;
    if (work_budget > 0) q.work_budget = (size_t)work_budget;
    spyfft::Cwt64Args fa{};
    std::vector<double2> tw64, hspec64;
    if (q.precision64) {                     // spyhip_cwt_plan_set_precision
        q.L64 = conv_length64(nsig, ntaps);
        if (q.L64 > MAX_L64 || !spywil::plus_plan((int)q.L64, &fa.plan)) return -3;
        tw64 = spy::twiddle_table<double2>((int)q.L64);
        hspec64.resize((size_t)nscales * q.L64);
        for (int s = 0; s < nscales; ++s) kernel_spectrum(taps[s], 0, taps[s].re.size(), (size_t)q.L64, &hspec64[(size_t)s * q.L64]);
        fa.L = (int)q.L64; fa.tw64 = tw64.data(); fa.hspec64 = hspec64.data(); fa.centre = pl.centre.data();
    }
    const ExecRoute r = exec_route(pl, q);
    if (trace) {
        std::string t;
        for (const Step& s : r.steps) t += render_step(pl, r, s) + "\n";
        std::snprintf(trace, cap, "%s", t.c_str());
    }
    // the tables upload_groups of cwt.hip builds for the group set in use
    const std::vector<Group>& groups = r.sum_set ? pl.groups_sum : pl.groups;
    struct Tables { std::vector<float2> tw, hspec; };
    std::vector<Tables> tables(q.precision64 ? 0 : groups.size());
    for (size_t gi = 0; gi < tables.size(); ++gi) {
        const Group& g = groups[gi];
        const size_t NB = (size_t)1 << g.log2n;
        tables[gi].tw = spy::twiddle_table<float2>((int)NB);
        tables[gi].hspec.resize(g.nscales() * NB);
        for (int k = 0; k < g.nscales(); ++k) {
            const Taps& t = taps[g.scale_ids[k]];
            const bool piece = g.long_idx >= 0;
            kernel_spectrum(t, piece ? g.tap0 : 0, piece ? g.ntaps : t.re.size(), NB, &tables[gi].hspec[k * NB]);
        }
    }
    std::vector<double> trend(r.trend), trend_part(r.trend * TREND_SPLITS);
    std::vector<char> stage(r.stage_bytes);
    std::vector<float2> stage_long(r.stage_long);
    std::vector<float> xt(r.xt);
    std::vector<double2> work(r.work64);
    std::vector<int> fl;
    spyfft::CwtArgs a{};
    a.data = data; a.ld = ld; a.chan_idx = chan_idx;
    a.nsig = nsig; a.nchan = nchan; a.nscales = nscales; a.nscales_total = nscales;
    a.detrend = detrend; a.out_kind = out_kind; a.tpos = tpos;
    if (tpos) { fl = tfloor(tpos, nsig); a.tfloor = fl.data(); }
    a.ntime_out = tpos ? ntime_out : nsig; a.out = out; a.accumulate = accumulate;
    a.stage = stage.data();
    fa.work = work.data();
    for (const Step& s : r.steps) {
        spyfft::CwtArgs c = a;
        c.seg0 = s.seg0; c.nseg = s.nseg;
        c.seg_start = seg_start + s.seg0; c.trial_lo = trial_lo + s.seg0; c.trial_hi = trial_hi + s.seg0;
        if (detrend >= 0) c.trend = trend.data() + (size_t)s.seg0 * nchan * 2;
        if (r.xt && s.kind == StepKind::TRANSFORM) c.xt = xt.data();
        const dim3 grid((unsigned)s.gx, (unsigned)s.gy, (unsigned)s.gz);
        switch (s.kind) {
            case StepKind::MEAN_NP: emu::launch(grid, dim3(64), 0, [&] { spyfft::cwt_mean_np_kernel(c, trend.data()); }); break;
            case StepKind::TREND:
                emu::launch(grid, dim3(256), 0, [&] { spyfft::cwt_trend_partial_kernel(c, trend_part.data()); });
                emu::launch(dim3((unsigned)(((size_t)nseg * nchan + 255) / 256)), dim3(256), 0,
                            [&] { spyfft::cwt_trend_final_kernel(c, trend_part.data(), trend.data()); });
                break;
            case StepKind::INPUT_COPY: emu::launch(grid, dim3(256), 0, [&] { spyfft::cwt_stage_input_kernel(c, xt.data()); }); break;
            case StepKind::CWT64:
                fa.c = c; fa.wg0 = s.wg0;
                with_cwt64_kernel(s.outk, [&](auto kern) { emu::launch(grid, dim3(256), 0, [&] { kern(fa); }); return 0; });
                break;
            case StepKind::TRANSFORM: {
                const Group& gr = groups[s.group];
                c.nscales = gr.nscales();
                c.sidx = s.sidx == Sidx::COMPACT ? gr.sidx_stage.data() : gr.sidx.data();
                c.nscales_total = s.nrows;
                c.tw = tables[s.group].tw.data(); c.hspec = tables[s.group].hspec.data(); c.cshift = gr.cshift.data();
                c.V = gr.V; c.halo = gr.halo; c.nblocks = gr.nblocks;
                c.stage_add = s.add;
                if (s.target == Target::LONG_SIDE) c.stage = stage_long.data();
                const int rc = with_transform_kernel(gr.log2n, s.engine, s.outk, [&](auto kern, int threads, size_t lds) {
                    emu::launch(grid, dim3(threads), lds, [&] { kern(c); });
                    return 0;
                });
                if (rc) return rc;
                break;
            }
            case StepKind::LONG_CONVERT:
                emu::launch(grid, dim3(256), 0, [&] {
                    spyfft::cwt_long_convert_kernel(stage_long.data(), s.sidx == Sidx::COMPACT ? pl.lrow.data() : pl.long_scales.data(),
                                                    (int)pl.long_scales.size(), s.nseg, s.nrows, nchan, nsig, out_kind,
                                                    reinterpret_cast<float*>(stage.data()));
                });
                break;
            case StepKind::SCATTER:
                c.nseg = s.nsets; c.nscales = s.nrows;
                if (s.compact) { c.smap = pl.staged.data(); c.nscales_out = nscales; }
                with_scatter_kernel(s.scatter, [&](auto kern) { emu::launch(grid, dim3(256), 0, [&] { kern(c); }); return 0; });
                break;
        }
    }
    return r.err;
}

// L of spyhip_cwt_plan_set_precision for these tap counts
long long emu_cwt_conv_length64(int nsig, const int* ntaps, int nscales) {
    return spycwt::conv_length64(nsig, std::vector<int>(ntaps, ntaps + nscales));
}

// the plan-creation rule for the direct kernels (cwt_route.h)
int emu_cwt_direct_fits(const int* tpos, int nsig, const int* V, int ngroups, unsigned long long rowb, unsigned long long chanb) {
    return spycwt::cwt_direct_fits(tpos, nsig, V, ngroups, rowb, chanb) ? 1 : 0;
}

// ---- Wilson / Granger kernels.  Which kernel an entry runs, with which grid and LDS, is the decision of granger_route.h
// that granger.hip launches by; `name` (64 bytes, or NULL) receives the kernel's name.
using spywil::cd;
static void w_name(char* name, const char* s) { if (name) std::snprintf(name, 64, "%s", s); }
void emu_w_widen(const float* in, double* out, int C, long long n, double eps) {
    emu::launch(dim3(4), dim3(256), 0, [&] { spywil::widen_kernel(reinterpret_cast<const float2*>(in), reinterpret_cast<cd*>(out), C, n, eps); });
}
// Badd (n x n) joins op(B); with Ref the return value is max |Ref - A op(B)| / |Ref| and no product is stored (both: n >= 48)
double emu_w_gemm(const double* A_, const double* B_, double* C_, int n, int batch, long long sA, long long sB, long long sC, int opB,
                  int addI, const double* Badd_, const double* Ref_, char* name) {
    const cd *A = reinterpret_cast<const cd*>(A_), *B = reinterpret_cast<const cd*>(B_), *Badd = reinterpret_cast<const cd*>(Badd_),
             *Ref = reinterpret_cast<const cd*>(Ref_);
    cd* Cm = reinterpret_cast<cd*>(C_);
    const spywil::GemmRoute r = spywil::gemm_route(n, batch, opB, A == B && sA == sB, Badd != nullptr, Ref != nullptr);
    w_name(name, r.name);
    std::vector<double> partv((size_t)r.ntiles * batch + 1, -1.0);
    double* part = Ref ? partv.data() : nullptr;
    const dim3 grid(r.grid.x, r.grid.y, r.grid.z);
    switch (r.kernel) {
        case spywil::Gemm::TILED: emu::launch(grid, dim3(r.threads), r.lds, [&] { spywil::zgemm_kernel(A, B, Cm, n, sA, sB, sC, opB, addI); }); break;
        case spywil::Gemm::MFMA0: emu::launch(grid, dim3(r.threads), r.lds, [&] { spywil::zgemm_mfma_kernel<0>(A, B, Cm, n, sA, sB, sC, opB, addI, Badd, Ref, part, batch); }); break;
        case spywil::Gemm::MFMA1: emu::launch(grid, dim3(r.threads), r.lds, [&] { spywil::zgemm_mfma_kernel<1>(A, B, Cm, n, sA, sB, sC, opB, addI, Badd, Ref, part, batch); }); break;
        case spywil::Gemm::MFMA2: emu::launch(grid, dim3(r.threads), r.lds, [&] { spywil::zgemm_mfma_kernel<2>(A, B, Cm, n, sA, sB, sC, opB, addI, Badd, Ref, part, batch); }); break;
        case spywil::Gemm::MFMA3: emu::launch(grid, dim3(r.threads), r.lds, [&] { spywil::zgemm_mfma_kernel<3>(A, B, Cm, n, sA, sB, sC, opB, addI, Badd, Ref, part, batch); }); break;
    }
    if (r.kernel != spywil::Gemm::MFMA2) return 0.0;
    double out = -1.0;
    emu::launch(dim3(1), dim3(256), 0, [&] { spywil::maxred_kernel(part, r.ntiles * batch, &out); });
    return out;
}
void emu_w_skew(const double* g0, double* S, double* g0S, int n) {
    emu::launch(dim3((n * n + 255) / 256), dim3(256), 0, [&] { spywil::skew_kernel(reinterpret_cast<const cd*>(g0), reinterpret_cast<cd*>(S), reinterpret_cast<cd*>(g0S), n); });
}
// inverse of `batch` matrices in M, out of place from a copy of the input as the Wilson iteration calls it (M is
// overwritten first, so a kernel that read M instead of its source would show)
void emu_w_inv(double* M_, int n, int batch, int* info, int blocked, unsigned long long lds_per_block, char* name) {
    const spywil::InvRoute r = spywil::inv_route(n, blocked != 0, true, (size_t)lds_per_block);
    w_name(name, r.name);
    const size_t cnt = (size_t)batch * n * n;
    cd* M = reinterpret_cast<cd*>(M_);
    std::vector<cd> srcv(M, M + cnt);
    const cd* src = srcv.data();
    std::fill(M_, M_ + 2 * cnt, -777.0);
    if (r.copy_src) std::copy(src, src + cnt, M);
    switch (r.kernel) {
        case spywil::Inv::MFMA64: emu::launch(dim3(batch), dim3(r.threads), r.lds, [&] { spywil::zinv64_mfma_kernel(M, src, n, info); }); break;
        case spywil::Inv::MFMA32: emu::launch(dim3(batch), dim3(r.threads), r.lds, [&] { spywil::zinv_mfma_kernel(M, src, n, info); }); break;
        case spywil::Inv::BLOCKED16: emu::launch(dim3(batch), dim3(r.threads), r.lds, [&] { spywil::zinv_blocked_kernel(M, n, info); }); break;
        case spywil::Inv::PIVOTED: emu::launch(dim3(batch), dim3(r.threads), r.lds, [&] { spywil::zinv_kernel(M, n, info); }); break;
    }
}
void emu_w_chol(double* M, int n, int batch, int* info, unsigned long long lds_per_block, char* name) {
    const spywil::CholRoute r = spywil::chol_route(n, (size_t)lds_per_block);
    w_name(name, r.name);
    if (r.kernel == spywil::Chol::PANEL) emu::launch(dim3(batch), dim3(r.threads), r.lds, [&] { spywil::zchol_panel_kernel(reinterpret_cast<cd*>(M), n, info); });
    else emu::launch(dim3(batch), dim3(r.threads), r.lds, [&] { spywil::zchol_kernel(reinterpret_cast<cd*>(M), n, info); });
}
void emu_w_gamma0(const double* A, int F, int n, double* out) {
    emu::launch(dim3((n * n + 255) / 256), dim3(256), 0, [&] { spywil::gamma0_kernel(reinterpret_cast<const cd*>(A), F, n, reinterpret_cast<cd*>(out), 0, F); });
}
// the plus operator on the kernel family of the route; generic != 0: plus_kernel whatever the length (the radix-4 kernel
// plus4_kernel is compared with).  Returns -3 where no radix schedule exists.
int emu_w_plus(const double* g_, int F, int n, const double* tw_, double* gp_, double* g0_, unsigned long long lds_per_block, int num_cu,
               int generic, char* name) {
    const cd *g = reinterpret_cast<const cd*>(g_), *tw = reinterpret_cast<const cd*>(tw_);
    cd *gp = reinterpret_cast<cd*>(gp_), *g0 = reinterpret_cast<cd*>(g0_);
    const int L = 2 * (F - 1);
    const long long nent = (long long)n * n;
    spywil::PlusPlan pl{};
    if (!spywil::plus_plan(L, &pl)) return -3;
    spywil::PlusRoute r = spywil::plus_route(L, nent, (size_t)lds_per_block, num_cu);
    if (generic) { r = spywil::PlusRoute(); r.name = "spywil::plus_kernel"; r.grid = nent; r.lds = (size_t)2 * L * 16; }
    w_name(name, r.name);
    switch (r.kernel) {
        case spywil::Plus::PLUS4:
            switch (r.log2l) {
                case 8: run_plus4<8>(r, g_, F, nent, tw_, gp_, g0_); break;
                case 9: run_plus4<9>(r, g_, F, nent, tw_, gp_, g0_); break;
                case 10: run_plus4<10>(r, g_, F, nent, tw_, gp_, g0_); break;
                case 11: run_plus4<11>(r, g_, F, nent, tw_, gp_, g0_); break;
                default: run_plus4<12>(r, g_, F, nent, tw_, gp_, g0_); break;
            }
            break;
        case spywil::Plus::LDS:
            emu::launch(dim3((unsigned)r.grid), dim3(r.threads), r.lds, [&] { spywil::plus_kernel(g, F, nent, pl, tw, gp, g0); });
            break;
        case spywil::Plus::LONG: {
            std::vector<cd> scr(r.scratch_bytes / sizeof(cd));
            for (long long e0 = 0; e0 < nent; e0 += r.chunk)
                emu::launch(dim3((unsigned)std::min(r.chunk, nent - e0)), dim3(r.threads), 0,
                            [&] { spywil::plus_long_kernel(g, F, nent, pl, tw, gp, g0, scr.data(), e0); });
            break;
        }
    }
    return 0;
}
// the convergence check of the Wilson iteration for n channels and F bins: out = {fused, subset first, subset bins}
void emu_w_err_route(int n, int F, int full_check_forced, int* out) {
    const spywil::ErrRoute r = spywil::err_route(n, F, full_check_forced != 0);
    out[0] = r.fused; out[1] = r.subset_first; out[2] = r.subset_bins;
}
void emu_w_addS(double* gp, const double* g0, double* out0, int F, int n) {
    emu::launch(dim3(4), dim3(256), 0, [&] { spywil::add_S_kernel(reinterpret_cast<cd*>(gp), reinterpret_cast<const cd*>(g0), reinterpret_cast<cd*>(out0), F, n); });
}
double emu_w_relerr(const double* A, const double* B, long long n) {
    std::vector<double> part(8);
    emu::launch(dim3(8), dim3(256), 0, [&] { spywil::relerr_kernel(reinterpret_cast<const cd*>(A), reinterpret_cast<const cd*>(B), n, part.data()); });
    double m = 0; for (double v : part) if (v > m || v != v) m = v;
    return m;
}
void emu_w_power(const double* M, int n, int batch, int iters, double* lam) {
    emu::launch(dim3(batch), dim3(256), (size_t)2 * n * 16, [&] { spywil::power_kernel(reinterpret_cast<const cd*>(M), n, iters, lam); });
}
void emu_w_granger(const double* CSD, const double* H, const double* Sigma, int F, int n, float* out) {
    emu::launch(dim3(4), dim3(256), 0, [&] { spywil::granger_kernel(reinterpret_cast<const cd*>(CSD), reinterpret_cast<const cd*>(H), reinterpret_cast<const cd*>(Sigma), F, n, out); });
}

}  // extern "C"

// ---- reference-precision tapered FFT: compile-time schedules (mtmfft_dec64_kernel.h) and the any-length kernel
// (mtmfft_f64_kernel.h, incl. its Bluestein form)
template <class Cf>
static void run_dec64_mode(spyfft::F64Args fa, int nseg, int nchan, int outk, int mean) {
    MtmArgs& a = fa.m;
    const int G = Cf::G;
    const int npairs = Cf::HALF ? nchan : (nchan + 1) / 2;              // (HALF: single channels, as mtmfft_dec64_launch.h)
    a.npg = (npairs + G - 1) / G;
    int S = (Cf::HALF ? 32 : 16) / G; if (S < 1) S = 1; if (S > a.npg) S = a.npg;
    a.S = S;
    a.ncl = (a.npg + S - 1) / S;
    const long long nclusters = (long long)nseg * a.ncl;
    const unsigned grid = (unsigned)(((nclusters + 7) / 8) * S * 8);
    auto go = [&](auto fn) { emu::launch(dim3(grid), dim3(Cf::NTHREADS), Cf::LDS_BYTES, fn); };
    switch (outk * 2 + mean) {
        case 0: go([&] { spyfft::mtmfft_dec64_kernel<Cf, 0, false>(fa); }); break;
        case 1: go([&] { spyfft::mtmfft_dec64_kernel<Cf, 0, true>(fa); }); break;
        case 2: go([&] { spyfft::mtmfft_dec64_kernel<Cf, 1, false>(fa); }); break;
        case 3: go([&] { spyfft::mtmfft_dec64_kernel<Cf, 1, true>(fa); }); break;
        case 4: go([&] { spyfft::mtmfft_dec64_kernel<Cf, 2, false>(fa); }); break;
        default: go([&] { spyfft::mtmfft_dec64_kernel<Cf, 2, true>(fa); }); break;
    }
}

extern "C" int emu_mtmfft_f64(int nfft, int blue_m, const float* data, long long ld, const int* chan_idx,
                              const long long* seg_start, const long long* seg_lo, const long long* seg_hi, int nseg,
                              int nsig, int nchan, int ntaper, const double* tapers64, const double* tw64,
                              const double* chirp64, const double* bhat64, float scale, int detrend, int demean_taper,
                              int seg_f64, const int* fpos, int nfsel, int out_kind, int keeptapers, int use_dec, void* out) {
    spyfft::F64Args fa{};
    MtmArgs& a = fa.m;
    a.data = data; a.ld = ld; a.chan_idx = chan_idx;
    a.seg_start = seg_start; a.seg_lo = seg_lo; a.seg_hi = seg_hi;
    a.nseg = nseg; a.nsig = nsig; a.nchan = nchan; a.ntaper = ntaper;
    a.scale = scale; a.detrend = detrend; a.demean_taper = demean_taper; a.fpos = fpos; a.nfsel = nfsel;
    a.out_kind = out_kind; a.out = out; a.means = g_means; a.seg_f64 = seg_f64;
    fa.tapers64 = tapers64;
    fa.tw64 = reinterpret_cast<const double2*>(tw64);
    const int outk = out_kind == SPYHIP_OUT_FOURIER ? 2 : (out_kind == SPYHIP_OUT_POW ? 0 : 1);
    const int mean = keeptapers ? 0 : 1;
    if (use_dec == 2) {
        // HALF form (CfgD64::HALF): single channels through the schedule of nfft / 2; tables as spyhip_fft_plan_set_precision
        // builds them: tw64 of nfft / 2 for the passes, the length-nfft table for the half step
        const int rn = nfft == 2002 ? 2000 : nfft;       // (id 2002 = nfft 2000 with split exchanges)
        std::vector<double2> th((size_t)rn / 2);
        for (int m = 0; m < rn / 2; ++m) th[m] = reinterpret_cast<const double2*>(tw64)[2 * m];
        fa.tw64_full = fa.tw64;
        fa.tw64 = th.data();
        using spyfft::CfgD64;
        switch (nfft) {
            case 2000: run_dec64_mode<CfgD64<10, 10, 10, 1, 2, false, true, true, 1, true>>(fa, nseg, nchan, outk, mean); break;
            case 2002: run_dec64_mode<CfgD64<10, 10, 10, 1, 2, true, true, true, 1, true>>(fa, nseg, nchan, outk, mean); break;   // split exchanges
            case 1200: run_dec64_mode<CfgD64<10, 10, 2, 1, 4, false, true, true, 3, true>>(fa, nseg, nchan, outk, mean); break;   // 3 x 200
            case 1024: run_dec64_mode<CfgD64<16, 16, 2, 1, 2, false, true, false, 1, true>>(fa, nseg, nchan, outk, mean); break;  // powers from the table
            case 12000: run_dec64_mode<spyfft::D64H_12000>(fa, nseg, nchan, outk, mean); break;
            default: return -1;
        }
        return 0;
    }
    if (use_dec) {
        switch (nfft) {          // (512 / 2048 / 500 differ from 1024 / 4096 / 1000 in one radix only: left to the GPU tests)
            case 256: run_dec64_mode<spyfft::D64_256>(fa, nseg, nchan, outk, mean); break;
            case 1024: run_dec64_mode<spyfft::D64_1024>(fa, nseg, nchan, outk, mean); break;
            case 4096: run_dec64_mode<spyfft::D64_4096>(fa, nseg, nchan, outk, mean); break;
            case 8192: run_dec64_mode<spyfft::D64_8192>(fa, nseg, nchan, outk, mean); break;
            case 16384: run_dec64_mode<spyfft::D64_16384>(fa, nseg, nchan, outk, mean); break;
            case 200: run_dec64_mode<spyfft::D64_200>(fa, nseg, nchan, outk, mean); break;
            case 1000: run_dec64_mode<spyfft::D64_1000>(fa, nseg, nchan, outk, mean); break;
            case 2000: run_dec64_mode<spyfft::D64_2000>(fa, nseg, nchan, outk, mean); break;
            case 2500: run_dec64_mode<spyfft::D64_2500>(fa, nseg, nchan, outk, mean); break;
            case 4000: run_dec64_mode<spyfft::D64_4000>(fa, nseg, nchan, outk, mean); break;
            case 5000: run_dec64_mode<spyfft::D64_5000>(fa, nseg, nchan, outk, mean); break;
            case 10000: run_dec64_mode<spyfft::D64_10000>(fa, nseg, nchan, outk, mean); break;
            case 600: run_dec64_mode<spyfft::D64_600>(fa, nseg, nchan, outk, mean); break;
            case 100: run_dec64_mode<spyfft::D64_100>(fa, nseg, nchan, outk, mean); break;
            case 300: run_dec64_mode<spyfft::D64_300>(fa, nseg, nchan, outk, mean); break;
            case 400: run_dec64_mode<spyfft::D64_400>(fa, nseg, nchan, outk, mean); break;
            case 2400: run_dec64_mode<spyfft::D64_2400>(fa, nseg, nchan, outk, mean); break;
            case 3200: run_dec64_mode<spyfft::D64_3200>(fa, nseg, nchan, outk, mean); break;
            case 768: run_dec64_mode<spyfft::D64_768>(fa, nseg, nchan, outk, mean); break;
            case 1500: run_dec64_mode<spyfft::D64_1500>(fa, nseg, nchan, outk, mean); break;
            case 3000: run_dec64_mode<spyfft::D64_3000>(fa, nseg, nchan, outk, mean); break;
            case 3072: run_dec64_mode<spyfft::D64_3072>(fa, nseg, nchan, outk, mean); break;
            case 6000: run_dec64_mode<spyfft::D64_6000>(fa, nseg, nchan, outk, mean); break;
            case 7500: run_dec64_mode<spyfft::D64_7500>(fa, nseg, nchan, outk, mean); break;
            default: return -1;
        }
        return 0;
    }
    // any-length kernel; work arrays in "LDS" (the emulator's dynamic buffer has no size limit)
    const int L = blue_m ? blue_m : nfft;
    if (!spywil::plus_plan(L, &fa.plan)) return -2;
    fa.work = nullptr;
    fa.wg0 = 0;
    fa.blue_n = blue_m ? nfft : 0;
    fa.chirp64 = reinterpret_cast<const double2*>(chirp64);
    fa.bhat64 = reinterpret_cast<const double2*>(bhat64);
    const unsigned grid = (unsigned)((long long)nseg * ((nchan + 1) / 2));
    const size_t lds = (size_t)2 * L * sizeof(double2);
    auto go = [&](auto fn) { emu::launch(dim3(grid), dim3(256), lds, fn); };
    switch (outk * 2 + mean) {
        case 0: go([&] { spyfft::mtmfft_f64_any_kernel<0, false>(fa); }); break;
        case 1: go([&] { spyfft::mtmfft_f64_any_kernel<0, true>(fa); }); break;
        case 2: go([&] { spyfft::mtmfft_f64_any_kernel<1, false>(fa); }); break;
        case 3: go([&] { spyfft::mtmfft_f64_any_kernel<1, true>(fa); }); break;
        case 4: go([&] { spyfft::mtmfft_f64_any_kernel<2, false>(fa); }); break;
        default: go([&] { spyfft::mtmfft_f64_any_kernel<2, true>(fa); }); break;
    }
    return 0;
}
