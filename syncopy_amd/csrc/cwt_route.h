// Host decisions of the wavelet transform (K3): the sampled taps of a scale, which block engine a scale runs on, which
// scales share a launch, how long kernels are cut, which staging row a scale gets, and the ordered steps of a call with
// their grids and buffer sizes.  Pure logic on integers and host vectors, no HIP header and no runtime call, so that the
// policy is testable on any host (tests/test_cwt_route.py).  cwt.hip walks the steps with hipLaunchKernelGGL, on the
// device and, in the kernel emulator (tests/emu/cwt_emu.cpp), on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

#include "host_fft.h"

namespace spycwt {

constexpr double PI = 3.14159265358979323846264338327950288;
constexpr int CWT_PIECE = 8192;   // taps per piece of a long kernel: a 16384-point block then yields 8193 outputs
constexpr int MAX_LOG2N = 14;
constexpr size_t STAGE_BUDGET = (size_t)4 << 30;    // bytes of staging per chunk of segments
constexpr size_t WORK64_BUDGET = (size_t)2 << 30;   // bytes of float64 work arrays per launch
constexpr int TREND_SPLITS = 64;                    // slices of a trial in the partial trend sums (= spyfft::CWT_TREND_SPLITS)

// The block engines: X(log2 of the block length, channel pairs per workgroup of the staged kernel - channels for the
// unpacked 2^14 kernel -, channel pairs per workgroup of the direct kernel or 0 if there is none).  Direct workgroups are
// wider than the staged ones (G = 4 / 2 - the staged kernels' shape, 32- / 16-byte runs - measured 284 against 236
// us/trial at 128 ch x 16384 samples x 25 scales).
#define SPY_CWT_ENGINES(X) X(10, 4, 8) X(11, 2, 4) X(12, 1, 0) X(13, 1, 0) X(14, 1, 0)

struct Engine { int log2n, G, Gd; };
inline const Engine* engine(int log2n) {
    static const Engine table[] = {
#define SPY_CWT_ENGINE_ROW(L, G, GD) {L, G, GD},
        SPY_CWT_ENGINES(SPY_CWT_ENGINE_ROW)
#undef SPY_CWT_ENGINE_ROW
    };
    for (const Engine& e : table)
        if (e.log2n == log2n) return &e;
    return nullptr;
}
// f(integral_constant LOG2N, G, GD) of the engine of 2^log2n points; -1 if there is none
template <class F>
int for_engine(int log2n, F&& f) {
    switch (log2n) {
#define SPY_CWT_ENGINE_CASE(L, G, GD) \
        case L: return f(std::integral_constant<int, L>{}, std::integral_constant<int, G>{}, std::integral_constant<int, GD>{});
        SPY_CWT_ENGINES(SPY_CWT_ENGINE_CASE)
#undef SPY_CWT_ENGINE_CASE
        default: return -1;
    }
}

// OUTK of the kernel templates for an output kind of spyhip.h: 0 power, 1 any other real kind, 2 complex
constexpr int OUT_POW = 0, OUT_FOURIER = 2;
constexpr int outk_of(int output) { return output == OUT_FOURIER ? 2 : output == OUT_POW ? 0 : 1; }

template <class... A>
std::string fmt(const char* f, A... a) {
    char buf[256];
    std::snprintf(buf, sizeof buf, f, a...);
    return buf;
}

// ---------------------------------------------------------------------------------------------------------------- taps
// The sampled kernel of one scale (transform.py:96-103), trimmed to the taps that can overlap a signal of nsig samples,
// and the "same" centre of the trimmed kernel.  family 0: Morlet(w0 = p0) as Morlet.time / cwt_time sample it; family 1:
// the superlet formulation MorletSL with p0 = c_i cycles inside the Gaussian envelope of p1 = k_sd standard deviations
// (specest/superlet.py:268-363); family 2: Paul(m = p0), family 3: DOG(m = p0) - Ricker / Marr / Mexican_hat are DOG(2) -
// as Paul.time / DOG.time sample them (specest/wavelets/wavelets.py:140-223).  The transform convolves with a table of
// sampled taps, so every family runs on the same kernels.
struct Taps {
    std::vector<double> re, im;
    int c = 0;
};
inline Taps sample_taps(int family, double p0, double p1, double sc, double dt, int nsig) {
    const double w0 = p0;
    const double M = family == 1 ? 10.0 * sc * p0 / dt : 10.0 * sc / dt;       // superlet.py:366-375
    const double t0 = (-M + 1.0) / 2.0, t1 = (M + 1.0) / 2.0;
    long long L = (long long)std::ceil(t1 - t0);               // len(np.arange(t0, t1))
    if (L < 1) L = 1;
    const long long c = (L - 1) / 2;                            // fftconvolve mode="same" offset
    // y[n] = sum_m h[m] x[n + c - m], 0 <= n + c - m < nsig  =>  m in [c - (nsig-1), c + (nsig-1)]
    const long long m0 = std::max<long long>(0, c - (nsig - 1));
    const long long m1 = std::min<long long>(L, c + nsig);      // exclusive
    Taps k;
    k.c = (int)(c - m0);
    const double norm = std::sqrt(dt) / (sc * 8.0 * PI) * std::pow(PI, -0.25);
    const double corr = std::exp(-0.5 * w0 * w0);
    // MorletSL: sqrt(dt)/(4 pi) * k_sd / (s c (2 pi)^1.5) * exp(i t/s) * exp(-(k_sd t/s / (2 pi c))^2 / 2)
    const double norm_sl = std::sqrt(dt) / (4.0 * PI) * p1 / (sc * p0 * std::pow(2.0 * PI, 1.5));
    // Paul(m): 2^m i^m m! / sqrt(pi (2m)!) (1 - i x)^-(m+1); DOG(m): (-1)^(m+1) / sqrt(Gamma(m + 1/2)) He_m(x) exp(-x^2/2);
    // both with cwt_time's amplitude normalisation sqrt(dt) / (8 pi s)  (wavelets.py:140-223, transform.py:96-103)
    const int mo = family >= 2 ? (int)p0 : 0;
    const double norm_t = std::sqrt(dt) / (sc * 8.0 * PI);
    const double paul_c = family == 2 ? std::exp(mo * std::log(2.0) + std::lgamma(mo + 1.0) - 0.5 * (std::log(PI) + std::lgamma(2.0 * mo + 1.0))) : 0.0;
    const double dog_c = family == 3 ? ((mo + 1) % 2 ? -1.0 : 1.0) * std::exp(-0.5 * std::lgamma(mo + 0.5)) : 0.0;
    k.re.resize(m1 - m0);
    k.im.resize(m1 - m0);
    for (long long m = m0; m < m1; ++m) {
        const double x = (t0 + (double)m) * dt / sc;            // t / s
        if (family == 2) {
            // (1 - i x)^-(m+1) = r^-(m+1) exp(i (m+1) atan(x)),  times i^m
            const double r = std::sqrt(1.0 + x * x), ph = (mo + 1) * std::atan(x) + 0.5 * PI * mo;
            const double a = norm_t * paul_c * std::pow(r, -(double)(mo + 1));
            k.re[m - m0] = a * std::cos(ph);
            k.im[m - m0] = a * std::sin(ph);
            continue;
        }
        if (family == 3) {
            double h0 = 1.0, h1 = x;                            // probabilists' Hermite: He_{n+1} = x He_n - n He_{n-1}
            for (int q = 1; q < mo; ++q) { const double h2 = x * h1 - q * h0; h0 = h1; h1 = h2; }
            k.re[m - m0] = norm_t * dog_c * (mo == 0 ? 1.0 : h1) * std::exp(-0.5 * x * x);
            k.im[m - m0] = 0.0;
            continue;
        }
        if (family == 1) {
            const double u = p1 * x / (2.0 * PI * p0);
            const double g = norm_sl * std::exp(-0.5 * u * u);
            k.re[m - m0] = g * std::cos(x);
            k.im[m - m0] = g * std::sin(x);
            continue;
        }
        const double g = norm * std::exp(-0.5 * x * x);
        k.re[m - m0] = g * (std::cos(w0 * x) - corr);
        k.im[m - m0] = g * std::sin(w0 * x);
    }
    return k;
}

// FFT_NB(taps [m0, m0 + n) of k, zero-padded) / NB, the table a transform kernel multiplies a block's spectrum with: for a
// group's scale (m0 = 0, every tap), a piece of a long scale, and the float64 convolution of length NB = L
template <class T2>
void kernel_spectrum(const Taps& k, size_t m0, size_t n, size_t NB, T2* out) {
    std::vector<double> re(NB, 0.0), im(NB, 0.0);
    for (size_t m = 0; m < n; ++m) { re[m] = k.re[m0 + m]; im[m] = k.im[m0 + m]; }
    spy::fft_host(re, im);
    for (size_t q = 0; q < NB; ++q) {
        out[q].x = (decltype(T2::x))(re[q] / (double)NB);
        out[q].y = (decltype(T2::x))(im[q] / (double)NB);
    }
}

// tile reference of the direct kernels: the largest slot among the samples 0 ... n (0 if none)
inline std::vector<int> tfloor(const int* tpos, int nsig) {
    std::vector<int> fl(nsig);
    int last = -1;
    for (int n = 0; n < nsig; ++n) {
        if (tpos[n] >= 0) last = tpos[n];
        fl[n] = std::max(last, 0);
    }
    return fl;
}

// May the direct kernels (cwt2d_kernel) write a plan's outputs?  A tile of samples [o0, o0 + V) stores at the slot reached
// before it, sref = tfloor[o0], plus a 32-bit byte offset (slot - sref) * rowb + channel bytes, and tfloor is only a lower
// bound of the tile's slots if the slots increase with the samples.  So: slots increasing, and for every block of every
// group the direct kernels serve, the tile's slot span times `rowb` (bytes from one slot to the next: nscales * nchan *
// element size) plus `chanb` (nchan * element size) below 2^32.  Gapped slots (tpos[n] = 10000 n) make the span far larger
// than the block.  tpos = nullptr: slot n for sample n.  V[0 ... ngroups): outputs per block of each direct group.
inline bool cwt_direct_fits(const int* tpos, int nsig, const int* V, int ngroups, unsigned long long rowb,
                            unsigned long long chanb) {
    constexpr unsigned long long LIM = 1ull << 32;
    if (rowb >= LIM || chanb >= LIM) return false;
    if (tpos) {
        int last = -1;
        for (int n = 0; n < nsig; ++n)
            if (tpos[n] >= 0) {
                if (tpos[n] <= last) return false;
                last = tpos[n];
            }
    }
    for (int g = 0; g < ngroups; ++g) {
        if (V[g] < 1) return false;
        long long last = -1, sref = 0;      // (tfloor: the largest slot among samples 0 ... n, >= 0)
        for (int n = 0; n < nsig; ++n) {
            if (!tpos) last = n;
            else if (tpos[n] >= 0) last = tpos[n];
            const long long fl = last > 0 ? last : 0;
            if (n % V[g] == 0) sref = fl;
            if (n % V[g] == V[g] - 1 || n == nsig - 1) {
                const unsigned long long span = (unsigned long long)(fl - sref);
                if (span >= LIM || span * rowb + chanb >= LIM) return false;
            }
        }
    }
    return true;
}

// -------------------------------------------------------------------------------------------------------------- groups
// Scales whose (trimmed) kernel support needs the same block length share one launch: short kernels run on short blocks
// (less FFT work per output sample, two workgroups per CU) instead of on the block the longest one needs.
struct Group {
    int log2n = 0, V = 0, halo = 0, nblocks = 0;
    int long_idx = -1, piece = 0;   // long_idx >= 0: piece `piece` of the long_idx-th scale whose kernel exceeds a block,
    int tap0 = 0, ntaps = 0;        // its taps [tap0, tap0 + ntaps)
    bool direct = false;            // the engine has a direct kernel, which writes the output layout itself (no staging)
    std::vector<int> scale_ids;     // the plan's scale index of every scale of this launch (a piece: its one scale)
    std::vector<int> cshift;        // per scale: output n of block o0 sits at q = n - o0 + cshift
    std::vector<int> sidx;          // scale s of this launch -> row of the full staging buffer (a piece with real outputs:
                                    // of the complex side buffer)
    std::vector<int> sidx_stage;    // with direct groups: -> row of the compact staging buffer (same exception); empty for
                                    // a direct group
    int nscales() const { return (int)scale_ids.size(); }
};

// The block length of a kernel of `ntaps` taps: >= 4x the kernel (>= 75 % of a block is output) while that stays on the
// packed engine (<= 8192), else >= 2x, up to the 16384-point engine - and never below `floor`.  0: no block holds it, the
// kernel is cut into pieces.  Which floor pays depends on where the results go (measured at 128 ch x 16384 samples x 25
// scales 4 ... 100 Hz, us/trial: trial sums 169 / 162 / 146 / 189 at 1024 / 2048 / 4096 / 8192 - longer blocks waste less on
// the halo and the staged kernels take them; per-trial outputs 245 / 250 / 265: the direct kernels exist for 1024 and 2048
// points only).
inline int block_length(int ntaps, int floor) {
    int NB = floor;
    while (NB < 4 * (ntaps + 1) && NB < 8192) NB <<= 1;
    while (NB < 2 * (ntaps + 1) && NB < (1 << MAX_LOG2N)) NB <<= 1;
    return 2 * (ntaps + 1) > (1 << MAX_LOG2N) ? 0 : NB;
}
constexpr int SUM_FLOOR = 4096, SUM_FLOOR_FROM = 4096;   // trial sums of signals of >= 4096 samples: blocks of >= 4096 points

struct Plan {
    int err = 0;                    // 0, or the code spyhip_cwt_plan_create returns with `message`
    std::string message;
    int nsig = 0, nchan = 0, nscales = 0, output = 0, detrend = -1;
    std::vector<int> ntaps, centre; // per scale: trimmed taps and their "same" centre
    std::vector<Group> groups;      // one group per block length in use (floor 1024), then the pieces of the long scales
    std::vector<Group> groups_sum;  // the set trial sums run on pairs of trials with when it is not `groups`: floor 4096
    bool sum_pairs = false;         // do trial sums (accumulate = 2) run on pairs of trials?
    std::vector<int> long_scales;   // scales whose trimmed kernel has more taps than a block holds: run piece by piece
    std::vector<int> staged;        // compact staging: row -> scale, for the scales the direct kernels do not serve
    std::vector<int> lrow;          // long scale -> compact staging row
    bool direct_ok = true;          // cwt_direct_fits: slots increasing, 32-bit tile offsets
    const std::vector<Group>& sum_set() const { return groups_sum.empty() ? groups : groups_sum; }
};

// one group per block length among the scales a block holds; appends to `out`
inline void build_groups(Plan& p, int floor, std::vector<Group>& out) {
    for (int log2n = 10; log2n <= MAX_LOG2N; ++log2n) {
        const int NB = 1 << log2n;
        Group g;
        int right = 0, lmax = 1;
        for (int s = 0; s < p.nscales; ++s) {
            if (block_length(p.ntaps[s], floor) != NB) continue;
            g.scale_ids.push_back(s);
            lmax = std::max(lmax, p.ntaps[s]);
            g.halo = std::max(g.halo, p.ntaps[s] - 1 - p.centre[s]);              // reach to the left: L-1-c
            right = std::max(right, p.centre[s]);
        }
        if (g.scale_ids.empty()) continue;
        g.V = NB - g.halo - right;
        if (g.V < 1) {
            if (!p.err) {
                p.err = -3;
                p.message = fmt("cwt_plan_create: kernel support of %d taps exceeds the %d-point block FFT "
                                "(scale too large for this signal length)", lmax, NB);
            }
            return;
        }
        g.log2n = log2n;
        g.nblocks = (p.nsig + g.V - 1) / g.V;
        g.direct = engine(log2n)->Gd > 0;
        g.sidx = g.scale_ids;
        for (int s : g.scale_ids) g.cshift.push_back(g.halo + p.centre[s]);
        out.push_back(g);
    }
}

// The host description of a plan from the tap counts and centres of its scales (sample_taps).  tpos: nsig output slots
// (-1: sample not kept) or nullptr.
inline Plan plan_route(int nsig, int nchan, int output, int detrend, const std::vector<int>& ntaps, const std::vector<int>& centre,
                       const int* tpos) {
    Plan p;
    p.nsig = nsig; p.nchan = nchan; p.nscales = (int)ntaps.size(); p.output = output; p.detrend = detrend;
    p.ntaps = ntaps; p.centre = centre;
    const bool fourier = output == OUT_FOURIER;
    for (int s = 0; s < p.nscales; ++s)
        if (block_length(ntaps[s], 1024) == 0) p.long_scales.push_back(s);
    build_groups(p, 1024, p.groups);
    if (p.err) return p;
    // ---- kernels longer than a block: h = sum_p h_p (pieces of CWT_PIECE taps), y = sum_p h_p * x.  Piece p is an
    // overlap-save convolution of its own: taps [p PL, p PL + Lp), centre c_p = c - p PL (may be negative or beyond the
    // piece), input window from o0 - halo_p with halo_p = Lp - 1 - c_p, output n of block o0 at q = n - o0 + Lp - 1.
    // Complex outputs add up in the staging rows of the scale itself, real ones in the complex side buffer.
    for (size_t li = 0; li < p.long_scales.size(); ++li) {
        const int sc = p.long_scales[li];
        for (int pc = 0; pc * CWT_PIECE < ntaps[sc]; ++pc) {
            Group g;
            g.log2n = MAX_LOG2N; g.long_idx = (int)li; g.piece = pc;
            g.tap0 = pc * CWT_PIECE; g.ntaps = std::min(CWT_PIECE, ntaps[sc] - g.tap0);
            g.V = (1 << MAX_LOG2N) - (g.ntaps - 1);
            g.halo = g.ntaps - 1 - (centre[sc] - g.tap0);
            g.nblocks = (nsig + g.V - 1) / g.V;
            g.scale_ids = {sc};
            g.cshift = {g.ntaps - 1};
            g.sidx = {fourier ? sc : (int)li};
            p.groups.push_back(g);
        }
    }
    // ---- compact staging rows for the scales the direct kernels do not serve: the long scales first
    std::vector<int> row(p.nscales, -1);
    auto stage_row = [&](int sc) {
        if (row[sc] < 0) { row[sc] = (int)p.staged.size(); p.staged.push_back(sc); }
        return row[sc];
    };
    for (Group& g : p.groups)
        if (g.long_idx >= 0) {
            const int r = stage_row(g.scale_ids[0]);
            g.sidx_stage = {fourier ? r : g.long_idx};
        }
    for (Group& g : p.groups)
        if (!g.direct && g.long_idx < 0)
            for (int sc : g.scale_ids) g.sidx_stage.push_back(stage_row(sc));
    for (int sc : p.long_scales) p.lrow.push_back(row[sc]);
    // ---- trial sums: blocks of at least 4096 points for long signals, on pairs of trials where every group of the set
    // runs on the packed engine (the 16384-point kernel is not packed); otherwise the per-segment set, unpaired
    int top = 0;
    const int floor = nsig >= SUM_FLOOR_FROM ? SUM_FLOOR : 1024;
    for (int s = 0; s < p.nscales; ++s) {
        const int NB = block_length(ntaps[s], floor);
        top = std::max(top, NB ? NB : 1 << MAX_LOG2N);
    }
    p.sum_pairs = top <= 8192;
    if (p.sum_pairs && floor != 1024) {
        build_groups(p, floor, p.groups_sum);
        if (p.err) return p;
    }
    // ---- slots increasing with the samples, and every tile's stores within 32-bit byte offsets of its reference slot
    std::vector<int> vd;
    for (const Group& g : p.groups)
        if (g.direct) vd.push_back(g.V);
    const unsigned long long esz = fourier ? 8 : 4;
    const unsigned long long chanb = (unsigned long long)nchan * esz, rowb = (unsigned long long)p.nscales * chanb;
    if (!vd.empty() && !cwt_direct_fits(tpos, nsig, vd.data(), (int)vd.size(), rowb, chanb)) p.direct_ok = false;
    return p;
}

// length of the float64 convolution: L = 2^m >= max(16, nsig + taps - 1); a plan takes it up to MAX_L64
constexpr long long MAX_L64 = 1 << 22;
inline long long conv_length64(int nsig, const std::vector<int>& ntaps) {
    int lmax = 1;
    for (int n : ntaps) lmax = std::max(lmax, n);
    long long L = 16;
    while (L < (long long)nsig + (long long)lmax - 1) L <<= 1;
    return L;
}

// ------------------------------------------------------------------------------------------------------------ execution
enum class StepKind {
    MEAN_NP,        // cwt_mean_np_kernel: the reference's float32 mean in its own summation order
    TREND,          // cwt_trend_partial_kernel + cwt_trend_final_kernel
    INPUT_COPY,     // cwt_stage_input_kernel: channel-major copy of the chunk's signals
    CWT64,          // cwt64_kernel over the (segment, channel) items [wg0, wg0 + grid) of the chunk
    TRANSFORM,      // one group of scales on its block engine
    LONG_CONVERT,   // cwt_long_convert_kernel: the complex sums of the pieces into the staging rows of the long scales
    SCATTER         // transposition of the staging rows into the output
};
enum class EngineKind { PLAIN14, PACKED, PACKED_PAIRS, DIRECT };    // cwt_kernel, cwt2_kernel, cwt2_kernel<PAIRT>, cwt2d_kernel
enum class Sidx { FULL, COMPACT };            // Group::sidx / Group::sidx_stage; for LONG_CONVERT: long_scales / lrow
enum class Target { OUTPUT, STAGE, LONG_SIDE };
enum class Scatter { COMPLEX, WIDE, PLAIN };  // cwt_scatter_kernel<float2>, cwt_scatter_wide_kernel, cwt_scatter_kernel<float>

struct Step {
    StepKind kind;
    int seg0 = 0, nseg = 0;             // the segments [seg0, seg0 + nseg) of the call: the whole call or one chunk
    long long gx = 0, gy = 1, gz = 1;   // grid (TREND: of the partial sums; the final pass has (nseg nchan + 255) / 256)
    // TRANSFORM
    int group = -1;                     // index into the group set of the route
    EngineKind engine = EngineKind::PACKED;
    int G = 0;                          // channel pairs (PLAIN14, PACKED_PAIRS: channels) per workgroup
    int outk = 0;                       // 0 power, 1 other real kinds, 2 complex (every piece of a long scale)
    Sidx sidx = Sidx::FULL;             // TRANSFORM, LONG_CONVERT
    int nrows = 0;                      // rows per row set of the target (TRANSFORM); staging rows per row set (LONG_CONVERT, SCATTER)
    Target target = Target::STAGE;
    bool add = false;                   // add to the target's values (later pieces of a long scale)
    // CWT64
    long long wg0 = 0;
    // SCATTER
    Scatter scatter = Scatter::PLAIN;
    int nsets = 0;                      // row sets to add up / store
    bool compact = false;               // the staging rows are the compact ones: Plan::staged maps them to scales
};

struct ExecQuery {
    int nseg = 0, accumulate = 0;
    bool direct = true;                 // spyhip_cwt_plan_set_direct
    bool precision64 = false;           // spyhip_cwt_plan_set_precision
    long long L64 = 0;                  // its convolution length
    long long num_cu = 256;
    size_t stage_budget = STAGE_BUDGET, work_budget = WORK64_BUDGET;
};

struct ExecRoute {
    int err = 0;                        // 0, or the code spyhip_cwt_exec returns with `message` after the steps listed
    std::string message;
    bool pairs = false;                 // the transform steps take pairs of trials
    bool sum_set = false;               // `group` indexes Plan::groups_sum instead of Plan::groups
    int chunk = 0;                      // segments per chunk
    // what the steps index, in elements of the buffer's type
    size_t trend = 0;                   // double: mean and slope per (segment, channel); the partial sums: x TREND_SPLITS
    size_t stage_bytes = 0;
    size_t stage_long = 0;              // float2: (chunk, long scale, channel, time)
    size_t xt = 0;                      // float: channel-major input copy
    size_t work64 = 0;                  // double2: 3 L per workgroup of a launch
    std::vector<Step> steps;
};

// The steps of spyhip_cwt_exec.  Per-segment outputs (accumulate 0 / 1): scales on engines with a direct kernel leave it in
// the output layout; the others (and every scale of a plan with set_direct(0) or float64 precision) go through the
// time-contiguous staging buffer.  Trial sums (accumulate 2): every scale staged, the packed kernels carrying one channel
// of TWO consecutive segments per thread and storing the sum - a staging row set then holds a pair of segments.  As many
// row sets per chunk as fit the staging budget (at least one).
inline ExecRoute exec_route(const Plan& p, const ExecQuery& q) {
    ExecRoute r;
    const int nseg = q.nseg, nchan = p.nchan, nsig = p.nsig;
    auto fail = [&](int err, const char* text) { r.err = err; r.message = text; return r; };
    if (p.detrend >= 0) {
        r.trend = (size_t)nseg * nchan * 2;
        if (nseg > 65535) return fail(-1, "cwt_exec: more than 65535 segments per call");
        Step s{p.detrend == 0 ? StepKind::MEAN_NP : StepKind::TREND};
        s.nseg = nseg;
        s.gx = (nchan + 63) / 64;
        if (p.detrend == 0) s.gy = nseg;
        else { s.gy = TREND_SPLITS; s.gz = nseg; }
        r.steps.push_back(s);
    }
    const bool use_direct = q.direct && !q.precision64 && q.accumulate != 2;
    r.pairs = q.accumulate == 2 && !q.precision64 && p.sum_pairs;
    r.sum_set = r.pairs && !p.groups_sum.empty();
    const std::vector<Group>& groups = r.sum_set ? p.groups_sum : p.groups;
    const int nst = use_direct ? (int)p.staged.size() : p.nscales;          // staging rows per row set
    const bool fourier = p.output == OUT_FOURIER;
    const size_t esz = fourier ? 8 : 4;
    const size_t per_seg = (size_t)nst * nchan * nsig * esz;
    const int nsets = r.pairs ? (nseg + 1) / 2 : nseg;
    int chunk = nst ? (int)std::max<size_t>(1, std::min<size_t>((size_t)nsets, q.stage_budget / std::max<size_t>(per_seg, 1)))
                    : std::min(nseg, 65535);
    r.stage_bytes = per_seg * chunk;
    const int nlong = (int)p.long_scales.size();
    const bool long_side = nlong > 0 && !fourier;      // real outputs: the pieces are summed as complex numbers first
    if (long_side) r.stage_long = (size_t)chunk * nlong * nchan * nsig;
    if (r.pairs) chunk *= 2;                           // from here on: segments per chunk
    r.chunk = chunk;
    // channel-major copy of the chunk's signals for the float32 kernels (several channels per row: a gather otherwise)
    const bool use_xt = !q.precision64 && nchan > 1;
    if (use_xt) r.xt = (size_t)std::min(chunk, nseg) * nchan * nsig;
    long long per_launch = 0;
    if (q.precision64) {
        // float64 convolutions, one workgroup per (segment, channel), three length-L work arrays each
        const size_t per = (size_t)3 * q.L64 * 16;
        per_launch = std::max<long long>(2LL * q.num_cu, (long long)(q.work_budget / per));
        per_launch = std::min<long long>(per_launch, (long long)std::min(chunk, nseg) * nchan);
        r.work64 = (size_t)per_launch * 3 * q.L64;
    }
    for (int s0 = 0; s0 < nseg; s0 += chunk) {
        const int ns = std::min(chunk, nseg - s0);
        auto step = [&](StepKind k) { Step s{k}; s.seg0 = s0; s.nseg = ns; return s; };
        if (p.nscales > 65535 || ns > 65535) return fail(-1, "cwt_exec: grid too large");
        if (use_xt) {
            Step s = step(StepKind::INPUT_COPY);
            s.gx = (nsig + 63) / 64; s.gy = (nchan + 63) / 64; s.gz = ns;
            r.steps.push_back(s);
        }
        if (q.precision64) {
            const long long items = (long long)ns * nchan;
            for (long long w0 = 0; w0 < items; w0 += per_launch) {
                Step s = step(StepKind::CWT64);
                s.wg0 = w0;
                s.gx = std::min<long long>(per_launch, items - w0);
                s.outk = outk_of(p.output);
                r.steps.push_back(s);
            }
        }
        for (size_t gi = 0; gi < groups.size() && !q.precision64; ++gi) {     // one launch per block length
            const Group& gr = groups[gi];
            const Engine& e = *engine(gr.log2n);
            Step s = step(StepKind::TRANSFORM);
            s.group = (int)gi;
            s.outk = gr.long_idx >= 0 ? 2 : outk_of(p.output);
            long long nunit, nrowsets = ns;
            if (use_direct && gr.direct) {
                s.engine = EngineKind::DIRECT; s.G = e.Gd; s.target = Target::OUTPUT;
                s.nrows = p.nscales;
                nunit = (nchan + 1) / 2;
            } else {
                // work units per row set: channel pairs of a segment; (pairs) channels of a segment pair; channels (2^14)
                s.engine = r.pairs ? EngineKind::PACKED_PAIRS : gr.log2n <= 13 ? EngineKind::PACKED : EngineKind::PLAIN14;
                s.G = e.G;
                s.sidx = use_direct ? Sidx::COMPACT : Sidx::FULL;
                s.nrows = nst;
                if (gr.long_idx >= 0) {
                    s.add = gr.piece > 0;
                    if (long_side) { s.target = Target::LONG_SIDE; s.nrows = nlong; s.sidx = Sidx::FULL; }
                }
                nunit = s.engine == EngineKind::PACKED ? (nchan + 1) / 2 : nchan;
                if (r.pairs) nrowsets = (ns + 1) / 2;
            }
            s.gx = nrowsets * ((nunit + s.G - 1) / s.G) * gr.nblocks;
            if (s.gx > 0x7fffffffLL) return fail(-1, "cwt_exec: grid too large");
            r.steps.push_back(s);
        }
        if (nst == 0) continue;                       // every scale left its kernel in the output layout
        if (long_side && !q.precision64) {
            Step s = step(StepKind::LONG_CONVERT);
            s.gx = ((long long)ns * nlong * nchan * nsig + 255) / 256;
            if (s.gx > 0x7fffffffLL) return fail(-1, "cwt_exec: grid too large");
            s.sidx = use_direct ? Sidx::COMPACT : Sidx::FULL;
            s.nrows = nst;
            r.steps.push_back(s);
        }
        Step s = step(StepKind::SCATTER);
        s.nsets = r.pairs ? (ns + 1) / 2 : ns;        // row sets to add up, nst staging rows each
        s.nrows = nst;
        s.compact = use_direct;
        // real outputs of long trials: tiles of 256 samples x 16 channels (1-KiB reads of the staging rows: 51 -> 46 us/trial
        // at 128 ch x 16384 samples x 25 scales)
        s.scatter = fourier ? Scatter::COMPLEX : ((nsig & 3) == 0 && nsig >= 1024) ? Scatter::WIDE : Scatter::PLAIN;
        s.gx = s.scatter == Scatter::WIDE ? (nsig + 255) / 256 : (nsig + 63) / 64;
        s.gy = nst;
        s.gz = q.accumulate == 2 ? 1 : ns;
        r.steps.push_back(s);
    }
    return r;
}

}  // namespace spycwt
