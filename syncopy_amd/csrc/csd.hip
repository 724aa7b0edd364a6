// Host side of K4/K5: cross-spectral accumulation, finalisation and coherence
// normalisation (spyhip_csd_accumulate / spyhip_csd_finalize / spyhip_coh_normalize).  Which kernels an update takes is
// decided in csd_route.h; this file launches the steps of a route.
#include <algorithm>

#include <cstdlib>

#include "spy_common.h"
#include "csd_route.h"
#include "csd_kernel.h"
#include "csd3m_launch.h"
#include "csdh_launch.h"

using spycsd::CsdArgs;
using spycsd::CsdStep;
using spycsd::StepKind;

static_assert(spycsd::ACCUM_CHUNK_BYTES == (size_t)spycsd::CSD_THREADS * spycsd::CSD_PF * sizeof(float2),
              "csd_route.h: a chunk holds at most 512 threads x CSD_PF staged elements");

namespace {

// SPYHIP_CSD_F32 in the environment (any value, the empty one included): 256 channels stay on the float32 kernels
bool env_f32() {
    static const bool on = std::getenv("SPYHIP_CSD_F32") != nullptr;
    return on;
}

template <int TA, int TB, int FAST = 0>
int launch_accum(spyhip_ctx* ctx, CsdArgs a, const CsdStep& s) {
    auto kern = spycsd::csd_accum_kernel<TA, TB, FAST>;
    a.kb = s.geo.kb;
    SPY_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.geo.lds));
    if (s.geo.grid <= 0) return 0;
    hipLaunchKernelGGL(kern, dim3((unsigned)s.geo.grid, (unsigned)s.split.nsplit), dim3(spycsd::CSD_THREADS), s.geo.lds,
                       ctx->stream, a);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_accum(spyhip_ctx* ctx, const CsdArgs& a, const CsdStep& s) {
    switch (s.ta * 10 + s.fast) {
        case 50: return launch_accum<5, 4>(ctx, a, s);
        case 51: return launch_accum<5, 4, 1>(ctx, a, s);
        case 52: return launch_accum<5, 4, 2>(ctx, a, s);
        case 53: return launch_accum<5, 4, 3>(ctx, a, s);
        case 30: return launch_accum<3, 2>(ctx, a, s);
        default: return launch_accum<1, 1>(ctx, a, s);
    }
}

// The re-cut tail (csd_route.h: tail_split).  Splits > 0 leave partial sums in library scratch that a fixed-order
// reduction adds afterwards (deterministic, no atomics).
int launch_tail(spyhip_ctx* ctx, CsdArgs a, const CsdStep& s) {
    const int nsplit = s.split.nsplit;
    if (nsplit < 2) return launch_accum<1, 1>(ctx, a, s);
    const int f0 = (int)(s.item0 / a.ntiles), nf = a.F - f0;
    const size_t need = (size_t)(nsplit - 1) * nf * a.C * a.C * sizeof(float2);
    if (spy::reserve_scratch(ctx, need)) return -2;
    a.rows_per_split = s.split.rows_per_split;
    a.part = reinterpret_cast<float2*>(ctx->scratch);
    a.part_f0 = f0;
    a.part_nf = nf;
    int rc = launch_accum<1, 1>(ctx, a, s);
    if (rc) return rc;
    const long long n = (long long)nf * a.C * a.C;
    const long long blocks = std::min<long long>((n + 255) / 256, ctx->limits.elementwise_blocks);
    hipLaunchKernelGGL(spycsd::csd_reduce_parts_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, a.acc, a.part,
                       nsplit - 1, f0, nf, a.C);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

// acc[f, i, j] += x[f, i] conj(x[f, j]) (i >= j) for ONE row of spectra: the last row of an odd channel count above 512
// (the 3M kernels' 16-byte copies would read 8 bytes past the end of the spectra there)
__global__ void __launch_bounds__(256) csd_rank1_kernel(const float2* __restrict__ x, int F, int C, float2* __restrict__ acc) {
    const long long per = (long long)C * C, tot = (long long)F * per, stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += stride) {
        const long long f = e / per, r = e - f * per;
        const int i = (int)(r / C), j = (int)(r - (long long)i * C);
        if (j > i) continue;
        const float2 a = x[f * C + i], b = x[f * C + j];
        float2 o = acc[e];
        o.x += a.x * b.x + a.y * b.y;
        o.y += a.y * b.x - a.x * b.y;
        acc[e] = o;
    }
}

// Launch the steps of a route in order.  spec_d / acc_d: the spectra (row 0) and the accumulator of the update.
int run_route(spyhip_ctx* ctx, const spycsd::CsdRoute& r, const void* spec_d, void* acc_d, int nfreq, int nchan, int blocked) {
    if (r.err) { spy::set_error("%s", r.message.c_str()); return r.err; }
    CsdArgs base{};
    base.F = nfreq; base.C = nchan;
    base.acc = reinterpret_cast<float2*>(acc_d);
    base.nt = r.nt; base.ntiles = r.ntiles; base.nitems = r.nitems; base.cpad = r.cpad;
    base.blocked = blocked;
    base.fast_per = r.fast_per; base.fast_nwgf = r.fast_nwgf;
    for (const CsdStep& s : r.steps) {
        CsdArgs a = base;
        a.spec = reinterpret_cast<const float2*>(spec_d) + (size_t)s.row0 * nfreq * nchan;
        a.nrows = s.nrows;
        a.item_base = s.item0; a.item_end = s.item1;
        a.ctot = s.n0 ? nchan : 0;
        a.ch0 = s.ch0; a.n0 = s.n0; a.ch1 = s.ch1; a.n1 = s.n1;
        int rc = 0;
        switch (s.kind) {
            case StepKind::ACCUM: rc = launch_accum(ctx, a, s); break;
            case StepKind::TAIL: rc = launch_tail(ctx, a, s); break;
            case StepKind::M3_EXACT: rc = spycsd::m3_launch(256, ctx->stream, a, s.nprow); break;
            case StepKind::M3_PADDED: rc = spycsd::m3_launch_padded(s.chp, ctx->stream, a, s.nprow); break;
            case StepKind::M4_BLOCK: rc = spycsd::m4_launch_block(ctx->stream, a, s.nprow); break;
            case StepKind::M3_RECT: rc = spycsd::m3_launch_rect(ctx->stream, a, s.nprow); break;
            case StepKind::M4_RECT: rc = spycsd::m4_launch_rect(ctx->stream, a, s.nprow); break;
            case StepKind::RANK1: {
                const long long tot = (long long)nfreq * nchan * nchan;
                hipLaunchKernelGGL(csd_rank1_kernel, dim3((unsigned)std::min<long long>((tot + 255) / 256, ctx->limits.workgroups)),
                                   dim3(256), 0, ctx->stream, a.spec, nfreq, nchan, a.acc);
                SPY_HIP_CHECK(hipGetLastError());
                break;
            }
        }
        if (rc == -100) { spy::set_error("csd_accumulate: no 3M kernel for %d channels", s.n0 ? s.n0 : nchan); return -1; }
        if (rc) return rc;
    }
    return 0;
}

spycsd::CsdQuery make_query(const spyhip_ctx* ctx, int64_t nrows, int nfreq, int nchan, int blocked) {
    spycsd::CsdQuery q;
    q.nchan = nchan; q.nfreq = nfreq; q.nrows = nrows;
    q.blocked = blocked != 0;
    q.phase_exact = ctx->csd_phase_exact != 0;
    q.num_cu = ctx->num_cu;
    q.lds_per_block = ctx->lds_per_block;
    q.have_m3 = ctx->have_m3;       // (null in the library: csd3m_{a..h}.hip + csd3m_x.hip hold every width up to 512)
    return q;
}

int csd_accumulate_impl(spyhip_ctx* ctx, const void* spec_d, int64_t nrows, int nfreq, int nchan, void* acc_d, int blocked) {
    if (!ctx || !spec_d || !acc_d) { spy::set_error("csd_accumulate: null argument"); return -1; }
    if (nrows < 0 || nfreq < 1 || nchan < 1) { spy::set_error("csd_accumulate: bad shape"); return -1; }
    if (nrows == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    return run_route(ctx, spycsd::csd_route(make_query(ctx, nrows, nfreq, nchan, blocked)), spec_d, acc_d, nfreq, nchan, blocked);
}

}  // namespace

extern "C" int spyhip_csd_set_phase_exact(spyhip_ctx* ctx, int on) {
    if (!ctx) { spy::set_error("csd_set_phase_exact: null context"); return -1; }
    ctx->csd_phase_exact = on ? 1 : 0;
    return 0;
}

extern "C" int spyhip_csd_kernel_name(spyhip_ctx* ctx, int nchan, int blocked, char* buf, int cap) {
    if (!ctx || !buf || cap < 1 || nchan < 1) { spy::set_error("csd_kernel_name: null argument / bad shape"); return -1; }
    std::snprintf(buf, (size_t)cap, "%s", spycsd::csd_kernel_name(make_query(ctx, 1, 1, nchan, blocked), !env_f32()).c_str());
    return 0;
}

extern "C" int spyhip_csd_accumulate(spyhip_ctx* ctx, const void* spec_d, int64_t nrows, int nfreq, int nchan,
                                     void* acc_d) {
    if (ctx) ctx->k4h_nf = 0;
    return csd_accumulate_impl(ctx, spec_d, nrows, nfreq, nchan, acc_d, 0);
}

// K4h (csdh_kernel.h): 256 channels on the half-precision matrix cores with split float32 operands.  The frequencies
// beyond the last full round of workgroups go to the re-cut float32 tail like on the other paths (csd_route.h: csdh_route).
// [f0, f0 + nf): the frequencies of this call - a caller that wants the results of a range while the next is still being
// accumulated (the coherence pipeline: normalisation and host copy of range r under the products of range r + 1) launches
// range by range.
static int csd_accumulate_split_range(spyhip_ctx* ctx, const void* spec_d, int64_t nrows, int nfreq, int nchan, void* acc_d,
                                      const float* absmax_d, int f0, int nf) {
    if (!spec_d || !acc_d || nfreq < 1 || f0 < 0 || nf < 0 || f0 + nf > nfreq) {
        spy::set_error("csd_accumulate_split: null argument / bad shape");
        return -1;
    }
    if (nf == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    if (!ctx->k4h_done) SPY_HIP_CHECK(hipEventCreateWithFlags(&ctx->k4h_done, hipEventDisableTiming));
    else SPY_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->k4h_done, 0));      // the previous call's flag readers are through
    const size_t need = (size_t)nfreq * sizeof(int) + 256 * sizeof(float);
    if (need > ctx->k4h_bytes) {
        if (ctx->k4h_buf) { SPY_HIP_CHECK(hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->k4h_buf); ctx->k4h_buf = nullptr; ctx->k4h_bytes = 0; }
        SPY_HIP_CHECK(hipMalloc(&ctx->k4h_buf, need));
        SPY_HIP_CHECK(hipMemsetAsync(ctx->k4h_buf, 0, need, ctx->stream));      // (ranges not launched yet read as "not flagged")
        ctx->k4h_bytes = need;
    }
    float* const own_max = reinterpret_cast<float*>(ctx->k4h_buf);
    int* const flags = reinterpret_cast<int*>(own_max + 256);
    const float2* spec = reinterpret_cast<const float2*>(spec_d);
    if (!absmax_d) {
        SPY_HIP_CHECK(hipMemsetAsync(own_max, 0, 256 * sizeof(float), ctx->stream));
        int rc = spycsd::csdh_absmax(ctx->stream, spec, (long long)nrows * nfreq * 256, 256, own_max);
        if (rc) return rc;
        absmax_d = own_max;
    }
    const spycsd::CsdhRoute r = spycsd::csdh_route(make_query(ctx, nrows, nfreq, 256, 0), f0, nf);
    if (r.err) { spy::set_error("%s", r.message.c_str()); return r.err; }
    int rc = 0;
    if (r.h1 > r.h0)
        rc = spycsd::csdh_run(ctx->stream, spec, nrows, nfreq, reinterpret_cast<float2*>(acc_d), absmax_d, flags, r.h0, r.h1 - r.h0,
                              ctx->csd_phase_exact != 0);
    ctx->k4h_nf = r.f_main;
    if (!rc) SPY_HIP_CHECK(hipEventRecord(ctx->k4h_done, ctx->stream));         // (behind csdh_kernel and its only_flagged stand-in)
    if (rc) return rc;
    return run_route(ctx, r.tail, spec_d, acc_d, nfreq, 256, 0);
}

extern "C" int spyhip_csd_accumulate_split(spyhip_ctx* ctx, const void* spec_d, int64_t nrows, int nfreq, int nchan,
                                           void* acc_d, const float* absmax_d) {
    if (!ctx || nchan != 256 || nrows < 1 || env_f32()) {
        if (ctx) ctx->k4h_nf = 0;           // spyhip_csd_split_fallbacks reports THIS call: nothing went to the half-precision kernel
        return csd_accumulate_impl(ctx, spec_d, nrows, nfreq, nchan, acc_d, 0);
    }
    return csd_accumulate_split_range(ctx, spec_d, nrows, nfreq, nchan, acc_d, absmax_d, 0, nfreq);
}

extern "C" int spyhip_csd_accumulate_split_range(spyhip_ctx* ctx, const void* spec_d, int64_t nrows, int nfreq, int nchan,
                                                 void* acc_d, const float* absmax_d, int f0, int nf) {
    if (!ctx || nchan != 256 || nrows < 1 || env_f32() || !absmax_d) {
        spy::set_error("csd_accumulate_split_range: 256 channels, at least one row and the range of the spectra (absmax_d) are required");
        return -1;
    }
    return csd_accumulate_split_range(ctx, spec_d, nrows, nfreq, nchan, acc_d, absmax_d, f0, nf);
}

extern "C" int spyhip_csd_split_fallbacks(spyhip_ctx* ctx, int* count) {
    if (!ctx || !count) { spy::set_error("csd_split_fallbacks: null argument"); return -1; }
    *count = 0;
    if (!ctx->k4h_buf || ctx->k4h_nf <= 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    std::vector<int> h((size_t)ctx->k4h_nf);
    SPY_HIP_CHECK(hipMemcpyAsync(h.data(), reinterpret_cast<const char*>(ctx->k4h_buf) + 256 * sizeof(float), h.size() * sizeof(int),
                                 hipMemcpyDeviceToHost, ctx->stream));
    SPY_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int v : h) *count += v != 0;
    return 0;
}

extern "C" int spyhip_csd_accumulate_blocked(spyhip_ctx* ctx, const void* spec_d, int64_t nrows, int nfreq, int nchan,
                                             void* acc_d) {
    return csd_accumulate_impl(ctx, spec_d, nrows, nfreq, nchan, acc_d, 1);
}

extern "C" int spyhip_csd_finalize(spyhip_ctx* ctx, void* acc_d, int nfreq, int nchan, double scale) {
    if (!ctx || !acc_d) { spy::set_error("csd_finalize: null argument"); return -1; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const long long blocks = (long long)nfreq * spycsd::tri_tiles(nchan);
    if (blocks > 0x7fffffffLL) { spy::set_error("csd_finalize: grid too large"); return -1; }
    hipLaunchKernelGGL(spycsd::csd_finalize_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                       reinterpret_cast<float2*>(acc_d), nfreq, nchan, (float)scale);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_coh_from_accumulator(spyhip_ctx* ctx, const void* acc_d, int nfreq, int nchan, double scale,
                                           int output, void* out_d) {
    if (!ctx || !acc_d || !out_d) { spy::set_error("coh_from_accumulator: null argument"); return -1; }
    if (output < SPYHIP_OUT_POW || output > SPYHIP_OUT_ABSIMAG) { spy::set_error("coh_from_accumulator: bad output %d", output); return -1; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const long long blocks = (long long)nfreq * spycsd::tri_tiles(nchan);
    if (blocks > 0x7fffffffLL) { spy::set_error("coh_from_accumulator: grid too large"); return -1; }
    if (output == SPYHIP_OUT_FOURIER)
        hipLaunchKernelGGL(spycsd::coh_from_acc_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                           reinterpret_cast<const float2*>(acc_d), nfreq, nchan, (float)scale, output, out_d);
    else
        hipLaunchKernelGGL(spycsd::coh_from_acc_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                           reinterpret_cast<const float2*>(acc_d), nfreq, nchan, (float)scale, output, out_d);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

static int tril_move(spyhip_ctx* ctx, void* acc_d, int nfreq, int nchan, void* packed_d, bool unpack) {
    if (!ctx || !acc_d || !packed_d) { spy::set_error("csd_tril: null argument"); return -1; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const long long n = (long long)nfreq * nchan * nchan;
    const long long blocks = std::min<long long>((n + 255) / 256, 4 * ctx->limits.elementwise_blocks);
    if (unpack)
        hipLaunchKernelGGL(spycsd::csd_tril_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                           reinterpret_cast<float2*>(acc_d), reinterpret_cast<float2*>(packed_d), nfreq, nchan);
    else
        hipLaunchKernelGGL(spycsd::csd_tril_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                           reinterpret_cast<float2*>(acc_d), reinterpret_cast<float2*>(packed_d), nfreq, nchan);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_csd_tril_pack(spyhip_ctx* ctx, const void* acc_d, int nfreq, int nchan, void* packed_d) {
    return tril_move(ctx, const_cast<void*>(acc_d), nfreq, nchan, packed_d, false);
}

extern "C" int spyhip_csd_tril_unpack(spyhip_ctx* ctx, const void* packed_d, int nfreq, int nchan, void* acc_d) {
    return tril_move(ctx, acc_d, nfreq, nchan, const_cast<void*>(packed_d), true);
}

extern "C" int spyhip_coh_normalize(spyhip_ctx* ctx, const void* csd_d, int nfreq, int nchan, int output,
                                    void* out_d) {
    if (!ctx || !csd_d || !out_d) { spy::set_error("coh_normalize: null argument"); return -1; }
    if (output < SPYHIP_OUT_POW || output > SPYHIP_OUT_ABSIMAG) { spy::set_error("coh_normalize: bad output %d", output); return -1; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const long long n = (long long)nfreq * nchan * nchan;
    const long long blocks = std::min<long long>((n + 255) / 256, 2 * ctx->limits.elementwise_blocks);
    if (output == SPYHIP_OUT_FOURIER)
        hipLaunchKernelGGL(spycsd::coh_normalize_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                           reinterpret_cast<const float2*>(csd_d), nfreq, nchan, output, out_d);
    else
        hipLaunchKernelGGL(spycsd::coh_normalize_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                           reinterpret_cast<const float2*>(csd_d), nfreq, nchan, output, out_d);
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

#include "jack_kernel.h"

extern "C" int spyhip_jack_coh_accumulate(spyhip_ctx* ctx, const void* spec_d, int ntrials, int ntaper, int nfreq,
                                          int nchan, const void* csd_d, const void* direct_d, int output,
                                          int64_t ntrials_total, void* sum_d, void* sum_d2) {
    if (!ctx || !spec_d || !csd_d || !direct_d || !sum_d || !sum_d2) { spy::set_error("jack_coh_accumulate: null argument"); return -1; }
    if (ntrials < 0 || ntaper < 1 || nfreq < 1 || nchan < 1 || ntrials_total < 2) { spy::set_error("jack_coh_accumulate: bad shape"); return -1; }
    if (output < SPYHIP_OUT_POW || output > SPYHIP_OUT_ABSIMAG) { spy::set_error("bad output kind %d", output); return -1; }
    if (ntrials == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    spycsd::JackArgs a{};
    a.spec = reinterpret_cast<const float2*>(spec_d);
    a.S = reinterpret_cast<const float2*>(csd_d);
    a.direct = direct_d;
    a.ntrials = ntrials; a.K = ntaper; a.F = nfreq; a.C = nchan; a.kind = output;
    a.T = (float)ntrials_total;
    a.sum_d = reinterpret_cast<double*>(sum_d);
    a.sum_d2 = reinterpret_cast<double*>(sum_d2);
    const long long blocks = 8LL * ((nfreq + 7) / 8) * spycsd::tri_tiles(nchan);
    if (blocks > 0x7fffffffLL) { spy::set_error("jack_coh_accumulate: grid too large"); return -1; }
    const size_t lds = 2 * (size_t)2 * ntaper * 32 * sizeof(float2);
    if (lds > ctx->lds_per_block) { spy::set_error("jack_coh_accumulate: %d tapers do not fit the LDS staging buffer", ntaper); return -3; }
    if (output == SPYHIP_OUT_FOURIER) {
        SPY_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(spycsd::jack_coh_kernel<true>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(spycsd::jack_coh_kernel<true>, dim3((unsigned)blocks), dim3(256), lds, ctx->stream, a);
    } else {
        SPY_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(spycsd::jack_coh_kernel<false>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(spycsd::jack_coh_kernel<false>, dim3((unsigned)blocks), dim3(256), lds, ctx->stream, a);
    }
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}
