// Host side of K3 (spyhip_cwt_plan_create / spyhip_cwt_exec): validation, uploads of the tables the route describes
// (cwt_route.h: taps, groups, staging rows) and a loop that walks the route's steps.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <string>

#include "spy_common.h"
#include "cwt_launch.h"

using spyfft::CwtArgs;

// device tables of one group of scales (spycwt::Group)
struct CwtGroupTables {
    spy::DevBuf<float2> tw, hspec;
    spy::DevBuf<int> cshift, sidx;
    spy::DevBuf<int> sidx_stage;   // with direct groups: scale s of this launch -> row of the (compact) staging buffer
};
using CwtGroupSet = std::vector<std::unique_ptr<CwtGroupTables>>;

struct spyhip_cwt_plan {
    spyhip_ctx* ctx = nullptr;
    spycwt::Plan r;               // the host description: groups, pieces, staging rows (cwt_route.h)
    int ntime_out = 0;
    // the sampled kernels are kept on the host: trial sums of long signals take their own groups (Plan::groups_sum), built
    // at the first such call, and reference precision its float64 spectra, built when asked for
    std::vector<spycwt::Taps> taps;
    CwtGroupSet groups, groups_sum;
    bool identity_time = true;
    spy::DevBuf<int> tpos, tfloor;
    spy::DevBuf<float> xt;        // channel-major copy of the chunk's pre-selected signals (cwt_stage_input_kernel)
    spy::DevBuf<double> trend, trend_part;
    spy::DevBuf<char> stage;      // time-contiguous staging of one chunk of segments
    bool direct = true;           // spyhip_cwt_plan_set_direct: groups flagged `direct` skip the staging buffer
    spy::DevBuf<int> smap;        // staging row -> scale index (device copy of Plan::staged)
    spy::DevBuf<int> lidx_stage;  // long scale -> staging row
    spy::DevBuf<int> lidx;        // the long scales' indices on the device
    spy::DevBuf<float2> stage_long;   // (chunk, long scale, channel, time) complex sums of the pieces (real outputs)
    // reference precision (spyhip_cwt_plan_set_precision, cwt64_kernel.h)
    bool precision64 = false;
    int L64 = 0;
    spywil::PlusPlan plan64{};
    spy::DevBuf<double2> tw64, hspec64, work64;
    spy::DevBuf<int> centre64;
};

// twiddles, kernel spectra and index tables of every group of `set`
static int upload_groups(spyhip_cwt_plan* p, const std::vector<spycwt::Group>& set, CwtGroupSet& out) {
    const hipStream_t s = p->ctx->stream;
    for (const spycwt::Group& g : set) {
        const size_t NB = (size_t)1 << g.log2n;
        std::vector<float2> hs(g.nscales() * NB);
        for (int q = 0; q < g.nscales(); ++q) {
            const spycwt::Taps& k = p->taps[g.scale_ids[q]];
            const bool piece = g.long_idx >= 0;
            spycwt::kernel_spectrum(k, piece ? g.tap0 : 0, piece ? g.ntaps : k.re.size(), NB, &hs[q * NB]);
        }
        out.emplace_back(new CwtGroupTables());
        CwtGroupTables& d = *out.back();
        if (d.tw.upload(spy::twiddle_table<float2>((int)NB), s) || d.hspec.upload(hs, s) || d.cshift.upload(g.cshift, s) ||
            d.sidx.upload(g.sidx, s) || (!g.sidx_stage.empty() && d.sidx_stage.upload(g.sidx_stage, s)))
            return -2;
    }
    return 0;
}

static int cwt_plan_create_impl(spyhip_ctx* ctx, int nsig, int nchan, int nscales, const double* scales, double dt,
                                int family, double p0, double p1, int detrend, int output, const int32_t* tpos,
                                int ntime_out, spyhip_cwt_plan** out);

extern "C" int spyhip_cwt_plan_create(spyhip_ctx* ctx, int nsig, int nchan, int nscales, const double* scales,
                                      double dt, double w0, int detrend, int output, const int32_t* tpos,
                                      int ntime_out, spyhip_cwt_plan** out) {
    return cwt_plan_create_impl(ctx, nsig, nchan, nscales, scales, dt, 0, w0, 0.0, detrend, output, tpos, ntime_out, out);
}

extern "C" int spyhip_cwt_plan_create_family(spyhip_ctx* ctx, int nsig, int nchan, int nscales, const double* scales,
                                             double dt, int family, double p0, double p1, int detrend, int output,
                                             const int32_t* tpos, int ntime_out, spyhip_cwt_plan** out) {
    if (family < 0 || family > 3) { spy::set_error("cwt_plan_create_family: family %d (0 Morlet, 1 MorletSL, 2 Paul, 3 DOG)", family); return -1; }
    if (family == 1 && (!(p0 > 0) || !(p1 > 0))) { spy::set_error("cwt_plan_create_family: cycles and k_sd must be positive"); return -1; }
    if (family >= 2 && (p0 < 1 || p0 > 60 || p0 != std::floor(p0))) { spy::set_error("cwt_plan_create_family: order m = %g (integer 1 ... 60)", p0); return -1; }
    return cwt_plan_create_impl(ctx, nsig, nchan, nscales, scales, dt, family, p0, p1, detrend, output, tpos, ntime_out, out);
}

extern "C" int spyhip_cwt_plan_create_sl(spyhip_ctx* ctx, int nsig, int nchan, int nscales, const double* scales,
                                         double dt, double cycles, double k_sd, int detrend, int output,
                                         const int32_t* tpos, int ntime_out, spyhip_cwt_plan** out) {
    if (!(cycles > 0) || !(k_sd > 0)) { spy::set_error("cwt_plan_create_sl: cycles and k_sd must be positive"); return -1; }
    return cwt_plan_create_impl(ctx, nsig, nchan, nscales, scales, dt, 1, cycles, k_sd, detrend, output, tpos,
                                ntime_out, out);
}

// (family, p0, p1: spycwt::sample_taps)
static int cwt_plan_create_impl(spyhip_ctx* ctx, int nsig, int nchan, int nscales, const double* scales, double dt,
                                int family, double p0, double p1, int detrend, int output, const int32_t* tpos,
                                int ntime_out, spyhip_cwt_plan** out) {
    if (!ctx || !scales || !out) { spy::set_error("cwt_plan_create: null argument"); return -1; }
    if (nsig < 1 || nchan < 1 || nscales < 1 || dt <= 0) { spy::set_error("cwt_plan_create: bad shape"); return -1; }
    if (output < SPYHIP_OUT_POW || output > SPYHIP_OUT_ABSIMAG) { spy::set_error("bad output kind %d", output); return -1; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    std::unique_ptr<spyhip_cwt_plan> p(new spyhip_cwt_plan());
    p->ctx = ctx;
    std::vector<int> ntaps, centre;
    for (int s = 0; s < nscales; ++s) {
        p->taps.push_back(spycwt::sample_taps(family, p0, p1, scales[s], dt, nsig));
        ntaps.push_back((int)p->taps[s].re.size());
        centre.push_back(p->taps[s].c);
    }
    p->r = spycwt::plan_route(nsig, nchan, output, detrend, ntaps, centre, tpos);
    if (p->r.err) { spy::set_error("%s", p->r.message.c_str()); return p->r.err; }
    const hipStream_t st = ctx->stream;
    if (upload_groups(p.get(), p->r.groups, p->groups)) return -2;
    if (!p->r.long_scales.empty() && (p->lidx.upload(p->r.long_scales, st) || p->lidx_stage.upload(p->r.lrow, st))) return -2;
    if (!p->r.staged.empty() && p->smap.upload(p->r.staged, st)) return -2;
    p->identity_time = (tpos == nullptr);
    p->ntime_out = tpos ? ntime_out : nsig;
    if (tpos) {
        std::vector<int> tp(tpos, tpos + nsig);
        for (int v : tp)
            if (v >= ntime_out) { spy::set_error("cwt_plan_create: tpos entry %d >= ntime_out %d", v, ntime_out); return -1; }
        // the direct kernels address a tile relative to the slot reached before it (cwt_direct_fits)
        if (p->tpos.upload(tp, st) || p->tfloor.upload(spycwt::tfloor(tpos, nsig), st)) return -2;
    }
    p->direct = p->r.direct_ok;
    *out = p.release();
    return 0;
}

extern "C" int spyhip_cwt_plan_set_precision(spyhip_cwt_plan* p, int reference) {
    if (!p) { spy::set_error("cwt_plan_set_precision: null plan"); return -1; }
    if (!reference) { p->precision64 = false; return 0; }
    if (!p->hspec64.p) {
        SPY_HIP_CHECK(hipSetDevice(p->ctx->device));
        const long long L = spycwt::conv_length64(p->r.nsig, p->r.ntaps);
        if (L > spycwt::MAX_L64) { spy::set_error("cwt_plan_set_precision: convolution length %lld beyond 2^22", L); return -3; }
        p->L64 = (int)L;
        if (!spywil::plus_plan(p->L64, &p->plan64)) { spy::set_error("cwt_plan_set_precision: no radix schedule"); return -3; }
        std::vector<double2> hs((size_t)p->r.nscales * L);
        for (int sc = 0; sc < p->r.nscales; ++sc)
            spycwt::kernel_spectrum(p->taps[sc], 0, p->taps[sc].re.size(), (size_t)L, &hs[(size_t)sc * L]);
        if (p->tw64.upload(spy::twiddle_table<double2>(p->L64), p->ctx->stream) || p->hspec64.upload(hs, p->ctx->stream) ||
            p->centre64.upload(p->r.centre, p->ctx->stream)) return -2;
    }
    p->precision64 = true;
    return 0;
}

extern "C" int spyhip_cwt_plan_destroy(spyhip_cwt_plan* p) {
    delete p;
    return 0;
}

// what a call of `nseg` segments asks of the route: the plan's options, the chip and the launch limits of its context
static spycwt::ExecQuery exec_query(const spyhip_cwt_plan* p, int nseg, int accumulate) {
    spycwt::ExecQuery q;
    q.nseg = nseg; q.accumulate = accumulate; q.direct = p->direct; q.precision64 = p->precision64; q.L64 = p->L64;
    q.num_cu = p->ctx->num_cu;
    const spyhip_limits& lim = p->ctx->limits;
    if (lim.cwt_stage_bytes > 0) q.stage_budget = (size_t)lim.cwt_stage_bytes;
    if (lim.cwt_work64_bytes > 0) q.work_budget = (size_t)lim.cwt_work64_bytes;
    return q;
}

extern "C" int spyhip_cwt_exec(spyhip_cwt_plan* p, const float* data_d, int64_t ld, const int32_t* chan_idx_d,
                               const int64_t* seg_start_d, const int64_t* trial_lo_d, const int64_t* trial_hi_d,
                               int nseg, void* out_d, int accumulate) {
    using namespace spycwt;
    if (!p || !data_d || !seg_start_d || !trial_lo_d || !trial_hi_d || !out_d) { spy::set_error("cwt_exec: null argument"); return -1; }
    if (nseg <= 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(p->ctx->device));
    const hipStream_t st = p->ctx->stream;
    const Plan& pl = p->r;
    const ExecRoute r = exec_route(pl, exec_query(p, nseg, accumulate));
    if (r.sum_set && p->groups_sum.empty() && upload_groups(p, pl.groups_sum, p->groups_sum)) {
        p->groups_sum.clear();
        return -2;
    }
    if (p->trend.reserve(r.trend, st) || p->trend_part.reserve(r.trend * TREND_SPLITS, st) || p->stage.reserve(r.stage_bytes, st) ||
        p->stage_long.reserve(r.stage_long, st) || p->xt.reserve(r.xt, st) || p->work64.reserve(r.work64, st))
        return -2;
    static_assert(TREND_SPLITS == spyfft::CWT_TREND_SPLITS, "the route sizes the partial trend sums");
    const std::vector<Group>& groups = r.sum_set ? pl.groups_sum : pl.groups;
    const CwtGroupSet& tables = r.sum_set ? p->groups_sum : p->groups;
    CwtArgs a{};
    a.data = data_d; a.ld = ld; a.chan_idx = chan_idx_d;
    a.nsig = pl.nsig; a.nchan = pl.nchan; a.nscales = pl.nscales;
    a.nscales_total = pl.nscales;
    a.detrend = pl.detrend; a.out_kind = pl.output;
    a.tpos = p->identity_time ? nullptr : p->tpos.p;
    a.tfloor = p->identity_time ? nullptr : p->tfloor.p;
    a.ntime_out = p->ntime_out; a.out = out_d; a.accumulate = accumulate;
    a.stage = p->stage.p;
    for (const Step& s : r.steps) {
        CwtArgs c = a;                               // the step's segments: the whole call, or one chunk
        c.seg0 = s.seg0; c.nseg = s.nseg;
        c.seg_start = reinterpret_cast<const long long*>(seg_start_d) + s.seg0;
        c.trial_lo = reinterpret_cast<const long long*>(trial_lo_d) + s.seg0;
        c.trial_hi = reinterpret_cast<const long long*>(trial_hi_d) + s.seg0;
        if (pl.detrend >= 0) c.trend = p->trend.p + (size_t)s.seg0 * pl.nchan * 2;
        if (r.xt && s.kind == StepKind::TRANSFORM) c.xt = p->xt.p;
        const dim3 grid((unsigned)s.gx, (unsigned)s.gy, (unsigned)s.gz);
        switch (s.kind) {
            case StepKind::MEAN_NP:
                hipLaunchKernelGGL(spyfft::cwt_mean_np_kernel, grid, dim3(64), 0, st, c, p->trend.p);
                break;
            case StepKind::TREND:
                hipLaunchKernelGGL(spyfft::cwt_trend_partial_kernel, grid, dim3(256), 0, st, c, p->trend_part.p);
                hipLaunchKernelGGL(spyfft::cwt_trend_final_kernel, dim3((unsigned)(((size_t)nseg * pl.nchan + 255) / 256)), dim3(256),
                                   0, st, c, p->trend_part.p, p->trend.p);
                break;
            case StepKind::INPUT_COPY:
                hipLaunchKernelGGL(spyfft::cwt_stage_input_kernel, grid, dim3(256), 0, st, c, p->xt.p);
                break;
            case StepKind::CWT64: {
                spyfft::Cwt64Args fa{};
                fa.c = c;
                fa.L = p->L64; fa.plan = p->plan64; fa.tw64 = p->tw64.p; fa.hspec64 = p->hspec64.p; fa.centre = p->centre64.p;
                fa.work = p->work64.p; fa.wg0 = s.wg0;
                with_cwt64_kernel(s.outk, [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, fa); return 0; });
                break;
            }
            case StepKind::TRANSFORM: {
                const Group& gr = groups[s.group];
                const CwtGroupTables& t = *tables[s.group];
                c.nscales = gr.nscales();
                c.sidx = s.sidx == Sidx::COMPACT ? t.sidx_stage.p : t.sidx.p;
                c.nscales_total = s.nrows;
                c.tw = t.tw.p; c.hspec = t.hspec.p; c.cshift = t.cshift.p;
                c.V = gr.V; c.halo = gr.halo; c.nblocks = gr.nblocks;
                c.stage_add = s.add;
                if (s.target == Target::LONG_SIDE) c.stage = p->stage_long.p;
                const int rc = with_transform_kernel(gr.log2n, s.engine, s.outk, [&](auto kern, int threads, size_t lds) {
                    SPY_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                    hipLaunchKernelGGL(kern, grid, dim3(threads), lds, st, c);
                    return 0;
                });
                if (rc == -1) spy::set_error("cwt_exec: unsupported block length 2^%d", gr.log2n);
                if (rc) return rc;
                break;
            }
            case StepKind::LONG_CONVERT:
                hipLaunchKernelGGL(spyfft::cwt_long_convert_kernel, grid, dim3(256), 0, st, p->stage_long.p,
                                   s.sidx == Sidx::COMPACT ? p->lidx_stage.p : p->lidx.p, (int)pl.long_scales.size(), s.nseg, s.nrows,
                                   pl.nchan, pl.nsig, pl.output, reinterpret_cast<float*>(p->stage.p));
                break;
            case StepKind::SCATTER:
                c.nseg = s.nsets;                     // row sets to add up ...
                c.nscales = s.nrows;                  // ... staging rows per row set ...
                if (s.compact) { c.smap = p->smap.p; c.nscales_out = pl.nscales; }      // ... and where they go in the output
                with_scatter_kernel(s.scatter, [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, c); return 0; });
                break;
        }
        SPY_HIP_CHECK(hipGetLastError());
    }
    if (r.err) spy::set_error("%s", r.message.c_str());
    return r.err;
}

extern "C" int spyhip_cwt_plan_set_direct(spyhip_cwt_plan* p, int on) {
    if (!p) { spy::set_error("cwt_plan_set_direct: null plan"); return -1; }
    if (on && !p->r.direct_ok) {                   // (slots not increasing / tiles beyond 32-bit offsets: staging only)
        spy::set_error("cwt_plan_set_direct: this plan's outputs cannot be written by the transform kernels (time slots not "
                       "increasing with the samples, or a tile's slots spanning 4 GiB or more of the output)");
        return -3;
    }
    p->direct = on != 0;
    return 0;
}

extern "C" int spyhip_slt_combine(spyhip_ctx* ctx, void* acc_d, const void* spec_d, int64_t nrows, int nscales,
                                  int nsub, int s0, int nchan, const double* expo, int init, int modulus_only) {
    if (!ctx || !acc_d || !spec_d || !expo) { spy::set_error("slt_combine: null argument"); return -1; }
    if (nrows < 0 || nscales < 1 || nsub < 1 || s0 < 0 || s0 + nsub > nscales || nchan < 1) {
        spy::set_error("slt_combine: bad shape");
        return -1;
    }
    if (nrows == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    // the kernel takes <= SLT_MAX_SCALES exponents by value: wider scale sets go in slices
    for (int q0 = 0; q0 < nsub; q0 += spyfft::SLT_MAX_SCALES) {
        const int nq = std::min(spyfft::SLT_MAX_SCALES, nsub - q0);
        spyfft::SltArgs a{};
        a.acc = reinterpret_cast<float2*>(acc_d);
        a.spec = reinterpret_cast<const float2*>(spec_d);
        a.nrows = nrows; a.nscales = nscales; a.nsub = nq; a.s0 = s0 + q0; a.nchan = nchan; a.init = init;
        a.nsub_total = nsub; a.q0 = q0; a.modulus_only = modulus_only & 3; a.square = (modulus_only >> 2) & 1;
        for (int q = 0; q < nq; ++q) a.expo[q] = expo[q0 + q];
        const long long blocks = ((long long)nrows * nq * nchan + 255) / 256;
        if (blocks > 0x7fffffffLL) { spy::set_error("slt_combine: grid too large"); return -1; }
        hipLaunchKernelGGL(spyfft::slt_combine_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, a);
    }
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int spyhip_spec_convert(spyhip_ctx* ctx, const void* in_d, int64_t n, int output, void* out_d) {
    if (!ctx || !in_d || !out_d) { spy::set_error("spec_convert: null argument"); return -1; }
    if (output < SPYHIP_OUT_POW || output > SPYHIP_OUT_ABSIMAG || output == SPYHIP_OUT_FOURIER) {
        spy::set_error("spec_convert: %d is not a real output kind", output);
        return -1;
    }
    if (n <= 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    const long long blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffLL) { spy::set_error("spec_convert: grid too large"); return -1; }
    hipLaunchKernelGGL(spyfft::spec_convert_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const float2*>(in_d), (long long)n, output, reinterpret_cast<float*>(out_d));
    SPY_HIP_CHECK(hipGetLastError());
    return 0;
}
