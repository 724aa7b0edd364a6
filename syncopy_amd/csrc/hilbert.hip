// The Hilbert option of spy.preprocessing (spyhip_hilbert_plan_create / spyhip_hilbert_exec of include/spyhip.h): plan
// objects that own the tables of one trial length, and the launches of the family hilbert_route.h names for it.
#include "hilbert_launch.h"
#include "host_fft.h"

#include <climits>
#include <memory>

struct spyhip_hilbert_plan {
    spyhip_ctx* ctx = nullptr;
    int64_t nsamp = 0;
    spyhil::Route r;
    spy::DevBuf<float2> tw, chirp, bhat;            // PACKED, BLUE
    spy::DevBuf<double2> tw64, chirp64, bhat64;     // ANY64
};

namespace {

using spyhil::Family;

int exec_packed(spyhip_hilbert_plan* p, spyhil::HilArgs& a, bool cplx) {
    const spyhil::Route& r = p->r;
    // offsets inside one trial are 32-bit byte offsets of the wider of the two arrays
    if ((int64_t)a.nsamp * a.nchan * 8 > (int64_t)UINT_MAX) {
        spy::set_error("hilbert_exec: %d samples x %d channels per trial (at most 2^29 - 1 elements at this length)", a.nsamp, a.nchan);
        return -1;
    }
    const spyhil::PackedGrid g = spyhil::packed_grid(a.ntrials, a.nchan, r.G);
    if (!g.grid) { spy::set_error("hilbert_exec: grid too large (%d trials x %d channels)", a.ntrials, a.nchan); return -1; }
    a.npg = g.npg; a.S = g.S; a.ncl = g.ncl;
    a.tw = p->tw.p; a.chirp = p->chirp.p; a.bhat = p->bhat.p;
    a.inv_n = 1.0f / (float)a.nsamp;
    const int rc = r.family == Family::BLUE ? spyhil::launch_blue(p->ctx->stream, a, r.log2n, cplx, g.grid)
                                            : spyhil::launch_packed(p->ctx->stream, a, r.log2n, cplx, g.grid);
    if (rc == spyhil::NO_INSTANCE) { spy::set_error("hilbert_exec: no kernel instance for %s", r.kernel_name.c_str()); return -1; }
    return rc;
}

int exec_any64(spyhip_hilbert_plan* p, const spyhil::HilArgs& h, bool cplx) {
    const spyhil::Route& r = p->r;
    spyhil::HilArgs64 a{};
    a.in = h.in; a.out = h.out; a.nan = h.nan;
    a.ntrials = h.ntrials; a.nsamp = h.nsamp; a.nchan = h.nchan; a.kind = h.kind;
    a.blue = r.bluestein ? 1 : 0;
    a.plan = r.plan;
    a.tw = p->tw64.p; a.chirp = p->chirp64.p; a.bhat = p->bhat64.p;
    const long long total = (long long)h.ntrials * ((h.nchan + 1) / 2);
    long long chunk = spyhil::any64_chunk(r.M);
    if (chunk > p->ctx->limits.any64_chunk) chunk = p->ctx->limits.any64_chunk;
    if (chunk > total) chunk = total;
    if (spy::reserve_scratch(p->ctx, (size_t)chunk * 2 * (size_t)r.M * sizeof(double2))) return -2;
    a.work = reinterpret_cast<double2*>(p->ctx->scratch);
    for (long long w0 = 0; w0 < total; w0 += chunk) {       // launches on one stream: each owns the work arrays in turn
        a.wg0 = w0;
        const unsigned g = (unsigned)(total - w0 < chunk ? total - w0 : chunk);
        if (cplx) hipLaunchKernelGGL(spyhil::hilbert_any64_kernel<true>, dim3(g), dim3(256), 0, p->ctx->stream, a);
        else hipLaunchKernelGGL(spyhil::hilbert_any64_kernel<false>, dim3(g), dim3(256), 0, p->ctx->stream, a);
        SPY_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" int spyhip_hilbert_plan_create(spyhip_ctx* ctx, int64_t nsamp, spyhip_hilbert_plan** out) {
    if (!ctx || !out) { spy::set_error("hilbert_plan_create: bad argument"); return -1; }
    *out = nullptr;
    std::unique_ptr<spyhip_hilbert_plan> p(new spyhip_hilbert_plan);
    p->ctx = ctx;
    p->nsamp = nsamp;
    p->r = spyhil::hilbert_route(nsamp);
    const spyhil::Route& r = p->r;
    if (r.err) { spy::set_error("%s", r.message.c_str()); return r.err; }
    SPY_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int N = (int)nsamp;
    if (r.family == Family::PACKED || r.family == Family::BLUE) {
        if (r.lds_bytes > ctx->lds_per_block) {
            spy::set_error("hilbert_plan_create: %s needs %zu bytes of LDS (> %zu)", r.kernel_name.c_str(), r.lds_bytes, ctx->lds_per_block);
            return -3;
        }
        if (p->tw.upload(spy::twiddle_table<float2>(r.M), s)) return -2;
        if (r.family == Family::BLUE) {
            std::vector<float2> chirp, bhat;
            spy::bluestein_tables(N, r.M, 0, &chirp, &bhat);
            if (p->chirp.upload(chirp, s) || p->bhat.upload(bhat, s)) return -2;
        }
    } else if (r.family == Family::ANY64) {
        if (p->tw64.upload(spy::twiddle_table<double2>(r.M), s)) return -2;
        if (r.bluestein) {
            std::vector<double2> chirp, bhat;
            spy::bluestein_tables(N, r.M, 0, &chirp, &bhat);
            if (p->chirp64.upload(chirp, s) || p->bhat64.upload(bhat, s)) return -2;
        }
    }
    *out = p.release();
    return 0;
}

extern "C" int spyhip_hilbert_plan_destroy(spyhip_hilbert_plan* p) {
    delete p;
    return 0;
}

extern "C" const char* spyhip_hilbert_plan_kernel_name(const spyhip_hilbert_plan* p) {
    return p ? p->r.kernel_name.c_str() : "";
}

extern "C" int spyhip_hilbert_exec(spyhip_hilbert_plan* p, const float* in_d, void* out_d, int64_t ntrials, int64_t nchan,
                                   int output, int* nan_d) {
    if (!p || !in_d || !out_d || !nan_d || static_cast<const void*>(in_d) == out_d) { spy::set_error("hilbert_exec: bad argument"); return -1; }
    if (output < SPYHIP_OUT_ABS || output > SPYHIP_OUT_ABSIMAG) { spy::set_error("hilbert_exec: output kind %d", output); return -1; }
    if (ntrials < 0 || nchan < 1 || ntrials > INT_MAX || nchan > INT_MAX / 2) {
        spy::set_error("hilbert_exec: %lld trials x %lld channels", (long long)ntrials, (long long)nchan);
        return -1;
    }
    if (ntrials == 0) return 0;
    SPY_HIP_CHECK(hipSetDevice(p->ctx->device));
    const bool cplx = output == SPYHIP_OUT_FOURIER;
    spyhil::HilArgs a{};
    a.in = in_d; a.out = out_d; a.nan = nan_d;
    a.ntrials = (int)ntrials; a.nsamp = (int)p->nsamp; a.nchan = (int)nchan; a.kind = output;
    switch (p->r.family) {
        case Family::COPY: {
            const long long n = (long long)ntrials * nchan;
            if ((n + 255) / 256 > INT_MAX) { spy::set_error("hilbert_exec: %lld trials x %lld channels", (long long)ntrials, (long long)nchan); return -1; }
            const dim3 g((unsigned)((n + 255) / 256)), b(256);
            if (cplx) hipLaunchKernelGGL(spyhil::hilbert_copy_kernel<true>, g, b, 0, p->ctx->stream, a);
            else hipLaunchKernelGGL(spyhil::hilbert_copy_kernel<false>, g, b, 0, p->ctx->stream, a);
            SPY_HIP_CHECK(hipGetLastError());
            return 0;
        }
        case Family::ANY64: return exec_any64(p, a, cplx);
        default: return exec_packed(p, a, cplx);
    }
}
