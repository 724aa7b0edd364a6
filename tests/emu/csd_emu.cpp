// CPU emulation of the cross-spectral stage (K4, K5, K9 and K7), TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's
// own launchers (syncopy_amd/csrc/csd.hip, ppc.hip) and kernels, on the runtime stand-in hip/hip_runtime.h.  The 3M entry
// points of csd3m_launch.h are defined here over the emulator's sample of widths (emu_m3_widths.h), each through the
// library's m3_launch_one.  K4h, the fp16 matrix-core kernel, has no CPU model: its two entry points refuse with
// EMU_NOT_EMULATED, and no other kernel runs in its place.  Built by __graft_entry__.build() and tests/csd_drive.py.
#include "hip_emu.h"

#include "../../syncopy_amd/csrc/csd.hip"
#include "../../syncopy_amd/csrc/ppc.hip"
#include "../../syncopy_amd/csrc/csd3m_launch_impl.h"
#include "emu_unit.h"

namespace spycsd {

int m3_launch_padded(int chp, hipStream_t stream, CsdArgs a, long long nprow) {
    switch (chp) {
#define EMU_M3(CH) case CH: return m3_launch_one<CH, false>(stream, a, nprow);
        EMU_M3_WIDTHS(EMU_M3)
#undef EMU_M3
        default: return -100;
    }
}
int m3_launch(int nchan, hipStream_t stream, CsdArgs a, long long nprow) {
    return nchan == 256 ? m3_launch_one<256>(stream, a, nprow) : m3_launch_padded(m3_padded(nchan), stream, a, nprow);
}
int m3_launch_rect(hipStream_t stream, CsdArgs a, long long nfreq) { return m3_launch_one<512, false, true>(stream, a, nfreq); }
int m4_launch_rect(hipStream_t stream, CsdArgs a, long long nfreq) { return m3_launch_one<512, false, true, true>(stream, a, nfreq); }
int m4_launch_block(hipStream_t stream, CsdArgs a, long long nfreq) { return m3_launch_one<256, false, false, true>(stream, a, nfreq); }

int csdh_run(hipStream_t, const float2*, long long, int, float2*, const float*, int*, int, int, bool) { return EMU_NOT_EMULATED; }
int csdh_absmax(hipStream_t, const float2*, long long, int, float*) { return EMU_NOT_EMULATED; }

}  // namespace spycsd

// A code for the first step of the route spyhip_csd_accumulate[_blocked] takes for this update (the call
// csd_accumulate_impl makes): 1 / 3 / 5 generic tiles per wave, 6 the instruction-lean path, 7 its wide variant, 8 / 9 the
// 3M kernel (exact 256 / padded), 10 / 11 the 256-channel block walk (3M / 4M); 0 nothing to launch, < 0 the route's error.
// first: what that step says of its launch - workgroups (-1 where the launcher derives them), threads, dynamic LDS bytes.
extern "C" int emu_csd_kernel_code(spyhip_ctx* ctx, long long nrows, int nfreq, int nchan, int blocked, long long* first) {
    const spycsd::CsdRoute r = spycsd::csd_route(make_query(ctx, nrows, nfreq, nchan, blocked));
    if (r.err || r.steps.empty()) return r.err;
    const CsdStep& s0 = r.steps.front();
    const bool tiled = s0.kind == StepKind::ACCUM, rank1 = s0.kind == StepKind::RANK1;
    first[0] = tiled ? s0.geo.grid : -1;
    first[1] = tiled ? spycsd::CSD_THREADS : rank1 ? 256 : 512;
    first[2] = tiled ? (long long)s0.geo.lds : rank1 ? 0 : spycsd::M3_LDS_BYTES;
    switch (s0.kind) {
        case StepKind::ACCUM: return s0.fast == 3 ? 7 : s0.fast ? 6 : s0.ta;
        case StepKind::M3_EXACT: return 8;
        case StepKind::M3_PADDED: return s0.n0 ? 10 : 9;
        case StepKind::M4_BLOCK: return 11;
        case StepKind::RANK1: return ctx->csd_phase_exact ? 11 : 10;
        default: return -1;
    }
}

// The test-only choice of csd_accum_kernel<ta, ta - 1> (1: <1, 1>) without asking the route - a shape the route gives to
// another kernel still reaches the generic one -, launched by the library's launch_accum with the geometry of accum_geometry.
extern "C" int emu_csd_accumulate_tpw(spyhip_ctx* ctx, const void* spec, long long nrows, int nfreq, int nchan, void* acc, int ta) {
    if ((ta != 1 && ta != 3 && ta != 5) || nrows < 0 || nfreq < 1 || nchan < 1) return -1;
    CsdArgs a{};
    a.F = nfreq; a.C = nchan;
    a.spec = reinterpret_cast<const float2*>(spec);
    a.acc = reinterpret_cast<float2*>(acc);
    a.nrows = nrows;
    a.nt = (nchan + 31) / 32; a.ntiles = (int)spycsd::tri_tiles(nchan); a.cpad = a.nt * 32;
    a.nitems = a.item_end = (long long)nfreq * a.ntiles;
    CsdStep s{StepKind::ACCUM};
    s.ta = ta;
    s.geo = spycsd::accum_geometry(ta, ta == 1 ? 1 : ta - 1, 0, a.ntiles, a.cpad, nfreq, nrows, 0, 0, ctx->lds_per_block, a.nitems);
    if (s.geo.err) return s.geo.err;
    return nrows > 0 ? launch_accum(ctx, a, s) : 0;
}
