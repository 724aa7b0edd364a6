// What every emulator unit that includes the library's own .hip files needs besides them, TEST INFRASTRUCTURE ONLY (see
// hip_emu.h): the emulator's thread-locals, the library's error sink, and a context for the tests.  Include it once, in
// the unit's one translation unit, with tests/emu on the include path (so that <hip/hip_runtime.h> is hip/hip_runtime.h).
#pragma once
#include "../../syncopy_amd/csrc/spy_common.h"
#include "emu_m3_widths.h"

namespace emu {
thread_local dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
thread_local BlockCtx* t_ctx = nullptr;
}  // namespace emu

void spy::set_error(const char*, ...) {}

// what a unit's stand-in for a part of the library without a CPU model returns: nothing else runs in its place
constexpr int EMU_NOT_EMULATED = -101;

// A context for the tests, the only writer of the launch limits: a value > 0 replaces the library's default.  The 3M
// instances it answers for are the emulator's sample.
extern "C" spyhip_ctx* emu_ctx(long long grid_yz, long long elementwise_blocks, long long workgroups, long long any64_chunk) {
    spyhip_ctx* ctx = new spyhip_ctx;
    if (grid_yz > 0) ctx->limits.grid_yz = grid_yz;
    if (elementwise_blocks > 0) ctx->limits.elementwise_blocks = elementwise_blocks;
    if (workgroups > 0) ctx->limits.workgroups = workgroups;
    if (any64_chunk > 0) ctx->limits.any64_chunk = any64_chunk;
    ctx->have_m3 = emu_have_m3;
    return ctx;
}
// the chip the launchers plan for, which no API sets either: a value > 0 replaces the context's
extern "C" void emu_ctx_set_chip(spyhip_ctx* ctx, int num_cu, long long lds_per_block) {
    if (num_cu > 0) ctx->num_cu = num_cu;
    if (lds_per_block > 0) ctx->lds_per_block = (size_t)lds_per_block;
}
extern "C" void* emu_ctx_scratch(spyhip_ctx* ctx) { return ctx->scratch; }      // (the column means of cov.hip)
extern "C" void emu_ctx_destroy(spyhip_ctx* ctx) {
    (void)hipFree(ctx->scratch);
    (void)hipFree(ctx->k4h_buf);
    delete ctx;
}
