// CPU emulation of the up-FIR-down kernel (syncopy_amd/csrc/resample_kernel.h), TEST INFRASTRUCTURE ONLY (see
// hip_emu.h).  Launches the kernel as resample.hip does, on small tiles: 2 waves share chunks of 8 taps, 4 or 1 outputs
// per lane, the most whose staged rows fit MAX_ROWS.  Built by tests/test_resample.py.
#include "hip_emu.h"

namespace emu {
thread_local dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
thread_local BlockCtx* t_ctx = nullptr;
}  // namespace emu

#include "../../syncopy_amd/csrc/resample_kernel.h"

namespace {
constexpr int NT = 2, KC = 8;
constexpr long long MAX_ROWS = 32;

template <int R>
void launch(const float* in, float* out, long long T, long long N, long long C, long long nout, const double* taps, int ntaps,
            int up, int down) {
    using Tile = spyres::UpfirdnTile<R, NT, KC>;
    const long long per_phase = (nout + up - 1) / up, ublocks = (per_phase + R - 1) / R;
    const dim3 g((unsigned)(ublocks * up), (unsigned)((C + 63) / 64), (unsigned)T), b(Tile::THREADS);
    emu::launch(g, b, (size_t)Tile::lds_bytes(down),
                [&] { spyres::upfirdn_kernel<R, NT, KC>(in, out, taps, ntaps, N, C, nout, up, down, ublocks); });
}
}  // namespace

extern "C" {

// returns the outputs per lane of the tile that ran
int emu_upfirdn(const float* in, float* out, long long T, long long N, long long C, long long nout, const double* taps,
                int ntaps, int up, int down) {
    if (spyres::UpfirdnTile<4, NT, KC>::rows(down) <= MAX_ROWS) {
        launch<4>(in, out, T, N, C, nout, taps, ntaps, up, down);
        return 4;
    }
    launch<1>(in, out, T, N, C, nout, taps, ntaps, up, down);
    return 1;
}

}  // extern "C"
