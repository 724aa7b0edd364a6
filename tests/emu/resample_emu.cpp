// CPU emulation of the up-FIR-down resampling, TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's own launcher
// (syncopy_amd/csrc/resample.hip) and kernel, on the runtime stand-in hip/hip_runtime.h.  Built by tests/test_resample.py.
#include "../../syncopy_amd/csrc/resample.hip"
#include "emu_unit.h"

// the same launcher on small tiles: 2 waves share chunks of 8 taps, 4 or 1 outputs per lane, at most 32 staged rows
// (SHAPES of test_resample.py is tuned to them)
extern "C" int emu_upfirdn_small(spyhip_ctx* ctx, const float* in, float* out, int64_t ntrials, int64_t nsamp, int64_t nchan,
                                 int64_t nout, const double* taps, int ntaps, int up, int down) {
    return upfirdn_launch<UfdCfg<2, 8, 32, 4, 1>>(ctx, in, out, ntrials, nsamp, nchan, nout, taps, ntaps, up, down);
}
