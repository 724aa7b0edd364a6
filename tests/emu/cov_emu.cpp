// CPU emulation of the channel covariance, TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's own launcher
// (syncopy_amd/csrc/cov.hip) and kernels, on the runtime stand-in hip/hip_runtime.h.  Built by tests/test_timelock.py.
#include "../../syncopy_amd/csrc/cov.hip"
#include "emu_unit.h"

// the same launcher with 2 waves per mean instead of 8 (the cases of test_emu_cov are tuned to it)
extern "C" int emu_cov_small(spyhip_ctx* ctx, const float* x, float* out, int64_t ntrials, int64_t n, int64_t nchan, int64_t ddof) {
    return cov_launch<2>(ctx, x, out, ntrials, n, nchan, ddof);
}
