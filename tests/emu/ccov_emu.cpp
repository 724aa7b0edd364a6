// CPU emulation of the cross-covariance lags (K8), TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's own launchers
// (syncopy_amd/csrc/ccov.hip) and kernels, on the runtime stand-in hip/hip_runtime.h.  Lag transforms above 8192 points
// go through spyhip_fft_plan_create / _exec, which the emulator does not run on the library's host code yet: the three
// entry points refuse here with EMU_NOT_EMULATED, and so does spyhip_ccov_from_accumulator for trials of more than 5461
// samples.  Built by tests/csd_drive.py.
#include "hip_emu.h"

#include "../../syncopy_amd/csrc/ccov.hip"
#include "emu_unit.h"

extern "C" int spyhip_fft_plan_create(spyhip_ctx*, int, int, int, int, const double*, double, int, int, const int32_t*, int, int, int,
                                      spyhip_fft_plan**) { return EMU_NOT_EMULATED; }
extern "C" int spyhip_fft_exec(spyhip_fft_plan*, const float*, int64_t, const int32_t*, const int64_t*, const int64_t*, const int64_t*,
                               int, void*) { return EMU_NOT_EMULATED; }
extern "C" int spyhip_fft_plan_destroy(spyhip_fft_plan*) { return EMU_NOT_EMULATED; }
