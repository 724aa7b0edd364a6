// CPU emulation of the envelope correlations, TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's own launchers
// (syncopy_amd/csrc/envcorr.hip) and kernels, on the runtime stand-in hip/hip_runtime.h.  Built by tests/test_envcorr.py.
#include "hip_emu.h"
#include "../../syncopy_amd/csrc/envcorr.hip"
#include "emu_unit.h"
