// CPU emulation of the phase-lag family, TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's own launchers
// (syncopy_amd/csrc/phaselag.hip) and kernels, on the runtime stand-in hip/hip_runtime.h.  Built by tests/test_phaselag.py.
#include "hip_emu.h"
#include "../../syncopy_amd/csrc/phaselag.hip"
#include "emu_unit.h"
