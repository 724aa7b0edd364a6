// CPU emulation of the phase slope index, TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's own launchers
// (syncopy_amd/csrc/phaseslope.hip) and kernels, on the runtime stand-in hip/hip_runtime.h.  Built by tests/test_psi.py.
#include "hip_emu.h"
#include "../../syncopy_amd/csrc/phaseslope.hip"
#include "emu_unit.h"
