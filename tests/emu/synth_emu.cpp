// CPU emulation of the synthetic-data kernels, TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's own launchers
// (syncopy_amd/csrc/synth.hip) and kernels, on the runtime stand-in hip/hip_runtime.h.  Built by tests/test_synth.py.
#include "hip_emu.h"
#include "../../syncopy_amd/csrc/synth.hip"
#include "emu_unit.h"
