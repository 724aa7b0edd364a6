// CPU emulation of the directed-measure finalizer, TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's own launcher
// (syncopy_amd/csrc/directed.hip) and kernels, on the runtime stand-in hip/hip_runtime.h.  Built by tests/test_directed.py.
#include "hip_emu.h"
#include "../../syncopy_amd/csrc/directed.hip"
#include "emu_unit.h"
