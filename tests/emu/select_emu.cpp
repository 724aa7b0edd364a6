// CPU emulation of the data selection, TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's own launcher
// (syncopy_amd/csrc/select.hip) and kernels, on the runtime stand-in hip/hip_runtime.h.  Built by tests/test_select.py.
#include "hip_emu.h"
#include "../../syncopy_amd/csrc/select.hip"
#include "emu_unit.h"
