// CPU emulation of the channel concatenation, TEST INFRASTRUCTURE ONLY (see hip_emu.h): the library's own launcher
// (syncopy_amd/csrc/concat.hip) and kernel, on the runtime stand-in hip/hip_runtime.h.  Built by tests/test_concat.py.
#include "hip_emu.h"
#include "../../syncopy_amd/csrc/concat.hip"
#include "emu_unit.h"
